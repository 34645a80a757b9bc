"""csrc/tsdflabel.hip through the host emulator behind the product's Python layer (contrib.InstanceTsdfVolume; torch CPU
tensors as device memory): the cases (a) .. (e) of tests/tsdflabel_cases.py -- the bytes of ``labels`` and of the volume
after every integrate, every label image, statistics table, grid and origin -- bitwise equal to the NumPy mirror
(tests/tsdflabel_ref.py); and the volume a labelled integrate leaves is, byte for byte, the plain integrate's."""
import numpy as np
import pytest
import torch

import tsdflabel_cases as C
from host_emul import emul
from morefusion_amd.contrib import TsdfVolume

pytestmark = pytest.mark.skipif(not emul.available(), reason="g++ not available")


@pytest.fixture()
def product(monkeypatch):
    emul.patch_lib(emul.build(["tsdf.hip", "tsdflabel.hip"]), monkeypatch)


@pytest.fixture(scope="module")
def mirror():
    return {name: C.run_mirror(C.make_case(name)) for name in C.CASES}


@pytest.mark.parametrize("name", C.CASES)
def test_case_bitwise_vs_mirror(product, mirror, name):
    C.assert_equal(C.run_product(C.make_case(name), "cpu"), mirror[name])


@pytest.mark.parametrize("name", C.CASES)
def test_labelled_integrate_leaves_the_plain_integrates_volume(product, name):
    """The same frames through TsdfVolume.integrate (mf_tsdf_integrate, no labels anywhere): the volume's bytes after
    every frame are those the labelled sequence left."""
    case = C.make_case(name)
    got = [r["volume"] for r, op in zip(C.run_product(case, "cpu"), case["ops"]) if op[0] == "integrate"]
    volume = {k: v for k, v in case["volume"].items() if k != "max_count"}
    plain, n = TsdfVolume(device="cpu", **volume), 0
    for op in case["ops"]:
        if op[0] == "integrate":
            skip = None if op[4] is None else torch.tensor([op[4]], dtype=torch.int32)
            plain.integrate(op[1], C.K, op[2], skip_if=skip)
            assert plain.volume.numpy().tobytes() == got[n].tobytes(), n
            n += 1
    assert n == len(got) >= 2 and (got[-1][..., 1] > 0).any()


def test_what_the_cases_show(mirror):
    """The properties the sequences are there for, read off the mirror's results."""
    a, b, c, d, e = (mirror[name] for name in C.CASES)
    assert a[0]["labels"][..., 1].max() == 1 and a[3]["labels"][..., 1].max() == 3
    assert (a[0]["labels"][..., 0] == 7).any() and not (a[3]["labels"][..., 0] == 7).any()
    assert b[3]["labels"][..., 1].max() == 2  # saturated at max_count = 2 after four frames
    before, after = c[1]["labels"], c[4]["labels"]  # the spheres' voxels changed hands
    assert ((before[..., 0] == 1) & (after[..., 0] == 3)).sum() > 50
    assert ((before[..., 0] == 3) & (after[..., 0] == 1)).sum() > 50
    assert d[1]["labels"].tobytes() == d[0]["labels"].tobytes() and d[1]["volume"].tobytes() == d[0]["volume"].tobytes()
    assert d[3]["labels"].tobytes() != d[1]["labels"].tobytes()
    assert e[1]["labels"].tobytes() == e[0]["labels"].tobytes() and e[1]["volume"].tobytes() != e[0]["volume"].tobytes()
    assert np.array_equal(a[6]["table"][[1, 3]], a[4]["table"][:2]) and a[6]["table"][0, 0] > 1000  # the 64-id call
