"""csrc/tsdfrender.hip through the host emulator behind the product's Python layer (contrib.TsdfVolume.render /
InstanceTsdfVolume.render; torch CPU tensors as device memory), built together with csrc/tsdf.hip and csrc/tsdflabel.hip:
on every case of tests/tsdfrender_cases.py and B = 2, 4, 8 the summary's bytes, depth, end code, label image and
``sampled`` are bitwise equal to the NumPy mirror (tests/tsdfrender_ref.py), and sampled <= visited <= the ray's
samples.  The old kernels of the same library give the same depth, code and labels on the same tensors."""
import numpy as np
import pytest
import torch

import tsdf_cases as TC
import tsdflabel_cases as LC
import tsdfrender_cases as C
import tsdfrender_ref as RR
from host_emul import emul
from morefusion_amd.contrib import InstanceTsdfVolume, ModelTracker, TsdfVolume

pytestmark = pytest.mark.skipif(not emul.available(), reason="g++ not available")


@pytest.fixture()
def product(monkeypatch):
    emul.patch_lib(emul.build(["tsdf.hip", "tsdflabel.hip", "tsdfrender.hip"]), monkeypatch)


@pytest.mark.parametrize("name", C.NAMES)
def test_cases_bitwise_vs_mirror(product, name):
    case = C.make_case(name)
    C.assert_equal(C.run_product(case, "cpu"), C.run_mirror(case))


def test_block_edge_16_and_a_volume_wider_than_one_workgroup(product):
    """B = 16 (the cases use 2, 4, 8) and nx = 300 > 256: the x run of a block row is split over two workgroups, the
    second of which is partial."""
    rs = np.random.RandomState(3)
    vol = TsdfVolume((300, 19, 35), 0.01, (0.0, 0.0, 0.0), device="cpu")
    data = np.ones((35, 19, 300, 2), np.float32)
    data[..., 1] = rs.rand(35, 19, 300) < 0.9995  # a few unseen voxels
    data[:, :, 100:180, 1] = 0.0                   # an unseen slab
    data[..., 0][rs.rand(35, 19, 300) < 0.0005] = 0.5
    vol.volume.copy_(torch.from_numpy(data))
    for B in RR.BLOCK_EDGES:
        exp = RR.block_summary(data, B)
        got = vol.block_summary(B).numpy()
        assert got.shape == exp.shape == vol.summary_shape(B) and np.array_equal(got, exp), B
        assert set(np.unique(exp).tolist()) == {RR.MIXED, RR.FREE, RR.UNKNOWN}, B
        assert len(np.unique(exp[:, :, 256 // B:])) > 1  # the second workgroup's blocks are not all alike


def test_render_equals_the_old_kernels_on_the_same_tensors(product):
    vol = InstanceTsdfVolume(device="cpu", **LC.VOLUME)
    for k in range(3):
        depth, label, T = LC.frame(k)
        vol.integrate(depth, LC.K, T, label=label)
    depth, code = vol.raycast(LC.K, LC.HELD_OUT, C.H, C.W, return_code=True)
    label = vol.label_image(depth, LC.K, LC.HELD_OUT, min_count=2)
    for B in RR.BLOCK_EDGES:
        got = vol.render(LC.K, LC.HELD_OUT, C.H, C.W, block=B, return_code=True, labels=True, min_count=2)
        for g, e in zip(got, (depth, label, code)):
            assert g.dtype == e.dtype and g.numpy().tobytes() == e.numpy().tobytes(), B
        assert torch.equal(vol.render(LC.K, LC.HELD_OUT, C.H, C.W, block=B), depth)
    assert (label != 0).sum() > 100


def test_python_layer_refusals(product):
    vol = TsdfVolume(device="cpu", **TC.make_case("a")["volume"])
    K, T = C.K_WIDE, TC.pose()
    with pytest.raises(ValueError, match="block"):
        vol.block_summary(3)
    with pytest.raises(ValueError, match="block"):
        vol.render(K, T, C.H, C.W, block=32)
    with pytest.raises(ValueError, match="summary"):
        vol.render(K, T, C.H, C.W, block=4, summary=vol.block_summary(8))
    with pytest.raises(ValueError, match="summary"):
        vol.render(K, T, C.H, C.W, block=4, summary=vol.block_summary(4).to(torch.int32))
    with pytest.raises(ValueError, match="step"):
        vol.render(K, T, C.H, C.W, step=0.0)
    with pytest.raises(ValueError, match="min_depth"):
        vol.render(K, T, C.H, C.W, min_depth=2.0, max_depth=1.0)
    with pytest.raises(ValueError, match="block"):
        ModelTracker(K, C.H, C.W, vol, skip_empty=True, block=5)
    inst = InstanceTsdfVolume(device="cpu", **LC.VOLUME)
    with pytest.raises(ValueError, match="min_count"):
        inst.render(K, T, C.H, C.W, labels=True, min_count=0)


def test_the_kernel_jumps(product):
    """On the main render with B = 4 (blocks of 16 cm, a step of 5 cm) fewer positions are computed than the rays have
    samples; a block of B = 2 holds at most two samples of a ray, so there is nothing to jump over.  The mirror's
    ``sampled`` is met all the same (test_cases_bitwise_vs_mirror)."""
    name, n = C.MAIN
    case = C.make_case(name)
    got, exp = C.run_product(case, "cpu")[n], C.run_mirror(case)[n]
    visited, total = int(got[4]["stats"][..., 1].sum()), int(exp[4]["total"].sum())
    assert int(exp[4]["sampled"].sum()) < visited < total, (visited, total)
    assert int(got[2]["stats"][..., 1].sum()) == int(exp[2]["total"].sum())
