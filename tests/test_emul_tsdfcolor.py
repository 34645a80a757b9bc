"""csrc/tsdfcolor.hip through the host emulator behind the product's Python layer (contrib.TsdfVolume(colors=True) /
contrib.InstanceTsdfVolume(colors=True); torch CPU tensors as device memory): the cases (a) .. (e) of
tests/tsdfcolor_cases.py -- the bytes of ``colors``, the volume and the labels after every integrate, every colour image,
every sampled set -- bitwise equal to the NumPy mirror (tests/tsdfcolor_ref.py); the colour pass leaves the volume and
the labels what the uncoloured run leaves; and the Python surface's argument checks."""
import numpy as np
import pytest
import torch

import tsdfcolor_cases as C
from host_emul import emul
from morefusion_amd.contrib import InstanceTsdfVolume, TsdfVolume

pytestmark = pytest.mark.skipif(not emul.available(), reason="g++ not available")


@pytest.fixture()
def product(monkeypatch):
    L = emul.build(["tsdf.hip", "tsdflabel.hip", "tsdfmesh.hip", "tsdfcolor.hip"])
    calls = []

    class Counting:
        def __getattr__(self, name):
            fn = getattr(L, name)

            def call(*args):
                calls.append(name)
                return fn(*args)
            return call
    emul.patch_lib(Counting(), monkeypatch)
    return calls


@pytest.fixture(scope="module")
def mirror():
    return {name: C.run_mirror(C.make_case(name)) for name in C.CASES}


@pytest.mark.parametrize("name", C.CASES)
def test_case_bitwise_vs_mirror(product, mirror, name):
    C.assert_equal(C.run_product(C.make_case(name), "cpu"), mirror[name])


@pytest.mark.parametrize("name", C.CASES)
def test_coloured_run_leaves_the_uncoloured_runs_volume_and_labels(product, name):
    """The same frames without ``color=`` into a volume built without ``colors=True``: the (tsdf, weight) and label
    bytes after every frame are those of the coloured run, and that run issues today's launches only."""
    case = C.make_case(name)
    got = [r for r, op in zip(C.run_product(case, "cpu"), case["ops"]) if op[0] == "integrate"]
    cls = InstanceTsdfVolume if case["instance"] else TsdfVolume
    plain, n = cls(device="cpu", **case["volume"]), 0
    assert plain.colors is None
    del product[:]
    for op in case["ops"]:
        if op[0] == "integrate":
            _, depth, T, label, skip, _ = op
            skip = None if skip is None else torch.tensor([skip], dtype=torch.int32)
            plain.integrate(depth, C.K, T, skip_if=skip, **({} if label is None else dict(label=label)))
            assert plain.volume.numpy().tobytes() == got[n]["volume"].tobytes(), n
            if case["instance"]:
                assert plain.labels.numpy().tobytes() == got[n]["labels"].tobytes(), n
            n += 1
    assert n == len(got) >= 3 and set(product) <= {"mf_tsdf_integrate", "mf_tsdf_integrate_labels"} and len(product) == n


def test_arguments_and_the_python_surface(product):
    K = np.array([[50.0, 0, 20], [0, 50.0, 16], [0, 0, 1]])
    d, T, rgb = np.ones((32, 40), np.float32), np.eye(4), np.full((32, 40, 3), 200, np.uint8)
    plain = TsdfVolume((8, 8, 8), 0.1, (0, 0, 0.5), device="cpu")
    assert plain.colors is None
    with pytest.raises(TypeError, match="colors=True"):
        plain.integrate(d, K, T, color=rgb)
    for call in (lambda: plain.color_image(d, K, T), lambda: plain.sample_colors(np.zeros((1, 3))),
                 lambda: plain.extract_mesh(colors=True)):
        with pytest.raises(TypeError, match="colors=True"):
            call()
    assert not plain.weight.any() and product == []
    for cls in (TsdfVolume, InstanceTsdfVolume):
        vol = cls((8, 8, 8), 0.1, (0, 0, 0.5), device="cpu", colors=True)
        assert vol.colors.shape == (8, 8, 8, 4) and vol.colors.dtype == torch.float32 and not vol.colors.any()
        extra = dict(label=np.ones((32, 40), np.int32)) if cls is InstanceTsdfVolume else {}
        with pytest.raises(TypeError, match="uint8"):
            vol.integrate(d, K, T, color=rgb.astype(np.float32), **extra)
        with pytest.raises(TypeError, match="uint8"):
            vol.integrate(d, K, T, color=torch.zeros((32, 40, 3), dtype=torch.int32), **extra)
        with pytest.raises(ValueError, match="like the depth"):
            vol.integrate(d, K, T, color=rgb[:, :39], **extra)
        with pytest.raises(ValueError, match="like the depth"):
            vol.integrate(d, K, T, color=np.zeros((32, 40, 4), np.uint8), **extra)
        with pytest.raises(ValueError, match="\\[N, 3\\]"):
            vol.sample_colors(np.zeros((4, 2)))
        assert not vol.weight.any() and not vol.colors.any() and product == []  # nothing above reached a kernel
        empty = vol.sample_colors(np.zeros((0, 3)))
        assert empty.shape == (0, 4) and empty.dtype == torch.uint8 and product == []  # N == 0: no launch
        vol.integrate(d, K, T, color=torch.as_tensor(rgb), **extra)
        assert product == ["mf_tsdf_integrate_labels" if extra else "mf_tsdf_integrate", "mf_tsdf_integrate_colors"]
        coloured = vol.colors[..., 3] > 0
        assert coloured.any() and (vol.colors[..., :3][coloured] == 200).all() and (vol.colors[..., 3][coloured] == 1).all()
        assert vol.reset() is vol and not vol.colors.any() and not vol.weight.any()
        del product[:]


def test_extract_mesh_appends_the_vertex_colours(product):
    case = C.make_case("a")
    vol = TsdfVolume(device="cpu", colors=True, **case["volume"])
    for op in case["ops"][:3]:
        vol.integrate(op[1], C.K, op[2], color=op[5])
    vertices, faces = vol.extract_mesh()
    del product[:]
    v, f, n, c = vol.extract_mesh(normals=True, colors=True)
    assert product == ["mf_tsdfmesh_workspace_bytes", "mf_tsdfmesh_count", "mf_tsdfmesh_emit", "mf_tsdf_sample_colors"]
    assert torch.equal(v, vertices) and torch.equal(f, faces) and n.shape == v.shape
    assert c.dtype == torch.uint8 and c.shape == (len(v), 4) and torch.equal(c, vol.sample_colors(vertices))
    assert len(vol.extract_mesh(colors=True)) == 3 and len(vol.extract_mesh(normals=True)) == 3


@pytest.fixture()
def tracker_product(monkeypatch):
    emul.patch_lib(emul.build(["tsdf.hip", "tsdflabel.hip", "tsdfcolor.hip", "camtrack.hip", "pickorder.hip"]),
                   monkeypatch)


def test_model_tracker_fuses_the_colour_under_its_skip_word(tracker_product):
    """track(depth, label, color) over the five case frames is integrating by hand at the poses it returned; a lost
    frame leaves all three tensors untouched; a colour needs a volume with colours."""
    from morefusion_amd.contrib import ModelTracker
    vol, by_hand, trk, lost = C.tracked_and_by_hand("cpu")
    assert not any(lost)
    for name in ("volume", "labels", "colors"):
        assert getattr(vol, name).numpy().tobytes() == getattr(by_hand, name).numpy().tobytes(), name
    assert vol.colors[..., 3].max() == 5 and (vol.colors[..., 3] > 0).sum() > 5000
    depth, label, rgb, _ = C.frame(2)
    gone = ModelTracker(C.K, C.H, C.W, vol, **dict(C.TRACKER_KNOBS, min_pairs=C.H * C.W + 1))
    gone._T_last = trk._T_last
    before = [getattr(vol, name).numpy().copy() for name in ("volume", "labels", "colors")]
    gone.track(depth, label, rgb)
    assert gone.lost
    for name, b in zip(("volume", "labels", "colors"), before):
        assert getattr(vol, name).numpy().tobytes() == b.tobytes(), name
    plain = ModelTracker(C.K, C.H, C.W, TsdfVolume(device="cpu", **C.VOLUME), **C.TRACKER_KNOBS)
    with pytest.raises(TypeError, match="colors=True"):
        plain.track(depth, color=rgb)
    assert not plain.volume.weight.any()
