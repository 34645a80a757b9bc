"""TSDF colour on the MI355X (csrc/tsdfcolor.hip through contrib.TsdfVolume(colors=True), InstanceTsdfVolume(colors=True)
and ModelTracker) against the NumPy mirror (tests/tsdfcolor_ref.py), bit for bit: the cases (a) .. (e) of
tests/tsdfcolor_cases.py; run-to-run identity; the volume and label bytes of a coloured run against the uncoloured run;
ModelTracker.track(depth, label, color) against integrating by hand at its poses; the skip word; the mesh's colours."""
import numpy as np
import pytest
import torch

import tsdfcolor_cases as C
from morefusion_amd.contrib import InstanceTsdfVolume, ModelTracker, TsdfVolume

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mirror():
    return {name: C.run_mirror(C.make_case(name)) for name in C.CASES}


@pytest.fixture(scope="module")
def device_runs():
    return {name: C.run_product(C.make_case(name), "cuda") for name in C.CASES}


@pytest.mark.parametrize("name", C.CASES)
def test_kernel_cases_bitwise_vs_mirror(device_runs, mirror, name):
    C.assert_equal(device_runs[name], mirror[name])


@pytest.mark.parametrize("name", "ae")
def test_two_runs_are_byte_identical(device_runs, name):
    again = C.run_product(C.make_case(name), "cuda")
    for n, (g, e) in enumerate(zip(again, device_runs[name])):
        assert set(g) == set(e)
        for key in g:
            assert g[key].tobytes() == e[key].tobytes(), (n, key)


@pytest.mark.parametrize("name", C.CASES)
def test_coloured_run_leaves_the_uncoloured_runs_volume_and_labels(device_runs, name):
    case = C.make_case(name)
    got = [r for r, op in zip(device_runs[name], case["ops"]) if op[0] == "integrate"]
    plain = (InstanceTsdfVolume if case["instance"] else TsdfVolume)(**case["volume"])
    assert plain.colors is None
    n = 0
    for op in case["ops"]:
        if op[0] == "integrate":
            _, depth, T, label, skip, _ = op
            skip = None if skip is None else torch.tensor([skip], dtype=torch.int32, device="cuda")
            plain.integrate(depth, C.K, T, skip_if=skip, **({} if label is None else dict(label=label)))
            assert plain.volume.cpu().numpy().tobytes() == got[n]["volume"].tobytes(), n
            if case["instance"]:
                assert plain.labels.cpu().numpy().tobytes() == got[n]["labels"].tobytes(), n
            n += 1
    assert n == len(got) >= 3


def test_model_tracker_fuses_what_integrating_at_its_poses_fuses():
    vol, by_hand, trk, lost = C.tracked_and_by_hand("cuda")
    assert not any(lost)
    for name in ("volume", "labels", "colors"):
        assert getattr(vol, name).cpu().numpy().tobytes() == getattr(by_hand, name).cpu().numpy().tobytes(), name
    assert vol.colors[..., 3].max() == 5 and (vol.colors[..., 3] > 0).sum() > 5000
    # a lost frame: the device skip word keeps all three tensors as they are
    depth, label, rgb, _ = C.frame(2)
    gone = ModelTracker(C.K, C.H, C.W, vol, **dict(C.TRACKER_KNOBS, min_pairs=C.H * C.W + 1))
    gone._T_last = trk._T_last
    before = [getattr(vol, name).cpu().numpy().copy() for name in ("volume", "labels", "colors")]
    gone.track(depth, label, rgb)
    assert gone.lost
    for name, b in zip(("volume", "labels", "colors"), before):
        assert getattr(vol, name).cpu().numpy().tobytes() == b.tobytes(), name


def test_a_set_skip_word_leaves_the_colours_untouched():
    vol = TsdfVolume(colors=True, **C.VOLUME)
    depth, _, rgb, T = C.frame(0)
    vol.integrate(depth, C.K, T, color=rgb)
    before = vol.colors.cpu().numpy().copy()
    assert (before[..., 3] == 1).sum() > 3000
    depth, _, rgb, T = C.frame(1)
    vol.integrate(depth, C.K, T, color=rgb, skip_if=torch.tensor([7], dtype=torch.int32, device="cuda"))
    assert vol.colors.cpu().numpy().tobytes() == before.tobytes() and vol.weight.max() == 1
    vol.integrate(depth, C.K, T, color=rgb, skip_if=torch.tensor([0], dtype=torch.int32, device="cuda"))
    assert vol.colors[..., 3].max() == 2 and vol.weight.max() == 2


def test_extract_mesh_with_colours_is_sample_colors_of_its_vertices(mirror):
    case = C.make_case("a")
    vol = TsdfVolume(colors=True, **case["volume"])
    for op in case["ops"][:3]:
        vol.integrate(op[1], C.K, op[2], color=op[5])
    vertices, faces, normals, colors = vol.extract_mesh(normals=True, colors=True)
    plain = vol.extract_mesh(normals=True)
    assert all(torch.equal(a, b) for a, b in zip((vertices, faces, normals), plain))
    assert colors.is_cuda and colors.dtype == torch.uint8 and tuple(colors.shape) == (len(vertices), 4)
    assert torch.equal(colors, vol.sample_colors(vertices))
    assert np.array_equal(colors.cpu().numpy(), mirror["a"][4]["vertex_colors"])
    assert vol.sample_colors(np.zeros((0, 3))).shape == (0, 4)
