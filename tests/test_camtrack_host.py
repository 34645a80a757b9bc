"""Camera tracking without a GPU: the accuracy of the NumPy mirror (tests/camtrack_ref.py) on synthetic sequences --
the condition the device inherits by being bitwise equal to it --, the argument validation of align_depth and
CameraTracker, and the reference policies of CameraTracker (on the host emulator) against the mirror's Tracker."""
import numpy as np
import pytest
import torch

import camtrack_cases as C
import camtrack_ref as R
from host_emul import emul
from morefusion_amd.contrib import CameraTracker, align_depth


@pytest.mark.parametrize("seed", C.ACCURACY_SEEDS)
def test_mirror_tracks_frame_to_frame_from_the_identity(seed):
    """On every frame the translation and the rotation error are at most a quarter of the identity pose's (a tracker
    that does not do that is not tracking), and at most twice what was recorded for the mirror in camtrack_cases.py
    (the factor covers platform-dependent NumPy details only: no libm function is on the path)."""
    frames = C.sequence(seed, 3, *C.ACCURACY_SHAPE)
    poses, trk = C.track_mirror(frames)
    assert np.array_equal(poses[0], np.eye(4)) and trk.status[0] == R.TRACKING
    errors = C.sequence_errors(frames, poses)
    print(f"seed {seed}: (t_err, r_err, identity's t_err, r_err) = {errors}")
    for (t_err, r_err, t_id, r_id), (t_rec, r_rec) in zip(errors, C.MIRROR_ERRORS[seed]):
        assert t_err <= t_id / 4 and r_err <= r_id / 4
        assert t_err <= 2 * t_rec and r_err <= 2 * r_rec


def test_align_depth_validates_its_arguments():
    d, K, T = np.ones((32, 40), np.float32), np.array([[50.0, 0, 20], [0, 50.0, 16], [0, 0, 1]]), np.eye(4)
    for kwargs, match in ((dict(levels=4, iterations=(1,) * 4), "at least 8 x 8"), (dict(levels=0, iterations=()), "levels"),
                          (dict(levels=9, iterations=(1,) * 9), "levels"),
                          (dict(levels=2, iterations=(1, 2, 3)), "3 iteration counts for 2 levels"),
                          (dict(levels=2, iterations=(1, -2)), ">= 0"),
                          (dict(levels=2, iterations=(1, 1), distance_threshold=-1.0), "distance_threshold"),
                          (dict(levels=2, iterations=(1, 1), angle_threshold=200.0), "angle_threshold"),
                          (dict(levels=2, iterations=(1, 1), min_pairs=-1), "min_pairs"),
                          (dict(levels=2, iterations=(1, 1), block_band=-0.1), "block_band")):
        with pytest.raises(ValueError, match=match):
            align_depth(d, d, K, T, device="cpu", **kwargs)
    ok = dict(levels=2, iterations=(1, 1), device="cpu")
    with pytest.raises(ValueError, match="differ in shape"):
        align_depth(d, d[:, :36], K, T, **ok)
    with pytest.raises(ValueError, match="T_ref_to_map"):
        align_depth(d, d, K, np.eye(3), **ok)
    with pytest.raises(ValueError, match="T_init"):
        align_depth(d, d, K, T, np.zeros((2, 4, 4)), **ok)
    with pytest.raises(ValueError, match="3 x 3"):
        align_depth(d, d, np.eye(4), T, **ok)
    with pytest.raises(ValueError, match="fx and fy"):
        align_depth(d, d, np.zeros((3, 3)), T, **ok)
    with pytest.raises(TypeError, match="float image"):
        align_depth(d.astype(np.int32), d, K, T, **ok)
    with pytest.raises(ValueError, match="dimensions"):
        align_depth(d[None, None], d, K, T, **ok)
    with pytest.raises(ValueError, match="alignments"):
        align_depth(np.ones((1025, 8, 8), np.float32), np.ones((1025, 8, 8), np.float32), K, T, levels=1,
                    iterations=(1,), device="cpu")


def test_camera_tracker_validates_its_arguments():
    K = np.array([[50.0, 0, 20], [0, 50.0, 16], [0, 0, 1]])
    with pytest.raises(ValueError, match="'previous' or 'first'"):
        CameraTracker(K, 32, 40, levels=2, iterations=(1, 1), reference="model", device="cpu")
    with pytest.raises(ValueError, match="at least 8 x 8"):
        CameraTracker(K, 30, 40, device="cpu")
    with pytest.raises(ValueError, match="iteration counts for 2 levels"):
        CameraTracker(K, 32, 40, levels=2, device="cpu")
    with pytest.raises(ValueError, match="T_first"):
        CameraTracker(K, 32, 40, levels=2, iterations=(1, 1), T_first=np.eye(3), device="cpu")


@pytest.fixture()
def product(monkeypatch):
    if not emul.available():
        pytest.skip("g++ not available")
    emul.patch_lib(emul.build(["camtrack.hip", "pickorder.hip"]), monkeypatch)


KNOBS = dict(levels=2, iterations=(3, 2), min_pairs=20)


@pytest.fixture(scope="module")
def frames():
    return C.sequence(4, 3, 30, 40)


@pytest.mark.parametrize("policy", ["previous", "first"])
def test_reference_policy_matches_the_mirror(product, frames, policy):
    anchor = np.array([[0.0, 0, 1, 0.5], [1, 0, 0, -0.25], [0, 1, 0, 2.0], [0, 0, 0, 1]])
    trk = CameraTracker(frames[0]["K"], 30, 40, reference=policy, T_first=anchor, device="cpu", **KNOBS)
    ref = R.Tracker(frames[0]["K"], reference=policy, T_first=anchor, **KNOBS)
    with pytest.raises(RuntimeError, match="no alignment yet"):
        trk.status
    for k, f in enumerate(frames):
        got = trk.track(torch.as_tensor(f["depth"]) if k % 2 else f["depth"])  # NumPy arrays and tensors alike
        assert isinstance(got, torch.Tensor) and got.dtype == torch.float64 and got.shape == (4, 4)
        assert np.array_equal(got.numpy(), ref.track(f["depth"])), k
        if k == 0:
            assert np.array_equal(got.numpy(), anchor)
        else:
            assert trk.status == ref.status[0] == R.TRACKING and not trk.lost
            assert np.array_equal(trk.stats, ref.stats[0])
    with pytest.raises(ValueError, match="30 x 40"):
        trk.track(np.ones((30, 41), np.float32))


def test_the_policies_differ_and_set_reference_is_either(product, frames):
    """Frame 2 against frame 1 ("previous") is not frame 2 against frame 0 ("first"); a "first" tracker whose
    reference is set to frame 1 at the pose the "previous" tracker found for it gives the "previous" answer."""
    K = frames[0]["K"]
    prev, first, manual = (CameraTracker(K, 30, 40, reference=p, device="cpu", **KNOBS)
                           for p in ("previous", "first", "first"))
    Tp = [prev.track(f["depth"]).numpy() for f in frames]
    Tf = [first.track(f["depth"]).numpy() for f in frames]
    assert np.array_equal(Tp[1], Tf[1]) and not np.array_equal(Tp[2], Tf[2])
    for f in frames[:2]:
        manual.track(f["depth"])
    manual.set_reference(frames[1]["depth"], Tp[1])
    assert np.array_equal(manual.track(frames[2]["depth"]).numpy(), Tp[2])
    # a tracker that starts from set_reference: the first track() already aligns
    fresh = CameraTracker(K, 30, 40, device="cpu", **KNOBS).set_reference(frames[0]["depth"], np.eye(4))
    assert np.array_equal(fresh.track(frames[1]["depth"]).numpy(), Tp[1])
