"""TSDF fusion on the MI355X (csrc/tsdf.hip through contrib.TsdfVolume / contrib.ModelTracker) against the NumPy mirror
(tests/tsdf_ref.py), bit for bit: the kernel cases (a) .. (e) of tests/tsdf_cases.py; one 480 x 640 frame into a 64^3
volume and its ray-cast; run-to-run identity; the 120 x 160 four-frame sequence through ModelTracker on device tensors
(which carries the host test's accuracy over to the device); and a forced loss that must leave the model untouched."""
import numpy as np
import pytest
import torch

import camtrack_cases as CC
import tsdf_cases as C
import tsdf_ref as R
from morefusion_amd.contrib import ModelTracker, TsdfVolume

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", ["a", "b", "c", "d", "e"])
def test_kernel_cases_bitwise_vs_mirror(name):
    case = C.make_case(name)
    C.assert_equal(C.run_product(case, "cuda"), C.run_mirror(case))


FULL_VOLUME = dict(dims=(64, 64, 64), pitch=0.025, origin=(-0.8, -0.9, 0.2))


@pytest.fixture(scope="module")
def full_frames():
    return CC.sequence(0, 2, 480, 640)


def _full_run(frames):
    vol = TsdfVolume(**FULL_VOLUME)
    vol.integrate(torch.as_tensor(frames[0]["depth"]).cuda(), frames[0]["K"], frames[0]["T_sensor_to_map"])
    depth, code = vol.raycast(frames[0]["K"], torch.as_tensor(frames[1]["T_sensor_to_map"]).cuda(), 480, 640,
                              return_code=True)
    return vol.volume.cpu().numpy(), depth.cpu().numpy(), code.cpu().numpy()


def test_full_frame_into_64_cubed_bitwise_vs_mirror(full_frames):
    f0, f1 = full_frames
    volume, depth, code = _full_run(full_frames)
    ref = R.Volume(**FULL_VOLUME)
    ref.integrate(f0["depth"], f0["K"], f0["T_sensor_to_map"])
    e_depth, e_code = ref.raycast(f0["K"], f1["T_sensor_to_map"], 480, 640)
    assert np.array_equal(volume, ref.volume)
    assert np.array_equal(code, e_code) and np.array_equal(depth, e_depth)
    hit = code == R.HIT
    # a hit needs two valid samples = up to 16 observed voxels; the frame has 3 % holes, so about 0.97^16 = 0.6 of
    # the rays that meet a surface inside the volume (more than half of the image) hit, the others are back faces
    assert hit.mean() > 0.25 and (depth[hit] > 0).all() and not depth[~hit].any()
    # the render is the scene: where both have a depth, frame 1's own image is within a voxel of it (median)
    both = hit & (f1["depth"] > 0)
    assert np.median(np.abs(depth[both] - f1["depth"][both])) < FULL_VOLUME["pitch"]


def test_two_identical_call_sequences_give_identical_bytes(full_frames):
    runs = [_full_run(full_frames) for _ in range(2)]
    for a, b in zip(*runs):
        assert a.tobytes() == b.tobytes()


def test_sequence_through_model_tracker_on_device_tensors():
    seed = CC.ACCURACY_SEEDS[0]
    frames = C.model_sequence(seed)
    exp, ref = C.track_model_mirror(frames)
    H, W = CC.ACCURACY_SHAPE
    vol = TsdfVolume(**C.MODEL_VOLUME)
    trk = ModelTracker(frames[0]["K"], H, W, vol)
    got = []
    for k, f in enumerate(frames):
        T = trk.track(torch.as_tensor(f["depth"]).cuda())
        assert T.is_cuda and T.dtype == torch.float64 and T.shape == (4, 4)
        got.append(T.cpu().numpy())
        if k:
            assert not trk.lost
    assert np.array_equal(np.stack(got), exp)
    assert np.array_equal(trk.stats, ref.stats[0])
    assert np.array_equal(vol.volume.cpu().numpy(), ref.volume.volume)
    for t_err, r_err, t_id, r_id in CC.sequence_errors(frames, got):
        assert t_err <= t_id / 4 and r_err <= r_id / 4


def test_a_lost_alignment_leaves_the_model_untouched():
    """min_pairs beyond the number of pixels: the alignment is lost.  Nothing reads the status between the alignment
    and the integrate (ModelTracker.track never does); the volume's bytes are equal before and after, the pose is
    the last one."""
    frames = C.model_sequence(CC.ACCURACY_SEEDS[0])[:2]
    H, W = CC.ACCURACY_SHAPE
    vol = TsdfVolume(**C.MODEL_VOLUME)
    trk = ModelTracker(frames[0]["K"], H, W, vol, min_pairs=H * W + 1)
    T0 = trk.track(frames[0]["depth"]).cpu().numpy()
    before = vol.volume.cpu().numpy().copy()
    assert (before[..., 1] > 0).any()
    T1 = trk.track(frames[1]["depth"]).cpu().numpy()
    after = vol.volume.cpu().numpy()
    assert after.tobytes() == before.tobytes()
    assert trk.lost and np.allclose(T1, T0, rtol=0, atol=1e-15)
    # and with the word clear the same frame does go in
    vol.integrate(frames[1]["depth"], frames[0]["K"], T1, skip_if=torch.zeros(1, dtype=torch.int32, device="cuda"))
    assert vol.volume.cpu().numpy().tobytes() != before.tobytes()
