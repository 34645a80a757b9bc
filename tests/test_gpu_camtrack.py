"""Camera tracking on the MI355X (csrc/camtrack.hip through contrib.camera_tracking) against the NumPy mirror
(tests/camtrack_ref.py), bit for bit: the kernel cases (a) .. (d) of tests/camtrack_cases.py; a 120 x 160 three-frame
sequence through CameraTracker on device tensors (which carries the host test's accuracy over to the device); one
480 x 640 pair in a single align_depth call; run-to-run identity; and the online example's frames driven with the
tracked poses instead of the ground truth."""
import numpy as np
import pytest
import torch

import camtrack_cases as C
import camtrack_ref as R
from morefusion_amd.contrib import CameraTracker, InstanceTracker, OctomapServer, align_depth

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", ["a", "b", "c", "d"])
def test_kernel_cases_bitwise_vs_mirror(name):
    case = C.make_case(name)
    got, exp = C.run_product(case, "cuda"), C.run_mirror(case)
    C.assert_equal(got, exp)
    lost = {"a": [0], "b": [0, R.LOST_PAIRS], "c": [R.LOST_PAIRS], "d": [0]}[name]
    assert got["status"].tolist() == lost
    for b, code in enumerate(lost):
        if code:
            assert np.array_equal(got["pose"][b], C.initial_pose(case)[b])


def test_sequence_through_camera_tracker_on_device_tensors():
    seed = C.ACCURACY_SEEDS[0]
    frames = C.sequence(seed, 3, *C.ACCURACY_SHAPE)
    exp, ref = C.track_mirror(frames)
    trk = CameraTracker(frames[0]["K"], *C.ACCURACY_SHAPE)
    got = []
    for k, f in enumerate(frames):
        T = trk.track(torch.as_tensor(f["depth"]).cuda())
        assert T.is_cuda and T.dtype == torch.float64
        got.append(T.cpu().numpy())
        if k:
            assert not trk.lost
    assert np.array_equal(np.stack(got), exp)
    assert np.array_equal(trk.stats, ref.stats[0])
    for t_err, r_err, t_id, r_id in C.sequence_errors(frames, got):
        assert t_err <= t_id / 4 and r_err <= r_id / 4


@pytest.fixture(scope="module")
def full_pair():
    f = C.sequence(0, 2, 480, 640)
    return f[1]["depth"], f[0]["depth"], f[0]["K"], f[0]["T_sensor_to_map"], f[1]["T_sensor_to_map"]


def test_full_frame_pair_bitwise_vs_mirror(full_pair):
    cur, ref, K, T_ref, T_true = full_pair
    T, status, stats, pose = align_depth(torch.as_tensor(cur).cuda(), torch.as_tensor(ref).cuda(), K,
                                         torch.as_tensor(T_ref).cuda(), return_pose=True)
    e_pose, e_T, e_status, e_stats = R.align(R.prepare(cur[None], K), R.prepare(ref[None], K), T_ref[None])
    assert np.array_equal(stats.cpu().numpy(), e_stats) and stats.shape == (1, 19, 3)
    assert np.array_equal(pose.cpu().numpy(), e_pose) and np.array_equal(T.cpu().numpy(), e_T)
    assert status.cpu().tolist() == e_status.tolist() == [R.TRACKING]
    t_err, r_err = R.pose_errors(e_T[0], T_true)
    t_id, r_id = R.pose_errors(np.eye(4), T_true)
    assert t_err <= t_id / 4 and r_err <= r_id / 4


def test_two_identical_calls_give_identical_bytes(full_pair):
    cur, ref, K, T_ref, _ = full_pair
    runs = [align_depth(cur, ref, K, T_ref, return_pose=True) for _ in range(2)]  # NumPy in, NumPy out
    assert all(isinstance(x, np.ndarray) for x in runs[0])
    for a, b in zip(*runs):
        assert a.tobytes() == b.tobytes()


def test_online_frames_with_tracked_poses_publish_the_same_instances():
    """examples/online_pose_refinement.py's sequence and loop, once with the ground-truth poses and once with
    CameraTracker's, anchored at frame 0's pose: the server publishes the same instance ids after every frame."""
    from morefusion_amd import geometry, synthetic
    from morefusion_amd.contrib.singleview_3d.models.model import PitchTableModels
    frames = synthetic.make_tracking_sequence(0, 3)
    models = PitchTableModels()
    pitch_of = lambda c: models.get_voxel_pitch(32, int(c))  # noqa: E731
    to_gpu = lambda x: torch.as_tensor(x).cuda()  # noqa: E731
    to_ground = np.array([[1, 0, 0, 0], [0, 0, 1, 0], [0, -1, 0, 0.2], [0, 0, 0, 1]], np.float64)
    K = frames[0]["K"]
    camera = CameraTracker(K, 480, 640, T_first=to_ground @ frames[0]["T_sensor_to_map"])
    published = {}
    for mode in ("truth", "tracked"):
        server = OctomapServer()
        tracker = InstanceTracker(server.mapping, thresholds=dict(min_mask=20, min_bbox=30, min_side=24))
        published[mode] = []
        for k, f in enumerate(frames):
            T = to_ground @ f["T_sensor_to_map"]
            if mode == "tracked":
                T_true, T = T, camera.track(to_gpu(f["depth"])).cpu().numpy()
                assert (k == 0) == np.array_equal(T, T_true) and np.allclose(T, T_true, rtol=0, atol=1e-3)
            pcd = geometry.pointcloud_from_depth(f["depth"], K[0, 0], K[1, 1], K[0, 2], K[1, 2])
            tracked, _, class_of, _ = tracker.track(to_gpu(pcd.astype(np.float32)), to_gpu(f["label_detected"]),
                                                    f["class_ids_by_detection"], K, T)
            server.insert_scan(tracker.pts_map.reshape(pcd.shape), tracked, class_of, pitch_of, origin=T[:3, 3])
            published[mode].append(list(server.publish_grids(T)["instance_ids"]))
    assert published["tracked"] == published["truth"] and len(published["truth"][-1]) >= 3
