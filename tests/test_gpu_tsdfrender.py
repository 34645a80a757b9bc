"""The TSDF render on the MI355X (csrc/tsdfrender.hip through contrib.TsdfVolume.render / InstanceTsdfVolume.render /
ModelTracker(skip_empty=True)): bit for bit against the NumPy mirror (tests/tsdfrender_ref.py) on the cases of
tests/tsdfrender_cases.py; against the old kernels on the same device tensors; a summary that is rebuilt after every
integrate; model tracking with and without skipping; proof that the kernel jumps; and one graph that holds summary and
render."""
import numpy as np
import pytest
import torch

import camtrack_cases as CC
import tsdf_cases as TC
import tsdf_ref as R
import tsdflabel_cases as LC
import tsdfrender_cases as C
import tsdfrender_ref as RR
from morefusion_amd import _lib
from morefusion_amd.contrib import InstanceTsdfVolume, ModelTracker, TsdfVolume

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", C.NAMES)
def test_cases_bitwise_vs_mirror(name):
    case = C.make_case(name)
    C.assert_equal(C.run_product(case, "cuda"), C.run_mirror(case))


def _labelled_volume():
    vol = InstanceTsdfVolume(**LC.VOLUME)
    for k in range(3):
        depth, label, T = LC.frame(k)
        vol.integrate(depth, LC.K, T, label=label)
    return vol


def test_render_equals_raycast_and_label_image_on_the_same_tensors():
    vol = _labelled_volume()
    for T in (LC.HELD_OUT, LC.frame_pose(1)):
        T = torch.as_tensor(T).cuda()
        depth, code = vol.raycast(LC.K, T, C.H, C.W, return_code=True)
        label = vol.label_image(depth, LC.K, T, min_count=2)
        for B in RR.BLOCK_EDGES:
            got = vol.render(LC.K, T, C.H, C.W, block=B, return_code=True, labels=True, min_count=2)
            for g, e in zip(got, (depth, label, code)):
                assert g.dtype == e.dtype and g.shape == e.shape and torch.equal(g, e), B
            assert torch.equal(vol.render(LC.K, T, C.H, C.W, block=B), depth)
        assert (label != 0).sum() > 100 and (code == 0).sum() > 200


def test_the_summary_is_rebuilt_after_an_integrate():
    case = C.make_case("deep")
    (_, d0, K, T0, _), (_, d1, _, T1, _) = [op for op in case["ops"] if op[0] == "integrate"]
    T2 = case["ops"][3][2]
    vol = TsdfVolume(**case["volume"])
    d0 = d0.copy()
    d0[:, C.W // 2:] = np.nan  # the first frame sees the left half only: the second one changes block codes
    vol.integrate(d0, K, T0)
    first, summary0 = vol.render(K, T2, C.H, C.W, block=4), vol.block_summary(4)
    assert torch.equal(first, vol.raycast(K, T2, C.H, C.W))
    vol.integrate(d1, K, T1)
    second = vol.render(K, T2, C.H, C.W, block=4)
    assert torch.equal(second, vol.raycast(K, T2, C.H, C.W))
    assert not torch.equal(second, first) and not torch.equal(vol.block_summary(4), summary0)  # the frame mattered


@pytest.fixture(scope="module")
def tracked():
    """ModelTracker over the four 120 x 160 frames with and without skipping -> per mode (poses, the volume's bytes,
    the volume), and the frames."""
    frames = TC.model_sequence(CC.ACCURACY_SEEDS[0])
    H, W = CC.ACCURACY_SHAPE
    out = {}
    for skip in (False, True):
        vol = TsdfVolume(**TC.MODEL_VOLUME)
        trk = ModelTracker(frames[0]["K"], H, W, vol, skip_empty=skip, block=8)
        poses = [trk.track(torch.as_tensor(f["depth"]).cuda()).cpu().numpy() for f in frames]
        assert not trk.lost
        out[skip] = (np.stack(poses), vol.volume.cpu().numpy(), vol, trk)
    return out, frames


def test_model_tracking_with_skipping_gives_the_same_poses_and_model(tracked):
    plain, skipping = tracked[0][False], tracked[0][True]
    assert plain[0].tobytes() == skipping[0].tobytes()
    assert plain[1].tobytes() == skipping[1].tobytes()
    assert not np.array_equal(plain[0][1], plain[0][0])  # (the camera moved)


def test_the_kernel_jumps_on_the_sequences_last_render(tracked):
    """The render ModelTracker took before the last frame: from the pose of frame 2, of the volume that held frames
    0 .. 2 -- the mirror fuses those frames at the tracked poses.  sum(visited) < the rays' samples, strictly, and
    sum(sampled) is the mirror's."""
    out, frames = tracked
    poses = out[True][0]
    H, W = CC.ACCURACY_SHAPE
    K = frames[0]["K"]
    ref = R.Volume(**TC.MODEL_VOLUME)
    vol = TsdfVolume(**TC.MODEL_VOLUME)
    for f, T in zip(frames[:3], poses[:3]):
        ref.integrate(f["depth"], K, T)
        vol.integrate(f["depth"], K, T)
    assert np.array_equal(vol.volume.cpu().numpy(), ref.volume)
    exp = RR.render_volume(ref, K, poses[2], H, W, 8)
    depth, code, stats = vol.render(K, poses[2], H, W, block=8, return_code=True, return_stats=True)
    stats = stats.cpu().numpy()
    assert depth.cpu().numpy().tobytes() == exp["depth"].tobytes() and code.cpu().numpy().tobytes() == exp["code"].tobytes()
    assert np.array_equal(stats[..., 0], exp["sampled"])
    assert (stats[..., 0] <= stats[..., 1]).all() and (stats[..., 1] <= exp["total"]).all()
    sampled, visited, total = int(stats[..., 0].sum()), int(stats[..., 1].sum()), int(exp["total"].sum())
    print(f"sampled {sampled}, visited {visited}, samples {total}")
    assert sampled == int(exp["sampled"].sum()) and visited < total


def test_summary_and_render_in_one_graph():
    """Both launches captured into one graph on preallocated tensors (no allocation, no synchronisation inside) and
    replayed once after the outputs were overwritten: the bytes of the eager calls."""
    vol = _labelled_volume()
    T = torch.as_tensor(LC.HELD_OUT).cuda()
    B, K = 4, LC.K
    want = vol.render(K, T, C.H, C.W, block=B, return_code=True, return_stats=True, labels=True)
    want_summary = vol.block_summary(B)
    summary = torch.empty_like(want_summary)
    depth, label, code, stats = (torch.empty_like(t) for t in want)
    step, max_steps = vol.truncation / 2.0, vol.max_steps(vol.truncation / 2.0)

    def run():
        L = _lib.lib()
        _lib.check(L.mf_tsdf_block_summary(_lib.ptr(vol.volume), *vol.dims, B, _lib.ptr(summary), _lib.stream_ptr()),
                   "mf_tsdf_block_summary")
        _lib.check(L.mf_tsdf_render(
            _lib.ptr(vol.volume), *vol.dims, *vol.origin, vol.pitch, step, 0.0, float("inf"), max_steps, C.H, C.W,
            float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2]), _lib.ptr(T), _lib.ptr(summary), B,
            _lib.ptr(vol.labels), 1, _lib.ptr(depth), _lib.ptr(code), _lib.ptr(label), _lib.ptr(stats),
            _lib.stream_ptr()), "mf_tsdf_render")

    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        run()
    for t in (summary, depth, label, code, stats):
        t.fill_(7)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(summary, want_summary)
    for got, exp in zip((depth, label, code, stats), want):
        assert torch.equal(got, exp)
