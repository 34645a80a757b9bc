"""mf_icc_refine_converge on the MI355X: refine until each scene's loss has converged, per scene, on the device,
against the FIXED loop on the same device (tests/icc_converge_ref.py: where each scene must stop and the bits it
must be frozen in come from the existing ``refine`` alone).  The CPU twin over the kernel source:
tests/test_emul_icc_converge.py."""
import ctypes

import numpy as np
import pytest
import torch

import icc_converge_ref as R
import morefusion_amd.synthetic as synthetic
from morefusion_amd import _lib
from morefusion_amd.contrib import IccScenes

pytestmark = pytest.mark.gpu


class GpuRunner:
    """``refine`` / ``refine_until_converged`` of IccScenes over NumPy arrays (copied in and out)."""

    def __init__(self, scenes, stream=None):
        self.S = IccScenes([R.scene_dict(s) for s in scenes], sdf_offset=0.02)
        self.n_scenes = self.S.n_scenes
        self.stream = stream

    def _call(self, fn, arrays, *args, losses=None, traj=None, **kw):
        dev = [torch.from_numpy(a.copy()).cuda() for a in arrays]
        dl = None if losses is None else torch.from_numpy(losses.copy()).cuda()
        dt = None if traj is None else torch.from_numpy(traj.copy()).cuda()
        if self.stream is not None:
            self.stream.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(self.stream):
                out = fn(*dev, *args, losses=dl, traj=dt, **kw)
            torch.cuda.current_stream().wait_stream(self.stream)
        else:
            out = fn(*dev, *args, losses=dl, traj=dt, **kw)
        torch.cuda.synchronize()
        for a, d in zip(arrays, dev):
            a[...] = d.cpu().numpy()
        if losses is not None:
            losses[...] = dl.cpu().numpy()
        if traj is not None:
            traj[...] = dt.cpu().numpy()
        return out

    def refine(self, q, t, m, v, n_iter, **kw):
        self._call(self.S.refine, (q, t, m, v), n_iter, **kw)

    def refine_until_converged(self, q, t, m, v, **kw):
        return self._call(self.S.refine_until_converged, (q, t, m, v), **kw).cpu().numpy()


@pytest.fixture(scope="module", params=sorted(R.RAGGED_CASES))
def ragged(request, fixtures3):
    case = R.RAGGED_CASES[request.param]
    scenes = R.ragged_scenes(fixtures3, seeds=case["seeds"], fractional=case["fractional"])
    runner = GpuRunner(scenes)
    assert runner.S.desc.grid_ne_binary == (0 if case["fractional"] else 1)
    assert _lib.lib().mf_icc_iteration_launches(ctypes.byref(runner.S.desc)) == (3 if case["fractional"] else 2)
    q0, t0 = R.pose0(scenes)
    cache = {}
    fixed = {n: R.Fixed(runner, q0, t0, n, final_cache=cache) for n in case["steps"]}
    return dict(case=case, runner=runner, q0=q0, t0=t0, off=R.scene_offsets(scenes), fixed=fixed)


@pytest.mark.parametrize("parity", [0, 1], ids=["even", "odd"])
def test_scenes_freeze_where_the_fixed_loop_says_bit_for_bit(ragged, parity):
    """The assertions of the emulator test on the device, both iteration layouts, max_iter even and odd; the even
    case runs on torch's default stream, the odd one on a side stream; each is replayed once (fresh observers)."""
    case, runner = ragged["case"], ragged["runner"]
    max_iter = [n for n in case["steps"] if n % 2 == parity][0]
    fixed = ragged["fixed"][max_iter]
    runner.stream = torch.cuda.Stream() if parity else None
    try:
        args = (runner, ragged["q0"], ragged["t0"], max_iter, case["thr"], case["window"], case["n_pass"])
        got = R.run_converge(*args)
        again = R.run_converge(*args)
    finally:
        runner.stream = None
    want = R.assert_converged_like_fixed(got, fixed, ragged["off"], case["thr"], case["window"], case["n_pass"],
                                         expect=case["steps"][max_iter])
    assert (want == max_iter).sum() >= 1 and len(set(want)) == len(want)
    for k in got:
        np.testing.assert_array_equal(got[k].view(np.uint32) if got[k].dtype == np.float32 else got[k],
                                      again[k].view(np.uint32) if again[k].dtype == np.float32 else again[k], err_msg=k)


def test_eight_scenes_in_xcd_order_freeze_at_different_steps():
    """8 scenes x 4 objects, 150 points each: 32 objects switch the XCD-contiguous workgroup order on.  Threshold
    0.0045, window 2, 2 passes, at most 12 iterations: the CPU oracle's losses put the stops at (12, 12, 9, 11, 8,
    11, 12, 11), but several of its window maxima sit within 5 % of the threshold, so the counts are NOT pinned from
    the oracle here: the mirror runs over the device's own fixed-loop losses, which are the very bits the device's
    observers see, and at least three different step counts must come out."""
    scenes = [R.thinned(synthetic.make_icc_scene(4, seed=60 + s), 150) for s in range(8)]
    runner = GpuRunner(scenes)
    plan = (ctypes.c_int64 * 15)()
    assert _lib.lib().mf_icc_plan(ctypes.byref(runner.S.desc), plan, 15) == 15 and plan[11] == 1  # xcd_order
    q0, t0 = R.pose0(scenes)
    fixed = R.Fixed(runner, q0, t0, 12)
    got = R.run_converge(runner, q0, t0, 12, 0.0045, 2, 2)
    want = R.assert_converged_like_fixed(got, fixed, R.scene_offsets(scenes), 0.0045, 2, 2)
    assert len(set(want.tolist())) >= 3 and want.min() > 3, want


def test_the_nodes_constants(ragged):
    """Threshold 0.009, window 10, 3 passes, at most 30 iterations -- the call as the node makes it -- with step0 = 5."""
    runner = ragged["runner"]
    fixed = R.Fixed(runner, ragged["q0"], ragged["t0"], 30, step0=5)
    got = R.run_converge(runner, ragged["q0"], ragged["t0"], 30, 0.009, 10, 3, step0=5)
    want = R.assert_converged_like_fixed(got, fixed, ragged["off"], 0.009, 10, 3)
    assert want.min() >= 4


def test_bad_arguments_are_refused_and_nothing_is_launched(ragged):
    S = ragged["runner"].S
    q, t = torch.from_numpy(ragged["q0"]).cuda(), torch.from_numpy(ragged["t0"]).cuda()
    m, v = torch.zeros((q.shape[0], 7), device="cuda"), torch.zeros((q.shape[0], 7), device="cuda")
    with pytest.raises(ValueError):
        S.refine_until_converged(q, t, m, v, window=17)
    n_steps = torch.full((S.n_scenes,), -1, dtype=torch.int32, device="cuda")
    rc = _lib.lib().mf_icc_refine_converge(ctypes.byref(S.desc), q.data_ptr(), t.data_ptr(), m.data_ptr(), v.data_ptr(),
                                           4, 0, 0.01, 0.001, 0.009, 10, 3, None, None, n_steps.data_ptr(), None,
                                           S.ws.data_ptr(), _lib.stream_ptr())
    assert rc < 0
    torch.cuda.synchronize()
    assert (n_steps == -1).all() and torch.equal(q.cpu(), torch.from_numpy(ragged["q0"])) and not m.any()
