"""TEST INFRASTRUCTURE: what the until-converged ICC loop (mf_icc_refine_converge) must give, derived from the FIXED
loop alone.  The yardstick is the existing ``refine``: from its ``losses`` one ``contrib.LossObserver`` per scene says
where each scene stops, its ``traj`` and one ``refine(n_iter=k)`` run per distinct ``k`` give the state a scene must
be frozen in.  Shared by tests/test_emul_icc_converge.py (kernel source on the CPU emulator) and
tests/test_gpu_icc_converge.py (the MI355X); both hand in a ``runner`` with ``refine`` / ``refine_until_converged``
over NumPy arrays."""
import numpy as np

import morefusion_amd.synthetic as synthetic
from morefusion_amd.contrib import LossObserver
from oracle import oracle_np as O

FILL = np.float32(-77.25)  # pre-fill of losses / traj: rows a frozen scene must not write still hold it


def scene_dict(sc):
    return dict(points=sc["points"], sdf=sc["sdf"], pitch=sc["pitch"], origin=sc["origin"],
                grid_target=sc["grid_target"], grid_nontarget_empty=sc["grid_nontarget_empty"])


def thinned(sc, max_points):
    """The scene with every object's point set cut to at most ``max_points`` (every k-th point)."""
    sc = dict(sc)
    step = [max(1, -(-len(p) // max_points)) for p in sc["points"]]
    sc["points"] = [p[::k].copy() for p, k in zip(sc["points"], step)]
    sc["sdf"] = [s[::k].copy() for s, k in zip(sc["sdf"], step)]
    return sc


def ragged_scenes(fixtures3, seeds=(45, 45), max_points=300, fractional=False):
    """Three scenes of 2, 3 and 1 objects: the three committed fixtures (two in the first scene, one in the second)
    plus lattice solids drawn with ``seeds`` (second scene, third scene).  ``fractional``: one no-entry grid gets
    values strictly between 0 and 1, which sends the batch down the two-kernel path (k_icc_tile -> k_icc_accum)."""
    scenes = [thinned(synthetic.make_icc_scene(2, seed=41, fixtures=fixtures3[:2]), max_points),
              thinned(synthetic.make_icc_scene(3, seed=seeds[0], fixtures=fixtures3[2:]), max_points),
              thinned(synthetic.make_icc_scene(1, seed=seeds[1]), max_points)]
    if fractional:
        rs = np.random.RandomState(0)
        g = scenes[1]["grid_nontarget_empty"].copy()
        g[0] = (g[0] * rs.uniform(0.05, 1.0, g[0].shape)).astype(np.float32)
        scenes[1]["grid_nontarget_empty"] = g
    return scenes


# The cases of the ragged batch: (max_delta_threshold, window, n_passed_threshold), chosen from the float32 losses of
# the CPU oracle's icc_refine (oracle/oracle_c.py, alpha 0.01, sdf_offset 0.02, 300 points per object) so that the
# scenes stop at different steps, all later than the earliest possible one (n_passed_threshold + 1), one scene never
# stops, and every window maximum that takes part in a decision is at least a factor 2 away from the threshold: a
# last-bit difference between the oracle's and the kernels' losses cannot move a decision.  |loss_i - loss_{i-1}|:
#   single pass, seeds (45, 45)                                             two-kernel, seeds (45, 47), fractional grid
#   scene 0: .01416 .01239 .00701 .00569 .00420 .00022 .00050 .00152        .01416 .01239 .00701 .00569 .00420 .00022 .00050 .00152 .00289 .00319
#   (scenes 1, 2: printed by `python tests/icc_converge_ref.py`)
# single pass: threshold 0.0014, window 1, 1 pass -> steps (7, max_iter, 5) at max_iter 8 and 9, margin 2.2;
# two-kernel:  threshold 0.00182, window 2, 1 pass -> steps (8, 9, max_iter) at max_iter 10 and 11, margin 2.04.
RAGGED_CASES = {
    "single_pass": dict(seeds=(45, 45), fractional=False, thr=0.0014, window=1, n_pass=1,
                        steps={8: (7, 8, 5), 9: (7, 9, 5)}),
    "two_kernel": dict(seeds=(45, 47), fractional=True, thr=0.00182, window=2, n_pass=1,
                       steps={10: (8, 9, 10), 11: (8, 9, 11)}),
}


def pose0(scenes):
    q = np.concatenate([np.stack([O.quaternion_from_matrix(T) for T in sc["transform_init"]]) for sc in scenes])
    t = np.concatenate([sc["transform_init"][:, :3, 3] for sc in scenes])
    return np.ascontiguousarray(q, np.float32), np.ascontiguousarray(t, np.float32)


def scene_offsets(scenes):
    return np.concatenate([[0], np.cumsum([len(sc["points"]) for sc in scenes])]).astype(int)


def mirror_n_steps(losses, max_delta_threshold, window, n_passed_threshold):
    """One LossObserver per scene over the fixed loop's losses [n, S] -> steps applied to each scene: the loop of the
    node, ``add`` after the step of iteration i, leave once ``validate()``."""
    n, S = losses.shape
    out = np.full(S, n, np.int32)
    for s in range(S):
        ob = LossObserver(max_delta_threshold, window, n_passed_threshold)
        for i in range(n):
            ob.add(losses[i, s])
            if ob.validate():
                out[s] = i + 1
                break
    return out


class Fixed:
    """The fixed loop's answers for one batch and start: ``refine(max_iter)`` once (losses, traj), and the final
    state of ``refine(k)`` for every k asked for, each computed once and handed out read-only."""

    def __init__(self, runner, q0, t0, max_iter, step0=0, alpha_q=0.01, alpha_t=0.001, final_cache=None):
        self.runner, self.q0, self.t0, self.max_iter = runner, q0, t0, max_iter
        self.kw = dict(step0=step0, alpha_q=alpha_q, alpha_t=alpha_t)
        self._final = final_cache if final_cache is not None else {}  # (refine(k) does not depend on max_iter)
        O_ = q0.shape[0]
        S = runner.n_scenes
        self.losses = np.zeros((max_iter, S), np.float32)
        self.traj = np.zeros((max_iter, O_, 7), np.float32)
        self._final[max_iter] = self._run(max_iter, self.losses, self.traj)
        for a in (self.losses, self.traj):
            a.setflags(write=False)

    def _run(self, k, losses=None, traj=None):
        q, t = self.q0.copy(), self.t0.copy()
        m, v = np.zeros((q.shape[0], 7), np.float32), np.zeros((q.shape[0], 7), np.float32)
        self.runner.refine(q, t, m, v, k, losses=losses, traj=traj, **self.kw)
        for a in (q, t, m, v):
            a.setflags(write=False)
        return q, t, m, v

    def final(self, k):
        if k not in self._final:
            self._final[k] = self._run(k)
        return self._final[k]


def run_converge(runner, q0, t0, max_iter, thr, window, n_pass, step0=0, alpha_q=0.01, alpha_t=0.001):
    q, t = q0.copy(), t0.copy()
    m, v = np.zeros((q.shape[0], 7), np.float32), np.zeros((q.shape[0], 7), np.float32)
    losses = np.full((max_iter, runner.n_scenes), FILL, np.float32)
    traj = np.full((max_iter, q.shape[0], 7), FILL, np.float32)
    n_steps = runner.refine_until_converged(q, t, m, v, max_iter=max_iter, step0=step0, alpha_q=alpha_q,
                                            alpha_t=alpha_t, max_delta_threshold=thr, window=window,
                                            n_passed_threshold=n_pass, losses=losses, traj=traj)
    return dict(q=q, t=t, m=m, v=v, losses=losses, traj=traj, n_steps=np.asarray(n_steps))


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def assert_converged_like_fixed(got, fixed, off, thr, window, n_pass, expect=None):
    """Everything the contract states, scene by scene, bit for bit against the fixed loop.  ``expect``: the step
    counts worked out from the CPU oracle's deltas when the case was written (a guard on the case itself)."""
    want = mirror_n_steps(fixed.losses, thr, window, n_pass)
    if expect is not None:
        np.testing.assert_array_equal(want, expect)
    np.testing.assert_array_equal(got["n_steps"], want)
    for s, k in enumerate(want):
        lo, hi = off[s], off[s + 1]
        q, t, m, v = fixed.final(int(k))
        for name, ref in (("q", q), ("t", t), ("m", m), ("v", v)):
            np.testing.assert_array_equal(bits(got[name][lo:hi]), bits(ref[lo:hi]), err_msg=f"scene {s} {name}")
        np.testing.assert_array_equal(bits(got["losses"][:k, s]), bits(fixed.losses[:k, s]))
        np.testing.assert_array_equal(bits(got["traj"][:k, lo:hi]), bits(fixed.traj[:k, lo:hi]))
        assert (got["losses"][k:, s] == FILL).all(), f"scene {s}: a loss row past its stop was written"
        assert (got["traj"][k:, lo:hi] == FILL).all(), f"scene {s}: a traj row past its stop was written"
    return want


class EmulRunner:
    """``refine`` / ``refine_until_converged`` over NumPy arrays on the emulated library (tests/host_emul)."""

    def __init__(self, lib, scenes, single_pass=None):
        import ctypes
        import emul
        self._ct, self.lib = ctypes, lib
        self.S = emul.EmulIccScenes(lib, [scene_dict(s) for s in scenes], sdf_offset=0.02, single_pass=single_pass)
        self.n_scenes = self.S.n_scenes
        self.refine = self.S.refine
        self.observer = np.zeros(max(lib.mf_icc_observer_bytes(self.n_scenes, 16), 8) // 8, np.float64)

    def converge_rc(self, q, t, m, v, max_iter, step0, alpha_q, alpha_t, thr, window, n_pass, losses, traj, n_steps,
                    observer):
        p = lambda a: None if a is None else a.ctypes.data  # noqa: E731
        return self.lib.mf_icc_refine_converge(
            self._ct.byref(self.S.desc), p(q), p(t), p(m), p(v), int(max_iter), int(step0), float(alpha_q),
            float(alpha_t), float(thr), int(window), int(n_pass), p(losses), p(traj), p(n_steps), p(observer),
            self.S.ws_ptr, None)

    def refine_until_converged(self, q, t, m, v, max_iter=30, step0=0, alpha_q=0.01, alpha_t=0.001,
                               max_delta_threshold=0.009, window=10, n_passed_threshold=3, losses=None, traj=None):
        n_steps = np.full(self.n_scenes, -1, np.int32)
        rc = self.converge_rc(q, t, m, v, max_iter, step0, alpha_q, alpha_t, max_delta_threshold, window,
                              n_passed_threshold, losses, traj, n_steps, self.observer)
        assert rc == 0, rc
        return n_steps


if __name__ == "__main__":  # the oracle's deltas of every case, as quoted above
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from conftest import golden
    from oracle import oracle_c as OC
    fx = [golden(f"fixture_pose_refinement_0000000{i}.npz") for i in range(3)]
    for name, case in RAGGED_CASES.items():
        for s, sc in enumerate(ragged_scenes(fx, seeds=case["seeds"], fractional=case["fractional"])):
            q0, t0 = pose0([sc])
            losses = OC.icc_refine(sc["points"], sc["sdf"], sc["pitch"], sc["origin"], sc["grid_target"],
                                   sc["grid_nontarget_empty"], q0, t0, n_iter=12, sdf_offset=0.02)[2]
            d = np.abs(np.diff(np.asarray(losses, np.float32).astype(np.float64)))
            print(name, "scene", s, np.array2string(d, precision=5, max_line_width=200))
