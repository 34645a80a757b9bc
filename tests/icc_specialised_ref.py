"""TEST INFRASTRUCTURE: the cases and checks of the specialised forms of the ICC iteration kernels (csrc/icc.hip:
k_icc_fused3<MAXNS>), shared by tests/test_emul_icc_specialised.py (CPU fiber emulator)
and tests/test_gpu_icc_specialised.py (MI355X).  The smallest scenes at which these kernels can go wrong: few points,
D = 16 unless stated, 12 iterations.

Run as a program it is the child process of the GPU test: every case once on cuda:0 under the environment it was
started with (MF_ICC_FUSED_FORM), results to the .npz named on the command line."""
import ctypes
import os
import sys

import numpy as np

N_ITER = 12
GENERIC, NS16, NS64 = 0, 1, 2      # mf_icc_debug_form: the form of the single-pass kernel
THR_1_UP = float(np.nextafter(np.float32(1), np.float32(2)))

# name -> objects per scene, points per object, D, threshold, MF_ICC_BIN_CAP, the form the plan must pick
CASES = {
    "single_object": dict(ns=(1,), pts=200, dim=16, thr=2, cap=None, form=NS16),         # no other grid: kd == 1 is dead
    "scene_of_3": dict(ns=(3,), pts=200, dim=16, thr=2, cap=None, form=NS16),
    "ragged_3_2": dict(ns=(3, 2), pts=150, dim=16, thr=2, cap=None, form=NS16),           # uniform_ns == 0
    "scene_of_16": dict(ns=(16,), pts=20, dim=16, thr=2, cap=None, form=NS16),            # the boundary of MAXNS = 16 ...
    "scene_of_17": dict(ns=(17,), pts=20, dim=16, thr=2, cap=None, form=NS64),            # ... and the other side
    "odd_dim_15": dict(ns=(3,), pts=200, dim=15, thr=2, cap=None, form=NS16),             # halves of 8 and 7 rows
    "overflow_forced": dict(ns=(3,), pts=200, dim=16, thr=2, cap="3", form=NS16),         # nearly every record overflows
    "kernel_size_5": dict(ns=(3,), pts=200, dim=16, thr=4, cap=None, form=GENERIC),       # hmax == 2: the fall-back
    # threshold 1: the host's upper bound of the kernel size is 3, every grid's real size is 1 -> the fall-back; its
    # float32 neighbour above: 1 or 3 depending on the grid's pitch -> the fall-back; 1.00001: 3 for every pitch
    "threshold_1": dict(ns=(3,), pts=200, dim=16, thr=1.0, cap=None, form=GENERIC),
    "threshold_1_next_up": dict(ns=(3,), pts=200, dim=16, thr=THR_1_UP, cap=None, form=GENERIC),
    "threshold_1_00001": dict(ns=(3,), pts=200, dim=16, thr=1.00001, cap=None, form=NS16),
}


def make_case(name):
    """-> (scene dicts with thinned point sets, q0 [O,4], t0 [O,3])"""
    import morefusion_amd.synthetic as synthetic
    from oracle import oracle_np as O
    c = CASES[name]
    scenes, q0, t0 = [], [], []
    for k, n in enumerate(c["ns"]):
        sc = synthetic.make_icc_scene(n, seed=70 + 10 * k + n, dim=c["dim"])
        pick = [np.linspace(0, len(p) - 1, c["pts"]).astype(np.int64) for p in sc["points"]]
        scenes.append(dict(points=[np.ascontiguousarray(p[i]) for p, i in zip(sc["points"], pick)],
                           sdf=[np.ascontiguousarray(s[i]) for s, i in zip(sc["sdf"], pick)],
                           pitch=sc["pitch"], origin=sc["origin"], grid_target=sc["grid_target"],
                           grid_nontarget_empty=sc["grid_nontarget_empty"]))
        q0.append(np.stack([O.quaternion_from_matrix(T) for T in sc["transform_init"]]).astype(np.float32))
        t0.append(sc["transform_init"][:, :3, 3].astype(np.float32).copy())
    return scenes, np.concatenate(q0), np.concatenate(t0)


def form_of(L, desc):
    """the form of the single-pass kernel, as the library that runs plans it (a test hook outside include/mfhip.h)"""
    return int(L.mf_icc_debug_form(ctypes.byref(desc)))


class knob_env:
    """MF_ICC_BIN_CAP of a case (and MF_ICC_FUSED_FORM, where given) in os.environ for the length of a block"""

    def __init__(self, cap, form=None):
        self.want = {"MF_ICC_BIN_CAP": cap}
        if form is not None:
            self.want["MF_ICC_FUSED_FORM"] = form

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.want}
        for k, v in self.want.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v

    def __exit__(self, *exc):
        for k, v in self.old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def oracle(name):
    """Per scene of the case: (losses [N_ITER], traj [N_ITER, n, 7]) of oracle_c.icc_refine"""
    from oracle import oracle_c as OC
    c = CASES[name]
    scenes, q0, t0 = make_case(name)
    out, lo = [], 0
    for s in scenes:
        n = len(s["points"])
        _, _, losses, traj = OC.icc_refine(s["points"], s["sdf"], s["pitch"], s["origin"], s["grid_target"],
                                           s["grid_nontarget_empty"], q0[lo:lo + n], t0[lo:lo + n], n_iter=4,
                                           voxel_dim=c["dim"], voxel_threshold=c["thr"], sdf_offset=0.02)
        out.append((losses, traj))
        lo += n
    return out


KEYS = ("q", "t", "m", "v", "losses", "traj")


def check_bitwise(a, b, what):
    for k in KEYS:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, (what, k)
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), (what, k)


def check_vs_oracle(name, got):
    """The first four losses of the free-running loop and the pose after its first step (traj[1]: one step from the
    initial state, which is also the oracle's) against oracle_c.icc_refine, with the tolerances tests/test_gpu_icc.py has
    for the same quantities (free-running losses[:4]: rtol 1e-5, atol 1e-6; the pose one step after a state shared
    with the oracle: within 1e-5)."""
    lo = 0
    for k, (losses_o, traj_o) in enumerate(oracle(name)):
        n = traj_o.shape[1]
        np.testing.assert_allclose(got["losses"][:4, k], losses_o[:4], rtol=1e-5, atol=1e-6, err_msg=name)
        assert np.abs(got["traj"][1, lo:lo + n] - traj_o[1]).max() < 1e-5, name
        lo += n
    assert np.nanmax(np.abs(got["traj"][1] - got["traj"][0])) > 1e-4   # it did move


def run_gpu(name):
    import torch

    import morefusion_amd as mf
    c = CASES[name]
    scenes, q0, t0 = make_case(name)
    with knob_env(c["cap"]):
        S = mf.contrib.IccScenes(scenes, voxel_dim=c["dim"], voxel_threshold=c["thr"], sdf_offset=0.02, device="cuda:0")
        O, ns = len(q0), len(scenes)
        q, t = torch.from_numpy(q0).cuda(), torch.from_numpy(t0).cuda()
        m, v = torch.zeros(O, 7).cuda(), torch.zeros(O, 7).cuda()
        losses, traj = torch.zeros(N_ITER, ns).cuda(), torch.zeros(N_ITER, O, 7).cuda()
        S.refine(q, t, m, v, N_ITER, step0=0, alpha_q=0.01, alpha_t=0.001, losses=losses, traj=traj)
        torch.cuda.synchronize()
        f = form_of(mf._lib.lib(), S.desc)
    out = {k: x.cpu().numpy() for k, x in zip(KEYS, (q, t, m, v, losses, traj))}
    out["form"] = np.array(f, np.int64)
    return out


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    res = {}
    for name_ in CASES:
        for k_, x_ in run_gpu(name_).items():
            res[f"{name_}/{k_}"] = x_
    np.savez(sys.argv[1], **res)
