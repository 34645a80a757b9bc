"""mf_occreg_* refusals (host-side argument checks), the Python validation of occupancy_registration_batch, its NaN
fall-back and ``active`` pass-through (through the host emulator), and the mirror's own end-to-end behaviour on the
synthetic frame the GPU tests refine.  No GPU."""
import ctypes

import numpy as np
import pytest
import torch

import morefusion_amd as mf
import occreg_cases as C
import occreg_ref as R
from host_emul import emul
from morefusion_amd.geometry.quaternion_from_matrix import quaternion_from_matrix, translation_from_matrix

needs_gxx = pytest.mark.skipif(not emul.available(), reason="g++ not available")
f32 = np.float32


def test_workspace_bytes_refuses_invalid_descriptors():
    ws = mf._lib.lib().mf_occreg_workspace_bytes
    assert ws(1, 0, 1) == 0 and ws(8, 8000, 32 ** 3) == 0       # every grid fits LDS: no workspace
    assert ws(3, 100, 33 * 32 * 32) == 4 * 3 * 33 * 32 * 32      # a distance field per object
    for bad in ((0, 10, 10), (-1, 10, 10), (65536, 10, 10), (1, -1, 10), (1, 1 << 31, 10), (1, 10, 0), (1, 10, 1 << 31)):
        assert ws(*bad) < 0, bad


class _Emul:
    def __init__(self):
        self.lib = emul.build(["occreg.hip"])

    to_dev = staticmethod(lambda a: a)
    to_np = staticmethod(lambda a: a)
    ptr = staticmethod(emul.ptr)


@pytest.fixture(scope="module")
def be():
    return _Emul()


@needs_gxx
def test_launchers_refuse_invalid_descriptors(be):
    """B <= 0, a dimension < 1, thr <= 0 or not finite, pitch <= 0, counts past int32, missing host mirrors: a
    negative code and no launch (the outputs keep their fill)."""
    objs = [C.micro_tie(), C.micro_known_answer()]

    def rc_of(mutate):
        bt = C.Batch(be, objs)
        mutate(bt)
        q, t = bt.q0.copy(), bt.t0.copy()
        loss, gq, gt = np.full(2, 7, f32), np.full((2, 4), 7, f32), np.full((2, 3), 7, f32)
        a = be.lib.mf_occreg_loss_grad(ctypes.byref(bt.desc), q.ctypes.data, t.ctypes.data, loss.ctypes.data,
                                       gq.ctypes.data, gt.ctypes.data, None, None)
        m, v = np.zeros((2, 7), f32), np.zeros((2, 7), f32)
        b = be.lib.mf_occreg_refine(ctypes.byref(bt.desc), q.ctypes.data, t.ctypes.data, m.ctypes.data, v.ctypes.data,
                                    2, 0, 0.1, 0.01, None, None, None, None)
        if a < 0:  # refused: nothing was launched, every output keeps its fill
            assert (loss == 7).all() and (gq == 7).all() and (gt == 7).all()
        if b < 0:
            assert np.array_equal(q, bt.q0) and np.array_equal(t, bt.t0) and not m.any() and not v.any()
        return a, b

    assert rc_of(lambda bt: None) == (0, 0)

    def set_host(name, index, value):
        def f(bt):
            bt.host[name].reshape(-1)[index] = value
        return f

    cases = {
        "no objects": lambda bt: setattr(bt.desc, "n_objects", 0),
        "negative objects": lambda bt: setattr(bt.desc, "n_objects", -2),
        "dimension 0": set_host("dims", 4, 0),
        "threshold 0": set_host("threshold", 1, 0.0),
        "threshold negative": set_host("threshold", 0, -1.0),
        "threshold NaN": set_host("threshold", 0, np.nan),
        "threshold inf": set_host("threshold", 0, np.inf),
        "pitch 0": set_host("pitch", 1, 0.0),
        "pitch negative": set_host("pitch", 0, -0.01),
        "pitch inf": set_host("pitch", 0, np.inf),
        "grid larger than max_voxels": lambda bt: setattr(bt.desc, "max_voxels", 100),
        "max_voxels 0": lambda bt: setattr(bt.desc, "max_voxels", 0),
        "points past the total": lambda bt: setattr(bt.desc, "n_points_total", 3),
        "decreasing offsets": set_host("pts_off", 1, 5),
        "no host mirror": lambda bt: setattr(bt.desc, "host_dims", None),
    }
    for name, mutate in cases.items():
        a, b = rc_of(mutate)
        assert a < 0 and b < 0, name
    bt = C.Batch(be, objs)
    q, t, m = bt.q0.copy(), bt.t0.copy(), np.zeros((2, 7), f32)
    args = (ctypes.byref(bt.desc), q.ctypes.data, t.ctypes.data)
    assert be.lib.mf_occreg_refine(*args, m.ctypes.data, m.ctypes.data, -1, 0, 0.1, 0.01, None, None, None, None) < 0
    assert be.lib.mf_occreg_refine(*args, None, m.ctypes.data, 1, 0, 0.1, 0.01, None, None, None, None) < 0
    assert be.lib.mf_occreg_refine(*args, m.ctypes.data, m.ctypes.data, 0, 0, 0.1, 0.01, None, None, None, None) == 0
    # a grid beyond the LDS limit without a workspace
    big = dict(C.micro_tie(), grid=np.zeros((2, 33, 32, 32), f32))
    bt = C.Batch(be, [big])
    assert be.lib.mf_occreg_loss_grad(ctypes.byref(bt.desc), q.ctypes.data, t.ctypes.data, q.ctypes.data, q.ctypes.data,
                                      q.ctypes.data, None, None) < 0


def _wrapper_args(objs):
    return dict(points_source=[o["points"] for o in objs], grids_target=[o["grid"] for o in objs],
                pitch=[float(o["pitch"]) for o in objs], origin=np.stack([o["origin"] for o in objs]),
                threshold=[float(o["thr"]) for o in objs],
                transforms_init=np.stack([C.pose_matrix(o["q"], o["t"]) for o in objs]), device="cpu")


def test_wrapper_validation_raises_before_any_launch(monkeypatch):
    monkeypatch.setattr(mf._lib, "lib", lambda: (_ for _ in ()).throw(AssertionError("reached the library")))
    batch = mf.contrib.occupancy_registration_batch
    ok = _wrapper_args([C.micro_tie(), C.micro_known_answer()])

    def bad(exc, **kw):
        with pytest.raises(exc):
            batch(**dict(ok, **kw))

    g = ok["grids_target"]
    bad(TypeError, grids_target=[g[0].astype(np.float64), g[1]])       # the link's own condition: float32
    bad(TypeError, grids_target=[g[0][:1], g[1]])                        # ... and 2 or 3 channels
    bad(TypeError, grids_target=[np.concatenate([g[0], g[0]]), g[1]])
    bad(TypeError, grids_target=[g[0][0], g[1]])                         # ... of a 3-D grid each
    bad(TypeError, grids_target="grids")
    bad(TypeError, points_source=np.zeros((2, 5, 3), f32))
    bad(ValueError, grids_target=g[:1])
    bad(ValueError, points_source=[np.zeros((4, 2), f32), np.zeros((4, 3), f32)])
    bad(ValueError, pitch=[0.01, 0.0])
    bad(ValueError, pitch=[0.01, 0.01, 0.01])
    bad(ValueError, threshold=-1.0)
    bad(ValueError, threshold=float("nan"))
    bad(ValueError, threshold=64.5)                                      # the kernel's cap, as a ValueError
    bad(ValueError, pose_init=(np.zeros((2, 3), f32), np.zeros((2, 3), f32)))
    bad(ValueError, origin=np.zeros((3, 3), f32))
    bad(ValueError, transforms_init=np.eye(4, dtype=f32))
    bad(ValueError, iteration=-1)
    bad(ValueError, active=[True])
    with pytest.raises(ValueError):
        batch([], [], pitch=1.0, origin=(0, 0, 0), threshold=1.0, transforms_init=np.zeros((0, 4, 4)), device="cpu")


@needs_gxx
def test_wrapper_nan_fallback_active_passthrough_and_history(be, monkeypatch):
    """Through the emulator: the wrapper's results equal the mirror's; an object whose points miss its grid is flagged
    and keeps transforms_init, an inactive one keeps it too; scalar / stacked arguments are broadcast."""
    emul.patch_lib(be.lib, monkeypatch)
    objs = [C.batch_objects()[i] for i in (1, 4, 5, 0)]
    kw = _wrapper_args(objs)
    T, nan, losses, traj = mf.contrib.occupancy_registration_batch(
        **kw, iteration=3, alpha=0.1, active=[True, True, False, True], return_history=True)
    assert nan.tolist() == [False, True, False, False] and losses.shape == (3, 4) and traj.shape == (4, 4, 7)
    init = torch.as_tensor(kw["transforms_init"])
    assert torch.equal(T[1], init[1]) and torch.equal(T[2], init[2])
    assert torch.isnan(losses[:, 1]).all() and not losses[:, 2].any()
    for k, b in ((0, 1), (3, 0)):
        o = C.batch_objects()[b]
        occ, unocc = C.occ_unocc(o)
        q0 = quaternion_from_matrix(kw["transforms_init"][k].astype(np.float64)).astype(f32)
        t0 = translation_from_matrix(kw["transforms_init"][k].astype(np.float64)).astype(f32)
        ref = R.refine(o["points"], occ, unocc, q0, t0, 3, pitch=o["pitch"], origin=o["origin"], threshold=o["thr"],
                       alpha_q=f32(0.1), alpha_t=f32(0.1 * 0.1))
        assert C.same_bits(losses[:, k].numpy(), ref["losses"]) and C.same_bits(traj[:, k].numpy(), ref["traj"])
        assert np.array_equal(T[k].numpy(), C.pose_matrix(ref["q"], ref["t"]))
        assert not np.array_equal(T[k].numpy(), kw["transforms_init"][k])
    # one stacked tensor, scalar pitch / threshold, one origin for all
    o = C.batch_objects()[1]
    two = dict(points_source=[o["points"], o["points"]], grids_target=torch.as_tensor(np.stack([o["grid"]] * 2)),
               pitch=float(o["pitch"]), origin=o["origin"], threshold=float(o["thr"]),
               transforms_init=np.stack([C.pose_matrix(o["q"], o["t"])] * 2), device="cpu")
    T2, nan2 = mf.contrib.occupancy_registration_batch(**two, iteration=3)
    assert torch.equal(T2[0], T[0]) and torch.equal(T2[1], T[0]) and not nan2.any()


def test_mirror_refines_the_synthetic_frame():
    """The yardstick of the GPU end-to-end tests, on the CPU: for the chosen seed the mirror's own refinement does
    not worsen ADD from an initial pose within 5 degrees / 5 mm of the truth."""
    for o in C.synthetic_frame():
        occ, unocc = C.occ_unocc(o)
        q0 = quaternion_from_matrix(o["T_init"].astype(np.float64)).astype(f32)
        t0 = translation_from_matrix(o["T_init"].astype(np.float64)).astype(f32)
        ref = R.refine(o["points"], occ, unocc, q0, t0, C.FRAME_ITERATIONS, pitch=o["pitch"], origin=o["origin"],
                       threshold=C.FRAME_THRESHOLD, alpha_q=f32(C.FRAME_ALPHA), alpha_t=f32(C.FRAME_ALPHA * 0.1))
        before = C.add_metric(o["points"], o["T_gt"], o["T_init"])
        after = C.add_metric(o["points"], o["T_gt"], C.pose_matrix(ref["q"], ref["t"]))
        print(f"ADD {before * 1000:.2f} mm -> {after * 1000:.2f} mm, loss {ref['losses'][0]:.4f} -> {ref['losses'][-1]:.4f}")
        assert np.isfinite(ref["losses"]).all() and after <= before
