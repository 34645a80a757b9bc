"""Shapes and checks shared by tests/test_emul_occreg.py (host emulator) and tests/test_gpu_occreg.py (MI355X):
csrc/occreg.hip against its NumPy mirror tests/occreg_ref.py, bit for bit."""
import ctypes
import functools
import os

import numpy as np

import occreg_ref as R
from morefusion_amd import _lib

f32 = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ALPHA_Q, ALPHA_T = f32(0.1), f32(0.01)


def _object(rs, P, dims, thr, channels, outside=0.0, all_outside=False, pitch=0.01):
    dims = np.asarray(dims)
    origin = (-0.5 * pitch * dims).astype(f32) + rs.uniform(-0.001, 0.001, 3).astype(f32)
    vox = rs.uniform(0.5, dims - 1.5, (P, 3))
    n_out = int(round(outside * P))
    if n_out:
        vox[:n_out] += (dims + 4.0) * rs.choice([-1.0, 1.0], (n_out, 3))
    if all_outside:
        vox += dims + 10.0
    points = (origin + pitch * vox).astype(f32)
    grid = rs.uniform(0, 1, (channels,) + tuple(dims)).astype(f32)
    grid[0] = (grid[0] > 0.6).astype(f32)
    q = np.array([1, 0, 0, 0], f32) + rs.uniform(-0.03, 0.03, 4).astype(f32)
    t = rs.uniform(-0.3 * pitch, 0.3 * pitch, 3).astype(f32)
    # rotate about the grid centre roughly: the points are centred on the origin of the object frame
    return dict(points=points, grid=grid, pitch=f32(pitch), origin=origin, thr=f32(thr), q=q, t=t, active=True)


@functools.lru_cache(maxsize=None)
def batch_objects():
    """The issue's five objects in one call, an inactive one, and a 33 x 32 x 32 grid (distance field in the
    workspace instead of LDS); 2- and 3-channel targets."""
    rs = np.random.RandomState(7)
    objs = [
        _object(rs, 1, (5, 6, 7), 1.0, 2),
        _object(rs, 37, (16, 16, 16), 1.5, 3),
        _object(rs, 300, (16, 16, 16), 2.0, 2, outside=1 / 3),
        _object(rs, R.POINT_TILE + 3, (32, 32, 32), 2.0, 3),
        _object(rs, 20, (16, 16, 16), 2.0, 2, all_outside=True),
        _object(rs, 25, (8, 8, 8), 1.5, 2),
        _object(rs, 20, (33, 32, 32), 1.5, 3),
    ]
    objs[5]["active"] = False
    assert int(np.prod(objs[6]["grid"].shape[1:])) > R.LDS_VOXELS >= int(np.prod(objs[3]["grid"].shape[1:]))
    return tuple(objs)


FINITE = (0, 1, 2, 3, 6)   # objects with a finite loss
NAN_OBJECT, INACTIVE = 4, 5


def occ_unocc(o):
    g = o["grid"]
    return g[0], (g[1] if g.shape[0] == 2 else np.maximum(g[1], g[2]))


def micro_tie():
    """Two points equidistant from voxel (2, 2, 2) (and no other voxel within thr of only one of them matters)."""
    grid = np.zeros((2, 5, 5, 5), f32)
    grid[0, 2, 2, 2] = 1
    grid[1] = 0.25
    pts = np.array([[1.5, 2.0, 2.0], [2.5, 2.0, 2.0]], f32)
    return dict(points=pts, grid=grid, pitch=f32(1.0), origin=np.zeros(3, f32), thr=f32(0.75),
                q=np.array([1, 0, 0, 0], f32), t=np.zeros(3, f32), active=True)


def micro_known_answer():
    """The reference's own test (functions_tests/geometry_tests/test_occupancy_grid_3d.py:28-38)."""
    grid = np.zeros((2, 5, 5, 5), f32)
    grid[0, :2] = 1
    grid[1, 3:] = 1
    pts = np.array([[0, 0.05, 0.1], [3.9, 3.95, 4.0]], f32)
    return dict(points=pts, grid=grid, pitch=f32(1.0), origin=np.zeros(3, f32), thr=f32(1.0),
                q=np.array([1, 0, 0, 0], f32), t=np.zeros(3, f32), active=True)


def micro_on_centre():
    grid = np.zeros((2, 4, 4, 4), f32)
    grid[0, 1, 1, 1] = 1
    grid[1] = 0.5
    pts = np.array([[1.0, 1.0, 1.0], [2.25, 2.0, 2.0]], f32)
    return dict(points=pts, grid=grid, pitch=f32(1.0), origin=np.zeros(3, f32), thr=f32(1.0),
                q=np.array([1, 0, 0, 0], f32), t=np.zeros(3, f32), active=True)


def same_bits(a, b):
    """Equal bit for bit; NaNs at equal positions (a NaN's sign and payload are not compared)."""
    a, b = np.ascontiguousarray(a, f32), np.ascontiguousarray(b, f32)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    return np.array_equal(np.where(np.isnan(a), 0, a.view(np.uint32)), np.where(np.isnan(b), 0, b.view(np.uint32)))


class Batch:
    """The descriptor of a list of objects over a backend: ``to_dev(ndarray) -> handle``, ``ptr(handle)``,
    ``to_np(handle)``; ``lib`` the bound library."""

    def __init__(self, backend, objs):
        self.be, self.objs, self.B = backend, objs, len(objs)
        pts_off, grid_off, dims = [0], [0], []
        for o in objs:
            pts_off.append(pts_off[-1] + o["points"].shape[0])
            dims.append(o["grid"].shape[1:])
            grid_off.append(grid_off[-1] + int(np.prod(dims[-1])))
        self.host = dict(
            pts_off=np.asarray(pts_off, np.int32), pitch=np.asarray([o["pitch"] for o in objs], f32),
            dims=np.asarray(dims, np.int32), threshold=np.asarray([o["thr"] for o in objs], f32))
        arrays = dict(
            points=np.concatenate([o["points"] for o in objs]).astype(f32),
            origin=np.stack([o["origin"] for o in objs]).astype(f32),
            grid_occ=np.concatenate([occ_unocc(o)[0].reshape(-1) for o in objs]),
            grid_unocc=np.concatenate([occ_unocc(o)[1].reshape(-1) for o in objs]),
            grid_off=np.asarray(grid_off, np.int32),
            active=np.asarray([o["active"] for o in objs], np.uint8), **self.host)
        self.dev = {k: backend.to_dev(np.ascontiguousarray(v)) for k, v in arrays.items()}
        self.max_vox = max(int(np.prod(d)) for d in dims)
        self.n_points = pts_off[-1]
        nbytes = backend.lib.mf_occreg_workspace_bytes(self.B, self.n_points, self.max_vox)
        assert nbytes >= 0
        self.ws = backend.to_dev(np.zeros(max(nbytes, 4), np.uint8))
        d = _lib.OccRegBatch()
        for k in ("points", "pts_off", "pitch", "origin", "dims", "threshold", "grid_occ", "grid_unocc", "grid_off",
                  "active"):
            setattr(d, k, backend.ptr(self.dev[k]))
        for k, v in self.host.items():
            setattr(d, "host_" + k, v.ctypes.data)
        d.n_objects, d.n_points_total, d.max_voxels, d.reserved = self.B, self.n_points, self.max_vox, 0
        self.desc = d
        self.q0 = np.stack([o["q"] for o in objs]).astype(f32)
        self.t0 = np.stack([o["t"] for o in objs]).astype(f32)

    def loss_grad(self, q=None, t=None):
        be = self.be
        q = be.to_dev(np.ascontiguousarray(self.q0 if q is None else q, f32))
        t = be.to_dev(np.ascontiguousarray(self.t0 if t is None else t, f32))
        loss, gq, gt = (be.to_dev(np.full(s, 7.0, f32)) for s in ((self.B,), (self.B, 4), (self.B, 3)))
        rc = be.lib.mf_occreg_loss_grad(ctypes.byref(self.desc), be.ptr(q), be.ptr(t), be.ptr(loss), be.ptr(gq),
                                        be.ptr(gt), be.ptr(self.ws), None)
        assert rc == 0, rc
        return be.to_np(loss), be.to_np(gq), be.to_np(gt)

    def refine(self, n_iter, history=True):
        be = self.be
        q, t = be.to_dev(self.q0.copy()), be.to_dev(self.t0.copy())
        m, v = be.to_dev(np.zeros((self.B, 7), f32)), be.to_dev(np.zeros((self.B, 7), f32))
        losses = be.to_dev(np.full((n_iter, self.B), 7.0, f32)) if history else None
        traj = be.to_dev(np.full((n_iter + 1, self.B, 7), 7.0, f32)) if history else None
        rc = be.lib.mf_occreg_refine(ctypes.byref(self.desc), be.ptr(q), be.ptr(t), be.ptr(m), be.ptr(v), n_iter, 0,
                                     float(ALPHA_Q), float(ALPHA_T), be.ptr(losses) if history else None,
                                     be.ptr(traj) if history else None, be.ptr(self.ws), None)
        assert rc == 0, rc
        out = dict(q=be.to_np(q), t=be.to_np(t), m=be.to_np(m), v=be.to_np(v))
        if history:
            out.update(losses=be.to_np(losses), traj=be.to_np(traj))
        return out


def mirror_loss_grad(o, q=None, t=None, aux=False):
    occ, unocc = occ_unocc(o)
    return R.loss_grad(o["points"], occ, unocc, o["q"] if q is None else q, o["t"] if t is None else t,
                       pitch=o["pitch"], origin=o["origin"], threshold=o["thr"], aux=aux)


@functools.lru_cache(maxsize=None)
def mirror_refine(index, n_iter, which="batch"):
    o = (batch_objects() if which == "batch" else long_objects())[index]
    occ, unocc = occ_unocc(o)
    return R.refine(o["points"], occ, unocc, o["q"], o["t"], n_iter, pitch=o["pitch"], origin=o["origin"],
                    threshold=o["thr"], alpha_q=ALPHA_Q, alpha_t=ALPHA_T)


def long_objects():
    return batch_objects()[:2]


# ---- the checks ---------------------------------------------------------------------------------------------------
def check_loss_grad_bitwise(be):
    objs = batch_objects()
    bt = Batch(be, objs)
    first = bt.loss_grad()
    for b, o in enumerate(objs):
        if b == INACTIVE:
            assert first[0][b] == 0 and not first[1][b].any() and not first[2][b].any()
            continue
        loss, gq, gt = mirror_loss_grad(o)
        print(f"object {b}: loss kernel {first[0][b]!r} mirror {loss!r}")
        assert same_bits(first[0][b], loss) and same_bits(first[1][b], gq) and same_bits(first[2][b], gt), b
        assert np.isnan(loss) == (b == NAN_OBJECT)
        if b != NAN_OBJECT:
            assert np.abs(gq).max() > 0 and np.abs(gt).max() > 0
    again = bt.loss_grad()
    assert all(same_bits(a, b) for a, b in zip(first, again))  # a second run: identical bits


def check_refine_bitwise(be, n_iter):
    objs = batch_objects()
    bt = Batch(be, objs)
    got = bt.refine(n_iter)
    for b, o in enumerate(objs):
        if b == INACTIVE:
            init = np.concatenate([o["q"], o["t"]])
            assert same_bits(got["traj"][:, b], np.tile(init, (n_iter + 1, 1))) and not got["losses"][:, b].any()
            assert same_bits(got["q"][b], o["q"]) and not got["m"][b].any()
            continue
        ref = mirror_refine(b, 7)
        assert same_bits(got["losses"][:, b], ref["losses"][:n_iter]), (b, got["losses"][:, b], ref["losses"][:n_iter])
        assert same_bits(got["traj"][:, b], ref["traj"][:n_iter + 1]), b
        assert same_bits(got["q"][b], ref["traj"][n_iter, :4]) and same_bits(got["t"][b], ref["traj"][n_iter, 4:])
        assert same_bits(got["m"][b], ref["m_hist"][n_iter]) and same_bits(got["v"][b], ref["v_hist"][n_iter]), b
        if b == NAN_OBJECT:  # NaN loss, zero gradient: the pose passes through
            assert np.isnan(got["losses"][:, b]).all() and same_bits(got["q"][b], o["q"])
        else:
            assert not same_bits(got["q"][b], o["q"])
    again = bt.refine(n_iter)
    assert all(same_bits(got[k], again[k]) for k in got)
    bare = bt.refine(n_iter, history=False)  # losses / traj NULL
    assert all(same_bits(got[k], bare[k]) for k in bare)


def check_refine_across_launches(be):
    """More iterations than one launch holds (MF_OCCREG_STEPS_PER_LAUNCH = 128): the state crosses launches."""
    n = 131
    bt = Batch(be, long_objects())
    got = bt.refine(n)
    for b in range(bt.B):
        ref = mirror_refine(b, n, "long")
        assert same_bits(got["losses"][:, b], ref["losses"]) and same_bits(got["traj"][:, b], ref["traj"]), b
        assert same_bits(got["m"][b], ref["m"]) and same_bits(got["v"][b], ref["v"])


def check_micro_cases(be):
    tie, known, centre = micro_tie(), micro_known_answer(), micro_on_centre()
    bt = Batch(be, [tie, known, centre])
    loss, gq, gt = bt.loss_grad()
    for b, o in enumerate((tie, known, centre)):
        ml, mgq, mgt, aux = mirror_loss_grad(o, aux=True)
        assert same_bits(loss[b], ml) and same_bits(gq[b], mgq) and same_bits(gt[b], mgt), b
        if b == 0:  # both points at distance 0.5 of voxel (2, 2, 2): both are selected, with opposite x gradients
            assert aux["n"].tolist() == [1, 1] and aux["g"][0, 0] == -aux["g"][1, 0] != 0
            assert gt[b][0] == 0 and np.isfinite(gq[b]).all()
        if b == 1:
            assert int((aux["m"] > 0).sum()) == 6 and np.isfinite(loss[b])
        if b == 2:  # a point on a voxel centre with thr <= 1: sqrt backward gives NaN, as in the reference
            assert np.isfinite(loss[b]) and np.isnan(gt[b]).all() and np.isnan(gq[b]).all()


def check_against_executed_reference(be):
    """mf_occreg_loss_grad at the pose of the reference's own executed link (golden occreg_* keys), with the
    tolerances tests/test_gpu_reference_cuda_text.py applies to the host-loop link."""
    g = dict(np.load(os.path.join(GOLDEN, "ref_cuda_link_gradients.npz"), allow_pickle=False))
    o = dict(points=g["occreg_model"].astype(f32), grid=g["occreg_grid_target"].astype(f32),
             pitch=f32(g["occreg_pitch"]), origin=np.asarray(g["occreg_origin"], f32), thr=f32(1.5),
             q=g["occreg_q"].astype(f32), t=g["occreg_t"].astype(f32), active=True)
    loss, gq, gt = Batch(be, [o]).loss_grad()
    print("loss", loss[0], "reference", float(g["occreg_loss"]))
    np.testing.assert_allclose(float(loss[0]), float(g["occreg_loss"]), rtol=2e-5, atol=2e-6)
    for got, want in ((gq[0], g["occreg_gq"]), (gt[0], g["occreg_gt"])):
        want = np.asarray(want, np.float64)
        np.testing.assert_allclose(np.asarray(got, np.float64), want, rtol=1e-3, atol=2e-4 * float(np.abs(want).max()))


# ---- a synthetic frame for the end-to-end checks ---------------------------------------------------------------
FRAME_SEED, FRAME_ITERATIONS, FRAME_ALPHA, FRAME_THRESHOLD = 2, 40, 0.01, 2.0  # (seed: see test_occreg_host.py)


@functools.lru_cache(maxsize=None)
def synthetic_frame(seed=FRAME_SEED, n=2, max_points=300):
    """n primitives with their 32^3 target / no-entry grids (synthetic.make_icc_scene); per object the surface points of
    the CAD lattice (at most ``max_points``), the true pose, and an initial pose = the truth perturbed about the
    object's centre by <= 5 degrees and <= 5 mm."""
    from morefusion_amd import synthetic
    sc = synthetic.make_icc_scene(n, seed=seed)
    rs = np.random.RandomState(seed + 100)
    objs = []
    for b in range(n):
        pitch = float(sc["pitch"][b])
        surf = sc["points"][b][sc["sdf"][b] < 1.2 * pitch]
        pts = surf[np.sort(rs.permutation(len(surf))[:max_points])].astype(f32)
        T_gt = sc["transform_gt"][b].astype(np.float64)
        dT = np.eye(4)
        dT[:3, :3] = synthetic.random_rotation(rs, np.deg2rad(5))
        shift = rs.normal(size=3)
        dT[:3, 3] = shift / np.linalg.norm(shift) * rs.uniform(0, 0.005)
        Cn = np.eye(4)
        Cn[:3, 3] = T_gt[:3, 3]
        T_init = Cn @ dT @ np.linalg.inv(Cn) @ T_gt
        objs.append(dict(points=pts, grid=np.stack([sc["grid_target"][b], sc["grid_nontarget_empty"][b]]).astype(f32),
                         pitch=f32(pitch), origin=sc["origin"][b].astype(f32), T_gt=T_gt.astype(f32),
                         T_init=T_init.astype(f32), class_id=int(sc["class_id"][b])))
    return tuple(objs)


def add_metric(points, T1, T2):
    p = np.asarray(points, np.float64)
    T1, T2 = np.asarray(T1, np.float64), np.asarray(T2, np.float64)
    return float(np.linalg.norm((p @ T1[:3, :3].T + T1[:3, 3]) - (p @ T2[:3, :3].T + T2[:3, 3]), axis=1).mean())


def pose_matrix(q, t):
    T = np.eye(4, dtype=f32)
    T[:3, :3] = R.quat_to_R(q).reshape(3, 3)
    T[:3, 3] = t
    return T
