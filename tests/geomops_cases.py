"""TEST INFRASTRUCTURE: the cases of the first-generation geometry kernels (csrc/occgrid_knn.hip, csrc/tdf.hip), shared by
tests/test_emul_geomops.py (kernel text on the host emulator, ``dev = "cpu"`` with ``_lib`` patched) and
tests/test_gpu_geomops.py (the MI355X, ``dev = "cuda"``).  Every check takes the device, builds torch tensors on it and
calls the C ABI through ``_lib.lib()`` and, where a wrapper reaches the branch, the wrapper as well; results are held to
the float32 mirror (oracle/oracle_np.py, oracle_c.py) bit for bit where they are discrete and to tests/geomops_ref.py
within its a-priori bounds.  Every case is seeded and built on the CPU; where a case needs a float64 margin (a unique
arg-min, a distance clear of a threshold) its constructor walks seeds until the float64 reference -- never a kernel --
shows that margin, and the check asserts it again.

Reference rules pinned here (read from the reference project):
  occupancy_grid_3d.py:82-84   F.min is an array min and relu / minimum are maximum(., 0) / minimum(., 1): one NaN point
                               makes every voxel of the grid NaN (fminf would have dropped it).
  occupancy_grid_3d.py:81-82   a point ON a voxel centre: F.min's backward hands that element the voxel's gradient,
                               Sqrt.backward divides it by 2 y = 0 and x ** 2 multiplies by 2 x = 0 -- 0 * inf, or 0 / 0
                               where relu / minimum pass nothing: the point's gradient is NaN either way.
  knn/nn.py:48, iterative_closest_point_link.py:35-38   argmin: the lowest index among equal distances; a NaN distance
                               is the minimum and the first one wins (a NaN query: index 0; a NaN reference row: that
                               row for every query).  In the ICP link ``NaN < 0.02`` is false: a NaN source row leaves
                               every target unmatched -- loss 0, no match.  (The reference's dense backward would then
                               multiply that row by zero into NaN entries of dR; the kernel sums over matches only and
                               returns zeros -- not pinned.)
  truncated_distance_function.py:72, :141   strict ``distance < truncation``; a NaN point writes nothing; a point on its
                               voxel's centre (idistance == 0) gets nothing from that voxel.
  truncated_distance_function.py:204   ``weight_inside / weight_inside.max()`` whatever the maximum: all weights
                               negative -> 0 / 0, the two weighted grids are NaN.
"""
import functools

import numpy as np
import torch

import geomops_ref as R
from morefusion_amd import _lib
from oracle import oracle_c as OC
from oracle import oracle_np as O

f32 = np.float32
SENT = f32(-12345.0)
ISENT = -7
PITCH = float(f32(0.0125))
ORIGIN = tuple(float(f32(v)) for v in (-0.05, 0.02, -0.03))

OCC_PS = (0, 1, 1023, 1024, 1025, 2049)
OCC_DIMS = ((3, 5, 17), (4, 8, 8), (257, 1, 1))
NN_RS = (1, 1023, 1024, 1025, 2049)
NN_QS = (1, 255, 256, 257)
ICP_SS = (1, 31, 32, 33, 1024, 1025)
ICP_TS = (1, 7, 8, 9, 17)
REFINE_LS = (1, 3, 64, 65)
TDF_PS = (4095, 4096, 4097, 8193)
TDF_KS = (3, 5, 7)
TDF_TILE_DIMS = ((40, 11, 9), (7, 30, 50))
POCC_DIMS = ((3, 3, 7), (4, 2, 8), (5, 13, 1), (257, 1, 1))
K_TILE, TDF_CHUNK = 1024, 4096


def T(a, dev):
    return torch.from_numpy(np.array(a)).to(dev)   # a copy: the cases' arrays are shared and read-only


def H(t):
    return t.detach().cpu().numpy()


def equal(got, want, what):
    """Bit-equal up to the payload of a NaN (the host writes 0 / 0 with the sign bit set, the device without)."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    np.testing.assert_array_equal(got, want, err_msg=what)
    if got.dtype == np.float32:
        np.testing.assert_array_equal(np.signbit(got) & ~np.isnan(got), np.signbit(want) & ~np.isnan(want), err_msg=what)


def _frozen(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


# ---- occupancy_grid_3d ---------------------------------------------------------------------------------------------------
def run_occgrid(dev, pts, pitch, origin, dims, thr, ggrid, gpoints0=None):
    L, X, Y, Z = _lib.lib(), *dims
    P = len(pts)
    p = T(np.asarray(pts, f32).reshape(-1, 3), dev)
    grid, dmin = T(np.full(dims, SENT, f32), dev), T(np.full(dims, SENT, f32), dev)
    assert L.mf_occupancy_grid_3d_fwd(p.data_ptr(), P, pitch, *origin, X, Y, Z, thr, grid.data_ptr(), dmin.data_ptr(),
                                      _lib.stream_ptr()) == 0
    gp = T(np.zeros((P, 3), f32) if gpoints0 is None else gpoints0, dev)
    gg = T(np.asarray(ggrid, f32), dev)
    assert L.mf_occupancy_grid_3d_bwd(gg.data_ptr(), p.data_ptr(), P, pitch, *origin, X, Y, Z, thr, dmin.data_ptr(),
                                      gp.data_ptr(), _lib.stream_ptr()) == 0
    return dict(grid=H(grid), dmin=H(dmin), gpoints=H(gp))


def run_occgrid_wrapper(dev, pts, pitch, origin, dims, thr, ggrid):
    """``OccupancyGrid3D`` is what ``functions.occupancy_grid_3d`` applies to a CUDA tensor (a CPU tensor would take the
    product's NumPy path, which is not a kernel)."""
    from morefusion_amd.functions.geometry.occupancy_grid_3d import OccupancyGrid3D
    p = T(np.asarray(pts, f32).reshape(-1, 3), dev).requires_grad_(True)
    grid = OccupancyGrid3D.apply(p, pitch, origin, dims, thr)
    grid.backward(T(np.asarray(ggrid, f32), dev))
    return dict(grid=H(grid), gpoints=H(p.grad))


def mirror_occgrid(pts, pitch, origin, dims, thr):
    if len(pts) == 0:
        return np.zeros(dims, f32), np.full(dims, np.inf, f32)
    with np.errstate(invalid="ignore"):
        return O.occupancy_grid_3d(np.asarray(pts, f32), pitch=pitch, origin=origin, dims=dims, threshold=thr,
                                   return_aux=True)


def check_occgrid(dev, c, tag):
    """Forward bit-equal to the mirror and within the float64 bound; backward within the bound of the float64 sum over
    the selected voxels, the selection shown to be decided (``occ_margin``)."""
    pts, dims, thr = c["points"], c["dims"], c["thr"]
    args = (pts, c["pitch"], c["origin"], dims, thr)
    got = run_occgrid(dev, *args, c["ggrid"])
    want_grid, want_dmin = mirror_occgrid(*args)
    equal(got["grid"], want_grid, f"{tag}: grid vs mirror")
    equal(got["dmin"], want_dmin, f"{tag}: dmin vs mirror")
    if len(pts):
        equal(got["grid"], OC.occupancy_grid_3d(pts, pitch=c["pitch"], origin=c["origin"], dims=dims, threshold=thr),
              f"{tag}: grid vs the C mirror")
    (g64, d64), (bg, bd) = R.occgrid(*args)
    R.assert_within(got["grid"], g64, bg, f"{tag} grid", "k_occgrid_fwd")
    if len(pts):
        R.assert_within(got["dmin"], d64, bd, f"{tag} dmin", "k_occgrid_fwd")
    if len(pts) == 0 or np.isnan(pts).any():
        return got
    margin, tied = R.occ_margin(pts, c["pitch"], c["origin"], dims)
    assert margin > 0 and tied, (tag, "the case does not decide which points are nearest", margin, tied)
    gp64, bgp = R.occgrid_bwd(c["ggrid"], *args, got["dmin"])
    R.assert_within(got["gpoints"], gp64, bgp, f"{tag} gpoints", "k_occgrid_bwd")
    w = run_occgrid_wrapper(dev, *args, c["ggrid"])
    equal(w["grid"], got["grid"], f"{tag}: wrapper grid")
    R.assert_within(w["gpoints"], gp64, bgp, f"{tag} wrapper gpoints", "k_occgrid_bwd")
    return got


@functools.lru_cache(maxsize=None)
def occ_case(P, dims):
    """Random points in and up to 3 voxels around the grid, threshold 2: voxels with r <= 0, 0 < r <= 1 and r > 1.
    P = 0, 1; 1023 / 1024 / 1025: one tile, a full tile, a second tile of one point; 2049: three tiles.  V = 255 / 256 /
    257: a partial block, a full one, a second block of one voxel; (3, 5, 17) and (257, 1, 1) exercise the Y * Z index
    decomposition."""
    for seed in range(40):
        rs = np.random.RandomState(7000 + 131 * P + dims[0] + 50 * seed)
        q = rs.uniform(-3.0, np.asarray(dims, np.float64) + 2.0, (P, 3))
        pts = (q * PITCH + np.asarray(ORIGIN)).astype(f32)
        ggrid = (rs.uniform(0.5, 1.5, dims) * rs.choice([-1.0, 1.0], dims)).astype(f32)
        if P < 2 or R.occ_margin(pts, PITCH, ORIGIN, dims)[0] > 0:
            return _frozen(dict(points=pts, pitch=PITCH, origin=ORIGIN, dims=dims, thr=2.0, ggrid=ggrid))
    raise AssertionError("no seed with a decided selection")


EXACT_THRS = (0.5, 1.0, 1.5, 2.5)


def check_occgrid_exact(dev, thr):
    """k_occgrid_bwd's edges in exactly representable numbers (pitch 1, origin 0): points 0 and 1 coincide at
    (1.5, 1, 1), nearest to voxels (1, 1, 1) and (2, 1, 1) at distance 0.5 -- both receive every term (``d == dmin``);
    point 2 sits on the centre of voxel (3, 3, 3).
      thr = 0.5: r == 0 at the two voxels, no other voxel is live for points 0 and 1 -> their gradient is exactly zero;
      thr = 1.5: r == 1 there, ``rr <= 1`` lets -g / +g through (their cotangents are +1 and -1, so x gets -2 from them);
      thr = 2.5: r == 2 > 1, nothing from them;  thr = 1.0: r == 1 at the centre voxel.
    Point 2 is NaN at every threshold: 0 * inf where the centre voxel is live (0.5, 1.0), 0 / 0 where it is not."""
    dims = (5, 5, 5)
    pts = np.array([[1.5, 1, 1], [1.5, 1, 1], [3, 3, 3]], f32)
    rs = np.random.RandomState(11)
    ggrid = (rs.uniform(0.5, 1.5, dims) * rs.choice([-1.0, 1.0], dims)).astype(f32)
    ggrid[1, 1, 1], ggrid[2, 1, 1] = 1.0, -1.0
    c = dict(points=pts, pitch=1.0, origin=(0.0, 0.0, 0.0), dims=dims, thr=thr, ggrid=ggrid)
    got = check_occgrid(dev, c, f"exact thr={thr}")
    gp = got["gpoints"]
    assert got["dmin"][1, 1, 1] == 0.5 and got["dmin"][2, 1, 1] == 0.5 and got["dmin"][3, 3, 3] == 0.0
    assert np.isnan(gp[2]).all(), gp[2]
    assert np.isfinite(gp[:2]).all()
    if thr == 0.5:
        assert (gp[:2] == 0).all(), gp[:2]
    if thr == 1.5:
        assert (gp[:2] != 0).any(axis=1).all(), gp[:2]


def check_occgrid_one_point_many_voxels(dev):
    """k_occgrid_bwd: ONE point, threshold 6 in a 12^3 grid -- the shell 5 <= d < 6 of several hundred live voxels all
    add to the same three addresses (float atomics on one address from every workgroup)."""
    dims = (12, 12, 12)
    rs = np.random.RandomState(12)
    pts = ((np.array([[5.3, 6.1, 5.7]]) * PITCH) + np.asarray(ORIGIN)).astype(f32)
    ggrid = rs.uniform(0.5, 1.5, dims).astype(f32)
    c = dict(points=pts, pitch=PITCH, origin=ORIGIN, dims=dims, thr=6.0, ggrid=ggrid)
    got = check_occgrid(dev, c, "one point")
    r = f32(6.0) - got["dmin"]
    assert ((r > 0) & (r <= 1)).sum() >= 300


def check_occgrid_nan_and_empty(dev):
    """k_occgrid_fwd with a NaN coordinate in the second tile (row 1027 of 1030): every voxel of grid and dmin is NaN,
    as an array min gives; and P = 0: grid 0, dmin +inf, the backward returns before the launch and leaves a buffer
    handed to it untouched."""
    dims = (3, 5, 17)
    c = dict(occ_case(1025, dims))
    pts = np.concatenate([c["points"], c["points"][:5]]).copy()
    pts[1027, 1] = np.nan
    c["points"] = pts
    got = check_occgrid(dev, c, "NaN point")
    assert np.isnan(got["grid"]).all() and np.isnan(got["dmin"]).all()
    e = dict(c, points=np.zeros((0, 3), f32))
    keep = np.full((4, 3), SENT, f32)
    got = run_occgrid(dev, e["points"], PITCH, ORIGIN, dims, 2.0, c["ggrid"], gpoints0=keep)
    assert (got["grid"] == 0).all() and np.isposinf(got["dmin"]).all()
    equal(got["gpoints"], keep, "P = 0: gpoints untouched")


# ---- nn -------------------------------------------------------------------------------------------------------------------
def mirror_nn(ref, query):
    with np.errstate(invalid="ignore"):
        idx = O.nn(ref, query)
        d = ref[idx] - query
        return idx, (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]


def run_nn(dev, ref, query):
    from morefusion_amd.geometry.nn import nn
    idx, dist = nn(T(ref, dev), T(query, dev), return_distance=True)
    L = _lib.lib()   # out_dist = NULL (what ``nn(ref, query)`` passes): the same indices
    r, q = T(ref, dev), T(query, dev)
    out = T(np.full(len(query), ISENT, np.int64), dev)
    assert L.mf_nn(r.data_ptr(), len(ref), q.data_ptr(), len(query), out.data_ptr(), None, _lib.stream_ptr()) == 0
    equal(H(out), H(idx), "mf_nn without out_dist")
    return H(idx), H(dist)


@functools.lru_cache(maxsize=None)
def nn_case(Rn, Q):
    """Random references; copies at (1023, 1024) -- the last row of tile 0 and the first of tile 1 -- and at (0, 2048)
    where R allows, and row 2 = row 1 (a tie inside one unrolled group of four); queries 0 .. 2 sit next to those rows
    so that the copies ARE the minimum."""
    for seed in range(40):
        rs = np.random.RandomState(9000 + 7 * Rn + Q + 1000 * seed)
        ref = rs.uniform(-0.1, 0.1, (Rn, 3)).astype(f32)
        later = []
        if Rn > 1024:
            ref[1024] = ref[1023]
            later.append(1024)
        if Rn > 2048:
            ref[2048] = ref[0]
            later.append(2048)
        if Rn > 2:
            ref[2] = ref[1]
            later.append(2)
        query = rs.uniform(-0.1, 0.1, (Q, 3)).astype(f32)
        for j, r in enumerate((min(1023, Rn - 1), 0, min(1, Rn - 1))[:Q]):
            query[(j * 97) % Q] = ref[r] + f32(1e-4)
        ssd, pb = R.nn_pairs(ref, query)
        if R.argmin_margin(ssd, pb, ref) > 0:
            return _frozen(dict(ref=ref, query=query, later=np.asarray(later, np.int64)))
    raise AssertionError("no seed with a unique nearest reference")


def check_nn(dev, Rn, Q):
    """k_nn: R = 1 / 1023 / 1024 / 1025 / 2049 (a tile of one row, a full tile, three tiles), Q = 255 / 256 / 257 (a
    partial block, a second block of one query).  Indices and out_dist bit-equal to the mirror; never the later copy of
    a tie; the chosen reference within the pair bound of the float64 minimum."""
    c = nn_case(Rn, Q)
    ref, query = c["ref"], c["query"]
    assert (Rn - 1) // K_TILE + 1 == {1: 1, 1023: 1, 1024: 1, 1025: 2, 2049: 3}[Rn]
    idx, dist = run_nn(dev, ref, query)
    want, wdist = mirror_nn(ref, query)
    equal(idx, want, "nn vs mirror")
    equal(idx, OC.nn(ref, query), "nn vs the C mirror")
    equal(dist, wdist, "out_dist vs mirror")
    assert not np.isin(idx, c["later"]).any()
    if Rn > 1024:
        assert (idx == 1023).any()
    ssd, pb = R.nn_pairs(ref, query)
    assert R.argmin_margin(ssd, pb, ref) > 0
    cols = np.arange(Q)
    k0 = ssd.argmin(axis=0)
    assert (ssd[idx, cols] - ssd[k0, cols] <= pb[idx, cols] + pb[k0, cols]).all()
    R.assert_within(dist, ssd[idx, cols], pb[idx, cols], f"R={Rn} Q={Q} out_dist", "k_nn")


def check_nn_nan(dev):
    """k_nn, argmin's NaN rule over two tiles (R = 1030): a NaN query -> every distance NaN, the first one wins: index 0,
    distance NaN; a reference row with a NaN coordinate (row 1027, second tile) -> that row for EVERY query, whatever
    was found in the first tile."""
    c = nn_case(1025, 5)
    ref = np.concatenate([c["ref"], c["ref"][:5] + f32(0.01)])
    query = c["query"].copy()
    query[2, 0] = np.nan
    idx, dist = run_nn(dev, ref, query)
    want, wdist = mirror_nn(ref, query)
    equal(idx, want, "NaN query vs mirror")
    equal(idx, OC.nn(ref, query), "NaN query vs the C mirror")
    equal(dist, wdist, "NaN query out_dist")
    assert idx[2] == 0 and np.isnan(dist[2]) and np.isfinite(dist[[0, 1, 3, 4]]).all()
    ref = ref.copy()
    ref[1027, 2] = np.nan
    idx, dist = run_nn(dev, ref, c["query"])
    equal(idx, mirror_nn(ref, c["query"])[0], "NaN reference vs mirror")
    equal(idx, OC.nn(ref, c["query"]), "NaN reference vs the C mirror")
    assert (idx == 1027).all() and np.isnan(dist).all()


# ---- mf_icp_loss_grad ---------------------------------------------------------------------------------------------------------
def run_icp(dev, source, target, Rt, thresh):
    L = _lib.lib()
    s, t, r = T(source, dev), T(target, dev), T(np.asarray(Rt, f32), dev)
    out = T(np.zeros(16, f32), dev)
    assert L.mf_icp_loss_grad(s.data_ptr(), len(source), t.data_ptr(), len(target), r.data_ptr(), float(f32(thresh)),
                              out.data_ptr(), _lib.stream_ptr()) == 0
    return H(out)


def check_icp_out(got, ref, tag):
    R.assert_within(got, ref["out"], ref["bound"], tag, "k_icp")
    assert got[1] == ref["out"][1] and got[2] == 0 and got[3] == 0


ICP_THRESH = 2.0 ** -11


@functools.lru_cache(maxsize=None)
def icp_case(S, Tn):
    """Targets = images of random sources under the pose plus noise of about the threshold's size (2^-11, exactly
    representable): some matched, some not."""
    from morefusion_amd.synthetic import random_rotation
    for seed in range(60):
        rs = np.random.RandomState(11000 + 13 * S + Tn + 1000 * seed)
        src = rs.uniform(-0.1, 0.1, (S, 3)).astype(f32)
        Rt = np.r_[np.asarray(random_rotation(rs, 0.5), np.float64).reshape(9), rs.uniform(-0.02, 0.02, 3)].astype(f32)
        img = src.astype(np.float64) @ Rt[:9].astype(np.float64).reshape(3, 3).T + Rt[9:]
        tgt = (img[rs.randint(0, S, Tn)] + rs.normal(0, 0.012, (Tn, 3))).astype(f32)
        ref = R.icp(src, tgt, Rt, ICP_THRESH)
        n = ref["out"][1]
        if ref["margin"] > 0 and (Tn < 7 or 0 < n < Tn):
            return _frozen(dict(source=src, target=tgt, Rt=Rt))
    raise AssertionError("no seed with decided matches")


def check_icp(dev, S, Tn):
    """k_icp: S = 1 / 31 / 32 / 33 (fewer sources than slices, one per slice, a second round of one lane), 1024 / 1025 (a
    full tile, a second tile of one source); T = 1 / 7 / 8 / 9 / 17 (a partial workgroup, a full one, a second and a third
    with one live target each).  Loss, match count, dR, dt within the bounds of the float64 sums."""
    c = icp_case(S, Tn)
    ref = R.icp(c["source"], c["target"], c["Rt"], ICP_THRESH)
    assert ref["margin"] > 0
    check_icp_out(run_icp(dev, c["source"], c["target"], c["Rt"], ICP_THRESH), ref, f"S={S} T={Tn}")


IDENT = np.r_[np.eye(3).reshape(9), np.zeros(3)].astype(f32)
ICP_TIE_PAIRS = ((9, 37), (37, 41), (40, 1024 + 3), (3, 1024 + 40), (1000, 1024 + 9))


def check_icp_equidistant(dev, lo, hi):
    """k_icp's butterfly rule: sources ``lo`` < ``hi`` are DIFFERENT points at exactly the same squared distance 2^-8 from
    the target at the origin (identity pose: every product is exact), in different slices (lo % 32 != hi % 32) and, for
    hi >= 1024, in different tiles.  The loss cannot tell them apart; dR and dt are those of ``lo``."""
    assert lo % 32 != hi % 32 and lo < hi
    rs = np.random.RandomState(lo * 7 + hi)
    S = 1070
    v = rs.normal(size=(S, 3))
    src = (v / np.linalg.norm(v, axis=1, keepdims=True) * rs.uniform(0.2, 0.3, (S, 1))).astype(f32)
    src[lo], src[hi] = (0.0625, 0, 0), (0, -0.0625, 0)
    tgt = np.array([[0, 0, 0], [5, 5, 5], [-5, 5, 5]], f32)
    ref = R.icp(src, tgt, IDENT, 2.0 ** -7)
    assert ref["match"].tolist() == [lo, -1, -1] and ref["out"][0] == 2.0 ** -8
    got = run_icp(dev, src, tgt, IDENT, 2.0 ** -7)
    check_icp_out(got, ref, f"tie {lo},{hi}")
    assert got[13] == 0.125 and got[14] == 0, ("the gradient is that of the later source", got[13:16])


def check_icp_thresh_edge_and_nan(dev):
    """k_icp's ``best < thresh``: the nearest source at squared distance exactly 2^-6 is excluded at thresh = 2^-6 and
    kept at the next float above it.  A NaN source row is the minimum of every target: nothing is matched, out stays 0."""
    rs = np.random.RandomState(5)
    src = rs.uniform(0.5, 1.0, (33, 3)).astype(f32)
    src[20] = (0.125, 0, 0)
    tgt = np.zeros((1, 3), f32)
    at = f32(2.0 ** -6)
    got = run_icp(dev, src, tgt, IDENT, at)
    assert (got == 0).all(), got
    above = np.nextafter(at, f32(1))
    got = run_icp(dev, src, tgt, IDENT, above)
    ref = R.icp(src, tgt, IDENT, above)
    assert ref["out"][1] == 1 and ref["out"][0] == 2.0 ** -6
    check_icp_out(got, ref, "one float above the threshold")
    c = icp_case(33, 9)
    src = c["source"].copy()
    src[17, 1] = np.nan
    got = run_icp(dev, src, c["target"], c["Rt"], 1.0)
    assert (got == 0).all(), got
    assert (R.icp(src, c["target"], c["Rt"], 1.0)["out"] == 0).all()


# ---- mf_icp_refine ------------------------------------------------------------------------------------------------------------
REFINE_THRESH = float(f32(0.02))


@functools.lru_cache(maxsize=None)
def refine_case(L):
    """L links, S in 5 .. 40, T in 1 .. 16 (at most two workgroups per link: a sum of two float atomics onto zero does
    not depend on their order, so a link's bits are reproducible).  L > 1: link 0 has ONE target; link 1's targets are 5 m
    away, none inside the threshold."""
    from morefusion_amd.synthetic import random_rotation
    rs = np.random.RandomState(13000 + L)
    src, tgt, q, t = [], [], [], []
    for l in range(L):
        S, Tn = int(rs.randint(5, 41)), int(rs.randint(2, 17))
        if L > 1 and l == 0:
            Tn = 1
        s = rs.uniform(-0.1, 0.1, (S, 3)).astype(f32)
        Rm = np.asarray(random_rotation(rs, 0.2), np.float64)
        g = s[rs.randint(0, S, Tn)].astype(np.float64) @ Rm.T + rs.uniform(-0.01, 0.01, 3) + rs.normal(0, 0.002, (Tn, 3))
        if L > 1 and l == 1:
            g = g + 5.0
        src.append(s)
        tgt.append(g.astype(f32))
        q.append((np.array([1.0, 0, 0, 0]) + rs.normal(0, 0.05, 4)).astype(f32))
        t.append(rs.uniform(-0.01, 0.01, 3).astype(f32))
    return dict(L=L, source=src, target=tgt, q=np.stack(q), t=np.stack(t))


def run_refine(dev, c, links, n_iter, state=None, step0=0):
    """The links ``links`` of the case as one batch, ``n_iter`` iterations from ``state`` = (q, t, m, v) (default: the
    case's poses, fresh moments) -> ((q, t, m, v), losses [n_iter, len(links)])."""
    L = _lib.lib()
    n = len(links)
    src = T(np.concatenate([c["source"][l] for l in links]), dev)
    tgt = T(np.concatenate([c["target"][l] for l in links]), dev)
    so = T(np.r_[0, np.cumsum([len(c["source"][l]) for l in links])].astype(np.int32), dev)
    to = T(np.r_[0, np.cumsum([len(c["target"][l]) for l in links])].astype(np.int32), dev)
    if state is None:
        state = (c["q"][links], c["t"][links], np.zeros((n, 7), f32), np.zeros((n, 7), f32))
    q, t, m, v = (T(np.asarray(a, f32).copy(), dev) for a in state)
    losses = T(np.full((n_iter, n), SENT, f32), dev)
    ws = T(np.full(28 * n, SENT, f32), dev)
    assert L.mf_icp_refine(src.data_ptr(), so.data_ptr(), tgt.data_ptr(), to.data_ptr(), n,
                           max(len(c["target"][l]) for l in links), REFINE_THRESH, q.data_ptr(), t.data_ptr(),
                           m.data_ptr(), v.data_ptr(), n_iter, step0, 0.01, 0.001, losses.data_ptr(), ws.data_ptr(),
                           _lib.stream_ptr()) == 0
    return tuple(H(a) for a in (q, t, m, v)), H(losses)


def check_refine(dev, L):
    """mf_icp_refine, 3 iterations: grid.x covers the longest link and the workgroups past a shorter link's targets
    return early (unequal T, one link with a single target); L = 64 / 65: k_icp_step's one full 64-lane block / a second
    block of one lane.  (a) 1 + 1 + 1 and 2 + 1 iterations with step0 carried equal the one call bit for bit; (b) a link
    refined alone has the bits it has in the batch; (c) every iteration's loss within the bound of the float64 loss at
    the pose the loop itself had then; (d) the link without a match: zero loss, zero gradient -- Adam's step of a zero
    gradient from zero moments is zero, the pose stays."""
    c = refine_case(L)
    every = list(range(L))
    assert len({len(g) for g in c["target"]}) > 1 or L == 1
    final, losses = run_refine(dev, c, every, 3)
    state, poses, step_losses = None, [(c["q"], c["t"])], []
    for k in range(3):
        state, lk = run_refine(dev, c, every, 1, state, step0=k)
        poses.append(state[:2])
        step_losses.append(lk[0])
    for a, b in zip(state, final):
        equal(a, b, "1 + 1 + 1 iterations vs 3")
    equal(np.stack(step_losses), losses, "losses of 1 + 1 + 1 iterations vs 3")
    s2, l2 = run_refine(dev, c, every, 2)
    s3, l3 = run_refine(dev, c, every, 1, s2, step0=2)
    for a, b in zip(s3, final):
        equal(a, b, "2 + 1 iterations vs 3")
    equal(np.concatenate([l2, l3]), losses, "losses of 2 + 1 iterations vs 3")
    alone = every if L <= 3 else [0, 1, 2, 31, 63, L - 1]
    for l in alone:
        fa, la = run_refine(dev, c, [l], 3)
        for a, b in zip(fa, final):
            equal(a[0], b[l], f"link {l} alone vs in the batch")
        equal(la[:, 0], losses[:, l], f"link {l} alone: losses")
    for l in (every if L <= 3 else alone):
        for k in range(3):
            Rt, bR = R.pose_Rt(poses[k][0][l], poses[k][1][l])
            ref = R.icp(c["source"][l], c["target"][l], Rt, REFINE_THRESH, bR=bR)
            assert ref["margin"] > 0, (l, k, "the pose does not decide the matches", ref["margin"])
            R.assert_within(losses[k, l:l + 1], ref["out"][:1], ref["bound"][:1], f"L={L} link {l} iteration {k} loss",
                            "mf_icp_refine")
    if L > 1:
        assert (losses[:, 1] == 0).all()
        equal(final[0][1], c["q"][1], "the link without a match: quaternion")
        equal(final[1][1], c["t"][1], "the link without a match: translation")
        assert (final[2][1] == 0).all() and (final[3][1] == 0).all()
        assert (losses[:, 0] > 0).all() and (final[0][0] != c["q"][0]).any()


# ---- truncated_distance_function ------------------------------------------------------------------------------------------------
def tdf_sy(X, Y, Z):
    """The launcher's tile rule (mf_truncated_distance_function_fwd)."""
    SY = max(1, min(Y, 4096 // Z))
    while SY > 4 and X * ((Y + SY - 1) // SY) < 256:
        SY = (SY + 1) // 2
    return SY


def tdf_ks(pitch, trunc):
    ks = int(np.ceil(f32(trunc) / f32(pitch)))
    return ks + 1 if ks % 2 == 0 else ks


def run_tdf(dev, pts, pitch, origin, dims, trunc, gtdf=None, expect=0):
    L, X, Y, Z = _lib.lib(), *dims
    P = len(pts)
    p = T(np.asarray(pts, f32).reshape(-1, 3), dev)
    tdf, flat = T(np.full(dims, SENT, f32), dev), T(np.full(dims, ISENT, np.int32), dev)
    rc = L.mf_truncated_distance_function_fwd(p.data_ptr(), P, pitch, *origin, X, Y, Z, trunc, tdf.data_ptr(),
                                              flat.data_ptr(), _lib.stream_ptr())
    assert (rc == 0) == (expect == 0), rc
    out = dict(tdf=H(tdf), flat=H(flat))
    if gtdf is not None and rc == 0:
        gp, gg = T(np.zeros((P, 3), f32), dev), T(np.asarray(gtdf, f32), dev)
        assert L.mf_truncated_distance_function_bwd(gg.data_ptr(), p.data_ptr(), flat.data_ptr(), P, pitch, *origin, X, Y,
                                                    Z, trunc, gp.data_ptr(), _lib.stream_ptr()) == 0
        out["gpoints"] = H(gp)
    return out


def check_tdf(dev, c, tag, twice=False):
    """tdf and flat bit-equal to the mirror; tdf within the float64 bound; flat's point within the bound of the float64
    minimum over the voxel's candidates; the backward within the bound of the float64 sum."""
    pts, dims = c["points"], c["dims"]
    args = (pts, c["pitch"], c["origin"], dims, c["trunc"])
    ks = tdf_ks(c["pitch"], c["trunc"])
    assert ks == c["ks"]
    got = run_tdf(dev, *args, gtdf=c["gtdf"])
    want_tdf, want_flat = OC.truncated_distance_function(pts, pitch=c["pitch"], origin=c["origin"], dims=dims,
                                                         truncation=c["trunc"])
    equal(got["tdf"], want_tdf, f"{tag}: tdf vs mirror")
    equal(got["flat"], want_flat, f"{tag}: flat vs mirror")
    ref, bound, best, dist_of = R.tdf(*args, ks)
    R.assert_within(got["tdf"], ref, bound, f"{tag} tdf", "k_tdf_fwd")
    flat = got["flat"].reshape(-1)
    own = flat >= 0
    dsel, bsel = dist_of(flat)
    assert (dsel[own] - best[own] <= bsel[own] + bound.reshape(-1)[own]).all()
    assert (best[~own] + bound.reshape(-1)[~own] >= float(f32(c["trunc"]))).all()
    g64, bg = R.tdf_bwd(c["gtdf"], pts, flat, c["pitch"], c["origin"], dims, ks)
    R.assert_within(got["gpoints"], g64, bg, f"{tag} gpoints", "k_tdf_bwd")
    if twice:
        again = run_tdf(dev, *args)
        assert got["tdf"].tobytes() == again["tdf"].tobytes() and got["flat"].tobytes() == again["flat"].tobytes()
        from morefusion_amd.functions.geometry.truncated_distance_function import TruncatedDistanceFunction
        wt, wf = TruncatedDistanceFunction.apply(T(pts, dev), c["pitch"], c["origin"], dims, c["trunc"])
        equal(H(wt), got["tdf"], f"{tag}: wrapper tdf")
        equal(H(wf), got["flat"], f"{tag}: wrapper flat")
    return got


@functools.lru_cache(maxsize=None)
def tdf_case(P, ks, dims=(10, 11, 9)):
    """Half of the points inside the 3 x 3 x 3 voxel block around the grid's middle (thousands of candidates meet in 27
    LDS words), the rest up to h voxels outside every face; two NaN rows; exact copies of rows 120 .. 129 at 3000 ..
    (same chunk) and, for P > 4096, of rows 100 .. at 4096 .. (the next chunk): the lower flat id must win."""
    rs = np.random.RandomState(15000 + P + ks + dims[0])
    h = ks // 2
    pitch = float(f32(0.01))
    origin = tuple(float(f32(v)) for v in (-0.03, 0.02, -0.05))
    trunc = float(f32(ks - 0.5) * f32(pitch))
    mid = np.asarray(dims) // 2
    q = rs.uniform(-h - 0.4, np.asarray(dims, np.float64) - 1 + h + 0.4, (P, 3))
    dense = rs.rand(P) < 0.55
    q[dense] = rs.uniform(mid - 1.45, mid + 1.45, (int(dense.sum()), 3))
    pts = (q * pitch + np.asarray(origin)).astype(f32)
    later = []
    if P > 3010:
        pts[3000:3010] = pts[120:130]
        later += list(range(3000, 3010))
    if P > TDF_CHUNK:
        n = min(50, P - TDF_CHUNK)
        pts[TDF_CHUNK:TDF_CHUNK + n] = pts[100:100 + n]
        later += list(range(TDF_CHUNK, TDF_CHUNK + n))
    pts[7] = np.nan
    pts[P - 3, 1] = np.nan
    gtdf = (rs.uniform(0.5, 1.5, dims) * rs.choice([-1.0, 1.0], dims)).astype(f32)
    return _frozen(dict(points=pts, pitch=pitch, origin=origin, dims=dims, trunc=trunc, ks=ks, gtdf=gtdf,
                        later=np.asarray(later, np.int64), dense=int(dense.sum())))


def check_tdf_chunks(dev, P, ks):
    """k_tdf_fwd<3> (ks = 3) / k_tdf_fwd<0> (5, 7): P = 4095 / 4096 take the one-round path, 4097 / 8193 the chunk loop (a
    second chunk of ONE point; three chunks with one point in the last) where both passes filter every chunk again and
    s_n restarts at 0.  Run twice: the same bytes."""
    c = tdf_case(P, ks)
    assert (P > TDF_CHUNK) == (P in (4097, 8193)) and c["dense"] >= P // 2
    got = check_tdf(dev, c, f"P={P} ks={ks}", twice=True)
    winners = got["flat"][got["flat"] >= 0] // ks ** 3
    assert not np.isin(winners, c["later"]).any()
    assert (got["flat"] >= 0).sum() > 300


def check_tdf_partial_tile(dev, dims):
    """k_tdf_fwd's last y-tile with sy < SY (Y % SY != 0, SY by the launcher's rule), 600 points."""
    SY = tdf_sy(*dims)
    assert dims[1] % SY != 0 and dims[1] > SY, (dims, SY)
    check_tdf(dev, tdf_case(600, 3, dims), f"dims={dims}")


def check_tdf_edges(dev):
    """k_tdf_fwd's strict ``dist < trunc`` in exact numbers (pitch 1, origin 0, truncation 1.5, ks = 3): point 0 at
    x = 5.5 rounds to voxel 6 and reaches voxel 7 at distance exactly 1.5 -> not written (flat -1); point 1 one float
    above 15.5 reaches voxel 17 at just under 1.5 -> written.  k_tdf_bwd: point 2 sits ON voxel (2, 3, 3): nothing from
    that voxel (n == 0), finite gradient from its neighbours.  P = 0: every voxel holds the truncation, flat -1, the
    backward returns before the launch."""
    dims = (20, 8, 8)
    pts = np.array([[5.5, 5, 5], [np.nextafter(f32(15.5), f32(16)), 5, 5], [2, 3, 3]], f32)
    rs = np.random.RandomState(3)
    c = dict(points=pts, pitch=1.0, origin=(0.0, 0.0, 0.0), dims=dims, trunc=1.5, ks=3,
             gtdf=rs.uniform(0.5, 1.5, dims).astype(f32))
    got = check_tdf(dev, c, "truncation edge")
    assert got["flat"][7, 5, 5] == -1 and got["tdf"][7, 5, 5] == 1.5
    assert got["flat"][17, 5, 5] // 27 == 1 and got["tdf"][17, 5, 5] < 1.5
    assert got["flat"][2, 3, 3] // 27 == 2 and got["tdf"][2, 3, 3] == 0
    assert np.isfinite(got["gpoints"]).all()
    e = run_tdf(dev, np.zeros((0, 3), f32), 1.0, (0.0, 0.0, 0.0), dims, 1.5, gtdf=c["gtdf"])
    assert (e["tdf"] == 1.5).all() and (e["flat"] == -1).all()


def check_tdf_one_point_many_voxels(dev):
    """k_tdf_bwd: ONE point owns the 343 voxels of a ks = 7 kernel: 343 float atomics per address."""
    c = dict(tdf_case(600, 7))
    c["points"] = c["points"][300:301].copy()
    c["points"][0] = (np.array([5.2, 5.4, 3.9]) * c["pitch"] + np.asarray(c["origin"])).astype(f32)
    got = check_tdf(dev, c, "one point")
    assert (got["flat"] >= 0).sum() == 343


def check_tdf_z_limit(dev):
    """The launcher's LDS-tile refusal, with buffers of those sizes: Z = 4096 runs, Z = 4097 is refused before the launch
    and writes nothing."""
    pts = np.array([[0, 0, 10.2], [0, 0, 4094.7]], f32)
    c = dict(points=pts, pitch=1.0, origin=(0.0, 0.0, 0.0), dims=(1, 1, 4096), trunc=1.5, ks=3,
             gtdf=np.ones((1, 1, 4096), f32))
    got = check_tdf(dev, c, "Z = 4096")
    assert got["flat"][0, 0, 4095] // 27 == 1
    r = run_tdf(dev, pts, 1.0, (0.0, 0.0, 0.0), (1, 1, 4097), 1.5, expect=-1)
    assert (r["tdf"] == SENT).all() and (r["flat"] == ISENT).all()


# ---- pseudo_occupancy_voxelization -----------------------------------------------------------------------------------------------
def check_pocc(dev, dims, negative=False):
    """k_pocc_wraw / k_pocc_grids through ``pseudo_occupancy_voxelization``: V = 63 / 64 / 65 / 257 (a partial wave, a
    full one, a second wave of one lane, a second block of one lane).  One point per voxel (threshold 1: ks = 1), ids
    shuffled, a few voxels without a point; the largest weight belongs to the LAST voxel -- the last, partial wave's
    wave_max.  ``negative``: every weight below 0 -> maximum 0, the weighted grids are 0 / 0 = NaN."""
    from morefusion_amd.functions.geometry.truncated_distance_function import pseudo_occupancy_voxelization
    V = int(np.prod(dims))
    rs = np.random.RandomState(17000 + V)
    vox = R._voxels(dims)
    q = vox + rs.uniform(-0.3, 0.3, vox.shape)
    keep = np.ones(V, bool)
    keep[rs.choice(V - 1, max(V // 10, 1), replace=False)] = False
    order = rs.permutation(int(keep.sum()))
    pts = (q[keep][order] * PITCH + np.asarray(ORIGIN)).astype(f32)
    sdf = rs.uniform(-0.01, 0.05, len(pts)).astype(f32)
    last = int(np.flatnonzero(order == keep.sum() - 1)[0])
    sdf[last] = 0.08
    if negative:
        sdf = -np.abs(sdf) - f32(0.001)
    off = 0.005 if not negative else 0.0
    kw = dict(pitch=PITCH, origin=ORIGIN, dims=dims, threshold=1, sdf_offset=off)
    grids = np.stack([H(g) for g in pseudo_occupancy_voxelization(T(pts, dev), T(sdf, dev), **kw)])
    with np.errstate(invalid="ignore", divide="ignore"):
        want, aux = O.pseudo_occupancy_voxelization(pts, sdf, return_aux=True, **kw)
    for k in range(3):
        equal(grids[k], want[k], f"pocc grid {k} vs mirror")
    assert aux["ksize"] == 1
    t = run_tdf(dev, pts, PITCH, ORIGIN, dims, float(aux["trunc"]))
    assert t["flat"].reshape(-1)[-1] == last
    if negative:
        assert np.isnan(grids[1:]).all() and np.isfinite(grids[0]).all()
    else:
        w = np.where(aux["pidx"] >= 0, sdf[np.maximum(aux["pidx"], 0)], -1).reshape(-1)
        assert int(np.argmax(w)) == V - 1
    g64, b = R.pocc(t["tdf"], t["flat"], sdf, 1, float(aux["trunc"]), off)
    R.assert_within(grids.reshape(3, -1), g64, b, f"dims={dims} grids", "k_pocc")
