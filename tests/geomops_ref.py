"""TEST INFRASTRUCTURE: float64 references of the first-generation geometry kernels and an a-priori error bound per
output element -- ``k_occgrid_fwd/_bwd``, ``k_nn``, ``k_icp`` (+ the losses of ``mf_icp_refine``) in csrc/occgrid_knn.hip,
``k_tdf_fwd/_bwd``, ``k_pocc_wraw/_grids`` in csrc/tdf.hip.  Everything is NumPy in float64, computed from the float32
INPUTS; nothing is read off a kernel's output except where that output is the next kernel's input (``dmin`` and
``flat`` for the two backwards, the poses of the refinement loop).

THE BOUND, as in tests/losschain_ref.py: to first order in u = 2^-24,

    (float32 roundings on the longest path of the stated operation order) * u * (sum of |terms|)

with one rounding per correctly rounded ``+ - *``; ``sqrtf`` and the float32 divide are ASSUMED accurate to 2 ulp =
``FN`` = 4 roundings (losschain_ref.py: ROCm's table is not at hand, nobody has measured them on the device).  A bound
of 0 means equal; a NaN in the reference means the result must be NaN.

Counts (k = roundings, the letters are the code's):

voxel coordinate   q = (p - o) / pitch: the difference 1, the divide FN -> eq = (1 + FN) u |q|.
occupancy grid     a = v - q (v an integer, exact): ea = eq + u |a|.  d = sqrt((a^2 + b^2) + c^2): three roundings on d^2
                   halve to 1.5 (charged 2), sqrt FN -> bd = |ea|_2 + (2 + FN) u d.  dmin = min_p d_p: fminf selects,
                   it does not round -> the float32 minimum lies in [min_p (d_p - bd_p), d_k0 + bd_k0], k0 the float64
                   arg-min.  grid = min(max(thr - dmin, 0), 1): one more rounding on |thr - dmin|; the clamps are
                   1-Lipschitz.
occupancy backward g_d / (2 d) FN, 2 a exact, the product 1, the divide by pitch FN, d itself bd / d:
                   term = a g / (d pitch), bterm = |term| ((2 FN + 2) u + bd / d) + ea |g| / (d pitch);
                   gpoints = sum over the n selected voxels, float atomics in ANY order: (n + 0) u sum |term| on top of
                   sum bterm ("(terms + c) u sum |term|", c inside bterm).  Selected = every point whose distance equals
                   the voxel's minimum (chainer's F.min); live = the float32 decision r > 0 and max(r, 0) <= 1 on the
                   float32 dmin the forward wrote, ONE float32 subtraction and therefore reproduced exactly.
nn                 d = r - q per coordinate: e = u |d|; ssd = (dx^2 + dy^2) + dz^2:
                   pair = sum_i (2 |d_i| e_i + e_i^2) + 3 u ssd (losschain_ref.pair_bound).
icp                s' = ((R0 x + R1 y) + R2 z) + t: 4 roundings on C = sum |R_j x_j| + |t| (+ sum bR_j |x_j| where R
                   itself came from quat_to_R in float32, bR = 21 u (...) of losschain_ref.transformation_matrix);
                   d = s' - target: e = 4 u C + u |d| + (R's share).  ssd as nn.  loss = sum of matched ssd: 8 targets
                   of a workgroup in order, then one float atomic per workgroup -> depth = 8 + workgroups;
                   dR_ab = sum 2 d_a m_b (2 x exact, one product), dt_a = sum 2 d_a.  matches is a count: exact.
tdf                a = q - v: ea = eq + u |a|; n = sqrt((ax^2 + ay^2) + az^2): bn = |ea|_2 + (2 + FN) u n;
                   dist = pitch n: b = pitch bn + u dist.
tdf backward       term = a / n g: divide FN, product 1, n's bn / n: bterm = |term| ((FN + 1) u + bn / n) + ea |g| / n;
                   float atomics over the point's n voxels: n u sum |term|.
pseudo occupancy   g = 1 - tdf / trunc: divide FN, difference 1 on 1 + |tdf / trunc|; wi = w / M: FN; ws = 1 - wi: one
                   more on 1 + |wi|; the two products one more each.
"""
import numpy as np

from losschain_ref import FN, U, compare, pair_bound, transformation_matrix

RATIOS = {}     # kernel -> worst |got - ref| / bound of the checks made in this process (reporting only)

f32 = np.float32


def assert_within(got, ref, bound, what, kernel):
    """Every element of ``got`` within ``bound`` of ``ref``; prints the worst one before it asserts."""
    ok, worst, i = compare(got, ref, bound)
    RATIOS[kernel] = max(RATIOS.get(kernel, 0.0), worst if np.isfinite(worst) else np.inf)
    g, r, b = (np.asarray(a, np.float64)[i] if np.asarray(a).size else np.nan for a in (got, ref, bound))
    print(f"GEOMOPS {kernel} {what}: worst |got-ref|/bound = {worst:.3f} at {i} (got {g!r}, ref {r!r}, bound {b:.3e})")
    assert ok, (kernel, what, worst, i, float(g), float(r), float(b))
    return worst


def report():
    for k in sorted(RATIOS):
        print(f"GEOMOPS worst ratio {k}: {RATIOS[k]:.3f}")


def _f64(*arrays):
    return tuple(np.asarray(a, np.float64) for a in arrays)


def voxel_coords(points, pitch, origin):
    """-> (q [P,3], eq): the float64 voxel coordinates of float32 points and the bound of the float32 ones."""
    p, o = _f64(np.asarray(points, f32).reshape(-1, 3), np.asarray(origin, f32))
    q = (p - o) / float(f32(pitch))
    return q, (1 + FN) * U * np.abs(q)


def _voxels(dims):
    X, Y, Z = dims
    I, J, K = np.meshgrid(np.arange(X), np.arange(Y), np.arange(Z), indexing="ij")
    return np.stack([I, J, K], -1).reshape(-1, 3).astype(np.float64)


# ---- occupancy_grid_3d ---------------------------------------------------------------------------------------------------
def _occ_geometry(points, pitch, origin, dims):
    q, eq = voxel_coords(points, pitch, origin)
    a = _voxels(dims)[:, None, :] - q[None]                # [V,P,3]
    ea = eq[None] + U * np.abs(a)
    d = np.sqrt((a * a).sum(-1))
    bd = np.sqrt((ea * ea).sum(-1)) + (2 + FN) * U * d
    return a, ea, d, bd


def occgrid(points, pitch, origin, dims, threshold):
    """-> ((grid, dmin) [X,Y,Z], (bounds)).  No point: dmin = +inf, grid = 0, exact.  A NaN coordinate anywhere: every
    voxel of both is NaN (the reference's F.min is an array min, which propagates a NaN)."""
    V = int(np.prod(dims))
    thr = float(f32(threshold))
    if len(points) == 0:
        return (np.zeros(dims), np.full(dims, np.inf)), (np.zeros(dims), np.zeros(dims))
    if np.isnan(np.asarray(points)).any():
        return (np.full(dims, np.nan), np.full(dims, np.nan)), (np.zeros(dims), np.zeros(dims))
    _, _, d, bd = _occ_geometry(points, pitch, origin, dims)
    k0 = d.argmin(axis=1)
    rows = np.arange(V)
    dmin = d[rows, k0]
    bdm = np.maximum(bd[rows, k0], dmin - (d - bd).min(axis=1))
    grid = np.clip(thr - dmin, 0.0, 1.0)
    bgrid = bdm + U * np.abs(thr - dmin)
    return (grid.reshape(dims), dmin.reshape(dims)), (bgrid.reshape(dims), bdm.reshape(dims))


def occgrid_bwd(ggrid, points, pitch, origin, dims, threshold, dmin32):
    """-> (gpoints [P,3], bound): ``dmin32`` is the float32 array the forward wrote (the backward's input); the selection
    is the float64 one, which ``occ_margin`` shows to be float32's.  A selected point at distance 0 gets NaN (0 * inf, or 0 / 0 where no gradient
    passes: chainer's Sqrt.backward divides by 2 y whatever arrives)."""
    h = float(f32(pitch))
    a, ea, d, bd = _occ_geometry(points, pitch, origin, dims)
    dm = d.min(axis=1)
    sel = d == dm[:, None]
    r = f32(threshold) - np.asarray(dmin32, f32).reshape(-1)              # the kernel's float32 subtraction
    live = (r > 0) & (np.maximum(r, f32(0)) <= f32(1))
    g = np.where(live, np.asarray(ggrid, np.float64).reshape(-1), 0.0)
    use = sel & (live | (dm == 0))[:, None]
    with np.errstate(invalid="ignore", divide="ignore"):
        term = a * (g[:, None] / (d * h))[..., None]                        # 0 * (g / 0): NaN
        bterm = np.abs(term) * ((2 * FN + 2) * U + (bd / d)[..., None]) + ea * (np.abs(g)[:, None] / (d * h))[..., None]
    term = np.where(use[..., None], term, 0.0)
    bterm = np.where(use[..., None] & ~np.isnan(term), bterm, 0.0)
    n = use.sum(axis=0)
    gp = term.sum(axis=0)
    bound = bterm.sum(axis=0) + (n[:, None] * U) * np.abs(np.nan_to_num(term)).sum(axis=0)
    bound = np.where(np.isnan(gp), 0.0, bound)
    return gp, bound


def occ_margin(points, pitch, origin, dims):
    """-> (margin, tied_rows_equal): over ALL voxels, the smallest (float64 gap of a point that is not at the voxel's
    minimum to that minimum) minus (the sum of the two distance bounds) -- positive: float32 selects the same points;
    points that tie in float64 must be equal rows, which float32 ties as well."""
    _, _, d, bd = _occ_geometry(points, pitch, origin, dims)
    if d.shape[1] < 2:
        return np.inf, True
    dm = d.min(axis=1)
    sel = d == dm[:, None]
    k0 = d.argmin(axis=1)
    slack = np.where(sel, np.inf, (d - dm[:, None]) - (bd + bd[np.arange(len(d)), k0][:, None]))
    q = np.asarray(points, f32)
    tied = all((q[np.flatnonzero(s)] == q[np.flatnonzero(s)[0]]).all() for s in sel[sel.sum(axis=1) > 1])
    return float(slack.min()), tied


# ---- nn -------------------------------------------------------------------------------------------------------------------
def nn_pairs(ref, query):
    """-> (ssd [R,Q] in float64, pair bound [R,Q])."""
    r, q = _f64(ref, query)
    with np.errstate(invalid="ignore"):
        d = r[:, None, :] - q[None, :, :]
        return (d * d).sum(-1), pair_bound(d, U * np.abs(d))


def argmin_margin(ssd, pb, rows):
    """Over the columns: the smallest (gap of a candidate to the column's minimum) minus (the two pair bounds), the
    candidates whose ROW of ``rows`` equals the winner's (exact duplicates: ties by construction) left out."""
    k0 = ssd.argmin(axis=0)
    cols = np.arange(ssd.shape[1])
    same = (rows[:, None, :] == rows[k0][None, :, :]).all(-1)
    slack = np.where(same, np.inf, (ssd - ssd[k0, cols]) - (pb + pb[k0, cols]))
    return float(slack.min()) if slack.size else np.inf


# ---- ICP --------------------------------------------------------------------------------------------------------------------
def icp(source, target, Rt, thresh, bR=None):
    """One link: Rt = the 12 float32 the kernel reads (R row-major, then t), ``bR`` [3,3] the bound of R where it is itself
    a float32 result.  -> dict(out [16] = loss, matches, -, -, dR [9], dt [3]; bound [16]; margin: the smallest of (a) the
    arg-min margins, (b) |ssd - thresh| - pair bound over the targets).  The match of a target is the lowest index among
    the sources at its float64 minimum; a NaN source (or pose) is the minimum of every target (argmin propagates it),
    and NaN < thresh is false: no match, zero sums."""
    src, tgt, Rt = _f64(source, target, Rt)
    R, t = Rt[:9].reshape(3, 3), Rt[9:]
    thr = float(f32(thresh))
    out, bound = np.zeros(16), np.zeros(16)
    img = src @ R.T + t
    if np.isnan(img).any() or len(src) == 0 or len(tgt) == 0:
        return dict(out=out, bound=bound, margin=np.inf, match=np.zeros(0, np.int64))
    C = np.abs(src) @ np.abs(R).T + np.abs(t)
    eR = np.abs(src) @ bR.T if bR is not None else 0.0
    d = img[None, :, :] - tgt[:, None, :]                                  # [T,S,3]
    e = 4 * U * C[None] + U * np.abs(d) + eR
    ssd = (d * d).sum(-1)
    pb = pair_bound(d, e)
    k = ssd.argmin(axis=1)
    rows = np.arange(len(tgt))
    best = ssd[rows, k]
    keep = best < thr
    margin = min(argmin_margin(ssd.T, pb.T, np.asarray(source, f32)),
                 float((np.abs(best - thr) - pb[rows, k]).min()))
    depth = 8 + (len(tgt) + 7) // 8
    dk, ek, mk = d[rows, k][keep], e[rows, k][keep], src[k][keep]
    out[0], out[1] = best[keep].sum(), keep.sum()
    bound[0] = pb[rows, k][keep].sum() + depth * U * best[keep].sum()
    gR = 2.0 * dk[:, :, None] * mk[:, None, :]                             # [n,3,3]
    out[4:13] = gR.sum(0).reshape(9)
    bound[4:13] = ((2.0 * ek[:, :, None] * np.abs(mk[:, None, :]) + U * np.abs(gR)).sum(0)
                   + depth * U * np.abs(gR).sum(0)).reshape(9)
    out[13:16] = 2.0 * dk.sum(0)
    bound[13:16] = 2.0 * ek.sum(0) + depth * U * 2.0 * np.abs(dk).sum(0)
    return dict(out=out, bound=bound, margin=margin, match=np.where(keep, k, -1))


def pose_Rt(q, t):
    """-> (Rt [12] in float64 from the float32 pose, bR [3,3]): quat_to_R's result and bound."""
    T, b = transformation_matrix(np.asarray(q, f32)[None], np.asarray(t, f32)[None])
    return np.r_[T[0, :3, :3].reshape(9), T[0, :3, 3]], b[0, :3, :3]


# ---- truncated distance function ------------------------------------------------------------------------------------------
def _round_half_away(x):
    return np.sign(x) * np.floor(np.abs(x) + 0.5)


def tdf(points, pitch, origin, dims, truncation, ks):
    """-> (tdf [X,Y,Z], bound, dist_of(flat) -> (float64 distance of flat's point to its voxel, its bound)).  The
    candidate voxels of a point are round(q32) + the kernel offsets, q32 the FLOAT32 voxel coordinate (a discrete
    decision, made as the kernel makes it); distances in float64; a voxel no candidate reaches holds the truncation."""
    X, Y, Z = dims
    pts = np.asarray(points, f32).reshape(-1, 3)
    h32, o32 = f32(pitch), np.asarray(origin, f32)
    with np.errstate(invalid="ignore"):
        r = _round_half_away(((pts - o32) / h32).astype(np.float64))
    q, eq = voxel_coords(pts, pitch, origin)
    h = float(h32)
    trunc = float(f32(truncation))
    best = np.full(X * Y * Z, np.inf)
    bbest = np.zeros(X * Y * Z)
    ok = ~np.isnan(q).any(axis=1)
    off = np.arange(ks) - ks // 2
    for ax in off:
        for ay in off:
            for az in off:
                v = r[ok] + np.array([ax, ay, az], np.float64)
                inb = ((v >= 0) & (v < np.array([X, Y, Z]))).all(axis=1)
                a = q[ok][inb] - v[inb]
                ea = eq[ok][inb] + U * np.abs(a)
                n = np.sqrt((a * a).sum(-1))
                dist = h * n
                b = h * (np.sqrt((ea * ea).sum(-1)) + (2 + FN) * U * n) + U * dist
                lin = ((v[inb, 0] * Y + v[inb, 1]) * Z + v[inb, 2]).astype(np.int64)
                order = np.lexsort((dist, lin))
                first = np.ones(len(order), bool)
                first[1:] = lin[order][1:] != lin[order][:-1]
                w = order[first]
                better = dist[w] < best[lin[w]]
                best[lin[w][better]] = dist[w][better]
                bbest[lin[w][better]] = b[w][better]
    ref = np.minimum(best, trunc)
    bound = np.where(best < np.inf, bbest, 0.0)

    def dist_of(flat):
        flat = np.asarray(flat).reshape(-1)
        vox = _voxels(dims)
        p = np.where(flat >= 0, flat // ks ** 3, 0)
        a = q[p] - vox
        ea = eq[p] + U * np.abs(a)
        n = np.sqrt((a * a).sum(-1))
        return h * n, h * (np.sqrt((ea * ea).sum(-1)) + (2 + FN) * U * n) + U * h * n
    return ref.reshape(dims), bound.reshape(dims), best, dist_of


def tdf_bwd(gtdf, points, flat, pitch, origin, dims, ks):
    """-> (gpoints [P,3], bound): the unit vector from flat's voxel to flat's point times the voxel's cotangent, summed
    per point; a point ON its voxel's centre (n == 0) receives nothing from that voxel."""
    q, eq = voxel_coords(points, pitch, origin)
    flat = np.asarray(flat).reshape(-1)
    g = np.asarray(gtdf, np.float64).reshape(-1)
    vox = _voxels(dims)
    gp, bound, cnt, mag = np.zeros_like(q), np.zeros_like(q), np.zeros(len(q)), np.zeros_like(q)
    own = np.flatnonzero(flat >= 0)
    p = flat[own] // ks ** 3
    a = q[p] - vox[own]
    ea = eq[p] + U * np.abs(a)
    n = np.sqrt((a * a).sum(-1))
    bn = np.sqrt((ea * ea).sum(-1)) + (2 + FN) * U * n
    ok = n > 0
    p, a, ea, n, bn, gg = p[ok], a[ok], ea[ok], n[ok][:, None], bn[ok][:, None], g[own][ok][:, None]
    term = a / n * gg
    bterm = np.abs(term) * ((FN + 1) * U + bn / n) + ea * np.abs(gg) / n
    np.add.at(gp, p, term)
    np.add.at(bound, p, bterm)
    np.add.at(mag, p, np.abs(term))
    np.add.at(cnt, p, 1.0)
    return gp, bound + cnt[:, None] * U * mag


# ---- pseudo occupancy -----------------------------------------------------------------------------------------------------
def pocc(tdf32, flat, sdf, K, truncation, sdf_offset):
    """-> (grids [3,V], bound [3,V]) from the float32 tdf / flat the forward wrote.  The raw weight (sdf + offset, clamped
    at 0) is ONE float32 addition, reproduced exactly; M = its maximum; every weight 0: 0 / 0, NaN in the two weighted
    grids (the reference divides by ``weight_inside.max()`` whatever it is)."""
    t, = _f64(np.asarray(tdf32, f32).reshape(-1))
    flat = np.asarray(flat).reshape(-1)
    trunc = float(f32(truncation))
    w = np.where(flat >= 0, np.asarray(sdf, f32)[np.where(flat >= 0, flat // K, 0)], f32(-1)) + f32(sdf_offset)
    neg = w < 0
    w = np.where(neg, f32(0), w).astype(np.float64)
    M = w.max()
    with np.errstate(invalid="ignore", divide="ignore"):
        wi = w / M
    ws = np.where(neg, wi, 1.0 - wi)
    g = 1.0 - t / trunc
    bg = (FN + 1) * U * (1.0 + np.abs(t / trunc))
    bwi = FN * U * np.abs(wi)
    bws = np.where(neg, bwi, bwi + U * (1.0 + np.abs(wi)))
    grids = np.stack([g, g * ws, g * wi])
    bound = np.stack([bg, bg * np.abs(ws) + np.abs(g) * bws + U * np.abs(g * ws),
                      bg * np.abs(wi) + np.abs(g) * bwi + U * np.abs(g * wi)])
    return grids, np.where(np.isnan(grids), 0.0, bound)
