"""Restatements of open3d's point-to-point ICP (morefusion/contrib/icp_registration.py) for the tests.

MIRROR (voxel_down_sample, register, register_iterative): csrc/icpreg.hip's documented arithmetic in float64
scalar / elementwise NumPy operations -- the lane-strided sums and the stride-halving tree over 256 partials,
the one-sided Jacobi SVD, the 2 x 2-minor 4 x 4 inverse -- no BLAS matmul, so it is bitwise what the kernels
compute.  The nearest target is the lexicographic minimum of (d2, index) over d2 < r2: a brute-force scan gives
the same answer as the kernel's exact grid search.

INDEPENDENT (*_independent): np.linalg.svd Umeyama, brute-force NN, plain NumPy sums -- agrees with the mirror
to rounding, not bit for bit."""
import math

import numpy as np

LANES = 256
JACOBI_SWEEPS = 32
JACOBI_TOL = 1e-15
RANK_TOL = 1e-13
CONV_TOL = 1e-6


# ---- voxel_down_sample -------------------------------------------------------------------------------------------
def voxel_down_sample(points, voxel_size):
    p = np.asarray(points, np.float64).reshape(-1, 3)
    p = p[~np.isnan(p).any(axis=1)]
    if len(p) == 0:
        return np.zeros((0, 3))
    v = float(voxel_size)
    vmin = p.min(axis=0) - v * 0.5
    n = np.floor((p.max(axis=0) - vmin) / v).astype(np.int64) + 1
    idx = np.floor((p - vmin) / v).astype(np.int64)
    key = (idx[:, 0] * n[1] + idx[:, 1]) * n[2] + idx[:, 2]
    order = np.lexsort((np.arange(len(p)), key))  # by voxel, then input order
    key_s = key[order]
    first = np.r_[True, key_s[1:] != key_s[:-1]]
    starts = np.flatnonzero(first)
    counts = np.diff(np.r_[starts, len(p)])
    acc = np.zeros((len(starts), 3))
    for k in range(int(counts.max())):  # sequential per voxel, in input order
        m = counts > k
        acc[m] += p[order[starts[m] + k]]
    return acc / counts[:, None].astype(np.float64)


def voxel_down_sample_independent(points, voxel_size):
    p = np.asarray(points, np.float64).reshape(-1, 3)
    p = p[~np.isnan(p).any(axis=1)]
    vmin = p.min(axis=0) - voxel_size * 0.5
    idx = np.floor((p - vmin) / voxel_size).astype(np.int64)
    uniq, inv = np.unique(idx, axis=0, return_inverse=True)  # lexicographic rows
    acc = np.zeros((len(uniq), 3))
    np.add.at(acc, inv.reshape(-1), p)  # unbuffered, in input order
    return acc / np.bincount(inv.reshape(-1))[:, None]


# ---- 4 x 4 / 3 x 3 algebra, as csrc/icpreg.hip ----------------------------------------------------------------------
def inv4(m):
    a = [float(x) for x in np.asarray(m, np.float64).reshape(16)]
    s0 = a[0] * a[5] - a[4] * a[1]
    s1 = a[0] * a[6] - a[4] * a[2]
    s2 = a[0] * a[7] - a[4] * a[3]
    s3 = a[1] * a[6] - a[5] * a[2]
    s4 = a[1] * a[7] - a[5] * a[3]
    s5 = a[2] * a[7] - a[6] * a[3]
    c5 = a[10] * a[15] - a[14] * a[11]
    c4 = a[9] * a[15] - a[13] * a[11]
    c3 = a[9] * a[14] - a[13] * a[10]
    c2 = a[8] * a[15] - a[12] * a[11]
    c1 = a[8] * a[14] - a[12] * a[10]
    c0 = a[8] * a[13] - a[12] * a[9]
    det = s0 * c5 - s1 * c4 + s2 * c3 + s3 * c2 - s4 * c1 + s5 * c0
    d = 1.0 / det
    o = [(a[5] * c5 - a[6] * c4 + a[7] * c3) * d, (-a[1] * c5 + a[2] * c4 - a[3] * c3) * d,
         (a[13] * s5 - a[14] * s4 + a[15] * s3) * d, (-a[9] * s5 + a[10] * s4 - a[11] * s3) * d,
         (-a[4] * c5 + a[6] * c2 - a[7] * c1) * d, (a[0] * c5 - a[2] * c2 + a[3] * c1) * d,
         (-a[12] * s5 + a[14] * s2 - a[15] * s1) * d, (a[8] * s5 - a[10] * s2 + a[11] * s1) * d,
         (a[4] * c4 - a[5] * c2 + a[7] * c0) * d, (-a[0] * c4 + a[1] * c2 - a[3] * c0) * d,
         (a[12] * s4 - a[13] * s2 + a[15] * s0) * d, (-a[8] * s4 + a[9] * s2 - a[11] * s0) * d,
         (-a[4] * c3 + a[5] * c1 - a[6] * c0) * d, (a[0] * c3 - a[1] * c1 + a[2] * c0) * d,
         (-a[12] * s3 + a[13] * s1 - a[14] * s0) * d, (a[8] * s3 - a[9] * s1 + a[10] * s0) * d]
    return np.array(o).reshape(4, 4)


def mul4(a, b):
    a = np.asarray(a, np.float64).reshape(16).tolist()
    b = np.asarray(b, np.float64).reshape(16).tolist()
    return np.array([((a[4 * i] * b[j] + a[4 * i + 1] * b[4 + j]) + a[4 * i + 2] * b[8 + j]) + a[4 * i + 3] * b[12 + j]
                     for i in range(4) for j in range(4)]).reshape(4, 4)


def det3(m):
    return (m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6])) + m[2] * (m[3] * m[7] - m[4] * m[6])


def umeyama(sig, ms, mt):
    """Eigen::umeyama(no scaling) from sigma (row-major 9) and the means: one-sided Jacobi SVD."""
    a = [float(x) for x in sig]
    v = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0]
    for _ in range(JACOBI_SWEEPS):
        rotated = False
        for p, q in ((0, 1), (0, 2), (1, 2)):
            alpha = (a[p] * a[p] + a[3 + p] * a[3 + p]) + a[6 + p] * a[6 + p]
            beta = (a[q] * a[q] + a[3 + q] * a[3 + q]) + a[6 + q] * a[6 + q]
            gamma = (a[p] * a[q] + a[3 + p] * a[3 + q]) + a[6 + p] * a[6 + q]
            if not abs(gamma) > JACOBI_TOL * math.sqrt(alpha * beta):
                continue
            rotated = True
            zeta = (beta - alpha) / (2.0 * gamma)
            t = (1.0 if zeta >= 0.0 else -1.0) / (abs(zeta) + math.sqrt(1.0 + zeta * zeta))
            c = 1.0 / math.sqrt(1.0 + t * t)
            s = c * t
            for i in range(3):
                x, y = a[3 * i + p], a[3 * i + q]
                a[3 * i + p], a[3 * i + q] = c * x - s * y, s * x + c * y
                x, y = v[3 * i + p], v[3 * i + q]
                v[3 * i + p], v[3 * i + q] = c * x - s * y, s * x + c * y
        if not rotated:
            break
    sv = [math.sqrt((a[j] * a[j] + a[3 + j] * a[3 + j]) + a[6 + j] * a[6 + j]) for j in range(3)]
    o = [0, 1, 2]
    if sv[o[1]] > sv[o[0]]:
        o[0], o[1] = o[1], o[0]
    if sv[o[2]] > sv[o[1]]:
        o[1], o[2] = o[2], o[1]
    if sv[o[1]] > sv[o[0]]:
        o[0], o[1] = o[1], o[0]
    U = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0]
    V = [v[3 * i + o[k]] for i in range(3) for k in range(3)]
    smax = sv[o[0]]
    rank = 0
    if smax > 0.0:
        for k in range(3):
            if sv[o[k]] > RANK_TOL * smax:
                rank = k + 1
    for k in range(rank):
        for i in range(3):
            U[3 * i + k] = a[3 * i + o[k]] / sv[o[k]]
    if rank == 1:
        e = 0
        if abs(U[3]) < abs(U[3 * e]):
            e = 1
        if abs(U[6]) < abs(U[3 * e]):
            e = 2
        w = [(1.0 if i == e else 0.0) - U[3 * e] * U[3 * i] for i in range(3)]
        nw = math.sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2])
        for i in range(3):
            U[3 * i + 1] = w[i] / nw
    if 1 <= rank <= 2:
        U[2] = U[3] * U[7] - U[6] * U[4]
        U[5] = U[6] * U[1] - U[0] * U[7]
        U[8] = U[0] * U[4] - U[3] * U[1]
    sgn = -1.0 if det3(U) * det3(V) < 0.0 else 1.0
    upd = np.eye(4)
    for i in range(3):
        for j in range(3):
            upd[i, j] = (U[3 * i] * V[3 * j] + U[3 * i + 1] * V[3 * j + 1]) + (U[3 * i + 2] * sgn) * V[3 * j + 2]
    for i in range(3):
        upd[i, 3] = mt[i] - ((upd[i, 0] * ms[0] + upd[i, 1] * ms[1]) + upd[i, 2] * ms[2])
    return upd


# ---- the ICP loop -------------------------------------------------------------------------------------------------
def xform(m, p):
    m = np.asarray(m, np.float64)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    w = ((m[3, 0] * x + m[3, 1] * y) + m[3, 2] * z) + m[3, 3]
    return np.stack([(((m[a, 0] * x + m[a, 1] * y) + m[a, 2] * z) + m[a, 3]) / w for a in range(3)], axis=1)


def nearest(q, tgt, r2, chunk=2048):
    """(index or -1, d2) per query: lexicographic min of (d2, index) over d2 < r2, d2 = (dx^2 + dy^2) + dz^2."""
    idx = np.full(len(q), -1, np.int64)
    best = np.zeros(len(q))
    if len(tgt) == 0:
        return idx, best
    for c0 in range(0, len(q), chunk):
        d = q[c0:c0 + chunk, None, :] - tgt[None, :, :]
        d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        d2 = np.where(d2 < r2, d2, np.inf)
        j = np.argmin(d2, axis=1)  # first minimum = lowest index among equal d2
        bd = d2[np.arange(len(j)), j]
        ok = np.isfinite(bd)
        idx[c0:c0 + chunk] = np.where(ok, j, -1)
        best[c0:c0 + chunk] = np.where(ok, bd, 0.0)
    return idx, best


def lane_sum(vals):
    """[n, k] -> [k]: lane l sums rows l, l + 256, ... in order, then the stride-halving tree."""
    n, k = vals.shape
    part = np.zeros((LANES, k))
    for r0 in range(0, n, LANES):
        blk = vals[r0:r0 + LANES]
        part[:len(blk)] = part[:len(blk)] + blk
    s = LANES // 2
    while s > 0:
        part[:s] = part[:s] + part[s:2 * s]
        s //= 2
    return part[0]


class _Result:
    def __init__(self, cur, tgt, r2):
        self.corr, d2 = nearest(cur, tgt, r2)
        m = self.corr >= 0
        self.n = int(m.sum())
        tc = np.where(m[:, None], tgt[np.maximum(self.corr, 0)], 0.0)
        sums = lane_sum(np.concatenate([np.where(m, d2, 0.0)[:, None], np.where(m[:, None], cur, 0.0), tc], axis=1))
        if self.n > 0:
            inv_n = 1.0 / float(self.n)
            self.ms, self.mt = sums[1:4] * inv_n, sums[4:7] * inv_n
            self.fitness = float(self.n) / float(len(cur))
            self.rmse = math.sqrt(sums[0] / float(self.n))
        else:
            self.fitness = self.rmse = 0.0


def _update(res, cur, tgt):
    if res.n == 0:
        return np.eye(4)
    m = res.corr >= 0
    ds = np.where(m[:, None], cur - res.ms, 0.0)
    dt = np.where(m[:, None], tgt[np.maximum(res.corr, 0)] - res.mt, 0.0)
    outer = np.stack([dt[:, a] * ds[:, c] for a in range(3) for c in range(3)], axis=1)
    acc = lane_sum(np.where(m[:, None], outer, 0.0))
    inv_n = 1.0 / float(res.n)
    return umeyama([inv_n * x for x in acc], res.ms, res.mt)


def register(pcd_depth, pcd_cad, transform_init=None, iteration=100, voxel_size=0.01):
    """-> dict(transform cad -> cam, transformation depth -> cad, fitness, inlier_rmse, n_iter, history
    (transforms [iteration + 1, 4, 4], fitness, rmse), source, target)."""
    src = voxel_down_sample(pcd_depth, voxel_size)
    tgt = voxel_down_sample(pcd_cad, voxel_size)
    init = np.eye(4) if transform_init is None else np.asarray(transform_init, np.float64)
    r = 2.0 * voxel_size
    r2 = r * r
    T = inv4(init)
    cur = xform(T, src)
    res = _Result(cur, tgt, r2)
    hist = [(init, res.fitness, res.rmse)]
    it = 0
    while it < iteration:
        it += 1
        upd = _update(res, cur, tgt)
        T = mul4(upd, T)
        cur = xform(upd, cur)
        prev, res = res, _Result(cur, tgt, r2)
        hist.append((inv4(T), res.fitness, res.rmse))
        if abs(prev.fitness - res.fitness) < CONV_TOL and abs(prev.rmse - res.rmse) < CONV_TOL:
            break
    return _finish(T, inv4(T), res, it, hist, iteration, src, tgt)


def register_iterative(pcd_depth, pcd_cad, transform_init=None, iteration=100, voxel_size=0.01):
    """register_iterative's steps: per step registration_icp(init = inverse(X), max_iteration = 1)."""
    src = voxel_down_sample(pcd_depth, voxel_size)
    tgt = voxel_down_sample(pcd_cad, voxel_size)
    init = np.eye(4) if transform_init is None else np.asarray(transform_init, np.float64)
    r2 = (2.0 * voxel_size) * (2.0 * voxel_size)
    X = init
    hist = []
    T = inv4(X)
    res = None
    for it in range(1, iteration + 1):
        T = inv4(X)
        cur = xform(T, src)
        res = _Result(cur, tgt, r2)
        if it == 1:
            hist.append((init, res.fitness, res.rmse))
        upd = _update(res, cur, tgt)
        T = mul4(upd, T)
        cur = xform(upd, cur)
        res = _Result(cur, tgt, r2)
        X = inv4(T)
        hist.append((X, res.fitness, res.rmse))
    if iteration == 0:
        res = _Result(xform(T, src), tgt, r2)
        hist.append((init, res.fitness, res.rmse))
    return _finish(T, X, res, iteration, hist, iteration, src, tgt)


def _finish(T, X, res, it, hist, iteration, src, tgt):
    while len(hist) < iteration + 1:
        hist.append(hist[-1])
    return dict(transform=X, transformation=T, fitness=res.fitness, inlier_rmse=res.rmse, n_iter=it,
                history=(np.stack([h[0] for h in hist]), np.array([h[1] for h in hist]), np.array([h[2] for h in hist])),
                source=src, target=tgt)


# ---- independent restatement ---------------------------------------------------------------------------------------
def umeyama_independent(s, t):
    ms, mt = s.mean(axis=0), t.mean(axis=0)
    sig = (t - mt).T @ (s - ms) / len(s)
    U, _, Vt = np.linalg.svd(sig)
    S = np.eye(3)
    if np.linalg.det(U) * np.linalg.det(Vt) < 0:
        S[2, 2] = -1
    R = U @ S @ Vt
    out = np.eye(4)
    out[:3, :3] = R
    out[:3, 3] = mt - R @ ms
    return out


def register_independent(pcd_depth, pcd_cad, transform_init=None, iteration=100, voxel_size=0.01):
    src = voxel_down_sample_independent(pcd_depth, voxel_size)
    tgt = voxel_down_sample_independent(pcd_cad, voxel_size)
    init = np.eye(4) if transform_init is None else np.asarray(transform_init, np.float64)
    r2 = (2 * voxel_size) ** 2

    def evaluate(T):
        cur = src @ T[:3, :3].T + T[:3, 3]
        d2 = ((cur[:, None, :] - tgt[None]) ** 2).sum(-1)
        j = d2.argmin(axis=1)
        bd = d2[np.arange(len(j)), j]
        m = bd < r2
        if not m.any():
            return cur, j, m, 0.0, 0.0
        return cur, j, m, m.sum() / len(src), math.sqrt(bd[m].sum() / m.sum())

    T = np.linalg.inv(init)
    cur, j, m, fit, rmse = evaluate(T)
    it = 0
    while it < iteration:
        it += 1
        upd = umeyama_independent(cur[m], tgt[j[m]]) if m.any() else np.eye(4)
        T = upd @ T
        pf, pr = fit, rmse
        cur, j, m, fit, rmse = evaluate(T)
        if abs(pf - fit) < CONV_TOL and abs(pr - rmse) < CONV_TOL:
            break
    return dict(transform=np.linalg.inv(T), fitness=fit, inlier_rmse=rmse, n_iter=it)


# ---- fixtures ------------------------------------------------------------------------------------------------------
def fixture_inputs(path):
    """The reference's ICP driver input (check_iterative_closest_point_link.py:27-36)."""
    d = np.load(path)
    pcd_depth = np.argwhere(d["grid_target"] >= 0.5) * float(d["pitch"]) + d["origin"]
    return pcd_depth.astype(np.float64), d["pcd_cad"].astype(np.float64), d["transform_init"].astype(np.float64)
