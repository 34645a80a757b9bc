"""NumPy mirror of csrc/occreg.hip (TEST INFRASTRUCTURE): the arithmetic of OccupancyRegistration in float32 with the
kernel's exact orders, so that kernel results can be compared bit for bit.

Orders (the header of csrc/occreg.hip):
  * a point's window is [floor(pf - thr), ceil(pf + thr)] per axis, clamped to the grid;
  * dmin = min over the points whose window holds the voxel of d = sqrt((a a + b b) + c c) where d < thr (else +inf);
  * sums over voxels / points: float64 sums of the float32 terms (products formed in float64: exact); lane k of 256
    adds elements k, k + 256, ... in order, then the 256 partials are folded by a stride-halving tree; the loss and
    the scalars of the gradient are evaluated in float64 from those sums and rounded once;
  * a point's gradient: its window in (i, j, k) lexicographic order, the sum divided by pitch once.
"""
import math

import numpy as np

f32 = np.float32
LANES = 256
POINT_TILE = 1024     # MF_OCCREG_POINT_TILE
LDS_VOXELS = 32768    # MF_OCCREG_LDS_VOXELS


def quat_to_R(q):
    q = np.asarray(q, f32)
    n = ((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]
    s = np.sqrt(f32(2.0) / n)
    qs = q * s
    Q = np.outer(qs, qs).astype(f32)
    one = f32(1.0)
    return np.array([one - Q[2, 2] - Q[3, 3], Q[1, 2] - Q[3, 0], Q[1, 3] + Q[2, 0],
                     Q[1, 2] + Q[3, 0], one - Q[1, 1] - Q[3, 3], Q[2, 3] - Q[1, 0],
                     Q[1, 3] - Q[2, 0], Q[2, 3] + Q[1, 0], one - Q[1, 1] - Q[2, 2]], f32)


def quat_backward(q, gR):
    q = np.asarray(q, f32)
    gQ = np.zeros((4, 4), f32)
    gQ[1, 0] = -gR[5] + gR[7]
    gQ[1, 1] = -gR[4] - gR[8]
    gQ[1, 2] = gR[1] + gR[3]
    gQ[1, 3] = gR[2] + gR[6]
    gQ[2, 0] = gR[2] - gR[6]
    gQ[2, 2] = -gR[0] - gR[8]
    gQ[2, 3] = gR[5] + gR[7]
    gQ[3, 0] = -gR[1] + gR[3]
    gQ[3, 3] = -gR[0] - gR[4]
    n = ((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]
    s = np.sqrt(f32(2.0) / n)
    qs = q * s
    gqs = np.zeros(4, f32)
    for i in range(4):
        a, b = f32(0.0), f32(0.0)
        for j in range(4):
            a = a + gQ[i, j] * qs[j]
            b = b + gQ[j, i] * qs[j]
        gqs[i] = a + b
    dot = ((gqs[0] * q[0] + gqs[1] * q[1]) + gqs[2] * q[2]) + gqs[3] * q[3]
    return np.array([s * gqs[i] - (s / n) * dot * q[i] for i in range(4)], f32)


def adam_alphas(alpha_q, alpha_t, step):
    """chainer Adam's bias-corrected step sizes at step ``step`` (1-based): in double, cast once."""
    fix1 = 1.0 - math.pow(0.9, float(step))
    fix2 = 1.0 - math.pow(0.999, float(step))
    return (f32(float(f32(alpha_q)) * math.sqrt(fix2) / fix1), f32(float(f32(alpha_t)) * math.sqrt(fix2) / fix1))


def adam_pose_step(gq, gt, aq, at, q, t, m, v):
    """mf::adam_pose_step: q, t, m, v (float32 arrays) updated in place."""
    omb1, omb2, eps = f32(1.0 - 0.9), f32(1.0 - 0.999), f32(1e-8)
    for i in range(7):
        gi = gq[i] if i < 4 else gt[i - 4]
        m[i] = m[i] + omb1 * (gi - m[i])
        v[i] = v[i] + omb2 * (gi * gi - v[i])
        upd = (aq if i < 4 else at) * m[i] / (np.sqrt(v[i]) + eps)
        if i < 4:
            q[i] = q[i] - upd
        else:
            t[i - 4] = t[i - 4] - upd


def lane_tree_sum(x):
    """x [n] or [n, C] -> the kernel's float64 sum: lane k adds rows k, k + 256, ... in order, then the tree."""
    x = np.asarray(x, np.float64)
    x2 = x.reshape(x.shape[0], -1)
    n, C = x2.shape
    rows = -(-n // LANES) if n else 0
    pad = np.zeros((rows * LANES, C), np.float64)
    pad[:n] = x2
    p = np.zeros((LANES, C), np.float64)
    for r in range(rows):
        p = p + pad[r * LANES:(r + 1) * LANES]
    s = LANES // 2
    while s:
        p[:s] = p[:s] + p[s:2 * s]
        s //= 2
    return p[0] if x.ndim > 1 else p[0, 0]


def grid_coords(points, q, t, pitch, origin):
    """pf = (transform_points(points) - origin) / pitch with mf::quat_to_R: [P, 3] float32."""
    R = quat_to_R(q).reshape(3, 3)
    p = np.asarray(points, f32).reshape(-1, 3)
    t = np.asarray(t, f32)
    o = np.asarray(origin, f32)
    x, y, z = p[:, 0:1], p[:, 1:2], p[:, 2:3]
    moved = ((R[None, :, 0] * x + R[None, :, 1] * y) + R[None, :, 2] * z) + t[None]
    return ((moved - o[None]) / f32(pitch)).astype(f32)


def _windows(pf, dims, thr):
    thr = f32(thr)
    lo = np.maximum(np.floor(pf - thr), f32(0.0))
    hi = np.minimum(np.ceil(pf + thr), (np.asarray(dims, f32) - f32(1.0))[None])
    ok = (lo <= hi).all(axis=1)
    lo = np.where(ok[:, None], lo, 0).astype(np.int64)
    hi = np.where(ok[:, None], hi, -1).astype(np.int64)
    return lo, hi, ok


def _window_walk(pf, dims, thr):
    """Yields, for every window offset in lexicographic order, (in-window mask [P], flat voxel index [P], a, b, c, d)."""
    lo, hi, ok = _windows(pf, dims, thr)
    X, Y, Z = (int(d) for d in dims)
    ext = (hi - lo + 1).max(axis=0) if len(pf) else np.zeros(3, np.int64)
    for di in range(int(max(ext[0], 0))):
        i = lo[:, 0] + di
        a = i.astype(f32) - pf[:, 0]
        aa = a * a
        for dj in range(int(max(ext[1], 0))):
            j = lo[:, 1] + dj
            b = j.astype(f32) - pf[:, 1]
            ab = aa + b * b
            for dk in range(int(max(ext[2], 0))):
                k = lo[:, 2] + dk
                c = k.astype(f32) - pf[:, 2]
                d = np.sqrt(ab + c * c)
                inw = ok & (i <= hi[:, 0]) & (j <= hi[:, 1]) & (k <= hi[:, 2])
                v = np.where(inw, (i * Y + j) * Z + k, 0)
                yield inw, v, a, b, c, d


def distance_field(pf, dims, thr):
    """dmin [X Y Z] float32 of the pruned scatter: +inf where no point is within thr."""
    V = int(np.prod(dims))
    dmin = np.full(V, np.inf, f32)
    for inw, v, _, _, _, d in _window_walk(pf, dims, thr):
        sel = inw & (d < f32(thr))
        np.minimum.at(dmin, v[sel], d[sel])
    return dmin


def soft_grid(dmin, thr):
    with np.errstate(invalid="ignore"):
        m = f32(thr) - dmin
    m = np.where(m > 0, m, f32(0.0))
    return np.where(m < 1, m, f32(1.0)).astype(f32)


def loss_grad(points, occ, unocc, q, t, *, pitch, origin, threshold, aux=False):
    """One object: (loss, gq [4], gt [3]) as csrc/occreg.hip computes them.  ``aux``: also a dict with m, the
    per-point gradient g [P, 3], the number of selecting voxels n [P] and the sum of |term| per component [P, 3]."""
    points = np.asarray(points, f32).reshape(-1, 3)
    dims = occ.shape
    occ = np.ascontiguousarray(occ, f32).reshape(-1)
    unocc = np.ascontiguousarray(unocc, f32).reshape(-1)
    thr, pitch = f32(threshold), f32(pitch)
    pf = grid_coords(points, q, t, pitch, origin)
    dmin = distance_field(pf, dims, thr)
    m = soft_grid(dmin, thr)
    live = m > 0
    m64 = m.astype(np.float64)
    A = lane_tree_sum(np.where(live, unocc.astype(np.float64) * m64, 0.0))
    Sm = lane_tree_sum(m64)
    Bq = lane_tree_sum(np.where(live, occ.astype(np.float64) * m64, 0.0))
    So = lane_tree_sum(occ)
    with np.errstate(all="ignore"):
        pen = A / Sm
        loss = f32(pen - Bq / So)
        iSm, c2, iSo = f32(1.0 / Sm), f32(pen / Sm), f32(1.0 / So)
        P = points.shape[0]
        g = np.zeros((P, 3), f32)
        n_sel = np.zeros(P, np.int64)
        absum = np.zeros((P, 3), np.float64)
        terms = []  # (selection, g_d, a, b, c, d) in window order, for the float64 evaluation
        for inw, v, a, b, c, d in _window_walk(pf, dims, thr):
            dm = dmin[v]
            r = thr - dm
            g_d = -((unocc[v] * iSm - c2) - occ[v] * iSo)
            sel = inw & (r > 0) & (r <= 1) & (d == dm) & (g_d != 0)
            if not sel.any():
                continue
            g_dd = g_d / (f32(2.0) * d)
            for ax, comp in enumerate((a, b, c)):
                term = -(f32(2.0) * comp * g_dd)
                g[:, ax] = g[:, ax] + np.where(sel, term, f32(0.0))
                absum[:, ax] += np.where(sel, np.abs(term.astype(np.float64)), 0.0)
            n_sel += sel
            if aux:
                terms.append((sel, g_d, a, b, c, d))
        g = (g / pitch).astype(f32)
        g64, p64 = g.astype(np.float64), points.astype(np.float64)
        contrib = np.concatenate([(g64[:, :, None] * p64[:, None, :]).reshape(P, 9), g64], axis=1)
        red = (lane_tree_sum(contrib) if P else np.zeros(12)).astype(f32)
        gq = quat_backward(q, red[:9])
        gt = red[9:12].copy()
    if aux:
        return loss, gq, gt, dict(m=m.reshape(dims), g=g, n=n_sel, absum=absum / float(pitch), terms=terms, pf=pf,
                                  sums=(A, Sm, Bq, So))
    return loss, gq, gt


def point_gradients_f64(aux, pitch):
    """The same formula as the mirror's per-point gradient -- the same selected voxels, g_d and offsets -- summed in
    float64: [P, 3]."""
    P = aux["g"].shape[0]
    g = np.zeros((P, 3), np.float64)
    with np.errstate(all="ignore"):
        for sel, g_d, a, b, c, d in aux["terms"]:
            g_dd = g_d.astype(np.float64) / (2.0 * d.astype(np.float64))
            for ax, comp in enumerate((a, b, c)):
                g[:, ax] += np.where(sel, -(2.0 * comp.astype(np.float64) * g_dd), 0.0)
    return g / float(pitch)


def refine(points, occ, unocc, q, t, n_iter, *, pitch, origin, threshold, alpha_q, alpha_t, step0=0, m=None, v=None):
    """mf_occreg_refine of one object -> dict(q, t, m, v, losses [n_iter], traj [n_iter + 1, 7])."""
    q, t = np.array(q, f32), np.array(t, f32)
    m = np.zeros(7, f32) if m is None else np.array(m, f32)
    v = np.zeros(7, f32) if v is None else np.array(v, f32)
    losses = np.zeros(n_iter, f32)
    traj = np.zeros((n_iter + 1, 7), f32)
    traj[0] = np.concatenate([q, t])
    m_hist, v_hist = [m.copy()], [v.copy()]
    with np.errstate(all="ignore"):
        for k in range(n_iter):
            loss, gq, gt = loss_grad(points, occ, unocc, q, t, pitch=pitch, origin=origin, threshold=threshold)
            losses[k] = loss
            aq, at = adam_alphas(alpha_q, alpha_t, step0 + k + 1)
            adam_pose_step(gq, gt, aq, at, q, t, m, v)
            traj[k + 1] = np.concatenate([q, t])
            m_hist.append(m.copy())
            v_hist.append(v.copy())
    return dict(q=q, t=t, m=m, v=v, losses=losses, traj=traj, m_hist=np.stack(m_hist), v_hist=np.stack(v_hist))


def loss_grad_f64(points, occ, unocc, q, t, *, pitch, origin, threshold):
    """The formula of section "arithmetic" evaluated in float64 from the float32 inputs, dense over voxels x points
    (the yardstick of the teacher-forced comparison): loss, gq, gt."""
    f = np.float64
    q, t = np.asarray(q, f), np.asarray(t, f)
    p = np.asarray(points, f).reshape(-1, 3)
    X, Y, Z = occ.shape
    occ, unocc = np.asarray(occ, f).reshape(-1), np.asarray(unocc, f).reshape(-1)
    n = q @ q
    s = np.sqrt(2.0 / n)
    qs = q * s
    Q = np.outer(qs, qs)
    R = np.array([[1 - Q[2, 2] - Q[3, 3], Q[1, 2] - Q[3, 0], Q[1, 3] + Q[2, 0]],
                  [Q[1, 2] + Q[3, 0], 1 - Q[1, 1] - Q[3, 3], Q[2, 3] - Q[1, 0]],
                  [Q[1, 3] - Q[2, 0], Q[2, 3] + Q[1, 0], 1 - Q[1, 1] - Q[2, 2]]])
    pf = (p @ R.T + t - np.asarray(origin, f)) / f(pitch)
    I, J, K = np.meshgrid(np.arange(X), np.arange(Y), np.arange(Z), indexing="ij")
    vox = np.stack([I, J, K], -1).reshape(-1, 3).astype(f)
    thr = f(threshold)
    V = vox.shape[0]
    dmin = np.empty(V)
    for s0 in range(0, V, 2048):
        d = vox[s0:s0 + 2048, None, :] - pf[None]
        dmin[s0:s0 + 2048] = np.sqrt((d ** 2).sum(-1)).min(1)
    m = np.minimum(np.maximum(thr - dmin, 0), 1)
    A, Sm, Bq, So = (unocc * m).sum(), m.sum(), (occ * m).sum(), occ.sum()
    loss = A / Sm - Bq / So
    gm = unocc / Sm - A / Sm ** 2 - occ / So
    r = thr - dmin
    g_d = np.where((r > 0) & (r <= 1), -gm, 0.0)
    gpf = np.zeros_like(pf)
    act = np.flatnonzero(g_d != 0)
    for s0 in range(0, act.size, 2048):
        idx = act[s0:s0 + 2048]
        d = vox[idx, None, :] - pf[None]
        dd = np.sqrt((d ** 2).sum(-1))
        sel = dd == dmin[idx, None]
        w = np.where(sel, g_d[idx, None] / np.where(sel, dd, 1.0), 0.0)  # g_d / (2 d) * 2
        gpf += (-(d * w[..., None])).sum(0)
    g = gpf / f(pitch)
    gR = g.T @ p
    gt = g.sum(0)
    # mf::quat_backward in float64
    gr = gR.reshape(-1)
    gQ = np.zeros((4, 4))
    gQ[1, 0] = -gr[5] + gr[7]
    gQ[1, 1] = -gr[4] - gr[8]
    gQ[1, 2] = gr[1] + gr[3]
    gQ[1, 3] = gr[2] + gr[6]
    gQ[2, 0] = gr[2] - gr[6]
    gQ[2, 2] = -gr[0] - gr[8]
    gQ[2, 3] = gr[5] + gr[7]
    gQ[3, 0] = -gr[1] + gr[3]
    gQ[3, 3] = -gr[0] - gr[4]
    gqs = gQ @ qs + gQ.T @ qs
    gq = s * gqs - (s / n) * (gqs @ q) * q
    return loss, gq, gt
