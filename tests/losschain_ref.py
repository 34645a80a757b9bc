"""TEST INFRASTRUCTURE: float64 references of the training loss chain and an a-priori error bound per output element.

The chain is pose epilogue -> transformation_matrix -> ADD / ADD-S -> confidence loss (``Model.loss_device``), forward
and backward: ``mf_pose_epilogue_train_*``, ``mf_transformation_matrix_*`` (csrc/pointops.hip, quat.h) and
``mf_average_distance_*``, ``mf_confidence_loss_*`` (csrc/loss.hip).  Everything here is NumPy in float64, written from
the contract in include/mfhip.h and the reference project's formulas (contrib/singleview_3d/models/model.py:262-273 and
:417-434, functions/geometry/quaternion_matrix.py, functions/loss/average_distance.py); where a gradient has a closed
form that is independent of the kernels' chain rule (the quaternion matrix), that form is used.

THE BOUND.  Every function returns, next to each result, ``bound`` with ``|float32 result - float64 result| <= bound``
element by element.  It is computed in float64 from the INPUTS alone, to first order in u = 2^-24, as

    (number of float32 roundings on the longest path of the stated operation order) * u * (sum of |terms|)

where a correctly rounded ``+ - *`` (and a float32 constant such as 1e-5f) is one rounding.  ROCm's HIP math
documentation with the ulp figures of ``expf``, ``logf``, ``sqrtf`` and the float32 divide does not come with the
installed toolchain, so each of the four is ASSUMED accurate to 2 ulp = ``FN`` = 4 roundings; nobody has measured them
on the device.  Sums over M model points or P points use the depth of the kernels' fixed reduction order
(include/mfhip.h, csrc/loss.hip's header): ``rounds`` additions per lane (lane l owns elements l, l + W, ...), then 6
butterfly steps over the 64 lanes of a wave, then the waves / objects in index order.  A bound of 0 means "exact":
zeros outside an object's class, copied translations, the bottom row of a transform, a residual that is exactly zero.
A NaN in the reference means the result must be NaN.  Nothing here is read off a kernel's output; a case over its bound
is a finding about the kernel or about a count below, to be shown by the operation order.

Counts (k = roundings charged, S = the sum of absolute values it multiplies):

pose_epilogue         rot_k = x_k / (sqrt(((x0^2 + x1^2) + x2^2) + x3^2) + 1e-5): squares and sums 4, sqrt halves them
                      and adds FN -> 6, the constant and the sum -> 7, the divide FN -> k = 11, S = |rot_k|.
                      trans = (p * pitch + origin) + raw * pitch: product, sum, sum -> k = 3,
                      S = |p pitch| + |origin| + |raw pitch|.
                      conf = 1 / (1 + exp(-x)): exp FN, sum 1, divide FN -> k = 9, S = conf.
pose_epilogue_grad    drot_k = g_k / d - x_k (x . g) / (s d d), d = s + 1e-5 (7, above): g_k / d 11; x . g 4 on sum |x_i
                      g_i|; s d d: 6 + 7 + 1 + 7 + 1 = 22, the divide FN, the product 1, the difference 1 -> k = 32,
                      S = |g_k / d| + |x_k| sum |x_i g_i| / (s d d); s = 0: g_k / 1e-5 (the second term vanishes).
                      dtrn = g pitch: k = 1.  dcnf = g c (1 - c): c 9, (1 - c) 9 c + 1, two products -> k = 12,
                      S = |g| c (1 + c).
transformation_matrix qs = q sqrt(2 / n), n = ((q0^2 + q1^2) + q2^2) + q3^2: n 4, 2 / n 8, sqrt 8, qs 9, Q_ij = qs_i qs_j
                      19, two differences -> k = 21, S = 1 + |Q_aa| + |Q_bb| on the diagonal, |Q_ab| + |Q_cd| off it.
                      The translation column and the bottom row are copies: bound 0.
transformation_matrix_grad   dR/dQ (sums of two cotangents, 1), gqs_i = sum_j (gQ_ij + gQ_ji) qs_j (qs 9, product 1, 3 + 1
                      sums -> 15 on A_i = sum_j (|gQ|_ij + |gQ|_ji) |qs_j|), dot = gqs . q (19 on D = sum A_i |q_i|),
                      gq_i = s gqs_i - (s / n) dot q_i: 8 + 15 + 1 = 24 and 16 + 19 + 1 + 1 = 37, the difference 1
                      -> k = 38, S = s A_i + (s / n) D |q_i|.  gt is a copy of the cotangent's last column: bound 0.
average_distance      image_i = ((R_i0 x + R_i1 y) + R_i2 z) + t_i: 4 on C_i = sum_j |R_ij x_j| + |t_i| (the coordinate
                      magnitudes, so that the cancellation in true' - pred is accounted for); the residual
                      d_i = true'_i - pred_i: e_i = 5 u (Ct_i + Cp_i).  n = sqrt((d0^2 + d1^2) + d2^2):
                      |dn| <= |e|_2 + 6 u n (3 roundings on n^2 halve to 1.5, sqrt FN).  out = (sum_m n_m) / M:
                      depth = rounds + 6 + 3 (M / 256 rounds per lane, butterfly, 4 waves), the divide FN ->
                      bound = (sum_m (|e_m|_2 + 6 u n_m) + (depth + 4) u sum_m n_m) / M.
                      A pair (query m, candidate k) of the ADD-S search: ssd = (d0^2 + d1^2) + d2^2 is off by at most
                      pair_bound = sum_i (2 |d_i| e_i + e_i^2) + 3 u ssd.
average_distance_grad gT_ij = sum_m -g (d_i / n) X_j, X = (x, y, z, 1), g = gout / M (FN): d_i / n is off by
                      U_i = e_i / n + |d_i| (|e|_2 + 6 u n) / n^2 + 4 u |d_i| / n, the two products add 2 to g's 4 ->
                      bound = sum_m |g| (U_i + 6 u |d_i| / n) |X_j| + depth u sum_m |g (d_i / n) X_j|.
confidence_loss       term = add c - lam log(c): <= 6 u S_p, S_p = |add c| + |lam log c| (product 1, log FN, product 1,
                      difference 1); object = (sum_p term) / cnt: rounds = ceil(P / 64) per lane + 6 butterfly + FN
                      -> (rounds + 16) u S_b, S_b = sum_p S_p / cnt; loss = (sum_b object) / B: B in order + FN
                      -> k = rounds + 16 + B + 4, S = sum_b S_b / B.
confidence_loss_grad  g = gloss / B / cnt (2 FN = 8); dadd = g c: k = 9; dconf = g (add - lam / c): lam / c FN, the
                      difference 1, the product 1 -> k = 14, S = |g| (|add| + |lam / c|).
"""
import numpy as np

U = 2.0 ** -24
FN = 4          # roundings charged to one sqrtf / expf / logf / float32 divide: 2 ulp, ASSUMED (see above)
EPS = 1e-5      # F.normalize's epsilon (chainer: x / (|x| + 1e-5))

RATIOS = {}     # what -> worst |got - ref| / bound of the checks made in this process (reporting only)


# ---- the comparator ---------------------------------------------------------------------------------------------
def compare(got, ref, bound):
    """-> (ok, worst ratio, index of the worst element).  Rules: where ``ref`` is NaN ``got`` must be NaN; elsewhere
    ``got`` must be finite and ``|got - ref| <= bound``; where ``bound == 0`` that means equal."""
    got, ref, bound = (np.asarray(a, np.float64) for a in (got, ref, bound))
    assert got.shape == ref.shape == bound.shape, (got.shape, ref.shape, bound.shape)
    if got.size == 0:
        return True, 0.0, ()
    nan = np.isnan(ref)
    with np.errstate(invalid="ignore", divide="ignore"):
        err = np.abs(got - ref)
        ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
    ratio = np.where(nan, np.where(np.isnan(got), 0.0, np.inf), ratio)
    ratio = np.where(~nan & ~np.isfinite(got), np.inf, ratio)
    i = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    worst = float(ratio[i])
    return worst <= 1.0, worst, tuple(int(v) for v in i)


def assert_within(got, ref, bound, what, op=None):
    """Every element of ``got`` within ``bound`` of ``ref``; prints the worst one before it asserts."""
    ok, worst, i = compare(got, ref, bound)
    key = op or what
    RATIOS[key] = max(RATIOS.get(key, 0.0), worst if np.isfinite(worst) else np.inf)
    g, r, b = (np.asarray(a, np.float64)[i] if np.asarray(a).size else np.nan for a in (got, ref, bound))
    print(f"LOSSCHAIN {what}: worst |got-ref|/bound = {worst:.3f} at {i} (got {g!r}, ref {r!r}, bound {b:.3e})")
    assert ok, (what, worst, i, float(g), float(r), float(b))
    return worst


# ---- pose epilogue ----------------------------------------------------------------------------------------------
def _f64(*arrays):
    return tuple(np.asarray(a, np.float64) for a in arrays)


def pose_epilogue(orot, otrn, ocnf, class_id, pts, origin, pitch, n_fg):
    """orot [n, 4 n_fg], otrn [n, 3 n_fg], ocnf [n, n_fg], class_id [B] (1-based), pts [n, 3], origin [B, 3], pitch [B],
    n = B P -> ((rot [B,P,4], trans [B,P,3], conf [B,P]), (their bounds)).  A class id outside 1 .. n_fg: NaN."""
    orot, otrn, ocnf, pts, origin, pitch = _f64(orot, otrn, ocnf, pts, origin, pitch)
    B = len(class_id)
    P = orot.shape[0] // B
    rot, trans, conf = np.full((B, P, 4), np.nan), np.full((B, P, 3), np.nan), np.full((B, P), np.nan)
    brot, btrans, bconf = np.zeros((B, P, 4)), np.zeros((B, P, 3)), np.zeros((B, P))
    for b in range(B):
        fg = int(class_id[b]) - 1
        if not 0 <= fg < n_fg:
            continue
        rows = slice(b * P, (b + 1) * P)
        x = orot[rows, 4 * fg:4 * fg + 4]
        d = np.sqrt((x * x).sum(axis=1)) + EPS
        rot[b] = x / d[:, None]
        brot[b] = 11 * U * np.abs(rot[b])
        a, r = pts[rows] * pitch[b], otrn[rows, 3 * fg:3 * fg + 3] * pitch[b]
        trans[b] = a + origin[b] + r
        btrans[b] = 3 * U * (np.abs(a) + np.abs(origin[b]) + np.abs(r))
        conf[b] = 1.0 / (1.0 + np.exp(-ocnf[rows, fg]))
        bconf[b] = (2 * FN + 1) * U * conf[b]
    return (rot, trans, conf), (brot, btrans, bconf)


def pose_epilogue_grad(orot, ocnf, class_id, pitch, grot, gtrans, gconf, n_fg):
    """Cotangents grot [B,P,4], gtrans [B,P,3], gconf [B,P] -> ((drot [n, 4 n_fg], dtrn [n, 3 n_fg], dcnf [n, n_fg]),
    (bounds)): the three FULL blocks, zeros (bound 0) outside the object's class and in every row of an object whose
    class id is outside 1 .. n_fg, whatever its cotangents hold."""
    orot, ocnf, pitch = _f64(orot, ocnf, pitch)
    B = len(class_id)
    n = orot.shape[0]
    P = n // B
    grot, gtrans, gconf = (np.asarray(a, np.float64).reshape(B, P, -1) for a in (grot, gtrans, gconf))
    drot, dtrn, dcnf = np.zeros((n, 4 * n_fg)), np.zeros((n, 3 * n_fg)), np.zeros((n, n_fg))
    bdrot, bdtrn, bdcnf = np.zeros_like(drot), np.zeros_like(dtrn), np.zeros_like(dcnf)
    for b in range(B):
        fg = int(class_id[b]) - 1
        if not 0 <= fg < n_fg:
            continue
        rows = slice(b * P, (b + 1) * P)
        x, g = orot[rows, 4 * fg:4 * fg + 4], grot[b]
        s = np.sqrt((x * x).sum(axis=1))[:, None]
        d = s + EPS
        dot, dabs = (x * g).sum(axis=1)[:, None], np.abs(x * g).sum(axis=1)[:, None]
        den = np.where(s > 0, s * d * d, 1.0)
        c2, c2abs = np.where(s > 0, dot / den, 0.0), np.where(s > 0, dabs / den, 0.0)
        drot[rows, 4 * fg:4 * fg + 4] = g / d - x * c2
        bdrot[rows, 4 * fg:4 * fg + 4] = 32 * U * (np.abs(g / d) + np.abs(x) * c2abs)
        dtrn[rows, 3 * fg:3 * fg + 3] = gtrans[b] * pitch[b]
        bdtrn[rows, 3 * fg:3 * fg + 3] = U * np.abs(gtrans[b] * pitch[b])
        c = 1.0 / (1.0 + np.exp(-ocnf[rows, fg]))
        dcnf[rows, fg] = gconf[b, :, 0] * c * (1.0 - c)
        bdcnf[rows, fg] = 12 * U * np.abs(gconf[b, :, 0]) * c * (1.0 + c)
    return (drot, dtrn, dcnf), (bdrot, bdtrn, bdcnf)


# ---- transformation_matrix ----------------------------------------------------------------------------------------
def transformation_matrix(q, t):
    """q [n,4] wxyz of ANY norm (the scaled form of quaternion_matrix: qs = q sqrt(2 / |q|^2)), t [n,3] ->
    (T [n,4,4], bound)."""
    q, t = _f64(q, t)
    nrm = (q * q).sum(axis=1, keepdims=True)
    qs = q * np.sqrt(2.0 / nrm)
    Q = qs[:, :, None] * qs[:, None, :]
    A = np.abs(Q)
    n = q.shape[0]
    T, bnd = np.zeros((n, 4, 4)), np.zeros((n, 4, 4))
    T[:, 3, 3] = 1.0
    T[:, :3, 3] = t
    diag = {0: (2, 3), 1: (1, 3), 2: (1, 2)}
    for i, (a, b) in diag.items():
        T[:, i, i] = 1.0 - Q[:, a, a] - Q[:, b, b]
        bnd[:, i, i] = 21 * U * (1.0 + A[:, a, a] + A[:, b, b])
    # R_ij = Q_(i+1)(j+1) -/+ Q_(k+1)0 with (i, j, k) a cyclic / anti-cyclic permutation of the axes
    for (i, j), (ab, cd, sign) in {(0, 1): ((1, 2), (3, 0), -1), (0, 2): ((1, 3), (2, 0), +1), (1, 0): ((1, 2), (3, 0), +1),
                                   (1, 2): ((2, 3), (1, 0), -1), (2, 0): ((1, 3), (2, 0), -1),
                                   (2, 1): ((2, 3), (1, 0), +1)}.items():
        T[:, i, j] = Q[:, ab[0], ab[1]] + sign * Q[:, cd[0], cd[1]]
        bnd[:, i, j] = 21 * U * (A[:, ab[0], ab[1]] + A[:, cd[0], cd[1]])
    return T, bnd


def transformation_matrix_grad(q, gT):
    """-> ((gq [n,4], gt [n,3]), (bounds)) from the cotangent gT [n,4,4]; its bottom row reaches neither.  The value is
    the closed form of d/dq of R = I + (2 / |q|^2) N(q), N the quadratic forms of the rotation matrix; the bound follows
    the stated order of the chain rule (module docstring)."""
    q, gT = _f64(q, gT)
    G = gT[:, :3, :3]
    w, x, y, z = (q[:, i] for i in range(4))
    g = lambda i, j: G[:, i, j]  # noqa: E731
    N = np.stack([np.stack([-(y * y + z * z), x * y - z * w, x * z + y * w], 1),
                  np.stack([x * y + z * w, -(x * x + z * z), y * z - x * w], 1),
                  np.stack([x * z - y * w, y * z + x * w, -(x * x + y * y)], 1)], 1)
    psi = (G * N).sum(axis=(1, 2))
    dpsi = np.stack([
        -g(0, 1) * z + g(0, 2) * y + g(1, 0) * z - g(1, 2) * x - g(2, 0) * y + g(2, 1) * x,
        g(0, 1) * y + g(0, 2) * z + g(1, 0) * y - 2 * g(1, 1) * x - g(1, 2) * w + g(2, 0) * z + g(2, 1) * w - 2 * g(2, 2) * x,
        -2 * g(0, 0) * y + g(0, 1) * x + g(0, 2) * w + g(1, 0) * x + g(1, 2) * z - g(2, 0) * w + g(2, 1) * z - 2 * g(2, 2) * y,
        -2 * g(0, 0) * z - g(0, 1) * w + g(0, 2) * x + g(1, 0) * w - 2 * g(1, 1) * z + g(1, 2) * y + g(2, 0) * x + g(2, 1) * y,
    ], 1)
    nrm = (q * q).sum(axis=1, keepdims=True)
    gq = (2.0 / nrm) * dpsi - (4.0 / (nrm * nrm)) * psi[:, None] * q
    # magnitudes in the order of the chain rule: |gQ|_ij = the two cotangents of dR/dQ's entry (i, j)
    a = np.abs(G)
    gQa = np.zeros((q.shape[0], 4, 4))
    for (i, j), (p, r) in {(1, 0): ((1, 2), (2, 1)), (1, 1): ((1, 1), (2, 2)), (1, 2): ((0, 1), (1, 0)),
                           (1, 3): ((0, 2), (2, 0)), (2, 0): ((0, 2), (2, 0)), (2, 2): ((0, 0), (2, 2)),
                           (2, 3): ((1, 2), (2, 1)), (3, 0): ((0, 1), (1, 0)), (3, 3): ((0, 0), (1, 1))}.items():
        gQa[:, i, j] = a[:, p[0], p[1]] + a[:, r[0], r[1]]
    s = np.sqrt(2.0 / nrm)
    qsa = np.abs(q) * s
    Ai = np.einsum("nij,nj->ni", gQa, qsa) + np.einsum("nji,nj->ni", gQa, qsa)
    D = (Ai * np.abs(q)).sum(axis=1, keepdims=True)
    bq = 38 * U * (s * Ai + (s / nrm) * D * np.abs(q))
    return (gq, gT[:, :3, 3].copy()), (bq, np.zeros((q.shape[0], 3)))


# ---- ADD / ADD-S ----------------------------------------------------------------------------------------------------
def _images(pts, T):
    """-> (T applied to pts [M,3], the coordinate magnitudes sum_j |R_ij x_j| + |t_i|)."""
    R, t = T[:3, :3], T[:3, 3]
    return pts @ R.T + t, np.abs(pts) @ np.abs(R).T + np.abs(t)


def pair_bound(d, e):
    """Error bound of a float32 squared distance whose residual is d [..., 3] with coordinate errors e [..., 3]."""
    return (2.0 * np.abs(d) * e + e * e).sum(axis=-1) + 3 * U * (d * d).sum(axis=-1)


def _depth(M):
    return (M + 255) // 256 + 6 + 3


def nearest(points, T_true, T_pred):
    """The ADD-S search of one (object, pose) in float64: -> (idx [M], the smallest squared distance per query [M]);
    lowest index among equal squared distances, 0 where every distance is NaN (a non-finite pose)."""
    pts, Tt, Tp = _f64(points, T_true, T_pred)
    true, _ = _images(pts, Tt)
    pred, _ = _images(pts, Tp)
    with np.errstate(invalid="ignore"):
        ssd = ((true[:, None, :] - pred[None, :, :]) ** 2).sum(axis=2)   # [candidate, query]
        idx = ssd.argmin(axis=0)
    return idx.astype(np.int64), ssd[idx, np.arange(len(pts))]


def argmin_slack(points, T_true, T_pred, idx):
    """For every query m of one (object, pose): (the float64 squared distance of candidate idx[m] minus the float64
    minimum, the bound of that difference) -- a float32 search may prefer idx[m] to the true arg-min k0 only if
    ssd(idx[m]) - ssd(k0) <= pair_bound(idx[m]) + pair_bound(k0)."""
    pts, Tt, Tp = _f64(points, T_true, T_pred)
    true, Ct = _images(pts, Tt)
    pred, Cp = _images(pts, Tp)
    k0, smin = nearest(points, T_true, T_pred)
    out = []
    for k in (np.asarray(idx, np.int64), k0):
        d = true[k] - pred
        out.append(((d * d).sum(axis=1), pair_bound(d, 5 * U * (Ct[k] + Cp))))
    (s_got, b_got), (_, b_min) = out
    return s_got - smin, b_got + b_min


def average_distance(points, T_true, T_pred, sym, idx=None):
    """points [B,M,3], T_true [B,4,4], T_pred [B,P,4,4], sym [B] -> (out [B,P], bound [B,P], idx [B,P,M]): out = mean_m
    |true'_m - pred_m| with true' the point's own true image (ADD) or, for sym[b], the true image of point idx[b,p,m]
    (ADD-S).  ``idx=None`` searches in float64 (``nearest``); ADD rows of idx hold 0 .. M-1.  A pose with a non-finite
    entry gives NaN."""
    pts, Tt, Tp = _f64(points, T_true, T_pred)
    B, M = pts.shape[:2]
    P = Tp.shape[1]
    out, bound = np.zeros((B, P)), np.zeros((B, P))
    used = np.zeros((B, P, M), np.int64)
    for b in range(B):
        true, Ct = _images(pts[b], Tt[b])
        for p in range(P):
            pred, Cp = _images(pts[b], Tp[b, p])
            if not sym[b]:
                k = np.arange(M)
            elif idx is None:
                k = nearest(pts[b], Tt[b], Tp[b, p])[0]
            else:
                k = np.asarray(idx[b, p], np.int64)
            used[b, p] = k
            d = true[k] - pred
            e = 5 * U * (Ct[k] + Cp)
            n = np.sqrt((d * d).sum(axis=1))
            E = np.sqrt((e * e).sum(axis=1)) + 6 * U * n
            out[b, p] = n.sum() / M
            bound[b, p] = (E.sum() + (_depth(M) + FN) * U * n.sum()) / M
    bound = np.where(np.isnan(out), 0.0, bound)
    return out, bound, used


def average_distance_grad(points, T_true, T_pred, sym, idx, gout):
    """-> (gT [B,P,4,4], bound): d(sum gout * out) / d T_pred with the arg-min frozen to idx [B,P,M]; rows 0 .. 2, row 3
    zero.  A point whose residual is exactly zero, or not a number (a non-finite pose), contributes zero."""
    pts, Tt, Tp, gout = _f64(points, T_true, T_pred, gout)
    B, M = pts.shape[:2]
    P = Tp.shape[1]
    gT, bound = np.zeros((B, P, 4, 4)), np.zeros((B, P, 4, 4))
    depth = _depth(M)
    for b in range(B):
        true, Ct = _images(pts[b], Tt[b])
        X = np.concatenate([pts[b], np.ones((M, 1))], axis=1)
        for p in range(P):
            pred, Cp = _images(pts[b], Tp[b, p])
            k = np.asarray(idx[b, p], np.int64) if sym[b] else np.arange(M)
            d = true[k] - pred
            e = 5 * U * (Ct[k] + Cp)
            n = np.sqrt((d * d).sum(axis=1))
            with np.errstate(invalid="ignore"):
                live = n > 0
            d, e, n, Xl = d[live], e[live], n[live][:, None], X[live]
            g = gout[b, p] / M
            uh = d / n
            E = np.sqrt((e * e).sum(axis=1))[:, None] + 6 * U * n
            Ui = e / n + np.abs(d) * E / (n * n) + FN * U * np.abs(uh)
            gT[b, p, :3] = -g * (uh.T @ Xl)
            bound[b, p, :3] = (abs(g) * (Ui + 6 * U * np.abs(uh))).T @ np.abs(Xl) + depth * U * abs(g) * (np.abs(uh).T @ np.abs(Xl))
    return gT, bound


# ---- confidence loss --------------------------------------------------------------------------------------------------
def confidence_loss(add, conf, lam):
    """add, conf [B,P], lam (the float32 value the kernel receives) -> (loss, bound, cnt [B]): the mean over objects of the
    mean over the points with conf > 0 of add conf - lam log(conf).  An object without such a point gives NaN for the
    object and for the total."""
    add, conf = _f64(add, conf)
    lam = float(np.float32(lam))
    B, P = add.shape
    keep = conf > 0
    cnt = keep.sum(axis=1)
    c = np.where(keep, conf, 1.0)
    a, l = np.where(keep, add * c, 0.0), np.where(keep, lam * np.log(c), 0.0)
    with np.errstate(invalid="ignore", divide="ignore"):
        obj = (a - l).sum(axis=1) / cnt
        S = (np.abs(a) + np.abs(l)).sum(axis=1) / cnt
    loss = obj.sum() / B
    k = (P + 63) // 64 + 6 + 6 + FN + B + FN
    return loss, (0.0 if np.isnan(loss) else k * U * S.sum() / B), cnt.astype(np.int32)


def confidence_loss_grad(add, conf, lam, gloss):
    """-> ((dadd, dconf) [B,P], (bounds)): zeros where conf <= 0, hence in every row of an object without a confident
    point; the other objects' rows are finite."""
    add, conf = _f64(add, conf)
    lam = float(np.float32(lam))
    B, P = add.shape
    keep = conf > 0
    cnt = keep.sum(axis=1, keepdims=True)
    g = float(gloss) / B / np.maximum(cnt, 1)
    c = np.where(keep, conf, 1.0)
    dadd = np.where(keep, g * c, 0.0)
    dconf = np.where(keep, g * (add - lam / c), 0.0)
    bdadd = (2 * FN + 1) * U * np.abs(dadd)
    bdconf = np.where(keep, (2 * FN + FN + 2) * U * np.abs(g) * (np.abs(add) + np.abs(lam / c)), 0.0)
    return (dadd, dconf), (bdadd, bdconf)
