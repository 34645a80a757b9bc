"""TEST INFRASTRUCTURE: NumPy float64 mirror of the camera tracker (include/mfhip.h "camera tracking"), written from
that description: the depth pyramid, the vertex and normal maps, and the point-to-plane Gauss-Newton loop with its
fixed summation orders.  Bitwise equal to csrc/camtrack.hip (DESIGN.md "Camera tracking").  No np.sum over a long
axis: every sum below is a loop of elementwise adds in the documented order.

Orders.  Residual launch: pixel p (row-major) belongs to workgroup g = p // 1024, round s = (p % 1024) // 256 and
lane t = p % 256; a lane adds its pairs in the order s = 0 .. 3; the 64 lanes of a wave fold by x[l] += x[l + h] for
h = 32 .. 1; the waves add as ((w0 + w1) + w2) + w3.  Solve: sub-sum j = 0 .. 7 adds the workgroups g = j, j + 8, ..
in turn, the total is s0 + s1 + .. + s7 left to right.  The normals are those of tests/picking_ref.py (mf_pick_normals).
"""
import math

import numpy as np

import picking_ref

LANES, ROUNDS, WAVE, SUB = 256, 4, 64, 8
GROUP = LANES * ROUNDS
TRACKING, LOST_PAIRS, LOST_PIVOT = 0, 1, 2
DEFAULTS = dict(levels=3, iterations=(10, 5, 4), block_band=0.05, distance_threshold=0.1,
                cos_angle_threshold=math.cos(math.radians(20.0)), min_pairs=100)


def level_intrinsics(K, levels):
    out = [(float(K[0][0]), float(K[1][1]), float(K[0][2]), float(K[1][2]))]
    for _ in range(1, levels):
        fx, fy, cx, cy = out[-1]
        out.append((fx / 2.0, fy / 2.0, (cx - 0.5) / 2.0, (cy - 0.5) / 2.0))
    return out


def downsample(depth, band):
    """float32 [H, W] -> float32 [H // 2, W // 2]: the banded mean of each 2 x 2 block."""
    H, W = depth.shape
    h, w = H // 2, W // 2
    d = [depth[dy:2 * h:2, dx:2 * w:2] for dy, dx in ((0, 0), (0, 1), (1, 0), (1, 1))]
    with np.errstate(invalid="ignore"):
        valid = [x > 0 for x in d]
        dmin = np.full((h, w), np.inf, np.float32)
        for x, ok in zip(d, valid):
            dmin = np.where(ok & (x < dmin), x, dmin)
        total, count = np.zeros((h, w)), np.zeros((h, w))
        for x, ok in zip(d, valid):
            use = ok & (x.astype(np.float64) - dmin.astype(np.float64) <= band)
            total = np.where(use, total + x.astype(np.float64), total)
            count = np.where(use, count + 1.0, count)
        return np.where(count > 0, total / count, np.nan).astype(np.float32)


def vertex_map(depth, intr):
    fx, fy, cx, cy = intr
    H, W = depth.shape
    with np.errstate(invalid="ignore"):
        z = np.where(depth > 0, depth, np.nan).astype(np.float64)
    col, row = np.arange(W, dtype=np.float64)[None, :], np.arange(H, dtype=np.float64)[:, None]
    return np.stack([(z * (col - cx)) / fx, (z * (row - cy)) / fy, z + 0.0 * col], -1)


def prepare(depth, K, levels=3, block_band=0.05):
    """depth float32 [B, H, W] -> [level] of dict(depth [B, h, w] float32, vertex, normal [B, h, w, 3], intr)."""
    depth = np.asarray(depth, np.float32)
    intr = level_intrinsics(K, levels)
    pyramid, cur = [], depth
    for l in range(levels):
        if l:
            cur = np.stack([downsample(d, block_band) for d in cur])
        vertex = np.stack([vertex_map(d, intr[l]) for d in cur])
        normal = np.stack([picking_ref.normals(v) for v in vertex])
        pyramid.append(dict(depth=cur, vertex=vertex, normal=normal, intr=intr[l]))
    return pyramid


def quat_normalise(q):
    n = math.sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3])
    return np.array([q[0] / n, q[1] / n, q[2] / n, q[3] / n])


def quat_matrix(q):
    w, x, y, z = (float(v) for v in q)
    return np.array([[1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - w * z), 2.0 * (x * z + w * y)],
                     [2.0 * (x * y + w * z), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - w * x)],
                     [2.0 * (x * z - w * y), 2.0 * (y * z + w * x), 1.0 - 2.0 * (x * x + y * y)]])


def quat_from_matrix(m):
    m = np.asarray(m, np.float64)
    m00, m01, m02, m10, m11, m12, m20, m21, m22 = (float(m[i, j]) for i in range(3) for j in range(3))
    tr = (m00 + m11) + m22
    if tr > 0.0:
        s = math.sqrt(tr + 1.0) * 2.0
        q = [0.25 * s, (m21 - m12) / s, (m02 - m20) / s, (m10 - m01) / s]
    elif m00 > m11 and m00 > m22:
        s = math.sqrt(((1.0 + m00) - m11) - m22) * 2.0
        q = [(m21 - m12) / s, 0.25 * s, (m01 + m10) / s, (m02 + m20) / s]
    elif m11 > m22:
        s = math.sqrt(((1.0 + m11) - m00) - m22) * 2.0
        q = [(m02 - m20) / s, (m01 + m10) / s, 0.25 * s, (m12 + m21) / s]
    else:
        s = math.sqrt(((1.0 + m22) - m00) - m11) * 2.0
        q = [(m10 - m01) / s, (m02 + m20) / s, (m12 + m21) / s, 0.25 * s]
    return quat_normalise(q)


def pose_matrix(pose):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = quat_matrix(pose[:4]), pose[4:]
    return T


def _rot(R, v):
    """R [3, 3], v [N, 3] -> rows ((R_i0 v0 + R_i1 v1) + R_i2 v2)."""
    return np.stack([(R[i, 0] * v[:, 0] + R[i, 1] * v[:, 1]) + R[i, 2] * v[:, 2] for i in range(3)], -1)


def residual_terms(cur, ref, pose, T_ref, distance_threshold, cos_angle_threshold):
    """One image pair at one level -> (terms [P, 28], counted bool [P]) per pixel of the current image."""
    fx, fy, cx, cy = cur["intr"]
    H, W = cur["vertex"].shape[:2]
    v, n = cur["vertex"].reshape(-1, 3), cur["normal"].reshape(-1, 3)
    rv_map, rn_map = ref["vertex"].reshape(-1, 3), ref["normal"].reshape(-1, 3)
    R, t = quat_matrix(pose[:4]), pose[4:]
    Rr, tr = np.asarray(T_ref, np.float64)[:3, :3], np.asarray(T_ref, np.float64)[:3, 3]
    Ri = Rr.T
    ti = np.array([-((Rr[0, i] * tr[0] + Rr[1, i] * tr[1]) + Rr[2, i] * tr[2]) for i in range(3)])
    with np.errstate(all="ignore"):
        ok = ~(np.isnan(v).any(1) | np.isnan(n).any(1))
        vg = _rot(R, v) + t
        ng = _rot(R, n)
        pr = _rot(Ri, vg) + ti
        ok &= pr[:, 2] > 0.0
        uf = np.floor(((fx * pr[:, 0]) / pr[:, 2] + cx) + 0.5)
        vf = np.floor(((fy * pr[:, 1]) / pr[:, 2] + cy) + 0.5)
        ok &= (uf >= 0.0) & (uf < W) & (vf >= 0.0) & (vf < H)
        idx = np.where(ok, vf * W + uf, 0).astype(np.int64)
        rv, rn = rv_map[idx], rn_map[idx]
        ok &= ~(np.isnan(rv).any(1) | np.isnan(rn).any(1))
        rvg = _rot(Rr, rv) + tr
        rng = _rot(Rr, rn)
        d = rvg - vg
        ok &= ~(np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]) > distance_threshold)
        ok &= ~((ng[:, 0] * rng[:, 0] + ng[:, 1] * rng[:, 1]) + ng[:, 2] * rng[:, 2] < cos_angle_threshold)
        res = (rng[:, 0] * d[:, 0] + rng[:, 1] * d[:, 1]) + rng[:, 2] * d[:, 2]
        J = [rng[:, 0], rng[:, 1], rng[:, 2], vg[:, 1] * rng[:, 2] - vg[:, 2] * rng[:, 1],
             vg[:, 2] * rng[:, 0] - vg[:, 0] * rng[:, 2], vg[:, 0] * rng[:, 1] - vg[:, 1] * rng[:, 0]]
        terms = [J[i] * J[j] for i in range(6) for j in range(i, 6)] + [J[i] * res for i in range(6)] + [res * res]
    return np.stack(terms, -1), ok


def partials(terms, counted):
    """[P, 28], [P] -> one row of 29 per workgroup, in the residual launch's order."""
    P = terms.shape[0]
    groups = -(-P // GROUP)
    v = np.zeros((groups * GROUP, 29))
    keep = np.zeros(groups * GROUP, bool)
    v[:P, :28], keep[:P] = terms, counted
    v[:, 28] = 1.0
    v = v.reshape(groups, ROUNDS, LANES, 29)
    keep = keep.reshape(groups, ROUNDS, LANES)
    s = np.zeros((groups, LANES, 29))
    for r in range(ROUNDS):
        s = np.where(keep[:, r, :, None], s + v[:, r], s)
    s = s.reshape(groups, LANES // WAVE, WAVE, 29)
    h = WAVE // 2
    while h >= 1:
        s[:, :, :h] = s[:, :, :h] + s[:, :, h:2 * h]
        h //= 2
    w = s[:, :, 0]
    return ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]


def total_of(part):
    sub = []
    for j in range(SUB):
        s = np.zeros(29)
        for g in range(j, part.shape[0], SUB):
            s = s + part[g]
        sub.append(s)
    total = sub[0]
    for j in range(1, SUB):
        total = total + sub[j]
    return total


def solve(total):
    """29 sums -> (xi [6], None) or (None, LOST_PIVOT)."""
    A = np.zeros((6, 6))
    k = 0
    for i in range(6):
        for j in range(i, 6):
            A[i, j] = A[j, i] = total[k]
            k += 1
    b = [float(x) for x in total[21:27]]
    L = [[0.0] * 6 for _ in range(6)]
    for c in range(6):
        d = float(A[c, c])
        for m in range(c):
            d -= L[c][m] * L[c][m]
        if not d > 0.0:
            return None, LOST_PIVOT
        L[c][c] = math.sqrt(d)
        for i in range(c + 1, 6):
            s = float(A[i, c])
            for m in range(c):
                s -= L[i][m] * L[c][m]
            L[i][c] = s / L[c][c]
    y, x = [0.0] * 6, [0.0] * 6
    for i in range(6):
        s = b[i]
        for m in range(i):
            s -= L[i][m] * y[m]
        y[i] = s / L[i][i]
    for i in range(5, -1, -1):
        s = y[i]
        for m in range(i + 1, 6):
            s -= L[m][i] * x[m]
        x[i] = s / L[i][i]
    return x, None


def update(pose, x):
    dq = quat_normalise([1.0, x[3] / 2.0, x[4] / 2.0, x[5] / 2.0])
    Rinc = quat_matrix(dq)
    t = [float(v) for v in pose[4:]]
    tn = [(Rinc[i, 0] * t[0] + Rinc[i, 1] * t[1]) + Rinc[i, 2] * t[2] for i in range(3)]
    a0, a1, a2, a3 = (float(v) for v in dq)
    b0, b1, b2, b3 = (float(v) for v in pose[:4])
    q = quat_normalise([((a0 * b0 - a1 * b1) - a2 * b2) - a3 * b3, ((a0 * b1 + a1 * b0) + a2 * b3) - a3 * b2,
                        ((a0 * b2 - a1 * b3) + a2 * b0) + a3 * b1, ((a0 * b3 + a1 * b2) - a2 * b1) + a3 * b0])
    return np.concatenate([q, [tn[0] + x[0], tn[1] + x[1], tn[2] + x[2]]])


def align(cur, ref, T_ref_to_map, T_init=None, iterations=(10, 5, 4), distance_threshold=0.1,
          cos_angle_threshold=DEFAULTS["cos_angle_threshold"], min_pairs=100):
    """Pyramids of ``prepare`` (B images each) -> (pose [B, 7], T [B, 4, 4], status int32 [B], stats [B, n, 3])."""
    levels = len(cur)
    assert len(iterations) == levels
    T_ref_to_map = np.asarray(T_ref_to_map, np.float64).reshape(-1, 4, 4)
    T_init = T_ref_to_map if T_init is None else np.asarray(T_init, np.float64).reshape(-1, 4, 4)
    B, n_iters = T_ref_to_map.shape[0], int(sum(iterations))
    pose = np.zeros((B, 7))
    status = np.zeros(B, np.int32)
    stats = np.zeros((B, n_iters, 3))
    for b in range(B):
        pose0 = np.concatenate([quat_from_matrix(T_init[b]), T_init[b][:3, 3]])
        p, it = pose0.copy(), 0
        for l in range(levels - 1, -1, -1):
            c = {k: (v[b] if k != "intr" else v) for k, v in cur[l].items()}
            r = {k: (v[b] if k != "intr" else v) for k, v in ref[l].items()}
            for _ in range(iterations[levels - 1 - l]):
                if status[b] == TRACKING:
                    total = total_of(partials(*residual_terms(c, r, p, T_ref_to_map[b], distance_threshold,
                                                              cos_angle_threshold)))
                    pairs = int(total[28])
                    x, why = (None, LOST_PAIRS) if pairs < min_pairs else solve(total)
                    if x is None:
                        status[b], p = why, pose0.copy()
                        stats[b, it] = pairs, total[27], 0.0
                    else:
                        p = update(p, x)
                        stats[b, it] = pairs, total[27], math.sqrt(
                            ((((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2]) + x[3] * x[3]) + x[4] * x[4]) + x[5] * x[5])
                it += 1
        pose[b] = p
    return pose, np.stack([pose_matrix(p) for p in pose]), status, stats


def pose_errors(T, T_true):
    """(translation error in m, rotation error in rad) of T against T_true."""
    D = np.linalg.inv(T_true) @ T
    c = min(1.0, max(-1.0, (np.trace(D[:3, :3]) - 1.0) / 2.0))
    return float(np.linalg.norm(T[:3, 3] - T_true[:3, 3])), float(math.acos(c))


class Tracker:
    """The mirror of contrib.CameraTracker (reference = "previous" or "first"), one image per call."""

    def __init__(self, K, reference="previous", T_first=None, **knobs):
        self.K, self.policy = K, reference
        self.T_first = np.eye(4) if T_first is None else np.asarray(T_first, np.float64)
        self.knobs = dict(DEFAULTS, **knobs)
        self.ref = self.T_ref = None
        self.T_last = None
        self.status, self.stats = None, None

    def track(self, depth, T_init=None):
        k = self.knobs
        pyr = prepare(np.asarray(depth, np.float32)[None], self.K, k["levels"], k["block_band"])
        if self.ref is None:
            self.ref, self.T_ref, self.T_last = pyr, self.T_first.copy(), self.T_first.copy()
            return self.T_last
        init = self.T_last if T_init is None else np.asarray(T_init, np.float64)
        _, T, self.status, self.stats = align(pyr, self.ref, self.T_ref[None], init[None], k["iterations"],
                                              k["distance_threshold"], k["cos_angle_threshold"], k["min_pairs"])
        self.T_last = T[0]
        if self.policy == "previous":  # (lost or not: the status is never read back to decide)
            self.ref, self.T_ref = pyr, T[0]
        return self.T_last
