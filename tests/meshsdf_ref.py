"""TEST INFRASTRUCTURE: NumPy mirror of csrc/meshsdf.hip (mesh signed distance, solid voxelization).

Same face records, the same face order and the same operation order as the kernel, expression for expression;
every face of a query is evaluated with the kernel's formulas (vectorised over the faces of a chunk of queries,
the branch chain of Ericson's routine as an ordered ``np.select``), the winding sum runs sequentially in face
order and the arg-min keeps the first minimum.  Bitwise equal to the kernel except ``winding`` (device and libm
``atan2`` may differ by an ulp).  ``workers`` > 1 runs query chunks in threads (NumPy releases the GIL)."""
import concurrent.futures

import numpy as np

FOUR_PI = 12.566370614359172
ON_SURFACE = 1e-8


def prepare(vertices, faces):
    """[F, 16] face records: a, b, c, ab, ac, kind (0 triangle, 1 segment: start / direction in ab / ac, 2 skipped)."""
    v = np.asarray(vertices, np.float64).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    F = f.shape[0]
    rec = np.zeros((F, 16), np.float64)
    bad = ((f < 0) | (f >= v.shape[0])).any(axis=1)
    fi = np.where(bad[:, None], 0, f)
    if v.shape[0] == 0:
        rec[:, 15] = 2.0
        return rec
    p = [v[fi[:, k]] for k in range(3)]
    ab = p[1] - p[0]
    ac = p[2] - p[0]
    nx = ab[:, 1] * ac[:, 2] - ab[:, 2] * ac[:, 1]
    ny = ab[:, 2] * ac[:, 0] - ab[:, 0] * ac[:, 2]
    nz = ab[:, 0] * ac[:, 1] - ab[:, 1] * ac[:, 0]
    seg = (nx == 0.0) & (ny == 0.0) & (nz == 0.0)
    s0, e = ab.copy(), ac.copy()
    best = np.full(F, -1.0)
    for k in range(3):  # the longest edge ab, bc, ca (strict >: the first on a tie)
        s, t = p[k], p[(k + 1) % 3]
        d = t - s
        l2 = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]
        take = l2 > best
        best = np.where(take, l2, best)
        s0 = np.where(take[:, None], s, s0)
        e = np.where(take[:, None], d, e)
    rec[:, 0:3], rec[:, 3:6], rec[:, 6:9] = p
    rec[:, 9:12] = np.where(seg[:, None], s0, ab)
    rec[:, 12:15] = np.where(seg[:, None], e, ac)
    rec[:, 15] = np.where(seg, 1.0, 0.0)
    rec[bad] = 0.0
    rec[bad, 15] = 2.0
    return rec


def _dot(ax, ay, az, bx, by, bz):
    return ax * bx + ay * by + az * bz


def _chunk(rec, P, tol):
    """Queries P [n, 3] against every face record -> dist, face, winding, sdf, occupied."""
    n = P.shape[0]
    F = rec.shape[0]
    if F == 0:
        d = np.full(n, np.inf)
        return d, np.full(n, -1, np.int32), np.zeros(n), -d, d <= tol
    px, py, pz = (P[:, k:k + 1] for k in range(3))
    a = [rec[None, :, k] for k in range(0, 3)]
    b = [rec[None, :, k] for k in range(3, 6)]
    c = [rec[None, :, k] for k in range(6, 9)]
    abx, aby, abz = (rec[None, :, k] for k in range(9, 12))
    acx, acy, acz = (rec[None, :, k] for k in range(12, 15))
    kind = rec[:, 15]
    apx, apy, apz = px - a[0], py - a[1], pz - a[2]
    bpx, bpy, bpz = px - b[0], py - b[1], pz - b[2]
    cpx, cpy, cpz = px - c[0], py - c[1], pz - c[2]
    # Ericson 5.1.5 (triangle records)
    d1 = _dot(abx, aby, abz, apx, apy, apz)
    d2 = _dot(acx, acy, acz, apx, apy, apz)
    d3 = _dot(abx, aby, abz, bpx, bpy, bpz)
    d4 = _dot(acx, acy, acz, bpx, bpy, bpz)
    d5 = _dot(abx, aby, abz, cpx, cpy, cpz)
    d6 = _dot(acx, acy, acz, cpx, cpy, cpz)
    vc = d1 * d4 - d3 * d2
    vb = d5 * d2 - d1 * d6
    va = d3 * d6 - d5 * d4
    conds = [
        (d1 <= 0.0) & (d2 <= 0.0),
        (d3 >= 0.0) & (d4 <= d3),
        (vc <= 0.0) & (d1 >= 0.0) & (d3 <= 0.0),
        (d6 >= 0.0) & (d5 <= d6),
        (vb <= 0.0) & (d2 >= 0.0) & (d6 <= 0.0),
        (va <= 0.0) & ((d4 - d3) >= 0.0) & ((d5 - d6) >= 0.0),
    ]
    v_ab = d1 / (d1 - d3)
    w_ac = d2 / (d2 - d6)
    w_bc = (d4 - d3) / ((d4 - d3) + (d5 - d6))
    denom = 1.0 / (va + vb + vc)
    v_in, w_in = vb * denom, vc * denom
    ab3, ac3 = (abx, aby, abz), (acx, acy, acz)
    q = []
    for k in range(3):
        q.append(np.select(conds, [
            np.broadcast_to(a[k], d1.shape), np.broadcast_to(b[k], d1.shape), a[k] + v_ab * ab3[k],
            np.broadcast_to(c[k], d1.shape), a[k] + w_ac * ac3[k], b[k] + w_bc * (c[k] - b[k])],
            a[k] + ab3[k] * v_in + ac3[k] * w_in))
    dx, dy, dz = px - q[0], py - q[1], pz - q[2]
    d2_tri = dx * dx + dy * dy + dz * dz
    # segment records: start in ab, direction in ac
    ee = acx * acx + acy * acy + acz * acz
    t = ((px - abx) * acx + (py - aby) * acy + (pz - abz) * acz) / ee
    t = np.where(t < 0.0, 0.0, np.where(t > 1.0, 1.0, t))
    t = np.where(ee > 0.0, t, 0.0)
    sx, sy, sz = px - (abx + t * acx), py - (aby + t * acy), pz - (abz + t * acz)
    d2_seg = sx * sx + sy * sy + sz * sz
    d2_all = np.where(kind[None] == 0.0, d2_tri, np.where(kind[None] == 1.0, d2_seg, np.inf))
    # winding (triangle records)
    la = np.sqrt(apx * apx + apy * apy + apz * apz)
    lb = np.sqrt(bpx * bpx + bpy * bpy + bpz * bpz)
    lc = np.sqrt(cpx * cpx + cpy * cpy + cpz * cpz)
    det = -(apx * (bpy * cpz - bpz * cpy) + apy * (bpz * cpx - bpx * cpz) + apz * (bpx * cpy - bpy * cpx))
    den = la * lb * lc + _dot(apx, apy, apz, bpx, bpy, bpz) * lc + _dot(apx, apy, apz, cpx, cpy, cpz) * lb \
        + _dot(bpx, bpy, bpz, cpx, cpy, cpz) * la
    omega = np.where(kind[None] == 0.0, 2.0 * np.arctan2(det, den), 0.0)
    S = np.zeros(n)
    for f in range(F):  # sequential, face-index order
        S = S + omega[:, f]
    # arg-min: first strict minimum (NaN never wins; none below +inf -> face -1)
    d2n = np.where(np.isnan(d2_all), np.inf, d2_all)
    idx = np.argmin(d2n, axis=1)
    best = d2n[np.arange(n), idx]
    face = np.where(best < np.inf, idx, -1).astype(np.int32)
    dist = np.sqrt(best)
    w = S / FOUR_PI
    inside = (w >= 0.5) | (dist <= ON_SURFACE)
    return dist, face, w, np.where(inside, dist, -dist), (w >= 0.5) | (dist <= tol)


def query(rec, points, tol=None, chunk=32, workers=1):
    """Mirror of k_meshsdf_query over explicit points: dict of dist, face, winding, sdf, occupied
    (``tol``: occupancy distance threshold; default = the inside rule's 1e-8)."""
    P = np.asarray(points, np.float64).reshape(-1, 3)
    tol = ON_SURFACE if tol is None else tol
    parts = [P[i:i + chunk] for i in range(0, P.shape[0], chunk)]
    with np.errstate(all="ignore"):
        if workers > 1 and len(parts) > 1:
            with concurrent.futures.ThreadPoolExecutor(workers) as ex:
                res = list(ex.map(lambda p: _chunk(rec, p, tol), parts))
        else:
            res = [_chunk(rec, p, tol) for p in parts]
    keys = ("dist", "face", "winding", "sdf", "occupied")
    if not res:
        return {"dist": np.zeros(0), "face": np.zeros(0, np.int32), "winding": np.zeros(0), "sdf": np.zeros(0),
                "occupied": np.zeros(0, bool)}
    return {k: np.concatenate([r[i] for r in res]) for i, k in enumerate(keys)}


def grid_params(vertices, dimension=64):
    """Origin = bbox min, cell h = largest bbox extent / dimension (all vertices)."""
    v = np.asarray(vertices, np.float64).reshape(-1, 3)
    vmin = v.min(axis=0)
    ext = (v.max(axis=0) - vmin).max()
    return vmin, ext / dimension


def grid_centres(origin, h, dimension, index=None):
    """Centres of the cells (all, (i, j, k) lexicographic, or the flat ``index`` subset): origin + (i + 0.5) h."""
    D = dimension
    j = np.arange(D ** 3, dtype=np.int64) if index is None else np.asarray(index, np.int64)
    ijk = np.stack([j // (D * D), (j // D) % D, j % D], axis=1).astype(np.float64)
    return np.asarray(origin, np.float64)[None] + (ijk + 0.5) * h


def solid_occupancy(vertices, faces, dimension=64, index=None, workers=1):
    """Mirror of the grid launch: occupancy of all cells (or of the flat ``index`` subset)."""
    origin, h = grid_params(vertices, dimension)
    rec = prepare(vertices, faces)
    r = query(rec, grid_centres(origin, h, dimension, index), tol=0.5 * h, workers=workers)
    return r["occupied"], origin, h, r


def signed_distance(vertices, faces, points, workers=1):
    return query(prepare(vertices, faces), points, workers=workers)


# ---- test geometry ------------------------------------------------------------------------------------------------
def box_mesh(lo=(0.0, 0.0, 0.0), hi=(1.0, 1.0, 1.0)):
    """Axis-aligned box, 8 vertices / 12 outward-wound triangles."""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    v = np.array([[(lo, hi)[x][0], (lo, hi)[y][1], (lo, hi)[z][2]] for x in (0, 1) for y in (0, 1) for z in (0, 1)])
    i = lambda x, y, z: 4 * x + 2 * y + z  # noqa: E731
    quads = [(i(0, 0, 0), i(0, 0, 1), i(0, 1, 1), i(0, 1, 0)), (i(1, 0, 0), i(1, 1, 0), i(1, 1, 1), i(1, 0, 1)),
             (i(0, 0, 0), i(1, 0, 0), i(1, 0, 1), i(0, 0, 1)), (i(0, 1, 0), i(0, 1, 1), i(1, 1, 1), i(1, 1, 0)),
             (i(0, 0, 0), i(0, 1, 0), i(1, 1, 0), i(1, 0, 0)), (i(0, 0, 1), i(1, 0, 1), i(1, 1, 1), i(0, 1, 1))]
    f = [(q[0], q[1], q[2]) for q in quads] + [(q[0], q[2], q[3]) for q in quads]
    return v, np.asarray(f, np.int32)


def box_sdf(points, lo, hi):
    """Analytic signed distance to a box, positive inside."""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    c = np.asarray(points, np.float64) - (lo + hi) / 2
    q = np.abs(c) - (hi - lo) / 2
    return -(np.linalg.norm(np.maximum(q, 0.0), axis=1) + np.minimum(q.max(axis=1), 0.0))


def icosphere(subdivisions=2, radius=1.0):
    """Icosahedron subdivided ``subdivisions`` times, vertices on the sphere; outward winding."""
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t),
         (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6),
         (7, 1, 8), (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10),
         (8, 6, 7), (9, 8, 1)]
    v = [np.asarray(x, np.float64) / np.linalg.norm(x) for x in v]
    for _ in range(subdivisions):
        mid, nf = {}, []

        def m(a, b):
            k = (min(a, b), max(a, b))
            if k not in mid:
                p = v[a] + v[b]
                v.append(p / np.linalg.norm(p))
                mid[k] = len(v) - 1
            return mid[k]
        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return np.asarray(v) * radius, np.asarray(f, np.int32)
