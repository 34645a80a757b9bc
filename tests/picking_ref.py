"""TEST INFRASTRUCTURE: NumPy mirror of csrc/pickorder.hip (occlusion counts, organised normals, grasp poses) and of
contrib.get_picking_order, float64, expression for expression.  Bitwise equal to the kernels (DESIGN.md "Picking
order"); ``normals`` is also bitwise equal to the executed reference (tests/golden/ref_pointcloud_normals.npz).

The fixed summation order of ``grasp`` (the two float sums: points, normals): the chosen cell's pixels are numbered
q = 0, 1, ... row-major over the cell's rectangle clipped to the box; lane t of 256 adds the pixels q = t, t + 256,
... in increasing q, skipping the pixels that do not count (outside the mask; for the normals also a NaN normal);
the 256 partial sums are folded by s[t] += s[t + h] for h = 128, 64, ..., 1.  The means are s[0] / count.
"""
import math

import numpy as np

import render_ref as RR

LANES = 256
OFFSETS = ((-2, 0), (-2, 2), (0, 2), (2, 2), (2, 0), (2, -2), (0, -2), (-2, -2))  # (dy, dx) of neighbour k


def occlusion(instance, ids):
    """instance int32 [N + 1, H, W] (0: composite, 1 + n: item n alone) -> whole [N], occluded_by [N, N], bbox [N, 4]."""
    n = len(ids)
    whole = np.zeros(n, np.int32)
    occ = np.zeros((n, n), np.int32)
    bbox = np.zeros((n, 4), np.int32)
    for i in range(n):
        mask = instance[1 + i] == ids[i]
        whole[i] = mask.sum()
        for j in range(n):
            occ[i, j] = (mask & (instance[0] == ids[j])).sum()
        if whole[i]:
            rows, cols = np.flatnonzero(mask.any(axis=1)), np.flatnonzero(mask.any(axis=0))
            bbox[i] = rows[0], cols[0], rows[-1] + 1, cols[-1] + 1
    return whole, occ, bbox


def normals(points, rect=None):
    """points float64 [H, W, 3] -> normals [H, W, 3], NaN outside rect = (y1, x1, y2, x2) (default: the image)."""
    P = np.asarray(points, np.float64)
    H, W = P.shape[:2]
    y1, x1, y2, x2 = (0, 0, H, W) if rect is None else rect
    y1, x1, y2, x2 = max(int(y1), 0), max(int(x1), 0), min(int(y2), H), min(int(x2), W)
    out = np.full((H, W, 3), np.nan)
    h, w = y2 - y1, x2 - x1
    if h <= 0 or w <= 0:
        return out
    p1 = P[y1:y2, x1:x2]
    pad = np.full((h + 4, w + 4, 3), np.nan)
    pad[2:-2, 2:-2] = p1
    with np.errstate(all="ignore"):
        e = np.stack([pad[2 + dy:2 + dy + h, 2 + dx:2 + dx + w] - p1 for dy, dx in OFFSETS])  # [8, h, w, 3]
        d = np.sqrt((e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2])
        cost = d + np.roll(d, -2, axis=0)  # pair k: neighbours k and (k + 2) % 8
        cost[np.isnan(cost)] = np.inf
        best = np.argmin(cost, axis=0)  # the first minimum
        a = np.take_along_axis(e, best[None, :, :, None], axis=0)[0]
        b = np.take_along_axis(e, ((best + 2) % 8)[None, :, :, None], axis=0)[0]
        n0 = a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1]
        n1 = a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2]
        n2 = a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]
        ln = np.sqrt((n0 * n0 + n1 * n1) + n2 * n2)
        out[y1:y2, x1:x2] = np.stack([n0 / ln, n1 / ln, n2 / ln], -1)
    return out


def backproject(depth, K):
    """pointcloud_from_depth in float64: ((z (col - cx)) / fx, (z (row - cy)) / fy, z)."""
    fx, fy, cx, cy = float(K[0][0]), float(K[1][1]), float(K[0][2]), float(K[1][2])
    z = np.asarray(depth).astype(np.float64)
    H, W = z.shape
    col, row = np.arange(W, dtype=np.float64)[None, :], np.arange(H, dtype=np.float64)[:, None]
    return np.stack([(z * (col - cx)) / fx, (z * (row - cy)) / fy, z + 0 * col], -1)


def _fixed_sum(values, counted):
    """values [Q, C] in pixel order q, counted bool [Q] -> the [C] sum in the order of this module's docstring."""
    Q, C = values.shape
    rounds = -(-Q // LANES)
    v = np.zeros((rounds * LANES, C))
    keep = np.zeros(rounds * LANES, bool)
    v[:Q], keep[:Q] = values, counted
    v, keep = v.reshape(rounds, LANES, C), keep.reshape(rounds, LANES)
    s = np.zeros((LANES, C))
    for k in range(rounds):
        s = np.where(keep[k][:, None], s + v[k], s)
    half = LANES // 2
    while half >= 1:
        s[:half] = s[:half] + s[half:2 * half]
        half //= 2
    return s[0]


def grasp(depth, instance, ids, bbox, K):
    """depth float32 / instance int32 [N + 1, H, W], bbox [N, 4] -> cell int32 [N], translation, normal float64 [N, 3]."""
    n = len(ids)
    cell = np.full(n, -1, np.int32)
    translation = np.full((n, 3), np.nan)
    normal = np.full((n, 3), np.nan)
    for i in range(n):
        y1, x1, y2, x2 = (int(v) for v in bbox[i])
        h, w = y2 - y1, x2 - x1
        if h <= 0 or w <= 0:
            continue
        mask = instance[1 + i] == ids[i]
        S = max(1, math.isqrt((h * w) // 30))
        gh, gw = -(-h // S), -(-w // S)
        regions = []  # (cell, centroid row, centroid col) in cell order
        for k in range(gh * gw):
            r0, c0 = y1 + (k // gw) * S, x1 + (k % gw) * S
            rr, cc = np.nonzero(mask[r0:min(r0 + S, y2), c0:min(c0 + S, x2)])
            if len(rr):
                regions.append((k, float(int((rr + r0).sum())) / float(len(rr)), float(int((cc + c0).sum())) / float(len(rr))))
        if not regions:
            continue
        sr = sc = 0.0
        for _, r, c in regions:
            sr, sc = sr + r, sc + c
        ar, ac = sr / float(len(regions)), sc / float(len(regions))
        best, arg = None, -1
        for k, r, c in regions:
            dr, dc = r - ar, c - ac
            dist = math.sqrt(dr * dr + dc * dc)
            if arg < 0 or dist < best:
                best, arg = dist, k
        cell[i] = arg
        r0, c0 = y1 + (arg // gw) * S, x1 + (arg % gw) * S
        r1, c1 = min(r0 + S, y2), min(c0 + S, x2)
        pcd = backproject(depth[1 + i], K)
        nrm = normals(pcd, (y1, x1, y2, x2))
        m = mask[r0:r1, c0:c1].reshape(-1)
        pts = pcd[r0:r1, c0:c1].reshape(-1, 3)
        nn = nrm[r0:r1, c0:c1].reshape(-1, 3)
        good = m & ~np.isnan(nn).any(axis=1)
        translation[i] = _fixed_sum(pts, m) / float(m.sum())
        if good.any():
            normal[i] = _fixed_sum(nn, good) / float(good.sum())
    return cell, translation, normal


def analysis(meshes, Ts, K, height, width, ids, mesh_index=None):
    """Mirror of contrib.occlusion_analysis up to the kernels' outputs: the renders (tests/render_ref.py), then
    whole, occluded_by, bbox, cell, translation, normal; also the renderer's depth / instance [N + 1, H, W]."""
    mesh_index = list(range(len(meshes))) if mesh_index is None else list(mesh_index)
    n = len(mesh_index)
    items = [meshes[m] for m in mesh_index]
    Ts = np.asarray(Ts, np.float64).reshape(-1, 4, 4)
    r = RR.render(items + items, np.concatenate([Ts, Ts]), K, height, width,
                  targets=[0] * n + list(range(1, n + 1)), instance_ids=list(ids) + list(ids))
    whole, occ, bbox = occlusion(r["instance"], ids)
    cell, translation, normal = grasp(r["depth"], r["instance"], ids, bbox, K)
    return dict(whole=whole, occluded_by=occ, bbox=bbox, cell=cell, translation=translation, normal=normal,
                depth=r["depth"], instance=r["instance"])


def get_picking_order(edges, target, nodes=()):
    """Mirror of contrib.get_picking_order, written as rounds over sets: returns (order, rounds) with ``rounds`` the
    list of the sets removed in turn (the last one {target})."""
    succ = {}
    for (i, j), w in edges.items():
        succ.setdefault(i, {})
        succ.setdefault(j, {})
        if i != j:
            succ[i][j] = w
    for v in list(nodes) + [target]:
        succ.setdefault(v, {})
    order, rounds = [], []
    while True:
        seen, frontier = {target}, {target}
        while frontier:
            frontier = {j for i in frontier for j in succ[i]} - seen
            seen |= frontier
        free = {v for v in seen if not succ[v]}
        if target in free:
            rounds.append({target})
            return order + [target], rounds
        if not free:
            cost = {v: sum(succ[v].values()) for v in seen if v != target}
            free = {min(cost, key=lambda v: (cost[v], v))}
        rounds.append(free)
        order += sorted(free)
        succ = {i: {j: w for j, w in out.items() if j not in free} for i, out in succ.items() if i not in free}
