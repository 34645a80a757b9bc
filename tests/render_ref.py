"""TEST INFRASTRUCTURE: NumPy mirror of csrc/render.hip (depth / instance rasteriser), float64, expression for
expression: the same transform, projection, canonical edge order, top-left rule, clipped box, plane depth and
key = (float32 depth bits, record index) minimum.  Bitwise equal to the kernels (DESIGN.md "Mesh rendering")."""
import numpy as np

EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)


def setup(vertices, faces, T, K, height, width, near=0.01):
    """Records of one item: dict of per-face arrays (valid, box x0 y0 x1 y1, edges [F, 3, 4], pos / owns [F, 3],
    plane [F, 4])."""
    v = np.asarray(vertices, np.float64).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    T = np.asarray(T, np.float64).reshape(4, 4)
    fx, fy, cx, cy = float(K[0][0]), float(K[1][1]), float(K[0][2]), float(K[1][2])
    F = f.shape[0]
    with np.errstate(all="ignore"):
        ok = ~((f < 0) | (f >= v.shape[0])).any(axis=1)
        fi = np.where(ok[:, None], f, 0)
        c = np.zeros((F, 3, 3))
        if v.shape[0]:
            p = v[fi]  # [F, 3 corners, 3]
            for a in range(3):
                c[..., a] = ((T[a, 0] * p[..., 0] + T[a, 1] * p[..., 1]) + T[a, 2] * p[..., 2]) + T[a, 3]
        else:
            ok[:] = False
        ok &= (c[..., 2] > near).all(axis=1)
        u = (fx * c[..., 0]) / c[..., 2] + cx
        w = (fy * c[..., 1]) / c[..., 2] + cy
        ok &= (np.abs(u) <= np.finfo(np.float64).max).all(axis=1) & (np.abs(w) <= np.finfo(np.float64).max).all(axis=1)
        edges = np.zeros((F, 3, 4))
        pos = np.zeros((F, 3), bool)
        owns = np.zeros((F, 3), bool)
        for k in range(3):
            a, b, o = k, (k + 1) % 3, (k + 2) % 3
            swap = (w[:, b] < w[:, a]) | ((w[:, b] == w[:, a]) & (u[:, b] < u[:, a]))
            ua, va = np.where(swap, u[:, b], u[:, a]), np.where(swap, w[:, b], w[:, a])
            ub, vb = np.where(swap, u[:, a], u[:, b]), np.where(swap, w[:, a], w[:, b])
            du, dv = ub - ua, vb - va
            s = du * (w[:, o] - va) - dv * (u[:, o] - ua)
            ok &= ~((s == 0.0) | np.isnan(s))
            edges[:, k] = np.stack([ua, va, du, dv], 1)
            pos[:, k] = s > 0.0
            owns[:, k] = np.where(dv > 0.0, ~pos[:, k], pos[:, k])
        e1, e2 = c[:, 1] - c[:, 0], c[:, 2] - c[:, 0]
        nx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
        ny = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
        nz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
        d = (nx * c[:, 0, 0] + ny * c[:, 0, 1]) + nz * c[:, 0, 2]
        x0 = np.maximum(np.ceil(u.min(axis=1)), 0.0)
        x1 = np.minimum(np.floor(u.max(axis=1)), float(width - 1))
        y0 = np.maximum(np.ceil(w.min(axis=1)), 0.0)
        y1 = np.minimum(np.floor(w.max(axis=1)), float(height - 1))
        ok &= (x0 <= x1) & (y0 <= y1)
    box = np.where(ok[:, None], np.stack([x0, y0, x1, y1], 1), 0).astype(np.int64)
    return dict(valid=ok, box=box, edges=edges, pos=pos, owns=owns, plane=np.stack([nx, ny, nz, d], 1),
                K=(fx, fy, cx, cy))


def _raster(rec, zbuf, rec0, width):
    fx, fy, cx, cy = rec["K"]
    for f in np.flatnonzero(rec["valid"]):
        x0, y0, x1, y1 = rec["box"][f]
        pv, pu = np.mgrid[y0:y1 + 1, x0:x1 + 1].astype(np.float64)
        inside = np.ones(pu.shape, bool)
        for k in range(3):
            ua, va, du, dv = rec["edges"][f, k]
            e = du * (pv - va) - dv * (pu - ua)
            inside &= np.where(e == 0.0, rec["owns"][f, k], (e > 0.0) if rec["pos"][f, k] else (e < 0.0))
        if not inside.any():
            continue
        nx, ny, nz, d = rec["plane"][f]
        with np.errstate(all="ignore"):
            rx, ry = (pu - cx) / fx, (pv - cy) / fy
            zf = (d / ((nx * rx + ny * ry) + nz)).astype(np.float32)
        inside &= (zf > 0) & (zf <= np.finfo(np.float32).max)
        idx = (pv[inside].astype(np.int64) * width + pu[inside].astype(np.int64))
        key = (zf[inside].view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.uint64(rec0 + f)
        zbuf[idx] = np.minimum(zbuf[idx], key)


def render(meshes, Ts, K, height, width, targets=None, instance_ids=None, near=0.01):
    """Mirror of geometry.render_meshes: items (meshes[n], Ts[n]) -> dict(depth f32 [T, H, W] (NaN), instance,
    face i32 [T, H, W] (-1), count i32 [N])."""
    n = len(meshes)
    targets = [0] * n if targets is None else [int(t) for t in targets]
    ids = list(range(n)) if instance_ids is None else [int(i) for i in instance_ids]
    n_targets = (max(targets) + 1) if n else 1
    zbuf = np.full((n_targets, height * width), EMPTY, np.uint64)
    rec_off = [0]
    for (v, f), T, t in zip(meshes, Ts, targets):
        rec = setup(v, f, T, K, height, width, near)
        _raster(rec, zbuf[t], rec_off[-1], width)
        rec_off.append(rec_off[-1] + len(np.asarray(f).reshape(-1, 3)))
    hit = zbuf != EMPTY
    r = (zbuf & np.uint64(0xFFFFFFFF)).astype(np.int64)
    item = np.clip(np.searchsorted(np.asarray(rec_off), r, side="right") - 1, 0, max(n - 1, 0))
    depth = np.where(hit, (zbuf >> np.uint64(32)).astype(np.uint32).view(np.float32), np.float32(np.nan))
    ids_a = np.asarray(ids + [0], np.int32)
    instance = np.where(hit, ids_a[item], -1).astype(np.int32)
    face = np.where(hit, r - np.asarray(rec_off)[item], -1).astype(np.int32)
    count = np.bincount(item[hit], minlength=n).astype(np.int32)[:n] if n else np.zeros(0, np.int32)
    shape = (n_targets, height, width)
    return dict(depth=depth.reshape(shape).astype(np.float32), instance=instance.reshape(shape),
                face=face.reshape(shape), count=count)


def full_grids(points, Ts, pitch, origin, dim=32):
    """Mirror of geometry.full_grids: the kernel's expression order (the tests restate _get_grid_full separately)."""
    n = len(points)
    gt = np.zeros((n, dim, dim, dim), np.int32)
    gn = np.zeros((n, dim, dim, dim), np.int32)
    for e in range(n):
        for i in range(n):
            p, T = np.asarray(points[i], np.float64).reshape(-1, 3), np.asarray(Ts[i], np.float64)
            idx = []
            for a in range(3):
                c = ((T[a, 0] * p[:, 0] + T[a, 1] * p[:, 1]) + T[a, 2] * p[:, 2]) + T[a, 3]
                idx.append(np.rint((c - origin[e][a]) / pitch[e]))
            idx = np.stack(idx, 1)
            keep = ((idx >= 0) & (idx < dim)).all(axis=1)
            I, J, Kk = idx[keep].astype(np.int64).T
            if i == e:
                gt[e, I, J, Kk] = 1
            else:
                label = (i if i < e else i - 1) + 1
                gn[e, I, J, Kk] = np.maximum(gn[e, I, J, Kk], label)
    return gt, gn
