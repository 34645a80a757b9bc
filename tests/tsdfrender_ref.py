"""TEST INFRASTRUCTURE: NumPy mirror of the TSDF render (include/mfhip.h "TSDF render"), written from that description:
the block summary by brute force over footprints, and the render as the per-sample classification with NO jumps -- a
sample in a FREE block is valid with F = 1, one in an UNKNOWN block is invalid, every other sample is evaluated as the
ray-cast of "TSDF fusion" evaluates it (the expressions of tests/tsdf_ref.py, in the header's association).  It yields
depth, code, label, ``sampled`` and the number of samples per ray; the label is tests/tsdflabel_ref.py's label image of
the depth.  Bitwise equal to csrc/tsdfrender.hip.  Every NumPy operation on coordinates is one IEEE operation per
element."""
import math

import numpy as np

import tsdf_ref as R
import tsdflabel_ref as LR

MIXED, FREE, UNKNOWN = range(3)
BLOCK_EDGES = (2, 4, 8, 16)


def summary_shape(dims, B):
    """(nb_z, nb_y, nb_x): ceil((n - 1) / B) per axis."""
    assert B in BLOCK_EDGES
    nx, ny, nz = dims
    return tuple(-(-(n - 1) // B) for n in (nz, ny, nx))


def block_summary(vol, B):
    """-> uint8 [nb_z, nb_y, nb_x]."""
    nz, ny, nx = vol.shape[:3]
    shape = summary_shape((nx, ny, nz), B)
    out = np.empty(shape, np.uint8)
    with np.errstate(invalid="ignore"):
        seen = vol[..., 1] > 0.0
        free = seen & (vol[..., 0] == np.float32(1.0))
    for K in range(shape[0]):
        for J in range(shape[1]):
            for I in range(shape[2]):
                foot = (slice(B * K, min(B * K + B, nz - 1) + 1), slice(B * J, min(B * J + B, ny - 1) + 1),
                        slice(B * I, min(B * I + B, nx - 1) + 1))
                out[K, J, I] = FREE if free[foot].all() else (UNKNOWN if not seen[foot].any() else MIXED)
    return out


def render(vol, summary, B, origin, pitch, step, min_depth, max_depth, max_steps, K, T, H, W, labels=None, min_count=1):
    """-> dict(depth float32 [H, W], code uint8, label int32 (zeros without ``labels``), sampled int32, total int32,
    before int8: how the last sample before the ray's end was obtained -- the one before the sample that ended it in a
    hit or a back face, the last one taken before LEFT or CAP: MIXED (evaluated; out of range too), FREE, UNKNOWN, or
    -1 if there was none)."""
    nz, ny, nx = vol.shape[:3]
    dims = (nx, ny, nz)
    assert summary.shape == summary_shape(dims, B) and summary.dtype == np.uint8
    nbz, nby, nbx = summary.shape
    fx, fy, cx, cy = float(K[0][0]), float(K[1][1]), float(K[0][2]), float(K[1][2])
    Rm, o = R._pose(T)
    pitch, step = float(pitch), float(step)
    org = [float(v) for v in origin]
    P = H * W
    row, col = np.divmod(np.arange(P), W)
    tsdf, weight, codes = vol[..., 0].reshape(-1), vol[..., 1].reshape(-1), summary.reshape(-1)
    depth, code = np.zeros(P, np.float32), np.full(P, 255, np.uint8)
    sampled, total = np.zeros(P, np.int32), np.zeros(P, np.int32)
    before = np.full(P, -1, np.int8)
    with np.errstate(all="ignore"):
        q0, q1 = (col.astype(np.float64) - cx) / fx, (row.astype(np.float64) - cy) / fy
        d = [(Rm[a, 0] * q0 + Rm[a, 1] * q1) + Rm[a, 2] for a in range(3)]
        enter, leave = np.full(P, float(min_depth)), np.full(P, float(max_depth))
        miss = np.zeros(P, bool)
        for a in range(3):
            lo, hi = org[a], org[a] + pitch * float(dims[a] - 1)
            sloped = (d[a] < 0.0) | (d[a] > 0.0)
            t1, t2 = (lo - o[a]) / d[a], (hi - o[a]) / d[a]
            first = t1 < t2
            tn, tf = np.where(first, t1, t2), np.where(first, t2, t1)
            enter = np.where(sloped, np.where(tn <= enter, enter, tn), enter)
            leave = np.where(sloped, np.where(tf >= leave, leave, tf), leave)
            miss |= ~sloped & ~((d[a] == 0.0) & (o[a] >= lo) & (o[a] <= hi))
        miss |= ~(enter <= leave)
        code[miss] = R.MISS
        live = np.flatnonzero(~miss)
        d = [x[live] for x in d]
        enter, leave = enter[live], leave[live]
        have, prev = np.zeros(live.size, bool), np.zeros(live.size)
        last = np.full(live.size, -1, np.int8)
        k = 0
        while live.size:
            s = enter + float(k) * step
            left = ~(s <= leave)
            code[live[left]] = R.LEFT
            capped = ~left & (k >= max_steps)
            code[live[capped]] = R.CAP
            taken = ~left & ~capped  # sample k exists for these rays
            total[live[taken]] += 1
            g = [((o[a] + s * d[a]) - org[a]) / pitch for a in range(3)]
            b = [np.floor(x) for x in g]
            inside = taken.copy()
            for a in range(3):
                inside &= (b[a] >= 0.0) & (b[a] <= float(dims[a] - 2))
            cell = [np.where(inside, b[a], 0.0).astype(np.int64) for a in range(3)]
            block = codes[((cell[2] // B) * nby + cell[1] // B) * nbx + cell[0] // B]
            free, unknown = inside & (block == FREE), inside & (block == UNKNOWN)
            loaded = inside & (block == MIXED)
            sampled[live[taken & ~free & ~unknown]] += 1
            base = (cell[2] * ny + cell[1]) * nx + cell[0]
            corner = {(dx, dy, dz): base + (dz * ny + dy) * nx + dx for dx in (0, 1) for dy in (0, 1) for dz in (0, 1)}
            valid = loaded.copy()
            for c in corner.values():
                valid &= weight[c] > 0.0
            V = {key: tsdf[c].astype(np.float64) for key, c in corner.items()}
            r = [g[a] - b[a] for a in range(3)]
            Vyz = {(dy, dz): V[0, dy, dz] + r[0] * (V[1, dy, dz] - V[0, dy, dz]) for dy in (0, 1) for dz in (0, 1)}
            Vz = {dz: Vyz[0, dz] + r[1] * (Vyz[1, dz] - Vyz[0, dz]) for dz in (0, 1)}
            F = np.where(free, 1.0, Vz[0] + r[2] * (Vz[1] - Vz[0]))
            valid |= free
            ends = valid & (F <= 0.0)
            hit = ends & have & (prev > 0.0)
            crossing = (enter + float(k - 1) * step) + step * (prev / (prev - F))
            depth[live[hit]] = crossing[hit].astype(np.float32)
            code[live[hit]] = R.HIT
            code[live[ends & ~hit]] = R.BACKFACE
            have = valid & ~ends
            prev = np.where(have, F, 0.0)
            go = ~(left | capped | ends)
            before[live[~go]] = last[~go]
            last = np.where(free, FREE, np.where(unknown, UNKNOWN, MIXED)).astype(np.int8)
            live, enter, leave, have, prev, last = live[go], enter[go], leave[go], have[go], prev[go], last[go]
            d = [x[go] for x in d]
            k += 1
    depth = depth.reshape(H, W)
    label = np.zeros((H, W), np.int32) if labels is None else LR.label_image(labels, origin, pitch, depth, K, T, min_count)
    return dict(depth=depth, code=code.reshape(H, W), label=label, sampled=sampled.reshape(H, W),
                total=total.reshape(H, W), before=before.reshape(H, W))


def render_volume(vol, K, T, H, W, B, step=None, min_depth=0.0, max_depth=None, max_steps=None, labels=False,
                  min_count=1):
    """``render`` of a mirror volume (tsdf_ref.Volume / tsdflabel_ref.InstanceVolume) with TsdfVolume.render's defaults;
    the summary is made from the volume as it is.  The result also holds ``summary``."""
    step = vol.truncation / 2.0 if step is None else float(step)
    max_depth = math.inf if max_depth is None else float(max_depth)
    max_steps = R.max_steps_of(vol.dims, vol.pitch, step) if max_steps is None else max_steps
    summary = block_summary(vol.volume, B)
    out = render(vol.volume, summary, B, vol.origin, vol.pitch, step, min_depth, max_depth, max_steps, K, T, H, W,
                 vol.labels if labels else None, min_count)
    return dict(out, summary=summary)
