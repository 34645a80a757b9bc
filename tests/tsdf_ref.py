"""TEST INFRASTRUCTURE: NumPy float64 mirror of TSDF fusion (include/mfhip.h "TSDF fusion"), written from that
description: ``integrate`` and ``raycast`` with every expression associated as the header writes it, and the loop of
contrib.ModelTracker on top of the camera-tracking mirror (tests/camtrack_ref.py).  Bitwise equal to csrc/tsdf.hip.
Every NumPy operation below is one IEEE operation per element (no np.sum, no dot, no fused step)."""
import math

import numpy as np

import camtrack_ref as CR

HIT, LEFT, BACKFACE, MISS, CAP = range(5)
# the requirements of integrate, in the header's order: the index of the first one a voxel failed (or UPDATED)
BEHIND, OUTSIDE, HOLE, OCCLUDED, UPDATED = range(5)


def fresh(dims):
    nx, ny, nz = dims
    vol = np.empty((nz, ny, nx, 2), np.float32)
    vol[..., 0], vol[..., 1] = 1.0, 0.0
    return vol


def _pose(T):
    T = np.asarray(T, np.float64).reshape(4, 4)
    return T[:3, :3], T[:3, 3]


def integrate(vol, origin, pitch, truncation, max_weight, depth, K, T, skip=0):
    """In place on ``vol`` float32 [nz, ny, nx, 2] -> int8 [nz, ny, nx]: which requirement each voxel failed
    (BEHIND .. OCCLUDED), UPDATED where it was written, -1 everywhere if ``skip`` is nonzero."""
    nz, ny, nx = vol.shape[:3]
    outcome = np.full((nz, ny, nx), -1, np.int8)
    if skip != 0:
        return outcome
    depth = np.asarray(depth, np.float32)
    H, W = depth.shape
    fx, fy, cx, cy = float(K[0][0]), float(K[1][1]), float(K[0][2]), float(K[1][2])
    R, t = _pose(T)
    pitch, truncation, max_weight = float(pitch), float(truncation), float(max_weight)
    k, j, i = np.meshgrid(np.arange(nz, dtype=np.float64), np.arange(ny, dtype=np.float64),
                          np.arange(nx, dtype=np.float64), indexing="ij")
    with np.errstate(all="ignore"):
        e0 = (float(origin[0]) + pitch * i) - t[0]
        e1 = (float(origin[1]) + pitch * j) - t[1]
        e2 = (float(origin[2]) + pitch * k) - t[2]
        x = (R[0, 0] * e0 + R[1, 0] * e1) + R[2, 0] * e2
        y = (R[0, 1] * e0 + R[1, 1] * e1) + R[2, 1] * e2
        z = (R[0, 2] * e0 + R[1, 2] * e1) + R[2, 2] * e2
        ok = z > 0.0
        outcome[~ok] = BEHIND
        col = np.floor((fx * (x / z) + cx) + 0.5)
        row = np.floor((fy * (y / z) + cy) + 0.5)
        inside = (col >= 0.0) & (col <= float(W - 1)) & (row >= 0.0) & (row <= float(H - 1))
        outcome[ok & ~inside] = OUTSIDE
        ok &= inside
        idx = np.where(ok, row * W + col, 0.0).astype(np.int64)
        D = depth.reshape(-1)[idx].astype(np.float64)
        seen = D > 0.0
        outcome[ok & ~seen] = HOLE
        ok &= seen
        sdf = D - z
        near = sdf >= -truncation
        outcome[ok & ~near] = OCCLUDED
        ok &= near
        f = sdf / truncation
        f = np.where(f > 1.0, 1.0, f)
        F_old, W_old = vol[..., 0].astype(np.float64), vol[..., 1].astype(np.float64)
        w = W_old + 1.0
        F = (F_old * W_old + f) / w
        w = np.where(w > max_weight, max_weight, w)
    outcome[ok] = UPDATED
    vol[..., 0] = np.where(ok, F.astype(np.float32), vol[..., 0])
    vol[..., 1] = np.where(ok, w.astype(np.float32), vol[..., 1])
    return outcome


def max_steps_of(dims, pitch, step):
    nx, ny, nz = dims
    diagonal = float(pitch) * math.sqrt(float((nx - 1) ** 2 + (ny - 1) ** 2 + (nz - 1) ** 2))
    return int(math.floor(diagonal / step)) + 2


def raycast(vol, origin, pitch, step, min_depth, max_depth, max_steps, K, T, H, W):
    """-> (depth float32 [H, W], code uint8 [H, W])."""
    nz, ny, nx = vol.shape[:3]
    dims = (nx, ny, nz)
    fx, fy, cx, cy = float(K[0][0]), float(K[1][1]), float(K[0][2]), float(K[1][2])
    R, o = _pose(T)
    pitch, step = float(pitch), float(step)
    org = [float(v) for v in origin]
    P = H * W
    row, col = np.divmod(np.arange(P), W)
    tsdf, weight = vol[..., 0].reshape(-1), vol[..., 1].reshape(-1)
    depth, code = np.zeros(P, np.float32), np.full(P, 255, np.uint8)
    with np.errstate(all="ignore"):
        q0, q1 = (col.astype(np.float64) - cx) / fx, (row.astype(np.float64) - cy) / fy
        d = [(R[a, 0] * q0 + R[a, 1] * q1) + R[a, 2] for a in range(3)]
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
        code[miss] = MISS
        live = np.flatnonzero(~miss)  # the rays still marching, with their state
        d = [x[live] for x in d]
        enter, leave = enter[live], leave[live]
        have, prev = np.zeros(live.size, bool), np.zeros(live.size)
        k = 0
        while live.size:
            s = enter + float(k) * step
            left = ~(s <= leave)
            code[live[left]] = LEFT
            capped = ~left & (k >= max_steps)
            code[live[capped]] = CAP
            g = [((o[a] + s * d[a]) - org[a]) / pitch for a in range(3)]
            b = [np.floor(x) for x in g]
            valid = ~left & ~capped
            for a in range(3):
                valid &= (b[a] >= 0.0) & (b[a] <= float(dims[a] - 2))
            base = np.where(valid, (b[2] * ny + b[1]) * nx + b[0], 0.0).astype(np.int64)
            corner = {(dx, dy, dz): base + (dz * ny + dy) * nx + dx for dx in (0, 1) for dy in (0, 1) for dz in (0, 1)}
            for c in corner.values():
                valid &= weight[c] > 0.0
            V = {key: tsdf[c].astype(np.float64) for key, c in corner.items()}
            r = [g[a] - b[a] for a in range(3)]
            Vyz = {(dy, dz): V[0, dy, dz] + r[0] * (V[1, dy, dz] - V[0, dy, dz]) for dy in (0, 1) for dz in (0, 1)}
            Vz = {dz: Vyz[0, dz] + r[1] * (Vyz[1, dz] - Vyz[0, dz]) for dz in (0, 1)}
            F = Vz[0] + r[2] * (Vz[1] - Vz[0])
            ends = valid & (F <= 0.0)
            hit = ends & have & (prev > 0.0)
            crossing = (enter + float(k - 1) * step) + step * (prev / (prev - F))
            depth[live[hit]] = crossing[hit].astype(np.float32)
            code[live[hit]] = HIT
            code[live[ends & ~hit]] = BACKFACE
            have = valid & ~ends
            prev = np.where(have, F, 0.0)
            go = ~(left | capped | ends)
            live, enter, leave, have, prev = live[go], enter[go], leave[go], have[go], prev[go]
            d = [x[go] for x in d]
            k += 1
    return depth.reshape(H, W), code.reshape(H, W)


class Volume:
    """The mirror of contrib.TsdfVolume."""

    def __init__(self, dims, pitch, origin, truncation=None, max_weight=64.0):
        self.dims, self.pitch, self.origin = tuple(dims), float(pitch), tuple(float(v) for v in origin)
        self.truncation = 4.0 * self.pitch if truncation is None else float(truncation)
        self.max_weight = float(max_weight)
        self.volume = fresh(self.dims)

    def integrate(self, depth, K, T, skip=0):
        return integrate(self.volume, self.origin, self.pitch, self.truncation, self.max_weight, depth, K, T, skip)

    def raycast(self, K, T, H, W, step=None, min_depth=0.0, max_depth=None, max_steps=None):
        step = self.truncation / 2.0 if step is None else float(step)
        max_depth = math.inf if max_depth is None else float(max_depth)
        max_steps = max_steps_of(self.dims, self.pitch, step) if max_steps is None else max_steps
        return raycast(self.volume, self.origin, self.pitch, step, min_depth, max_depth, max_steps, K, T, H, W)


class ModelTracker:
    """The mirror of contrib.ModelTracker: ray-cast from the last pose, align to that render from the last pose,
    integrate at the pose found unless the alignment was lost."""

    def __init__(self, K, height, width, volume, T_first=None, **knobs):
        self.K, self.H, self.W, self.volume = K, height, width, volume
        self.T_first = np.eye(4) if T_first is None else np.asarray(T_first, np.float64)
        self.knobs = dict(CR.DEFAULTS, **knobs)
        self.T_last = None
        self.status = self.stats = None

    def track(self, depth):
        k = self.knobs
        depth = np.asarray(depth, np.float32)
        if self.T_last is None:
            self.volume.integrate(depth, self.K, self.T_first)
            self.T_last = self.T_first.copy()
            return self.T_last
        reference, _ = self.volume.raycast(self.K, self.T_last, self.H, self.W)
        cur = CR.prepare(depth[None], self.K, k["levels"], k["block_band"])
        ref = CR.prepare(reference[None], self.K, k["levels"], k["block_band"])
        _, T, self.status, self.stats = CR.align(cur, ref, self.T_last[None], self.T_last[None], k["iterations"],
                                                  k["distance_threshold"], k["cos_angle_threshold"], k["min_pairs"])
        self.volume.integrate(depth, self.K, T[0], skip=int(self.status[0]))
        self.T_last = T[0]
        return self.T_last
