"""TEST INFRASTRUCTURE: NumPy mirror of the TSDF labels (include/mfhip.h "TSDF labels"), written from that description:
the labelled integrate, the label image, the instance statistics and the published grids, every float64 expression
associated as the header writes it, and the host arithmetic of contrib.InstanceTsdfVolume on top.  Bitwise equal to
csrc/tsdflabel.hip.  Every NumPy operation on coordinates is one IEEE operation per element (no np.sum, no dot, no
fused step); the statistics are integer sums, which have no order."""
import numpy as np

import tsdf_ref as R

MAX_INSTANCES = 64
# what a voxel did in a labelled integrate: the first reason for not voting, or the kind of vote (-1: skip word set)
NOT_UPDATED, FAR, UNCERTAIN, ZERO, BELOW, CLAIM, AGREE, SATURATE, DECREMENT, RELEASE = range(10)
# what an output voxel of publish_grids is
GROUND, OUTSIDE, UNDER_WEIGHT, TARGET, OTHER, BACKGROUND, UNOWNED, FREE, BETWEEN = range(9)


def fresh_labels(dims):
    nx, ny, nz = dims
    return np.zeros((nz, ny, nx, 2), np.int32)


def _intrinsics(K):
    return float(K[0][0]), float(K[1][1]), float(K[0][2]), float(K[1][2])


def _rigid(T, p):
    """T p of the header: ((T[a, 0] p_x + T[a, 1] p_y) + T[a, 2] p_z) + T[a, 3] per axis."""
    T = np.asarray(T, np.float64).reshape(4, 4)
    return [((T[a, 0] * p[0] + T[a, 1] * p[1]) + T[a, 2] * p[2]) + T[a, 3] for a in range(3)]


def _voxel_of(m, origin, pitch, dims):
    """-> (inside bool, flat voxel index int64 (0 outside))."""
    g = [np.floor((m[a] - float(origin[a])) / float(pitch) + 0.5) for a in range(3)]
    inside = np.ones(np.shape(g[0]), bool)
    for a in range(3):
        inside &= (g[a] >= 0.0) & (g[a] <= float(dims[a] - 1))
    nx, ny, _ = dims
    flat = np.where(inside, (g[2] * ny + g[1]) * nx + g[0], 0.0).astype(np.int64)
    return inside, flat


def inverse_pose(T):
    """T_map_to_sensor of T_sensor_to_map in float64: R^T and -R^T t, every sum left to right."""
    T = np.asarray(T, np.float64).reshape(4, 4)
    inv = np.eye(4)
    for a in range(3):
        for b in range(3):
            inv[a, b] = T[b, a]
        inv[a, 3] = -((T[0, a] * T[0, 3] + T[1, a] * T[1, 3]) + T[2, a] * T[2, 3])
    return inv


def integrate_labels(vol, labels, origin, pitch, truncation, max_weight, depth, K, T, label_image, max_count, skip=0):
    """In place on ``vol`` and ``labels`` -> int8 [nz, ny, nx]: what every voxel's vote was (NOT_UPDATED .. RELEASE),
    -1 everywhere if ``skip`` is nonzero."""
    nz, ny, nx = vol.shape[:3]
    assert max_count >= 1 and labels.shape == (nz, ny, nx, 2) and labels.dtype == np.int32
    outcome = R.integrate(vol, origin, pitch, truncation, max_weight, depth, K, T, skip)
    vote = np.full((nz, ny, nx), -1, np.int8)
    if skip != 0:
        return vote
    updated = outcome == R.UPDATED
    depth = np.asarray(depth, np.float32)
    label_image = np.asarray(label_image, np.int32)
    H, W = depth.shape
    assert label_image.shape == (H, W)
    fx, fy, cx, cy = _intrinsics(K)
    T = np.asarray(T, np.float64).reshape(4, 4)
    Rm, t = T[:3, :3], T[:3, 3]
    pitch, truncation = float(pitch), float(truncation)
    k, j, i = np.meshgrid(np.arange(nz, dtype=np.float64), np.arange(ny, dtype=np.float64),
                          np.arange(nx, dtype=np.float64), indexing="ij")
    with np.errstate(all="ignore"):  # the header's formulas of mf_tsdf_integrate, once more, for (row, col) and sdf
        e0 = (float(origin[0]) + pitch * i) - t[0]
        e1 = (float(origin[1]) + pitch * j) - t[1]
        e2 = (float(origin[2]) + pitch * k) - t[2]
        x = (Rm[0, 0] * e0 + Rm[1, 0] * e1) + Rm[2, 0] * e2
        y = (Rm[0, 1] * e0 + Rm[1, 1] * e1) + Rm[2, 1] * e2
        z = (Rm[0, 2] * e0 + Rm[1, 2] * e1) + Rm[2, 2] * e2
        col = np.floor((fx * (x / z) + cx) + 0.5)
        row = np.floor((fy * (y / z) + cy) + 0.5)
        idx = np.where(updated, row * W + col, 0.0).astype(np.int64)
        sdf = depth.reshape(-1)[idx].astype(np.float64) - z
    v = label_image.reshape(-1)[idx]
    near = updated & (sdf <= truncation)
    votes = near & ((v >= 1) | (v == -1))
    vote[:] = NOT_UPDATED
    vote[updated & ~near] = FAR
    vote[near & (v == -2)] = UNCERTAIN
    vote[near & (v == 0)] = ZERO
    vote[near & (v < -2)] = BELOW
    label, count = labels[..., 0], labels[..., 1]
    claim = votes & (count == 0)
    agree = votes & ~claim & (label == v)
    differ = votes & ~claim & ~agree
    vote[claim] = CLAIM
    vote[agree & (count + 1 <= max_count)] = AGREE
    vote[agree & (count + 1 > max_count)] = SATURATE
    vote[differ & (count > 1)] = DECREMENT
    vote[differ & (count == 1)] = RELEASE
    new_count = np.where(claim, 1, np.where(agree, np.minimum(count + 1, max_count), np.where(differ, count - 1, count)))
    new_label = np.where(claim, v, np.where(differ & (new_count == 0), 0, label))
    labels[..., 0], labels[..., 1] = new_label.astype(np.int32), new_count.astype(np.int32)
    return vote


def label_image(labels, origin, pitch, depth, K, T, min_count=1):
    """-> int32 [H, W]."""
    nz, ny, nx = labels.shape[:3]
    depth = np.asarray(depth, np.float32)
    H, W = depth.shape
    fx, fy, cx, cy = _intrinsics(K)
    row, col = np.mgrid[:H, :W]
    with np.errstate(all="ignore"):
        d = depth.astype(np.float64)
        seen = d > 0.0
        q0, q1 = (col.astype(np.float64) - cx) / fx, (row.astype(np.float64) - cy) / fy
        m = _rigid(T, [q0 * d, q1 * d, d])
        inside, flat = _voxel_of(m, origin, pitch, (nx, ny, nz))
    pair = labels.reshape(-1, 2)[flat]
    return np.where(seen & inside & (pair[..., 1] >= min_count), pair[..., 0], 0).astype(np.int32)


def instance_stats(vol, labels, min_weight, min_count, ids):
    """-> int64 [B, 10]: {count, sum i, j, k, min i, j, k, max i, j, k} per id."""
    nz, ny, nx = vol.shape[:3]
    ids = np.asarray(ids, np.int32)
    assert 1 <= len(ids) <= MAX_INSTANCES and (np.diff(ids.astype(np.int64)) > 0).all()
    table = np.zeros((len(ids), 10), np.int64)
    table[:, 4:7], table[:, 7:10] = (nx, ny, nz), -1
    solid = (vol[..., 1].astype(np.float64) >= float(min_weight)) & (vol[..., 0] <= 0) & (labels[..., 1] >= min_count)
    for b, i in enumerate(ids):
        k, j, i_ = np.nonzero(solid & (labels[..., 0] == i))
        if k.size:
            idx = np.stack([i_, j, k], 1).astype(np.int64)
            table[b] = np.concatenate([[k.size], idx.sum(0), idx.min(0), idx.max(0)])
    return table


def stats_in_map_frame(table, origin, pitch):
    """The host half of InstanceTsdfVolume.instance_stats: -> dict(count int64 [B], center, bbx_min, bbx_max float64
    [B, 3]); ``origin + pitch * (sum / count)`` and ``origin + pitch * min`` / ``max``, NaN for an id without voxels."""
    table = np.asarray(table, np.int64)
    count = table[:, 0].copy()
    origin, empty = np.asarray(origin, np.float64), (count == 0)[:, None]
    with np.errstate(all="ignore"):
        center = origin + float(pitch) * (table[:, 1:4].astype(np.float64) / count[:, None].astype(np.float64))
    lo = origin + float(pitch) * table[:, 4:7].astype(np.float64)
    hi = origin + float(pitch) * table[:, 7:10].astype(np.float64)
    return dict(count=count, center=np.where(empty, np.nan, center), bbx_min=np.where(empty, np.nan, lo),
                bbx_max=np.where(empty, np.nan, hi))


def publish_grids(vol, labels, origin, pitch, ids, grid_pitch, centers, T_map_to_sensor, T_sensor_to_map, min_weight,
                  min_count, empty_above, ground_z, flags, D):
    """-> dict(origin float64 [B, 3], grid_target, grid_noentry float32 [B, D, D, D], grid_nontarget_empty uint8,
    outcome int8 [B, D, D, D] (GROUND .. BETWEEN))."""
    nz, ny, nx = vol.shape[:3]
    ids, B = np.asarray(ids, np.int32), len(ids)
    grid_pitch, centers = np.asarray(grid_pitch, np.float64), np.asarray(centers, np.float64).reshape(B, 3)
    out_origin = np.zeros((B, 3))
    gt, ne = np.zeros((B, D, D, D), np.float32), np.zeros((B, D, D, D), np.float32)
    outcome = np.zeros((B, D, D, D), np.int8)
    index = np.meshgrid(*[np.arange(D, dtype=np.float64)] * 3, indexing="ij")  # [x][y][z]
    tsdf, weight, pair = vol[..., 0].reshape(-1), vol[..., 1].reshape(-1), labels.reshape(-1, 2)
    for b in range(B):
        p = float(grid_pitch[b])
        centre = _rigid(T_map_to_sensor, [float(c) for c in centers[b]])
        with np.errstate(all="ignore"):
            for a in range(3):
                out_origin[b, a] = centre[a] - (float(D) / 2.0 - 0.5) * p
            s = [out_origin[b, a] + p * index[a] for a in range(3)]
            m = _rigid(T_sensor_to_map, s)
            ground = np.full((D, D, D), bool(flags & 1)) & (m[2] < float(ground_z))
            inside, flat = _voxel_of(m, origin, pitch, (nx, ny, nz))
        F, w, (l, c) = tsdf[flat], weight[flat].astype(np.float64), (pair[flat][..., 0], pair[flat][..., 1])
        known = ~ground & inside & (w >= float(min_weight))
        solid = known & (F <= 0)
        owned = solid & (c >= min_count)
        target = owned & (l == ids[b])
        other = owned & ~target & (l != 0)
        free = known & ~solid & bool(flags & 2) & (F.astype(np.float64) >= float(empty_above))
        o = np.full((D, D, D), BETWEEN, np.int8)
        o[ground], o[~ground & ~inside], o[~ground & inside & ~known] = GROUND, OUTSIDE, UNDER_WEIGHT
        o[solid & ~target & ~other], o[target], o[other & (l >= 1)], o[other & (l < 0)] = UNOWNED, TARGET, OTHER, BACKGROUND
        o[free] = FREE
        outcome[b] = o
        gt[b] = target
        ne[b] = ground | other | free
    return dict(origin=out_origin, grid_target=gt, grid_noentry=ne, grid_nontarget_empty=(ne != 0).astype(np.uint8),
                outcome=outcome)


class InstanceVolume(R.Volume):
    """The mirror of contrib.InstanceTsdfVolume."""

    def __init__(self, dims, pitch, origin, truncation=None, max_weight=64.0, max_count=64):
        super().__init__(dims, pitch, origin, truncation, max_weight)
        self.max_count = int(max_count)
        self.labels = fresh_labels(self.dims)

    def integrate(self, depth, K, T, label=None, skip=0):
        if label is None:
            return super().integrate(depth, K, T, skip)
        return integrate_labels(self.volume, self.labels, self.origin, self.pitch, self.truncation, self.max_weight,
                                depth, K, T, label, self.max_count, skip)

    def label_image(self, depth, K, T, min_count=1):
        return label_image(self.labels, self.origin, self.pitch, depth, K, T, min_count)

    def instance_table(self, ids, min_weight=1.0, min_count=1):
        return instance_stats(self.volume, self.labels, min_weight, min_count, ids)

    def instance_stats(self, ids, min_weight=1.0, min_count=1):
        return stats_in_map_frame(self.instance_table(ids, min_weight, min_count), self.origin, self.pitch)

    def publish_grids(self, T_sensor_to_map, instance_ids, pitch, centers, dim=32, min_weight=1.0, min_count=1,
                      empty_above=0.5, ground_z=None, free_as_noentry=True):
        """``pitch``: per id, rounded to float32 as the product returns it."""
        flags = (0 if ground_z is None else 1) | (2 if free_as_noentry else 0)
        grid_pitch = np.asarray(pitch, np.float32).astype(np.float64)
        return publish_grids(self.volume, self.labels, self.origin, self.pitch, instance_ids, grid_pitch, centers,
                             inverse_pose(T_sensor_to_map), T_sensor_to_map, min_weight, min_count, empty_above,
                             0.0 if ground_z is None else ground_z, flags, dim)
