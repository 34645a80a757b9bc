"""TEST INFRASTRUCTURE: NumPy mirror of the TSDF colour (include/mfhip.h "TSDF colour"), written from that description:
the coloured integrate, SAMPLE, the colour image and the sampled points, every float64 expression associated as the
header writes it.  Bitwise equal to csrc/tsdfcolor.hip.  Every NumPy operation on coordinates and colours is one IEEE
operation per element (no np.sum, no dot, no fused step).  Which voxels a frame writes is asked of the existing mirror
(tests/tsdf_ref.py ``integrate`` on a scratch volume: the requirements read the depth alone), so the set that takes a
colour is by construction a subset of the one ``mf_tsdf_integrate`` writes."""
import numpy as np

import tsdf_ref as R
import tsdflabel_ref as LR

# what a voxel did in a coloured integrate (-1: skip word set)
NOT_UPDATED, FAR, COLOURED, SATURATED = range(4)


def fresh_colors(dims):
    nx, ny, nz = dims
    return np.zeros((nz, ny, nx, 4), np.float32)


def integrate_colors(colors, origin, pitch, truncation, max_weight, depth, rgb, K, T, skip=0):
    """In place on ``colors`` float32 [nz, ny, nx, 4] -> int8 [nz, ny, nx]: NOT_UPDATED .. SATURATED per voxel, -1
    everywhere if ``skip`` is nonzero."""
    nz, ny, nx = colors.shape[:3]
    assert colors.shape == (nz, ny, nx, 4) and colors.dtype == np.float32
    outcome = R.integrate(R.fresh((nx, ny, nz)), origin, pitch, truncation, max_weight, depth, K, T, skip)
    what = np.full((nz, ny, nx), -1, np.int8)
    if skip != 0:
        return what
    updated = outcome == R.UPDATED
    depth, rgb = np.asarray(depth, np.float32), np.asarray(rgb)
    H, W = depth.shape
    assert rgb.shape == (H, W, 3) and rgb.dtype == np.uint8
    fx, fy, cx, cy = LR._intrinsics(K)
    T = np.asarray(T, np.float64).reshape(4, 4)
    Rm, t = T[:3, :3], T[:3, 3]
    pitch, truncation, max_weight = float(pitch), float(truncation), float(max_weight)
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
        near = updated & (sdf <= truncation)
        pixel = rgb.reshape(-1, 3)[idx]
        Wc = colors[..., 3].astype(np.float64)
        w = Wc + 1.0
        for c in range(3):
            C = (colors[..., c].astype(np.float64) * Wc + pixel[..., c].astype(np.float64)) / w
            colors[..., c] = np.where(near, C.astype(np.float32), colors[..., c])
        capped = w > max_weight
        w = np.where(capped, max_weight, w)
        colors[..., 3] = np.where(near, w.astype(np.float32), colors[..., 3])
    what[:] = NOT_UPDATED
    what[updated & ~near] = FAR
    what[near] = COLOURED
    what[near & capped] = SATURATED
    return what


def _quantise(x):
    q = np.floor(x + 0.5)
    q = np.where(q >= 0.0, q, 0.0)
    return np.where(q > 255.0, 255.0, q).astype(np.uint8)


def sample(colors, origin, pitch, m, return_corners=False):
    """SAMPLE at the map-frame points ``m`` = [m_x, m_y, m_z] (arrays of one shape) -> uint8 [..., 4]; with
    ``return_corners`` also (usable bool [...], the number of coloured corners int [...], 0 where not usable)."""
    nz, ny, nx = colors.shape[:3]
    dims, pitch = (nx, ny, nz), float(pitch)
    flat = colors.reshape(-1, 4)
    with np.errstate(all="ignore"):
        g = [(np.asarray(m[a], np.float64) - float(origin[a])) / pitch for a in range(3)]
        b = [np.floor(x) for x in g]
        usable = np.ones(np.shape(g[0]), bool)
        for a in range(3):
            usable &= (b[a] >= 0.0) & (b[a] <= float(dims[a] - 2))
        r = [g[a] - b[a] for a in range(3)]
        wgt = [(1.0 - r[a], r[a]) for a in range(3)]
        base = np.where(usable, (b[2] * ny + b[1]) * nx + b[0], 0.0).astype(np.int64)
        S, A = np.zeros(base.shape), [np.zeros(base.shape) for _ in range(3)]
        n_coloured = np.zeros(base.shape, np.int64)
        for dx in (0, 1):
            for dy in (0, 1):
                for dz in (0, 1):
                    C = flat[base + (dz * ny + dy) * nx + dx]
                    w = (wgt[0][dx] * wgt[1][dy]) * wgt[2][dz]
                    has = usable & (C[..., 3] > 0)
                    n_coloured += has
                    S = np.where(has, S + w, S)
                    for c in range(3):
                        A[c] = np.where(has, A[c] + w * C[..., c].astype(np.float64), A[c])
        ok = usable & (S > 0.0)
        out = np.zeros(base.shape + (4,), np.uint8)
        for c in range(3):
            out[..., c] = np.where(ok, _quantise(A[c] / S), 0)
        out[..., 3] = np.where(ok, 255, 0)
    return (out, usable, n_coloured) if return_corners else out


def color_image(colors, origin, pitch, depth, K, T):
    """-> uint8 [H, W, 4]."""
    depth = np.asarray(depth, np.float32)
    H, W = depth.shape
    fx, fy, cx, cy = LR._intrinsics(K)
    row, col = np.mgrid[:H, :W]
    with np.errstate(all="ignore"):
        d = depth.astype(np.float64)
        seen = d > 0.0
        q0, q1 = (col.astype(np.float64) - cx) / fx, (row.astype(np.float64) - cy) / fy
        m = LR._rigid(T, [q0 * d, q1 * d, d])
    return np.where(seen[..., None], sample(colors, origin, pitch, m), 0).astype(np.uint8)


def sample_colors(colors, origin, pitch, points):
    """points float64 [N, 3] -> uint8 [N, 4]."""
    points = np.asarray(points, np.float64).reshape(-1, 3)
    return sample(colors, origin, pitch, [points[:, 0], points[:, 1], points[:, 2]])


class ColorVolume(LR.InstanceVolume):
    """The mirror of contrib.InstanceTsdfVolume(colors=True) (and, with label=None throughout, of
    contrib.TsdfVolume(colors=True))."""

    def __init__(self, dims, pitch, origin, truncation=None, max_weight=64.0, max_count=64):
        super().__init__(dims, pitch, origin, truncation, max_weight, max_count)
        self.colors = fresh_colors(self.dims)

    def integrate(self, depth, K, T, label=None, skip=0, color=None):
        out = super().integrate(depth, K, T, label=label, skip=skip)
        if color is None:
            return out
        return integrate_colors(self.colors, self.origin, self.pitch, self.truncation, self.max_weight, depth, color,
                                K, T, skip)

    def color_image(self, depth, K, T):
        return color_image(self.colors, self.origin, self.pitch, depth, K, T)

    def sample_colors(self, points):
        return sample_colors(self.colors, self.origin, self.pitch, points)
