"""TEST INFRASTRUCTURE: NumPy mirror of csrc/posemetric.hip's arithmetic contract (DESIGN.md "Pose metric"), float64,
nothing fused:

* transform  x' = ((R00 x + R01 y) + R02 z) + tx, rows y and z likewise; the + t dropped without ``translate``;
* squared distance (dx dx + dy dy) + dz dz; ADD-S: the minimum of the squares, then one sqrt;
* mean: lane l of 256 adds the distances of the points j = l, l + 256, ... in increasing j, the 256 partial sums are
  folded by s[l] += s[l + h] for h = 128, 64, ... 1, and the result is divided by P.
"""
import numpy as np

LANES = 256


def transform(points, T, translate=True):
    p = np.asarray(points, np.float64)
    T = np.asarray(T, np.float64)
    out = np.empty_like(p)
    for a in range(3):
        v = (T[a, 0] * p[:, 0] + T[a, 1] * p[:, 1]) + T[a, 2] * p[:, 2]
        out[:, a] = v + T[a, 3] if translate else v
    return out


def sq_dist(a, b):
    d = a - b
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def fixed_mean(d):
    P = d.shape[0]
    rows = -(-P // LANES)
    padded = np.zeros(rows * LANES, np.float64)
    padded[:P] = d
    s = np.zeros(LANES, np.float64)
    for r in range(rows):  # (adding the pad's + 0.0 leaves every bit of a non-negative sum alone)
        s = s + padded[r * LANES:(r + 1) * LANES]
    half = LANES // 2
    while half >= 1:
        s[:half] = s[:half] + s[half:2 * half]
        half //= 2
    return s[0] / np.float64(P)


def pair(points, T1, T2, translate=True, chunk=512):
    a, b = transform(points, T1, translate), transform(points, T2, translate)
    add = np.sqrt(sq_dist(a, b))
    best = np.empty(a.shape[0], np.float64)
    for lo in range(0, a.shape[0], chunk):
        best[lo:lo + chunk] = sq_dist(a[lo:lo + chunk, None, :], b[None, :, :]).min(axis=1)
    return fixed_mean(add), fixed_mean(np.sqrt(best))


def average_distance(points, transform1, transform2, translate=True, cloud_index=None):
    index = range(len(points)) if cloud_index is None else cloud_index
    pairs = [pair(points[c], transform1[i], transform2[i], translate) for i, c in enumerate(index)]
    return (np.array([p[0] for p in pairs], np.float64).reshape(len(pairs)),
            np.array([p[1] for p in pairs], np.float64).reshape(len(pairs)))
