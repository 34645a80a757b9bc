"""TEST INFRASTRUCTURE: NumPy mirror of csrc/augment.hip -- the generator and every stage, one example at a time.
It is the definition the kernels are held to bit for bit.  Conventions (cv2 and imgaug are not installed: restated
from their sources as remembered, parity with them unpinned -- DESIGN.md "Augmentation"):

  contrast   imgaug LinearContrast on uint8: table[v] = trunc(clip(127 + alpha (v - 127), 0, 255)) in float32
  RGB->HSV   cv2 8-bit: V = max, S = (diff * rint(255 * 4096 / V) + 2048) >> 12, H likewise with
             rint(180 * 4096 / (6 diff)), H in [0, 180)
  multiply   imgaug Multiply on uint8: trunc(clip(v * m, 0, 255)) in float32, for H too (no wrap at 180)
  HSV->RGB   cv2 8-bit: float32 sector formula on h * (6 / 180) wrapped into [0, 6), s / 255, v / 255; rint(x * 255)
  blur       5 taps (imgaug's kernel size rule gives 5 for sigma <= 1), weights rint(256 w) with the centre taking
             the remainder, rows then columns in integers, (sum + 2^15) >> 16, reflect-101; skipped below 1e-3
  resize     to rint(S scale) and back, cv2 INTER_CUBIC 8-bit: a = -0.75, weights short(rint(2048 w)) from
             float32, replicated border, (sum + 2^21) >> 22 saturated; equal sizes: no-op
"""
import numpy as np

from oracle import oracle_np as O

f32 = np.float32
M32 = 0xFFFFFFFF


def philox(seed, key, pixel, stream):
    """Philox4x32-10, key (seed, key), counter (pixel, stream, 0, 0); ``pixel`` an array -> uint32 [..., 4]."""
    c0 = np.asarray(pixel, np.uint64) & M32
    c1 = np.full_like(c0, stream)
    c2, c3 = np.zeros_like(c0), np.zeros_like(c0)
    k0, k1 = int(seed) & M32, int(key) & M32
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = ((p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0)) & M32, p1 & M32, \
            ((p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1)) & M32, p0 & M32
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return np.stack([c0, c1, c2, c3], -1).astype(np.uint32)


def label8(mask):
    """8-connected components: int32 image of canonical ids (a component's first pixel in raster order), -1 outside.
    Min-label hooking and pointer jumping until no pixel has a smaller label next to it."""
    H, W = mask.shape
    N = H * W
    par = np.arange(N + 1)  # parent pointers; N: the background
    flat = mask.ravel()
    idx = np.flatnonzero(flat)
    while True:
        lab = np.where(flat, par[:N], N).reshape(H, W)
        pad = np.pad(lab, 1, constant_values=N)
        m = lab.copy()
        for dy in range(3):
            for dx in range(3):
                m = np.minimum(m, pad[dy:dy + H, dx:dx + W])
        own, low = lab.ravel()[idx], m.ravel()[idx]
        if (low >= own).all():
            return np.where(mask, lab, -1).astype(np.int32)
        np.minimum.at(par, own, low)
        while True:
            nxt = par[par]
            if np.array_equal(nxt, par):
                break
            par = nxt


def augment_mask(rgb, pcd, prm, seed):
    """One example -> dict(rgb, pcd, keep, kept_mask, stats[12], labels, sizes)."""
    S = rgb.shape[0]
    stats = np.zeros(12, np.int32)
    stats[6] = -1
    labels, sizes = np.full((S, S), -1, np.int32), np.zeros((S, S), np.int32)
    empty = dict(rgb=np.zeros_like(rgb), pcd=np.full_like(pcd, np.nan), keep=False, kept_mask=np.zeros((S, S), bool),
                 stats=stats, labels=labels, sizes=sizes)
    mask = ~np.isnan(pcd).any(axis=2)
    if not mask.any():
        return empty
    y1, x1, y2, x2 = _bbox(mask)
    case, u = int(prm[0]), float(prm[1])
    if case == 0:
        y1 = ((y2 - y1) * 0.25) * u
    elif case == 1:
        y2 = S - ((y2 - y1) * 0.25) * u
    elif case == 2:
        x1 = ((x2 - x1) * 0.25) * u
    else:
        x2 = S - ((x2 - x1) * 0.25) * u
    y1, x1, y2, x2 = np.array([y1, x1, y2, x2], np.float64).round().astype(int)
    mask = mask.copy()
    mask[:y1, :] = 0
    mask[y2:, :] = 0
    mask[:, :x1] = 0
    mask[:, x2:] = 0
    stats[8:12] = (y1, x1, y2, x2)
    if not mask.any():
        return empty
    labels = label8(mask)
    ids, counts = np.unique(labels[mask], return_counts=True)  # ids ascending: ties go to the lowest id
    sizes = np.zeros((S, S), np.int32)
    sizes[mask] = counts[np.searchsorted(ids, labels[mask])]
    largest = ids[np.argmax(counts)]
    m = len(ids)
    K = min(int(np.floor(float(prm[2]) * m)), m)
    words = philox(seed, prm[9], ids, 0)[:, 0].astype(np.uint64)
    order = np.argsort((words << np.uint64(16)) | ids.astype(np.uint64), kind="stable")
    chosen = set(ids[order[:K]].tolist()) | {int(largest)}
    kept = mask & np.isin(labels, sorted(chosen))
    rgb2, pcd2 = rgb.copy(), pcd.copy()
    rgb2[~kept] = 0
    pcd2[~kept] = np.nan
    by1, bx1, by2, bx2 = _bbox(kept)
    stats[:8] = (by1, bx1, by2, bx2, m, K, largest, kept.sum())
    rgb3 = O.centerize(rgb2[by1:by2, bx1:bx2], (S, S))
    pcd3 = O.centerize(pcd2[by1:by2, bx1:bx2], (S, S), cval=np.nan, interpolation="nearest")
    return dict(rgb=rgb3, pcd=pcd3, keep=True, kept_mask=kept, stats=stats, labels=labels, sizes=sizes)


def _bbox(mask):
    ys, xs = np.flatnonzero(mask.any(axis=1)), np.flatnonzero(mask.any(axis=0))
    return int(ys[0]), int(xs[0]), int(ys[-1]) + 1, int(xs[-1]) + 1


def _trunc_u8(x):
    return np.clip(x, f32(0), f32(255)).astype(np.int64)


def colour(rgb, alpha, mh, ms, mv):
    """Contrast, RGB -> HSV, multipliers, HSV -> RGB on one uint8 image."""
    alpha, mh, ms, mv = f32(alpha), f32(mh), f32(ms), f32(mv)
    c = _trunc_u8(f32(127) + alpha * (rgb.astype(f32) - f32(127)))
    r, g, b = c[..., 0], c[..., 1], c[..., 2]
    v, vmin = c.max(-1), c.min(-1)
    diff = v - vmin
    with np.errstate(divide="ignore", invalid="ignore"):
        sdiv = np.where(v > 0, np.rint(1044480.0 / v), 0).astype(np.int64)
        hdiv = np.where(diff > 0, np.rint(737280.0 / (6.0 * diff)), 0).astype(np.int64)
    s = (diff * sdiv + 2048) >> 12
    h = np.where(v == r, g - b, np.where(v == g, b - r + 2 * diff, r - g + 4 * diff))
    h = (h * hdiv + 2048) >> 12
    h = np.where(h < 0, h + 180, h)
    s, v, h = _trunc_u8(s.astype(f32) * ms), _trunc_u8(v.astype(f32) * mv), _trunc_u8(h.astype(f32) * mh)
    fs, fv = s.astype(f32) * (f32(1) / f32(255)), v.astype(f32) * (f32(1) / f32(255))
    fh = h.astype(f32) * (f32(6) / f32(180))
    for _ in range(2):  # h <= 255: at most 8.5, one subtraction; the loop is the kernel's `while`
        fh = np.where(fh >= f32(6), fh - f32(6), fh).astype(f32)
    sector = np.floor(fh).astype(np.int64)
    fh = (fh - sector.astype(f32)).astype(f32)
    one = f32(1)
    tab = np.stack([fv, fv * (one - fs), fv * (one - fs * fh), fv * (one - fs * (one - fh))], -1).astype(f32)
    sector_data = np.array([[1, 3, 0], [1, 0, 2], [3, 0, 1], [0, 2, 1], [0, 1, 3], [2, 1, 0]])  # b, g, r
    idx = sector_data[sector]
    pick = lambda k: np.take_along_axis(tab, idx[..., k:k + 1], -1)[..., 0]  # noqa: E731
    fb, fg, fr = pick(0), pick(1), pick(2)
    grey = s == 0
    out = np.stack([np.where(grey, fv, fr), np.where(grey, fv, fg), np.where(grey, fv, fb)], -1).astype(f32)
    return np.clip(np.rint(out * f32(255)), 0, 255).astype(np.uint8)


def blur_weights(sigma):
    e1, e2 = np.exp(-1.0 / (2.0 * sigma * sigma)), np.exp(-4.0 / (2.0 * sigma * sigma))
    total = 1.0 + 2.0 * e1 + 2.0 * e2
    q1, q2 = int(np.rint(e1 / total * 256.0)), int(np.rint(e2 / total * 256.0))
    return np.array([q2, q1, 256 - 2 * q1 - 2 * q2, q1, q2], np.int64)


def blur(img, sigma):
    if sigma < 1e-3:
        return img.copy()
    q = blur_weights(sigma)
    a = np.pad(img.astype(np.int64), ((2, 2), (2, 2), (0, 0)), mode="reflect")
    H, W = img.shape[:2]
    h = sum(q[k] * a[:, k:k + W] for k in range(5))
    v = sum(q[j] * h[j:j + H] for j in range(5))
    return ((v + 32768) >> 16).astype(np.uint8)


def _cubic_taps(n_dst, scale, n_src):
    d = np.arange(n_dst, dtype=np.float64)
    f = ((d + 0.5) * scale - 0.5).astype(f32)
    s = np.floor(f).astype(np.int64)
    f = (f - s.astype(f32)).astype(f32)
    A, one = f32(-0.75), f32(1)
    c0 = ((A * (f + one) - f32(5) * A) * (f + one) + f32(8) * A) * (f + one) - f32(4) * A
    c1 = ((A + f32(2)) * f - (A + f32(3))) * f * f + one
    g = one - f
    c2 = ((A + f32(2)) * g - (A + f32(3))) * g * g + one
    c3 = one - c0 - c1 - c2
    w = np.rint(np.stack([c0, c1, c2, c3], -1).astype(f32) * f32(2048)).astype(np.int64)
    idx = np.clip(s[:, None] + np.arange(-1, 3)[None, :], 0, n_src - 1)
    return idx, w


def resize_cubic(img, size):
    n_src = img.shape[0]
    if size == n_src:
        return img.copy()
    scale = 1.0 / (float(size) / float(n_src))
    idx, w = _cubic_taps(size, scale, n_src)
    a = img.astype(np.int64)
    h = sum(w[None, :, k, None] * a[:, idx[:, k]] for k in range(4))          # [n_src, size, 3]
    v = sum(w[:, j, None, None] * h[idx[:, j]] for j in range(4))              # [size, size, 3]
    return np.clip((v + (1 << 21)) >> 22, 0, 255).astype(np.uint8)


def resized(S, scale):
    return min(max(int(np.rint(S * float(scale))), 1), S)


def augment_rgb(rgb, prm, stage="all"):
    S = rgb.shape[0]
    out = colour(rgb, prm[3], prm[4], prm[5], prm[6])
    if stage == "colour":
        return out
    out = blur(out, float(prm[7]))
    if stage == "blur":
        return out
    return resize_cubic(resize_cubic(out, resized(S, prm[8])), S)


def normals(seed, key, npix):
    """float64 [npix, 3]: Box-Muller on 53-bit uniforms from streams 2 and 3."""
    p = np.arange(npix)
    u53 = lambda a, b: (a >> np.uint32(5)).astype(np.float64) * 67108864.0 + (b >> np.uint32(6)).astype(np.float64)  # noqa: E731
    z = []
    for stream in (2, 3):
        w = philox(seed, key, p, stream)
        r = np.sqrt(-2.0 * np.log((u53(w[:, 0], w[:, 1]) + 1.0) * (1.0 / 9007199254740992.0)))
        t = 6.283185307179586 * (u53(w[:, 2], w[:, 3]) * (1.0 / 9007199254740992.0))
        z += [r * np.cos(t), r * np.sin(t)]
    return np.stack(z[:3], -1)


def dropout(seed, key, npix):
    return philox(seed, key, np.arange(npix), 1)[:, 0] < np.uint32(214748365)


def augment_pcd(pcd, prm, seed):
    S = pcd.shape[0]
    drop = dropout(seed, prm[9], S * S).reshape(S, S)
    z = normals(seed, prm[9], S * S).reshape(S, S, 3)
    out = (pcd.astype(np.float64) + 0.003 * z).astype(pcd.dtype)
    out[drop] = np.nan
    return out, drop


def augment_rgbd(rgb, pcd, params, seed):
    """Batch mirror of datasets.augmentation.augment_rgbd given the table and the seed."""
    outs = []
    for i in range(len(rgb)):
        m = augment_mask(rgb[i], pcd[i], params[i], seed)
        outs.append((augment_rgb(m["rgb"], params[i]), augment_pcd(m["pcd"], params[i], seed)[0], m["keep"]))
    return tuple(np.stack(x) for x in zip(*outs))
