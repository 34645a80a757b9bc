"""TEST INFRASTRUCTURE: float64 references of the 2-D decoder's elementwise and gather kernels
(csrc/backbone2d.hip, the row kernels of csrc/psp_tail.hip) with the absolute-value contraction ``S`` that the
per-element bound of tests/bf16_bound.py needs:

    fp32 result   |got - ref| <= 2 K 2^-24 S          bf16 result   ... + 2^-8 |ref|

What belongs to an operator's DEFINITION is mirrored here in NumPy float32, operation for operation -- the bilinear
source coordinate and its weights (torch's area_pixel_compute_scale for align_corners: ``scale = fl((in-1)/(out-1))``,
0 for one output; ``s = fl(scale * o)``, ``i0 = int(s)``, ``i1 = i0 + (i0 < in-1)``, ``l1 = s - i0`` (exact),
``l0 = fl(1 - l1)``), and for the tail rows the taps of ``PSPNetExtractor._tail_taps``.  Everything behind the weights
is float64 on the bf16 / fp32-rounded inputs: per-axis dense matrices Wy [Ho, H] and Wx [Wo, W], the forward
``Wy x Wx^T``, the backward ``Wy^T gy Wx`` -- the exact transpose -- and S the same contraction on absolute values.
K is the number of fp32 roundings on the longest chain of the kernel as written; every caller states its own.
An element with S == 0 (nothing reaches it, or only through weights that are exactly 0) must be exact.

The mirror against torch (``test_resize_mirror_vs_torch_float64`` in tests/test_emul_backbone2d.py).
``F.interpolate(x.double(), align_corners=True)`` takes the same coordinate in float64.  The float32 coordinate
``fl(fl(scale) * o)`` carries two roundings: |ds| <= 2 * 2^-24 * s <= 2^-23 * max(H, W).  Bilinear interpolation is
continuous and piecewise linear in s with slope (x[i+1] - x[i]) per axis (across an integer the pair of taps changes,
the value does not), so moving s by ds moves each of the two weights of that axis by at most |ds|; ``l0 = fl(1 - l1)``
adds one rounding <= 2^-24.  With dw = 2^-23 * max(H, W) + 2^-24 per axis, an output pixel (a product of two
two-tap rows) moves by at most 2 (dw_y + dw_x) max|x|, and an input-gradient pixel by that times the number of
output pixels that reach it -- ``mirror_allowance`` below, derived from the formats, not from any result.
"""
import numpy as np
import torch

import bf16_bound as BB


def f64(t):
    return t.detach().double().cpu().numpy()


def axis_taps(n_in, n_out):
    """-> (i0, i1 int64 [n_out]; l0, l1 float32 [n_out]) of one axis, the kernels' float32 arithmetic."""
    scale = np.float32(n_in - 1) / np.float32(n_out - 1) if n_out > 1 else np.float32(0.0)
    s = (scale * np.arange(n_out, dtype=np.float32)).astype(np.float32)
    i0 = s.astype(np.int32)                      # (truncation; s >= 0)
    i1 = i0 + (i0 < n_in - 1)
    l1 = (s - i0.astype(np.float32)).astype(np.float32)
    l0 = (np.float32(1.0) - l1).astype(np.float32)
    return i0.astype(np.int64), i1.astype(np.int64), l0, l1


def axis_matrix(n_in, n_out):
    """-> (Wm float64 [n_out, n_in], hits int64 [n_out, n_in]): the weights and how many taps of output o land on
    input i (0, 1 or 2; a tap with weight 0 still counts -- the kernels add it)."""
    i0, i1, l0, l1 = axis_taps(n_in, n_out)
    Wm, hits = np.zeros((n_out, n_in)), np.zeros((n_out, n_in), np.int64)
    o = np.arange(n_out)
    np.add.at(Wm, (o, i0), l0.astype(np.float64))
    np.add.at(Wm, (o, i1), l1.astype(np.float64))
    np.add.at(hits, (o, i0), 1)
    np.add.at(hits, (o, i1), 1)
    return Wm, hits


def resize_fwd_ref(x, Ho, Wo):
    """x [B, C, H, W] (any dtype) -> (ref, S) float64 tensors [B, C, Ho, Wo]."""
    x = f64(x)
    Wy, Wx = axis_matrix(x.shape[2], Ho)[0], axis_matrix(x.shape[3], Wo)[0]
    ref = np.einsum("oh,bchw,pw->bcop", Wy, x, Wx, optimize=True)
    S = np.einsum("oh,bchw,pw->bcop", Wy, np.abs(x), Wx, optimize=True)   # (the weights are >= 0)
    return torch.from_numpy(ref), torch.from_numpy(S)


def resize_bwd_ref(gy, H, W):
    """gy [B, C, Ho, Wo] -> (ref, S) float64 tensors [B, C, H, W]: the transpose of the forward map."""
    gy = f64(gy)
    Wy, Wx = axis_matrix(H, gy.shape[2])[0], axis_matrix(W, gy.shape[3])[0]
    ref = np.einsum("oh,bcop,pw->bchw", Wy, gy, Wx, optimize=True)
    S = np.einsum("oh,bcop,pw->bchw", Wy, np.abs(gy), Wx, optimize=True)
    return torch.from_numpy(ref), torch.from_numpy(S)


def resize_bwd_addends(H, W, Ho, Wo):
    """The largest number of output pixels any input pixel sums (pixels that reach it with weight 0 included)."""
    ny = (axis_matrix(H, Ho)[1] > 0).sum(0).max()
    nx = (axis_matrix(W, Wo)[1] > 0).sum(0).max()
    return int(ny) * int(nx)


def mirror_allowance(H, W, Ho, Wo, xmax, gmax):
    """(forward, backward) allowance of the float32 mirror against torch's float64 coordinate (module docstring)."""
    dw = 2.0 ** -23 * max(H, W) + 2.0 ** -24
    fwd = 2.0 * (dw + dw) * xmax
    return fwd, 2.0 * (dw + dw) * gmax * resize_bwd_addends(H, W, Ho, Wo)


def prelu_ref(x, dy, a):
    """-> dx (ref, S) [like x] and dslope (ref, S) [1]: x <= 0 (and -0.0) takes the slope side."""
    x, dy = f64(x), f64(dy)
    neg = ~(x > 0)
    dx = np.where(neg, a * dy, dy)
    prod = np.where(neg, dy * x, 0.0)
    return (torch.from_numpy(dx), torch.from_numpy(np.abs(dx)),
            torch.tensor([prod.sum()], dtype=torch.float64), torch.tensor([np.abs(prod).sum()], dtype=torch.float64))


def bn_ref(x, identity, mean, var, weight, bias, eps, relu, caxis):
    """((x - mean) * (weight / sqrt(var + eps)) + bias (+ identity)) in float64, channels along ``caxis`` of x;
    eps is taken as the float32 the ABI passes.  -> (ref, S)."""
    x = f64(x)
    shape = [1] * x.ndim
    shape[caxis] = -1
    m, v, w, b = (f64(t).reshape(shape) for t in (mean, var, weight, bias))
    sc = w / np.sqrt(v + float(np.float32(eps)))
    ref, S = (x - m) * sc + b, np.abs(x - m) * np.abs(sc) + np.abs(b)
    if identity is not None:
        ref, S = ref + f64(identity), S + np.abs(f64(identity))
    if relu:
        ref = np.maximum(ref, 0.0)     # 1-Lipschitz, applied before the rounding: the bound holds behind it
    return torch.from_numpy(ref), torch.from_numpy(S)


def tail_rows_fwd_f32(u, taps):
    """The window rows in the float32 formulation of PSPNetExtractor._tail (taps, four gathers, blend), from the
    channels-last map u [B, H, W, 64] (bf16 values in float32) -> [B * P, 576] float32, column c * 9 + k."""
    B, H, W, C = u.shape
    P = taps["P"]
    flat = u.reshape(B, H * W, C)

    def tap(iy, ix):
        return torch.gather(flat, 1, (iy * W + ix)[:, :, None].expand(B, P * 9, C))
    ly, lx = taps["ly"][:, :, None], taps["lx"][:, :, None]
    up = (1 - ly) * ((1 - lx) * tap(taps["y0"], taps["x0"]) + lx * tap(taps["y0"], taps["x1"])) + \
        ly * ((1 - lx) * tap(taps["y1"], taps["x0"]) + lx * tap(taps["y1"], taps["x1"]))
    return (up * taps["valid"][:, :, None]).reshape(B * P, 9, C).permute(0, 2, 1).reshape(B * P, 9 * C)


def tail_rows_bwd_ref(grows, taps, B, H, W):
    """The exact transpose of the forward map in float64: grows [B * P, 576] -> (ref, S, hits) [B, H, W, 64]; the
    weights are the float32 ``1 - l`` and ``l`` of the taps, multiplied in float64; ``hits`` counts the
    (sample, window element, corner) contributions that reach each source pixel."""
    P, C = taps["P"], 64
    g = f64(grows).reshape(B, P, C, 9).transpose(0, 1, 3, 2).reshape(B, P * 9, C)
    ly, lx = taps["ly"].float().numpy(), taps["lx"].float().numpy()
    wy = ((np.float32(1.0) - ly).astype(np.float64), ly.astype(np.float64))
    wx = ((np.float32(1.0) - lx).astype(np.float64), lx.astype(np.float64))
    ys, xs = (taps["y0"].numpy(), taps["y1"].numpy()), (taps["x0"].numpy(), taps["x1"].numpy())
    valid = taps["valid"].numpy()
    ref, S = np.zeros((B, H * W, C)), np.zeros((B, H * W, C))
    hits = np.zeros((B, H * W), np.int64)
    bb = np.broadcast_to(np.arange(B)[:, None], valid.shape)
    for a in (0, 1):
        for c in (0, 1):
            w = (wy[a] * wx[c] * valid)[:, :, None]
            idx = ys[a] * W + xs[c]
            np.add.at(ref, (bb, idx), w * g)
            np.add.at(S, (bb, idx), w * np.abs(g))
            np.add.at(hits, (bb, idx), valid.astype(np.int64))
    sh = (B, H, W, C)
    return torch.from_numpy(ref.reshape(sh)), torch.from_numpy(S.reshape(sh)), torch.from_numpy(hits.reshape(B, H, W))


def assert_within(got, ref, S, K, what, out_bf16=None):
    """bf16_bound.assert_within with a per-element K (a tensor broadcastable to ref): the bound is linear in K S, so
    S is scaled by K / max K and the largest K is passed on (and printed)."""
    if torch.is_tensor(K):
        kmax = max(int(K.max()), 1)
        return BB.assert_within(got, ref, S * (K.double() / kmax), kmax, what, out_bf16)
    return BB.assert_within(got, ref, S, K, what, out_bf16)
