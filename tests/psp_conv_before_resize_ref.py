"""float64 references shared by the conv-before-resize tests: PSPUpsample's resize -> 3 x 3 convolution
written as  bias + sum_t m_t(p) (U z_t)(p + d_t),  z_t = W_t x  (t = ky 3 + kx, d_t = (ky - 1, kx - 1), m_t the
convolution's zero padding on the UP-SAMPLED map)."""
import torch
import torch.nn.functional as F


def resize2x(x):
    """U: bilinear x2, align_corners, [B, C, H, W] float64"""
    return F.interpolate(x, (2 * x.shape[2], 2 * x.shape[3]), mode="bilinear", align_corners=True)


def tap_maps(x, w):
    """z [B, 9, Cout, H, W]: z_t = W_t x, the nine 1 x 1 convolutions at the low resolution"""
    Cout, Cin = w.shape[:2]
    wt = w.permute(2, 3, 0, 1).reshape(9 * Cout, Cin, 1, 1)  # row t Cout + co
    return F.conv2d(x, wt).reshape(x.shape[0], 9, Cout, x.shape[2], x.shape[3])


def masked_tap_sum(z):
    """sum_t m_t(p) (U z_t)(p + d_t) for z [B, 9, C, H, W] -> [B, C, 2H, 2W]: each up-sampled tap map is shifted by its
    offset with zeros entering from outside the map, taps added in increasing t"""
    B, _, C, H, W = z.shape
    out = torch.zeros(B, C, 2 * H, 2 * W, dtype=z.dtype)
    for t in range(9):
        ky, kx = divmod(t, 3)
        u = F.pad(resize2x(z[:, t]), (1, 1, 1, 1))  # zero ring: positions outside [0, 2H) x [0, 2W)
        out = out + u[:, :, ky:ky + 2 * H, kx:kx + 2 * W]
    return out


def resize_conv(x, w, bias=None):
    """the layer as PSPUpsample states it: conv3x3(U x) + bias, zero padding 1"""
    return F.conv2d(resize2x(x), w, bias, 1, 1)


def prelu(y, slope):
    return torch.where(y > 0, y, slope * y)


def regions(Ho, Wo):
    """boolean masks [Ho, Wo] of the corners, the edges without the corners, and the interior"""
    ry = torch.zeros(Ho, dtype=torch.bool)
    rx = torch.zeros(Wo, dtype=torch.bool)
    ry[0] = ry[-1] = rx[0] = rx[-1] = True
    corner = ry[:, None] & rx[None, :]
    edge = (ry[:, None] | rx[None, :]) & ~corner
    return {"corners": corner, "edges": edge, "interior": ~(ry[:, None] | rx[None, :])}


# ---- checks of the kernels, run on the GPU (test_gpu_psp_conv_before_resize.py) and on the CPU emulator ------------

def check_tapsum(ops2d, dev, side, B=2, C=8, slope=0.25):
    """ops2d.upsample_tapsum alone on random signed z [B, side, side, 9 C]: every element within
    64 * 2^-24 * sum |terms| of the float64 masked-tap formula (the n u bound of a 36-term fp32 sum plus the roundings
    of the bilinear weights), corners / edges / interior checked separately; hi + lo of the split output reproduces
    the fp32 output to 2^-16 |y|; two runs are bit-equal."""
    g = torch.Generator().manual_seed(100 + side)
    z = torch.randn(B, side, side, 9 * C, generator=g)
    bias = torch.randn(C, generator=g) + 0.5
    a = torch.tensor([slope])
    run = lambda: ops2d.upsample_tapsum(z.to(dev), bias.to(dev), act=2, slope=a.to(dev), out32=True, outs=True)  # noqa: E731
    y, ys = (t.cpu() for t in run())
    y2, ys2 = (t.cpu() for t in run())
    assert y.shape == (B, 2 * side, 2 * side, C) and ys.shape == (B, 2 * side, 2 * side, 2 * C)
    assert torch.equal(y, y2) and torch.equal(ys.view(torch.int16), ys2.view(torch.int16))
    z64 = z.double().reshape(B, side, side, 9, C).permute(0, 3, 4, 1, 2)  # [B, 9, C, H, W]
    b64 = bias.double()[None, :, None, None]
    want = prelu(masked_tap_sum(z64) + b64, slope).permute(0, 2, 3, 1)
    lim = 64 * 2.0 ** -24 * (masked_tap_sum(z64.abs()) + b64.abs()).permute(0, 2, 3, 1)
    err = (y.double() - want).abs()
    for name, m in regions(2 * side, 2 * side).items():
        if bool(m.any()):
            ratio = float((err[:, m] / lim[:, m]).max())
            print(f"tapsum side {side} {name}: max err / bound = {ratio:.3f}")
            assert ratio <= 1.0, (name, ratio)
    hl = ys[..., :C].double() + ys[..., C:].double()
    assert bool(((hl - y.double()).abs() <= 2.0 ** -16 * y.double().abs()).all())
    # only the split form, only the fp32 form: the same values
    _, ys3 = ops2d.upsample_tapsum(z.to(dev), bias.to(dev), act=2, slope=a.to(dev), out32=False, outs=True)
    assert torch.equal(ys3.cpu().view(torch.int16), ys.view(torch.int16))


def check_layer_pair(ops2d, dev, B, Cin, Cout, signed, side=8, slope=0.25):
    """resize + conv + PReLU through the new operators (to_split -> conv_taps_split -> upsample_tapsum) against the
    float64 resize -> conv of the same fp32 inputs: every element within 2^-15 conv(U |x|, |w|)_fp64 (same zero
    padding) -- the split GEMM's contract carried through U, whose weights are >= 0 and sum to 1."""
    import torch.nn as nn
    torch.manual_seed(1000 * B + Cin + int(signed))
    conv = nn.Conv2d(Cin, Cout, 3, 1, padding=1).to(dev).eval()
    x = torch.randn(B, Cin, side, side)
    if not signed:
        x = x.abs()
    a = torch.tensor([slope])
    with torch.no_grad():
        z = ops2d.conv_taps_split(ops2d.to_split(x.to(dev)), conv)
        y, _ = ops2d.upsample_tapsum(z, conv.bias.detach(), act=2, slope=a.to(dev))
    assert y.shape == (B, 2 * side, 2 * side, Cout)
    w64, b64 = conv.weight.detach().cpu().double(), conv.bias.detach().cpu().double()
    want = prelu(resize_conv(x.double(), w64, b64), slope).permute(0, 2, 3, 1)
    lim = 2.0 ** -15 * resize_conv(x.double().abs(), w64.abs()).permute(0, 2, 3, 1)
    err = (y.cpu().double() - want).abs()
    ratio = float((err / lim).max())
    print(f"layer pair B {B} Cin {Cin} Cout {Cout} signed {signed}: max err / bound = {ratio:.3f}")
    # (PReLU is 1-Lipschitz: the bound of the pre-activation holds after it)
    assert ratio <= 1.0, ratio
