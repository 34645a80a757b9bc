"""Checks shared by the front-end tests: the stem's max-pool into split form and res2 / res3 as
split-bf16 layers.  Run on the GPU (test_gpu_frontend_split.py) and on the CPU
emulator (test_emul_frontend_split.py); ``dev`` is where the operators' tensors live, references are CPU float64."""
import torch
import torch.nn as nn
import torch.nn.functional as F


# ---- the stem's max-pool -------------------------------------------------------------------------------------------

def pool_input(kind, side, B=2, C=64):
    g = torch.Generator().manual_seed(10 * side + len(kind))
    x = torch.randn(B, C, side, side, generator=g)
    if kind == "negative":  # a zero padding would win every border window
        x = -x.abs() - 0.125
    elif kind == "border":  # the maximum of every window that touches a border row / column lies ON it
        x[:, :, 0, :] += 8.0
        x[:, :, -1, :] += 8.0
        x[:, :, :, 0] += 8.0
        x[:, :, :, -1] += 8.0
    return x


def check_maxpool(ops2d, dev, kind, side, channels_last):
    """fp32 output torch.equal to F.max_pool2d, split output torch.equal to mf_split_bf16 of that output; the source is
    read in place, NCHW-strided or channels-last."""
    x = pool_input(kind, side)
    xd = x.to(dev)
    if channels_last:
        xd = xd.contiguous(memory_format=torch.channels_last)
    assert xd.stride(1) == (1 if channels_last else side * side)
    y32, ys = ops2d.maxpool_split(xd)
    want = F.max_pool2d(x, 3, 2, 1)  # (a maximum is exact: the CPU's is the GPU's)
    assert y32.shape == (2, side // 2, side // 2, 64) and ys.shape == (2, side // 2, side // 2, 128)
    assert torch.equal(y32.cpu().permute(0, 3, 1, 2), want)
    if kind == "negative":
        assert bool((y32 < 0).all())
    split = ops2d.to_split(y32.permute(0, 3, 1, 2))
    assert torch.equal(ys.cpu().view(torch.int16), split.cpu().view(torch.int16))
    only32, none = ops2d.maxpool_split(xd, outs=False)
    assert none is None and torch.equal(only32.cpu(), y32.cpu())


# ---- res2 / res3 layers: |y - y_fp64| <= 2^-15 conv(|x|, |w|)_fp64 per element -------------------------------------

FRONT_LAYERS = {  # name: (Cin, Cout, ks, stride, input side, residual)
    "res2.conv2_identity": (64, 64, 3, 1, 8, "identity"),
    "res3.conv1_s2": (64, 128, 3, 2, 16, None),
    "res3.residual_s2": (64, 128, 1, 2, 16, None),
    "res3.conv2_convres": (128, 128, 3, 1, 8, "conv"),
}


def check_front_layer(ops2d, dev, name, B):
    Cin, Cout, ks, stride, D, residual = FRONT_LAYERS[name]
    torch.manual_seed(100 * B + len(name))
    conv = nn.Conv2d(Cin, Cout, ks, stride, padding=ks // 2, bias=False).to(dev).eval()
    x = torch.randn(B, Cin, D, D)
    act = 0 if ks == 1 else 1
    w64 = conv.weight.detach().cpu().double()
    ref = F.conv2d(x.double(), w64, None, stride, ks // 2)
    bound = F.conv2d(x.double().abs(), w64.abs(), None, stride, ks // 2)
    res = None
    with torch.no_grad():
        if residual == "identity":
            r = torch.randn(B, Cout, D, D)
            res = r.permute(0, 2, 3, 1).contiguous().to(dev)
            ref = ref + r.double()
        elif residual == "conv":  # the block's 1 x 1 stride-2 shortcut of a twice larger 64-channel map
            rconv = nn.Conv2d(64, Cout, 1, 2, bias=False).to(dev).eval()
            x0 = torch.randn(B, 64, 2 * D, 2 * D)
            res, _ = ops2d.conv_split(ops2d.to_split(x0.to(dev)), rconv)
            wr64 = rconv.weight.detach().cpu().double()
            ref = ref + F.conv2d(x0.double(), wr64, None, 2)
            bound = bound + F.conv2d(x0.double().abs(), wr64.abs(), None, 2)
        y, ys = ops2d.conv_split(ops2d.to_split(x.to(dev)), conv, res=res, act=act, outs=True)
    Do = D // stride
    assert y.shape == (B, Do, Do, Cout) and ys.shape == (B, Do, Do, 2 * Cout)
    pre = ref.permute(0, 2, 3, 1)
    want = F.relu(pre) if act else pre
    lim = 2.0 ** -15 * bound.permute(0, 2, 3, 1) + 1e-30
    err = (y.cpu().double() - want).abs()
    ratio = float((err / lim).max())
    print(f"{name} B {B}: max err / bound = {ratio:.3f}")
    assert ratio <= 1.0, (name, B, ratio)  # (ReLU is 1-Lipschitz: the pre-activation's bound holds after it)
    yc = y.cpu()
    hi = ys.cpu()[..., :Cout].float()
    assert torch.equal(hi, yc.to(torch.bfloat16).float())
    assert torch.equal(ys.cpu()[..., Cout:].float(), (yc - hi).to(torch.bfloat16).float())
