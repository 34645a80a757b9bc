"""csrc/gemm_bf16.hip's 2-D split-bf16 convolution (mf_conv2d_split_*) and csrc/backbone2d.hip's split kernels on the
CPU (fiber emulator, lane-exact v_mfma_f32_32x32x16_bf16).

The GEMM is checked against float64 convolutions of the SAME hi / lo-rounded operands (hi hi + lo hi + hi lo): every
bf16 product is exact in fp32, so the only difference is the summation order (1e-4 of the largest output, as
test_emul_gemm_bf16.py).  The operand kernels (weight pack, split, resize + split) are bit-exact against a NumPy
restatement."""

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from host_emul import emul

pytestmark = pytest.mark.skipif(not emul.available(), reason="g++ not available")


@pytest.fixture(scope="module")
def L():
    return emul.build(["gemm_bf16.hip", "backbone2d.hip"])


@pytest.fixture(params=["tile128", "tile256"])
def tile(request, monkeypatch):
    """The 128 x 128 tile of the NT engine, and with MF_NT_BIG=2 the 256 x 256 ping-pong form wherever it fits."""
    monkeypatch.setenv("MF_NT_BIG", "2" if request.param == "tile256" else "0")
    return request.param


def p(t):
    return None if t is None else t.data_ptr()


def rne(x):
    """float32 array -> bf16 bit patterns (uint16), round to nearest even (NumPy restatement of mf::bf16_bits)."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def bf_float(bits):
    return (bits.astype(np.uint32) << 16).view(np.float32)


def split_np(x):
    """(hi, lo) bit patterns of float32 x: hi = bf16(x), lo = bf16(x - hi)."""
    x = np.asarray(x, np.float32)
    hi = rne(x)
    return hi, rne((x - bf_float(hi)).astype(np.float32))


def to_bf16_tensor(bits):
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).view(torch.bfloat16)


def hi_lo(t):
    """torch float32 tensor -> (hi, lo) as float64 tensors of the rounded values"""
    hi, lo = split_np(t.numpy())
    return torch.from_numpy(bf_float(hi).astype(np.float64)), torch.from_numpy(bf_float(lo).astype(np.float64))


def close(got, want, tol=1e-4):
    scale = float(want.abs().max()) or 1.0
    err = float((got.double() - want.double()).abs().max())
    assert err <= tol * scale, (err, scale)


def pack_np(W):
    """[Cout][Cin][k][k] float32 -> [Cout][k*k][3 Cin] bf16 bits [w_hi | w_hi | w_lo]"""
    Cout, Cin, k, _ = W.shape
    Wt = np.ascontiguousarray(W.reshape(Cout, Cin, k * k).transpose(0, 2, 1))
    hi, lo = split_np(Wt)
    return np.concatenate([hi, hi, lo], axis=2)


def split_input(x_cf):
    """[B][C][H][W] float32 -> the split operand [B][H][W][2C] (NumPy)"""
    hi, lo = split_np(x_cf.permute(0, 2, 3, 1).contiguous().numpy())
    return to_bf16_tensor(np.concatenate([hi, lo], axis=3))


def conv_ref(x_cf, W, stride, pad, dil):
    """float64 convolution of the rounded operands: hi hi + lo hi + hi lo"""
    xh, xl = hi_lo(x_cf)
    wh, wl = hi_lo(W)
    c = lambda a, b: F.conv2d(a, b, stride=stride, padding=pad, dilation=dil)  # noqa: E731
    return c(xh, wh) + c(xl, wh) + c(xh, wl)


GEOMS = [  # B, Cin, Cout, D, ks, stride, pad, dil
    (2, 16, 24, 8, 3, 1, 1, 1),
    (1, 24, 16, 8, 3, 1, 2, 2),   # 3 Cin = 72: K-tiles straddle the hi / lo / hi segments and the taps
    (1, 8, 32, 16, 3, 2, 1, 1),
    (1, 32, 16, 8, 3, 1, 4, 4),
    (2, 40, 16, 4, 1, 1, 0, 1),
    (1, 16, 8, 8, 1, 2, 0, 1),
]


def test_pack_bit_exact(L):
    rng = np.random.default_rng(0)
    for Cout, Cin, k in ((24, 16, 3), (8, 40, 1)):
        W = (rng.standard_normal((Cout, Cin, k, k)) * 0.1).astype(np.float32)
        wp = torch.empty(Cout, k * k, 3 * Cin, dtype=torch.bfloat16)
        Wt = torch.from_numpy(W)
        assert L.mf_conv2d_split_pack(p(Wt), Cout, Cin, k, p(wp), None) == 0
        assert np.array_equal(wp.view(torch.int16).numpy().view(np.uint16), pack_np(W))


def test_split_and_resize_bit_exact(L):
    torch.manual_seed(1)
    B, C, H, W = 2, 16, 5, 7
    x = torch.randn(B, C, H, W) * 3.0
    ldy, los, off = 48, 24, 8  # a channel block of a wider split map: hi at off + c, lo at off + los + c
    for src in (x, x.contiguous(memory_format=torch.channels_last)):
        y = torch.full((B, H, W, ldy), 7.0, dtype=torch.bfloat16)
        assert L.mf_split_bf16(p(src), *src.stride(), B, C, H, W, p(y[..., off:]), ldy, los, None) == 0
        hi, lo = split_np(x.permute(0, 2, 3, 1).numpy())
        got = y.view(torch.int16).numpy().view(np.uint16)
        assert np.array_equal(got[..., off:off + C], hi) and np.array_equal(got[..., off + los:off + los + C], lo)
        assert float((y[..., :off].float() - 7).abs().max()) == 0 and float((y[..., off + C:off + los].float() - 7).abs().max()) == 0
    # the resize, taken in fp32 (torch's align_corners arithmetic, no FMA), then split
    Ho, Wo = 10, 14
    xcl = x.permute(0, 2, 3, 1).contiguous()
    y = torch.zeros(B, Ho, Wo, 2 * C, dtype=torch.bfloat16)
    assert L.mf_upsample_bilinear_cl_split_fwd(p(xcl), p(y), B, H, W, Ho, Wo, C, 2 * C, C, None) == 0
    a = xcl.numpy()
    f32 = np.float32
    sy, sx = f32(H - 1) / f32(Ho - 1), f32(W - 1) / f32(Wo - 1)
    ref = np.empty((B, Ho, Wo, C), np.float32)
    for oy in range(Ho):
        fy = f32(sy * f32(oy))
        y0 = int(fy)
        yp = 1 if y0 < H - 1 else 0
        h1 = f32(fy - f32(y0)); h0 = f32(f32(1) - h1)
        for ox in range(Wo):
            fx = f32(sx * f32(ox))
            x0 = int(fx)
            xp = 1 if x0 < W - 1 else 0
            w1 = f32(fx - f32(x0)); w0 = f32(f32(1) - w1)
            t0 = (w0 * a[:, y0, x0] + w1 * a[:, y0, x0 + xp]).astype(f32)
            t1 = (w0 * a[:, y0 + yp, x0] + w1 * a[:, y0 + yp, x0 + xp]).astype(f32)
            ref[:, oy, ox] = (h0 * t0 + h1 * t1).astype(f32)
    hi, lo = split_np(ref)
    got = y.view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(got[..., :C], hi) and np.array_equal(got[..., C:], lo)
    # and it agrees with torch's resize to float32 rounding
    want = F.interpolate(x, (Ho, Wo), mode="bilinear", align_corners=True).permute(0, 2, 3, 1)
    assert float((torch.from_numpy(ref) - want).abs().max()) <= 1e-5 * float(want.abs().max())


def _run(L, xs, wp, geom, bias=None, res=None, slope=None, act=0, out32=None, outs=None, ws=None, nws=0,
         ldr=0, ldo32=0, ldos=0, los=0):
    B, Cin, Cout, D, ks, stride, pad, dil = geom
    rc = L.mf_conv2d_split_fwd(p(xs), p(wp), p(bias), p(res), ldr, p(slope), act, p(out32), ldo32, p(outs), ldos, los,
                               p(ws), nws, B, Cin, Cout, D, ks, stride, pad, dil, None)
    assert rc == 0


@pytest.mark.parametrize("geom", GEOMS)
def test_conv2d_split_forward(L, tile, geom):
    """act(conv + bias) to an fp32 map, every geometry, both tile forms."""
    B, Cin, Cout, D, ks, stride, pad, dil = geom
    torch.manual_seed(3)
    x = torch.randn(B, Cin, D, D)
    W = torch.randn(Cout, Cin, ks, ks) / (Cin * ks * ks) ** 0.5
    bias = torch.randn(Cout)
    ref = conv_ref(x, W, stride, pad, dil) + bias.double()[None, :, None, None]
    Do = ref.shape[2]
    xs = split_input(x)
    wp = torch.empty(Cout, ks * ks, 3 * Cin, dtype=torch.bfloat16)
    assert L.mf_conv2d_split_pack(p(W), Cout, Cin, ks, p(wp), None) == 0
    out = torch.full((B, Do, Do, Cout), 9.0)
    _run(L, xs, wp, geom, bias=bias, act=1, out32=out, ldo32=Cout)
    close(out, F.relu(ref).permute(0, 2, 3, 1))


def test_conv2d_split_epilogues(L, tile):
    """Every epilogue piece on one layer: bias, residual, ReLU / PReLU (slope read from memory), the fp32 output and the
    split output at channel offsets and pitches of wider maps, alone and together."""
    geom = (2, 16, 24, 8, 3, 1, 1, 1)
    B, Cin, Cout, D, ks, stride, pad, dil = geom
    torch.manual_seed(4)
    x = torch.randn(B, Cin, D, D)
    W = torch.randn(Cout, Cin, ks, ks) / (Cin * ks * ks) ** 0.5
    bias = torch.randn(Cout)
    slope = torch.tensor([0.25])
    resbuf = torch.randn(B, D, D, Cout + 16)
    res = resbuf[..., 8:8 + Cout]  # pitch Cout + 16, 16-byte aligned offset
    conv = conv_ref(x, W, stride, pad, dil).permute(0, 2, 3, 1)
    xs = split_input(x)
    wp = torch.empty(Cout, ks * ks, 3 * Cin, dtype=torch.bfloat16)
    assert L.mf_conv2d_split_pack(p(W), Cout, Cin, ks, p(wp), None) == 0
    for use_bias, use_res, act, o32, osp in ((0, 0, 0, 1, 0), (1, 1, 1, 1, 1), (0, 1, 2, 0, 1), (1, 0, 2, 1, 1),
                                             (1, 1, 0, 0, 1)):
        v = conv.clone()
        if use_bias:
            v += bias.double()
        if use_res:
            v += res.double()
        if act == 1:
            v = F.relu(v)
        elif act == 2:
            v = torch.where(v > 0, v, 0.25 * v)
        out = torch.full((B, D, D, Cout + 8), 9.0)
        ldos, los, soff = 2 * (Cout + 8) + 16, Cout + 8, 8
        spl = torch.full((B, D, D, ldos), 3.0, dtype=torch.bfloat16)
        _run(L, xs, wp, geom, bias=bias if use_bias else None, res=res if use_res else None, ldr=Cout + 16,
             slope=slope if act == 2 else None, act=act, out32=out[..., 8:] if o32 else None, ldo32=Cout + 8,
             outs=spl[..., soff:] if osp else None, ldos=ldos, los=los)
        if o32:
            close(out[..., 8:], v)
            assert float((out[..., :8] - 9).abs().max()) == 0
        else:
            assert float((out - 9).abs().max()) == 0
        if osp:
            hi, lo = spl[..., soff:soff + Cout].double(), spl[..., soff + los:soff + los + Cout].double()
            close(hi + lo, v)
            # the split of the kernel's own fp32 value: hi = bf16(v), |lo| <= half an ulp of hi
            assert float((hi - v).abs().max()) <= 2.0 ** -8 * float(v.abs().max())
            assert bool(((lo.abs() <= hi.abs() * 2.0 ** -8) | (hi == 0)).all())
            keep = torch.ones(ldos, dtype=torch.bool)
            keep[soff:soff + Cout] = False
            keep[soff + los:soff + los + Cout] = False
            assert float((spl[..., keep].float() - 3).abs().max()) == 0
        else:
            assert float((spl.float() - 3).abs().max()) == 0


@pytest.mark.parametrize("act", [1, 2])
def test_conv2d_split_splitk(L, monkeypatch, act):
    """The reduction split over fp32 slabs (forced: MF_NT_SPLITK=3 on the 256 x 256 form) -- the finish pass runs the
    same epilogue, once."""
    monkeypatch.setenv("MF_NT_BIG", "2")
    monkeypatch.setenv("MF_NT_SPLITK", "3")
    geom = (1, 24, 192, 8, 3, 1, 2, 2)
    B, Cin, Cout, D, ks, stride, pad, dil = geom
    torch.manual_seed(5)
    x = torch.randn(B, Cin, D, D)
    W = torch.randn(Cout, Cin, ks, ks) / (Cin * ks * ks) ** 0.5
    bias, res = torch.randn(Cout), torch.randn(B, D, D, Cout)
    slope = torch.tensor([-0.5])
    v = conv_ref(x, W, stride, pad, dil).permute(0, 2, 3, 1) + bias.double() + res.double()
    v = F.relu(v) if act == 1 else torch.where(v > 0, v, -0.5 * v)
    nws = L.mf_conv2d_split_workspace_bytes(*geom)
    assert nws == 3 * B * D * D * Cout * 4
    ws = torch.empty(nws, dtype=torch.uint8)
    xs = split_input(x)
    wp = torch.empty(Cout, ks * ks, 3 * Cin, dtype=torch.bfloat16)
    assert L.mf_conv2d_split_pack(p(W), Cout, Cin, ks, p(wp), None) == 0
    out = torch.empty(B, D, D, Cout)
    spl = torch.empty(B, D, D, 2 * Cout, dtype=torch.bfloat16)
    _run(L, xs, wp, geom, bias=bias, res=res, ldr=Cout, slope=slope, act=act, out32=out, ldo32=Cout, outs=spl,
         ldos=2 * Cout, los=Cout, ws=ws, nws=nws)
    close(out, v)
    # the split output is the split of the fp32 output, bit for bit
    hi, lo = split_np(out.numpy())
    got = spl.view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(got[..., :Cout], hi) and np.array_equal(got[..., Cout:], lo)


def test_conv2d_split_rejects(L):
    B, Cin, Cout = 1, 16, 16
    xs = torch.zeros(B, 8, 8, 2 * Cin, dtype=torch.bfloat16)
    wp = torch.zeros(Cout, 9, 3 * Cin, dtype=torch.bfloat16)
    out = torch.zeros(B, 8, 8, Cout)
    bad = dict(xs=p(xs), wp=p(wp), bias=None, res=None, ldr=0, slope=None, act=0, out32=p(out), ldo32=Cout, outs=None,
               ldos=0, los=0, ws=None, nws=0, B=B, Cin=Cin, Cout=Cout, D=8, ks=3, stride=1, pad=1, dil=1, st=None)
    assert L.mf_conv2d_split_fwd(*bad.values()) == 0
    for k, v in (("ks", 5), ("pad", 2), ("out32", None), ("act", 2), ("ldo32", 12), ("Cin", 12)):
        args = dict(bad)
        args[k] = v
        assert L.mf_conv2d_split_fwd(*args.values()) != 0, k
