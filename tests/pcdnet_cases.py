"""TEST INFRASTRUCTURE: the checks of the point-cloud baseline network's kernels (csrc/pcdnet.hip, and mf_pose_epilogue as
the network uses it), shared by tests/test_emul_pcdnet.py (host emulator, torch CPU tensors as device memory) and
tests/test_gpu_pcdnet.py (MI355X).  The mirror is tests/pcdnet_ref.py.

Shapes: B = 3, P = 37 (M = 111: a multiple of no tile, objects straddle the 16-row workgroups of the stem, the 64-row
waves and the 8 row lanes of the pool) and B = 1, P = 1.

Bounds (derived, not fitted): a convolution of the stem is an fp32 accumulation of at most 32 products and a bias, 35
terms with the products' own roundings: each element within 2^-22 * sum |x| |w| (+ |b|) of its float64 value; against
the mirror, which repeats the kernel's order, every output is bit-identical.  The sigmoid of the epilogue goes through
expf, which is not correctly rounded: within 2^-22 of the float64 sigmoid (values in (0, 1))."""
import ctypes

import numpy as np
import torch

import pcdnet_ref as PR
from morefusion_amd import _lib

SHAPES = ((3, 37), (1, 1))
N_FG = 21
NP4 = 88
H = W = 12


def t(a, dev, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(dev)


def bits(x):
    """bf16 tensor -> int16 bit patterns (NumPy)."""
    return x.detach().cpu().view(torch.int16).numpy()


def same_bits(got, ref, what):
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape and got.dtype == ref.dtype, (what, got.shape, ref.shape, got.dtype, ref.dtype)
    view = {4: np.int32, 2: np.int16, 8: np.int64}[got.dtype.itemsize]
    diff = np.ascontiguousarray(got).view(view) != np.ascontiguousarray(ref).view(view)
    assert not diff.any(), (what, int(diff.sum()), got[diff][:4], ref[diff][:4])


def stem_inputs(B, P, seed=0):
    rs = np.random.RandomState(seed)
    M = B * P
    x = rs.normal(size=(M, 32)).astype(np.float32)
    pcd = (rs.uniform(-0.2, 0.2, (B, H, W, 3)) + [0.0, 0.0, 0.6]).astype(np.float32)
    pix = rs.randint(0, H * W, M).astype(np.int64)
    center = np.median(pcd.reshape(B, -1, 3), axis=1).astype(np.float32)
    w = [rs.normal(size=s).astype(np.float32) * 0.3 for s in ((64, 32), (64,), (64, 3), (64,))]
    return x, pcd, pix, center, w


def run_stem(dev, B, P, centerize=True):
    x, pcd, pix, center, w = stem_inputs(B, P)
    M = B * P
    c = center if centerize else None
    pts = torch.full((M, 3), float("nan"), device=dev)
    f1 = torch.zeros((M, 256), dtype=torch.bfloat16, device=dev)
    xs = torch.zeros((M, 768), dtype=torch.bfloat16, device=dev)
    tx, tp, ti, tw = t(x, dev), t(pcd, dev), t(pix, dev), [t(a, dev) for a in w]
    tc = None if c is None else t(c, dev)
    _lib.check(_lib.lib().mf_pcdnet_stem(tx.data_ptr(), tp.data_ptr(), ti.data_ptr(), _lib.ptr(tc), tw[0].data_ptr(),
                                         tw[1].data_ptr(), tw[2].data_ptr(), tw[3].data_ptr(), B, P, H * W,
                                         pts.data_ptr(), f1.data_ptr(), 256, xs.data_ptr(), 768, 384, _lib.stream_ptr()),
               "mf_pcdnet_stem")
    return (x, pcd, pix, c, w), pts.cpu().numpy(), bits(f1), bits(xs)


def check_stem(dev):
    for B, P in SHAPES:
        for centerize in (True, False):
            (x, pcd, pix, c, w), pts, f1, xs = run_stem(dev, B, P, centerize)
            ref_pts, v = PR.stem(x, pcd, pix, c, *w, P)
            same_bits(pts, ref_pts, "stem: points")
            hi, lo = PR.split(v)
            # split outputs: hi = bf16_rne(v), lo = bf16_rne(v - hi) exactly, in both layouts
            same_bits(f1, np.concatenate([PR.bf16_bits(a) for a in (hi[:, :64], lo[:, :64], hi[:, 64:], lo[:, 64:])], 1),
                      "stem: feat1 rows")
            same_bits(xs[:, :128], PR.bf16_bits(hi), "stem: concat rows, hi")
            same_bits(xs[:, 384:512], PR.bf16_bits(lo), "stem: concat rows, lo")
            assert not xs[:, 128:384].any() and not xs[:, 512:].any()  # conv2's columns are not the stem's to write
            # the value the split form carries against float64, on the inputs the convolutions received
            val, S = PR.stem_f64(x, pts, *w)
            err = np.abs(v.astype(np.float64) - val)  # (v: the mirror's fp32 value, which the kernel's bits equal)
            print(f"PCDNET stem B={B} P={P} centerize={centerize}: worst err/bound {float((err / (2.0 ** -22 * S)).max()):.3f}")
            assert (np.abs(v.astype(np.float64) - val) <= 2.0 ** -22 * S).all()


def check_pool(dev):
    for B, P in SHAPES + ((2, 1000),):
        if dev == "cpu" and P > 100:
            continue
        rs = np.random.RandomState(B + P)
        C, ld = 128, 136
        h = np.maximum(rs.normal(size=(B * P, ld)), 0).astype(np.float32)
        th = t(h, dev)
        outs = []
        for _ in range(2):
            out = torch.full((B, C), float("nan"), device=dev)
            _lib.check(_lib.lib().mf_pcdnet_pool(th.data_ptr(), ld, B, P, C, out.data_ptr(), _lib.stream_ptr()),
                       "mf_pcdnet_pool")
            outs.append(out.cpu().numpy())
        same_bits(outs[0], PR.pool(h[:, :C], B, P), f"pool B={B} P={P}")
        same_bits(outs[1], outs[0], "pool: two runs")


def check_bias_relu_split(dev):
    for B, P in SHAPES:
        rs = np.random.RandomState(7 + P)
        M, N, G, ldy = B * P, 48, 16, 52
        y = rs.normal(size=(M, ldy)).astype(np.float32)
        gb = rs.normal(size=(B, N)).astype(np.float32)
        out = torch.zeros((M, 2 * N + 8), dtype=torch.bfloat16, device=dev)
        ty, tg = t(y, dev), t(gb, dev)
        _lib.check(_lib.lib().mf_pcdnet_bias_relu_split(ty.data_ptr(), ldy, tg.data_ptr(), B, P, N, G, out.data_ptr(),
                                                        2 * N + 8, _lib.stream_ptr()), "mf_pcdnet_bias_relu_split")
        v = PR.bias_relu(y[:, :N], gb, P)
        got = bits(out)
        same_bits(got[:, :2 * N], PR.head_layout(v, G), f"bias + relu + split B={B} P={P}")
        assert not got[:, 2 * N:].any()
        assert (v > 0).any() and (v == 0).any()


def check_epilogue(dev):
    for B, P in SHAPES:
        for centerize in (True, False):
            rs = np.random.RandomState(11 + P)
            M = B * P
            o = rs.normal(size=(M, 3 * NP4)).astype(np.float32)
            cid = rs.randint(1, N_FG + 1, B).astype(np.int64)
            cid[0] = N_FG  # the last class: the last columns of each block
            p = (rs.uniform(-0.2, 0.2, (M, 3)) + [0.0, 0.0, 0.6]).astype(np.float32)
            c = (rs.uniform(-0.05, 0.05, (B, 3)) + [0.0, 0.0, 0.6]).astype(np.float32)
            b = np.arange(M) // P
            pts = (p - c[b]) if centerize else p
            rot = torch.empty((M, 4), device=dev)
            trans = torch.empty((M, 3), device=dev)
            conf = torch.empty((M,), device=dev)
            to, tc, tp = t(o, dev), t(cid, dev), t(pts, dev)
            origin = t(c if centerize else np.zeros((B, 3), np.float32), dev)
            one = torch.ones((B,), device=dev)
            _lib.check(_lib.lib().mf_pose_epilogue(to.data_ptr(), 3 * NP4, NP4, tc.data_ptr(), tp.data_ptr(),
                                                   origin.data_ptr(), one.data_ptr(), B, P, N_FG, rot.data_ptr(),
                                                   trans.data_ptr(), conf.data_ptr(), _lib.stream_ptr()),
                       "mf_pose_epilogue")
            r_rot, r_trans, r_conf = PR.epilogue(o, NP4, cid, pts, c if centerize else None, P, N_FG)
            same_bits(rot.cpu().numpy(), r_rot, "epilogue: quaternion")
            same_bits(trans.cpu().numpy(), r_trans, "epilogue: translation")
            # the reference's order, restated independently: ((p - c) + c) + t
            tt = np.stack([o[np.arange(M), NP4 + 3 * (cid[b] - 1) + a] for a in range(3)], 1)
            same_bits(trans.cpu().numpy(), (((p - c[b]) + c[b]) + tt) if centerize else (p + tt), "epilogue: (p - c) + c")
            assert np.abs(conf.cpu().numpy().astype(np.float64) - r_conf).max() <= 2.0 ** -22
            if centerize and M > 100:
                assert ((p - c[b]) + c[b] != p).any()  # the case the order matters for


def check_refusals(dev):
    """Every launcher returns an error code, and launches nothing, for B <= 0, P <= 0, M > INT32_MAX, a misaligned
    pitch; the workspace functions refuse those and an n_fg beyond the limit.  Null pointers: nothing may be read."""
    L = _lib.lib()
    off = (ctypes.c_int64 * 13)()
    for B, P, nf in ((0, 5, 21), (5, 0, 21), (-1, 5, 21), (1 << 16, 1 << 15, 21), (2, 5, 0), (2, 5, 257)):
        assert L.mf_pcdnet_workspace_bytes(B, P, nf) < 0, (B, P, nf)
        assert L.mf_pcdnet_workspace_offsets(B, P, nf, ctypes.addressof(off)) < 0
    assert L.mf_pcdnet_workspace_offsets(2, 1000, 21, ctypes.addressof(off)) == 12
    assert list(off) == sorted(off) and all(o % 256 == 0 for o in off) and off[12] == L.mf_pcdnet_workspace_bytes(2, 1000, 21)
    assert off[12] >= 2000 * (3 * 4 + 256 * 2 + 768 * 2 + 1024 * 2 + 1024 * 4 + 1920 * 4 + 3840 * 2 + 1536 * 2 + 768 * 2 + 3 * 88 * 4)
    a = torch.zeros(64, device=dev)  # a valid, aligned address for the pointer checks
    p = a.data_ptr()
    s = _lib.stream_ptr()
    for B, P in ((0, 5), (5, 0), (-3, 5), (1 << 16, 1 << 15)):
        assert L.mf_pcdnet_stem(p, p, p, None, p, p, p, p, B, P, 144, p, p, 256, p, 768, 384, s) < 0
        assert L.mf_pcdnet_pool(p, 1024, B, P, 1024, p, s) < 0
        assert L.mf_pcdnet_bias_relu_split(p, 1920, p, B, P, 1920, 640, p, 3840, s) < 0
    assert L.mf_pcdnet_stem(p, p, p, None, p, p, p, p, 1, 1, 144, p, p, 252, p, 768, 384, s) < 0   # ld1 % 8
    assert L.mf_pcdnet_stem(p, p, p, None, p, p, p, p, 1, 1, 144, p, p, 256, p, 500, 384, s) < 0   # lo plane outside the row
    assert L.mf_pcdnet_stem(p, p, p, None, p, p, p, p, 1, 1, 144, p, p + 2, 256, p, 768, 384, s) < 0  # misaligned rows
    assert L.mf_pcdnet_stem(p, p, p, None, p, p, p, p, 1, 1, 0, p, p, 256, p, 768, 384, s) < 0     # no pixels
    assert L.mf_pcdnet_pool(p, 1022, 1, 1, 1024, p, s) < 0                                          # pitch < C
    assert L.mf_pcdnet_pool(p, 1026, 1, 1, 1024, p, s) < 0                                          # pitch % 4
    assert L.mf_pcdnet_pool(p, 1024, 1, 1, 1000, p, s) < 0                                          # C % 64
    assert L.mf_pcdnet_bias_relu_split(p, 1922, p, 1, 1, 1920, 640, p, 3840, s) < 0                 # ldy % 4
    assert L.mf_pcdnet_bias_relu_split(p, 1920, p, 1, 1, 1920, 640, p, 3836, s) < 0                 # ldo < 2 N
    assert L.mf_pcdnet_bias_relu_split(p, 1920, p, 1, 1, 1920, 600, p, 3840, s) < 0                 # G does not divide N
    assert L.mf_pcdnet_bias_relu_split(p, 1920, p, 1, 1, 1920, 640, p + 2, 3840, s) < 0             # misaligned output
    if dev != "cpu":  # (the emulator keeps no error text)
        assert b"mf_pcdnet" in L.mf_last_error_string()
    assert float(a.abs().sum()) == 0.0  # nothing was launched on it
