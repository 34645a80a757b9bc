"""TEST INFRASTRUCTURE: the bodies of the 2-D decoder's per-element cases (csrc/backbone2d.hip and the row kernels of
csrc/psp_tail.hip through the C ABI), shared by the emulator tests (CPU tensors as device memory) and
tests/test_gpu_backbone2d.py (the MI355X).  Every output element is compared with the float64 reference of
tests/decoder2d_ref.py under the bound of tests/bf16_bound.py; every K is derived next to its use from the kernel
as written, none is fitted.  Every case asserts through ``mf_backbone2d_last_path()`` that the branch it was written
for ran; the launchers' selection rules are restated here (``up_bwd_path``, ``bn_path``), so a case that no longer
reaches its branch fails instead of silently testing another kernel.

Channels-last tensors are built directly as [B, H, W, C]; references take [B, C, H, W] views of the same values.
"""
import numpy as np
import torch

import decoder2d_ref as R

BF = torch.bfloat16
SENT = -9.0   # sentinel of memory a kernel must leave alone
DIRECT, TILE, SMALL, BN_GENERIC, BN_GROUP = 1, 2, 3, 16, 32   # mf_backbone2d_last_path(); BN_GROUP + ppt


def p(t):
    return None if t is None else t.data_ptr()


def ok(code, L):
    assert code == 0, (code, L.mf_last_error_string().decode() if hasattr(L, "mf_last_error_string") else "")


def rnd(gen, *shape):
    return torch.randn(*shape, generator=gen)


# ----------------------------------------------------------------------------------------------- the launchers' rules
def _f32_scale(n_in, n_out):
    return np.float32(n_in - 1) / np.float32(n_out - 1) if n_out > 1 else np.float32(0.0)


def tile_lds_bytes(H, W, Ho, Wo):
    """mf_upsample_bilinear_cl_bwd's estimate of the tile kernel's output-gradient patch (8 x 8 input pixels x 64
    channels of bf16): (ceil(9 / scale) + 3) rows and columns of 128 bytes, the whole axis for a zero scale."""
    sy, sx = _f32_scale(H, Ho), _f32_scale(W, Wo)
    rows = int(np.ceil(np.float32(9.0) / sy)) + 3 if sy > 0 else Ho
    cols = int(np.ceil(np.float32(9.0) / sx)) + 3 if sx > 0 else Wo
    return rows * cols * 128


def up_bwd_path(C, H, W, Ho, Wo, bf16):
    """mf_upsample_bilinear_cl_bwd's rule restated: small input maps with large footprints first, then (bf16 only) the
    LDS tile when its patch estimate fits 64 KB, else the direct gather."""
    if C % 64 == 0 and H * W <= 64 and Ho * Wo >= 16 * H * W:
        return SMALL
    if bf16 and C % 64 == 0 and H >= 8 and W >= 8 and tile_lds_bytes(H, W, Ho, Wo) <= 64 * 1024:
        return TILE
    return DIRECT


def bn_path(C, npix, channels_last, params_aligned=True):
    """mf_bn_act_fwd's rule restated: channels-last with C / 8 dividing 256 and 16-byte aligned parameters -> one lane
    per channel group walking ppt pixels (doubled, up to 4, while twice the count still leaves >= 2048 workgroups)."""
    G = C // 8
    if not (channels_last and C % 8 == 0 and G <= 256 and 256 % G == 0 and params_aligned):
        return BN_GENERIC
    ppb, ppt = 256 // G, 1
    while ppt < 4 and npix // (ppb * ppt * 2) >= 2048:
        ppt *= 2
    return BN_GROUP + ppt


def small_trips(H, W, Ho, Wo):
    """k_up_bwd_small: the most candidates (up_lo .. up_hi on both axes, restated in float32) one input pixel has,
    in trips of the 64 pixel lanes."""
    def span(n_in, n_out):
        s = _f32_scale(n_in, n_out)
        if not s > 0:
            return n_out
        i = np.arange(n_in, dtype=np.float32)
        lo = np.maximum(0, np.floor((i - np.float32(1)) / s).astype(np.int64))
        hi = np.minimum(n_out - 1, np.ceil((i + np.float32(1)) / s).astype(np.int64))
        return int((hi - lo + 1).max())
    return -(-(span(H, Ho) * span(W, Wo)) // 64)


# --------------------------------------------------------------------------------------------------- bilinear resize
# K of the forward (k_up_fwd, k_up_fwd_cf): h0 (w0 a00 + w1 a01) + h1 (...) -- on the longest chain the roundings of
# l0 = 1 - l1, w0 * a, the inner sum, h0 * (.), the outer sum: 5, and one more for the second axis' l0: 6.
K_UP_FWD = 6


def k_up_bwd(H, W, Ho, Wo, path):
    """K of a resize backward.  Every kernel forms w = wy * wx (wy, wx each the rounded l0, or l0 + l1 when both
    taps of an output land on the pixel: 2 roundings per axis at most, + 1 for the product), then acc += w * g (1 for
    the product, 1 per addend): addends + 6 with ``addends`` the most output pixels any input pixel sums.  direct /
    tile / channels-first: one chain.  small: a lane's chain holds at most ``trips`` of the addends, then the 64
    partials are added in lane order: trips + 64 + 6."""
    if path == SMALL:
        return small_trips(H, W, Ho, Wo) + 64 + 6
    return R.resize_bwd_addends(H, W, Ho, Wo) + 6


def sparse_rows_cols(gen, g):
    """g [B, Ho, Wo, C] with about two thirds of its rows and of its columns zeroed: an input pixel then often sums
    ONE output row or column, so a pixel lost at the rim of a footprint is the whole value, not a 2^-8 of it."""
    B, Ho, Wo, _ = g.shape
    ry = (torch.rand(Ho, generator=gen) < 1 / 3).to(g.dtype)
    rx = (torch.rand(Wo, generator=gen) < 1 / 3).to(g.dtype)
    ry[torch.randint(0, Ho, (1,), generator=gen)] = 1
    rx[torch.randint(0, Wo, (1,), generator=gen)] = 1
    return g * ry[None, :, None, None] * rx[None, None, :, None]


def rim_rows_cols(g, H, W):
    """g [B, Ho, Wo, C] kept only on the output row and the output column whose bilinear weight onto some input row /
    column is the smallest positive one (from the float32 mirror): the input pixels of that row then sum NOTHING but
    the faintest pixel at the rim of their footprint -- a source coordinate that rounds to just below an integer
    leaves a weight of a few 2^-24 -- and a gather whose bounds stop one short returns 0 for a value whose S is all
    its own."""
    _, Ho, Wo, _ = g.shape
    keep = []
    for n_out, n_in in ((Ho, H), (Wo, W)):
        Wm = R.axis_matrix(n_in, n_out)[0]
        k = int(np.where(Wm > 0, Wm, np.inf).min(1).argmin())
        m = torch.zeros(n_out)
        m[k] = 1
        keep.append(m)
    ry, rx = keep
    mask = torch.clamp(ry[:, None] + rx[None, :], max=1)
    return g * mask[None, :, :, None]


def gradient_kinds(gen, g0, H, W):
    """The output gradients of a backward case [B, Ho, Wo, C]: dense, rows / columns zeroed at random, the rim probe."""
    return (("dense", g0), ("sparse", sparse_rows_cols(gen, g0)), ("rim", rim_rows_cols(g0, H, W)))


def resize_cl_case(L, dev, st, shape, size, bf16, expect_path, seed=1, what="resize"):
    """mf_upsample_bilinear_cl_fwd / _bwd on x [B, H, W, C] -> [B, Ho, Wo, C]: forward, backward of a dense and of a
    row / column-sparse gradient, all elements; the backward's branch asserted."""
    B, C, H, W = shape
    Ho, Wo = size
    dt = BF if bf16 else torch.float32
    gen = torch.Generator().manual_seed(seed)
    tag = f"{what} {'bf16' if bf16 else 'fp32'} {shape}->{size}"
    assert up_bwd_path(C, H, W, Ho, Wo, bf16) == expect_path, (tag, up_bwd_path(C, H, W, Ho, Wo, bf16))
    x = rnd(gen, B, H, W, C).to(dt)
    y = torch.full((B, Ho, Wo, C), SENT, dtype=dt, device=dev)
    xd = x.to(dev)
    ok(L.mf_upsample_bilinear_cl_fwd(p(xd), p(y), B, H, W, Ho, Wo, C, int(bf16), st()), L)
    ref, S = R.resize_fwd_ref(x.permute(0, 3, 1, 2), Ho, Wo)
    R.assert_within(y.cpu().permute(0, 3, 1, 2), ref, S, K_UP_FWD, f"{tag} fwd")
    K = k_up_bwd(H, W, Ho, Wo, expect_path)
    g0 = rnd(gen, B, Ho, Wo, C)
    for kind, g in gradient_kinds(gen, g0, H, W):
        g = g.to(dt)
        gd = g.to(dev)
        gx = torch.full((B, H, W, C), SENT, dtype=dt, device=dev)
        ok(L.mf_upsample_bilinear_cl_bwd(p(gd), p(gx), B, H, W, Ho, Wo, C, int(bf16), st()), L)
        assert L.mf_backbone2d_last_path() == expect_path, (tag, L.mf_backbone2d_last_path(), expect_path)
        ref, S = R.resize_bwd_ref(g.permute(0, 3, 1, 2), H, W)
        R.assert_within(gx.cpu().permute(0, 3, 1, 2), ref, S, K, f"{tag} bwd {kind} path {expect_path}")


def resize_cf_case(L, dev, st, shape, size, bf16, seed=2, what="resize cf"):
    """mf_upsample_bilinear_cf_fwd / _bwd on [B * C, H, W] (one lane per element, one chain: addends + 6)."""
    B, C, H, W = shape
    Ho, Wo = size
    dt = BF if bf16 else torch.float32
    gen = torch.Generator().manual_seed(seed)
    tag = f"{what} {'bf16' if bf16 else 'fp32'} {shape}->{size}"
    x = rnd(gen, B, C, H, W).to(dt)
    xd = x.to(dev)
    y = torch.full((B, C, Ho, Wo), SENT, dtype=dt, device=dev)
    ok(L.mf_upsample_bilinear_cf_fwd(p(xd), p(y), B * C, H, W, Ho, Wo, int(bf16), st()), L)
    ref, S = R.resize_fwd_ref(x, Ho, Wo)
    R.assert_within(y.cpu(), ref, S, K_UP_FWD, f"{tag} fwd")
    g0 = rnd(gen, B, C, Ho, Wo)
    for kind, g in gradient_kinds(gen, g0.permute(0, 2, 3, 1), H, W):
        g = g.permute(0, 3, 1, 2).contiguous().to(dt)
        gd = g.to(dev)
        gx = torch.full((B, C, H, W), SENT, dtype=dt, device=dev)
        ok(L.mf_upsample_bilinear_cf_bwd(p(gd), p(gx), B * C, H, W, Ho, Wo, int(bf16), st()), L)
        ref, S = R.resize_bwd_ref(g, H, W)
        R.assert_within(gx.cpu(), ref, S, k_up_bwd(H, W, Ho, Wo, DIRECT), f"{tag} bwd {kind}")


def resize_refusal_case(L, dev, st):
    """C % 8 != 0 and a pointer that is not 16-byte aligned: the error code, nothing written, the path left alone."""
    before = L.mf_backbone2d_last_path()
    x = torch.zeros(1 * 4 * 4 * 16 + 8, dtype=torch.float32, device=dev)
    y = torch.full((1 * 8 * 8 * 16 + 8,), SENT, dtype=torch.float32, device=dev)
    for fn in (L.mf_upsample_bilinear_cl_fwd, L.mf_upsample_bilinear_cl_bwd):
        assert fn(p(x), p(y), 1, 4, 4, 8, 8, 12, 0, st()) != 0          # C = 12
        assert fn(p(x) + 4, p(y), 1, 4, 4, 8, 8, 16, 0, st()) != 0      # the first operand 4 bytes off
        assert fn(p(x), p(y) + 4, 1, 4, 4, 8, 8, 16, 0, st()) != 0      # the second
    assert float((y.cpu() - SENT).abs().max()) == 0.0 and float(x.cpu().abs().max()) == 0.0
    assert L.mf_backbone2d_last_path() == before


# -------------------------------------------------------------------------------------------------------------- PReLU
def k_prelu_dslope(n):
    """K of mf_prelu_bwd's slope gradient, the chain of one addend: its product dy * x (1), the lane's 32 additions
    (4 chunks of 8), k_prelu_bwd's wave butterfly (6 levels) and four-wave sum (2), then k_prelu_finish: a lane adds
    ceil(partials / 256) values, the wave butterfly (6) and the four-wave sum (2)."""
    partials = -(-(n // 8) // 1024)
    return 1 + 32 + 6 + 2 + -(-partials // 256) + 6 + 2


def prelu_bwd_case(L, dev, st, n, slope, bf16, seed=3, what="prelu"):
    """mf_prelu_bwd over n elements: dx per element (one product a * dy: K = 1), dslope under its derived bound and
    bit-equal on a second launch.  x holds +0.0 and -0.0: both take the slope side."""
    dt = BF if bf16 else torch.float32
    gen = torch.Generator().manual_seed(seed)
    tag = f"{what} {'bf16' if bf16 else 'fp32'} n {n} slope {slope}"
    x, dy = rnd(gen, n).to(dt), rnd(gen, n).to(dt)
    x[0], x[1] = 0.0, -0.0
    x[n - 3], x[n - 2] = -0.0, 0.0
    a = torch.tensor([slope], dtype=torch.float32)
    nws = int(L.mf_prelu_bwd_workspace_floats(n))
    assert nws == -(-(n // 8) // 1024)
    xd, dyd, ad = x.to(dev), dy.to(dev), a.to(dev)
    outs = []
    for it in range(2):
        dx = torch.full((n,), SENT, dtype=dt, device=dev)
        da = torch.full((1,), SENT, dtype=torch.float32, device=dev)
        ws = torch.full((nws,), SENT, dtype=torch.float32, device=dev)
        ok(L.mf_prelu_bwd(p(xd), p(dyd), p(ad), p(dx), p(da), p(ws), n, int(bf16), st()), L)
        outs.append((dx.cpu(), da.cpu()))
    dx_ref, dx_S, da_ref, da_S = R.prelu_ref(x, dy, float(a[0]))
    R.assert_within(outs[0][0], dx_ref, dx_S, 1, f"{tag} dx")
    R.assert_within(outs[0][1], da_ref, da_S, k_prelu_dslope(n), f"{tag} dslope")
    assert torch.equal(outs[0][1], outs[1][1]) and torch.equal(outs[0][0], outs[1][0]), f"{tag}: second launch differs"


# ------------------------------------------------------------------------------------------- BatchNorm (+ add) (+ ReLU)
# K of mf_bn_act_fwd (both kernels): var + eps, sqrt, 1 / ., weight * invstd, x - mean, the product, + bias, + identity.
K_BN = 8


def bn_case(L, dev, st, C, npix, bf16, channels_last=True, misalign=False, B=1, expect_path=None, residuals=(False, True),
            seed=4, what="bn"):
    """mf_bn_act_fwd over [B * npix pixels, C] (channels-last) or [B, C, npix] (NCHW), with and without the residual,
    with and without the ReLU; the float64 reference of the normalisation is computed once and shared.
    ``misalign``: the four parameter vectors start 4 bytes past a 16-byte boundary."""
    dt = BF if bf16 else torch.float32
    gen = torch.Generator().manual_seed(seed)
    tag = f"{what} {'bf16' if bf16 else 'fp32'} C {C} pixels {B}x{npix} {'cl' if channels_last else 'nchw'}{' misaligned' if misalign else ''}"
    if expect_path is None:
        expect_path = bn_path(C, B * npix, channels_last, not misalign)
    assert bn_path(C, B * npix, channels_last, not misalign) == expect_path, (tag, bn_path(C, B * npix, channels_last, not misalign))
    shape = (B * npix, C) if channels_last else (B, C, npix)
    caxis = 1
    x, idn = rnd(gen, *shape).to(dt), rnd(gen, *shape).to(dt)
    off = 1 if misalign else 0
    par = [t.to(dev) for t in (rnd(gen, C + off), torch.rand(C + off, generator=gen) * 1.7 + 0.3, rnd(gen, C + off),
                               rnd(gen, C + off))]
    mean, var, weight, bias = (t[off:] for t in par)
    assert all(t.data_ptr() % 16 == (4 if misalign else 0) for t in (mean, var, weight, bias))
    eps = 1e-5
    xd, idd = x.to(dev), idn.to(dev)
    n = x.numel()
    base = {r: R.bn_ref(x, idn if r else None, mean, var, weight, bias, eps, False, caxis) for r in residuals}
    for residual in residuals:
        for relu in (0, 1):
            y = torch.full(shape, SENT, dtype=dt, device=dev)
            ok(L.mf_bn_act_fwd(p(xd), p(idd) if residual else None, p(mean), p(var), p(weight), p(bias), eps, p(y), n, C,
                               npix, int(channels_last), relu, int(bf16), st()), L)
            assert L.mf_backbone2d_last_path() == expect_path, (tag, L.mf_backbone2d_last_path(), expect_path)
            ref, S = base[residual]
            R.assert_within(y.cpu(), ref.clamp(min=0) if relu else ref, S, K_BN, f"{tag} residual={residual} relu={relu}")


# ---------------------------------------------------------------------------------------------------------- tail rows
def tail_pixels(gen, B, P, H, W):
    """pix [B, P] into the [2H, 2W] map: the four corners, a pixel on each border, 44 samples on the four output
    pixels around one source pixel (more than 40 samples load one address with atomics), the rest anywhere."""
    Ho, Wo = 2 * H, 2 * W
    pix = torch.randint(0, Ho * Wo, (B, P), generator=gen)
    fixed = [0, Wo - 1, (Ho - 1) * Wo, Ho * Wo - 1,                                  # corners
             Wo // 2, (Ho - 1) * Wo + Wo // 2, (Ho // 2) * Wo, (Ho // 2) * Wo + Wo - 1]  # borders
    cy, cx = min(H, Ho - 2), min(W, Wo - 2)
    hot = [(cy + d // 2) * Wo + cx + d % 2 for d in range(4)]
    fixed += [hot[i % 4] for i in range(44)]
    assert P > len(fixed) + 8
    pix[:, :len(fixed)] = torch.tensor(fixed)
    return pix


def tail_rows_case(L, dev, st, H, W, B=2, P=77, seed=5, what="tail rows"):
    """mf_psp_tail_rows_bf16_fwd / _bwd called directly.  Forward: bit-equal to the float32 formulation.  Backward:
    every element of gu2 against the exact transpose in float64 with K = contributions reaching that source pixel + 4
    -- a contribution is w * g with w = fl(fl(1 - ly) * fl(1 - lx)): 4 roundings; it is added in LDS and the patch
    sum with an fp32 atomic, and every addition an addend passes either takes in another contribution or another
    sample's patch, each of which holds at least one: at most ``contributions`` additions.  Exact zeros where nothing
    reaches.  (The atomics' order varies between launches on the GPU: no bit-reproducibility asserted.)"""
    from morefusion_amd.models.backbone2d import PSPNetExtractor
    assert P % 4
    gen = torch.Generator().manual_seed(seed)
    tag = f"{what} {H}x{W} B{B} P{P}"
    u = rnd(gen, B, H, W, 64).to(BF)
    pix = tail_pixels(gen, B, P, H, W)
    taps = PSPNetExtractor._tail_taps(pix, H, W)
    ud, pd = u.to(dev), pix.reshape(-1).contiguous().to(dev)
    rows = torch.full((B * P, 576), SENT, dtype=BF, device=dev)
    ok(L.mf_psp_tail_rows_bf16_fwd(p(ud), p(pd), B, P, H, W, p(rows), st()), L)
    assert torch.equal(rows.cpu(), R.tail_rows_fwd_f32(u.float(), taps).to(BF)), f"{tag}: forward rows differ"
    g = rnd(gen, B * P, 576).to(BF)
    gd = g.to(dev)
    acc = torch.full((B, H, W, 64), SENT, dtype=torch.float32, device=dev)
    gu = torch.full((B, H, W, 64), SENT, dtype=BF, device=dev)
    ok(L.mf_psp_tail_rows_bf16_bwd(p(gd), p(pd), B, P, H, W, p(acc), p(gu), st()), L)
    ref, S, hits = R.tail_rows_bwd_ref(g, taps, B, H, W)
    assert int(hits.max()) > 40 * 4, int(hits.max())
    got = gu.cpu()
    R.assert_within(got, ref, S, (hits + 4)[:, :, :, None].expand_as(ref), f"{tag} bwd")
    untouched = (hits == 0)
    if H * W > 100:
        assert bool(untouched.any())
    assert float(got.float()[untouched].abs().max() if bool(untouched.any()) else 0.0) == 0.0


# ------------------------------------------------------------------------------------------------------------ the cases
def case_id(v):
    if isinstance(v, dict):
        return "-".join(f"{k}{v[k]}" for k in v)
    if isinstance(v, tuple):
        return "x".join(str(i) for i in v)
    return {DIRECT: "direct", TILE: "tile", SMALL: "small"}.get(v, str(v)) if isinstance(v, int) else str(v)


# (shape [B, C, H, W], size, the backward's branch in bf16; a tile shape takes the direct kernel in fp32)
RESIZE_CL_CASES = [
    ((2, 128, 6, 6), (32, 32), SMALL),     # a footprint of > 64 output pixels: several lane trips; two channel blocks
    ((1, 64, 8, 8), (32, 32), SMALL),      # H W == 64 and Ho Wo == 16 H W: both thresholds met exactly
    ((1, 64, 2, 5), (9, 40), SMALL),
    ((1, 64, 1, 7), (16, 28), SMALL),      # one input row: every output row lands on it with l0 + l1
    ((1, 64, 1, 1), (8, 8), SMALL),
    ((1, 64, 3, 3), (1, 200), SMALL),      # one output row: zero scale in y, rows 1 and 2 of the input get exact zeros
    ((2, 128, 17, 27), (34, 54), TILE),    # ragged tiles, two channel blocks, two images
    ((1, 64, 9, 11), (18, 22), TILE),      # LDS estimate 23 x 22 x 128 = 64768 bytes, just under 64 KB
    ((1, 64, 16, 16), (24, 40), TILE),     # unequal ratios
    ((1, 64, 32, 32), (16, 16), TILE),     # down-sampling: input pixels no output touches get exact zeros
    ((1, 64, 8, 8), (8, 8), TILE),         # identity: every fractional weight 0
    # 25 -> 38 and 33 -> 56: fl(scale * (out - 1)) falls just below in - 1, so the last output row / column reaches the
    # last-but-one input row / column with a weight of 1.9e-6 (2 -> 42: 6e-8) -- the rim of the rim probe
    ((1, 64, 25, 33), (38, 56), TILE),
    ((1, 64, 2, 5), (42, 40), SMALL),
    ((1, 64, 8, 8), (31, 33), DIRECT),     # Ho Wo = 1023, one short of the small rule; LDS estimate too large for tile
    ((1, 8, 5, 7), (10, 14), DIRECT),
    ((1, 24, 8, 8), (16, 16), DIRECT),
]
# channels-first: element counts that are no multiple of 256; one down-sampling / transposing shape
RESIZE_CF_CASES = [((2, 3, 5, 7), (10, 14)), ((1, 5, 1, 1), (6, 6)), ((1, 2, 9, 4), (4, 9))]
RESIZE_MIRROR_SHAPES = [((1, 2) + sh[2:], sz) for sh, sz, _ in RESIZE_CL_CASES] + [((1, 2, 64, 64), (128, 128))]

# n: one chunk; a ragged single workgroup; a second workgroup holding one chunk; 257 partials (more than
# k_prelu_finish has lanes).  Slopes: the initial one, 0 and a negative one that is no power of two (a * dy rounds).
PRELU_CASES = [(8, 0.25), (8 * 1023, 0.25), (8 * 1023, 0.0), (8 * 1023, -0.3), (8 * 1024 + 8, -0.3), (8 * 1024 * 257, 0.25)]

BN_CASES = [
    dict(C=24, npix=50, bf16=0), dict(C=24, npix=50, bf16=1),                    # G = 3 does not divide 256: generic
    dict(C=64, npix=37, bf16=0, misalign=True), dict(C=64, npix=37, bf16=1, misalign=True),   # generic by alignment
    dict(C=8, npix=300, bf16=0), dict(C=8, npix=300, bf16=1),                    # G = 1: 256 pixels a block, ragged
    dict(C=16, npix=130, bf16=0), dict(C=16, npix=130, bf16=1),                  # G = 2
    dict(C=2048, npix=5, bf16=0), dict(C=2048, npix=5, bf16=1),                  # G = 256: one pixel a block
    dict(C=5, npix=8, B=3, bf16=0, channels_last=False), dict(C=5, npix=8, B=3, bf16=1, channels_last=False),  # NCHW, HW = 8
]
# G = 256 at the smallest pixel counts that give ppt = 2 (4096: the threshold itself) and ppt = 4 (8192 is the
# threshold; 8193 leaves the last workgroup one pixel of its four).  bf16 to keep them small; the GPU only.
# (one residual setting per case: the float64 reference of 17 million elements takes a second)
BN_PPT_CASES = [dict(C=2048, npix=npix, bf16=1, expect_path=BN_GROUP + ppt, residuals=(r,))
                for npix, ppt in ((4096, 2), (8193, 4)) for r in (False, True)]

TAIL_MAPS = [(2, 2), (3, 5), (8, 8), (16, 12)]
