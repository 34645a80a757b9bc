"""TEST INFRASTRUCTURE: the bodies of the bf16 engine cases (csrc/gemm_bf16.hip through the C ABI and bf16_ops),
shared by the emulator tests (CPU tensors as device memory) and tests/test_gpu_bf16_branches.py (the MI355X).
Every case compares EVERY output element with the float64 reference of tests/bf16_bound.py under its derived bound;
the cases do not know which tile or kernel the launcher picks -- the callers assert that, with the launchers' rules
restated below (shared with tests/test_emul_gemm_bf16_plan.py, which holds them against the library's own answer)."""
import ctypes

import torch
import torch.nn.functional as F

import bf16_bound as BB

BF = torch.bfloat16
SENT = -9.0   # sentinel of memory the kernel must leave alone


def p(t):
    return None if t is None else t.data_ptr()


def full_slabs(rows, split):
    """Every slab of a split reduction holds rows (the TN engine hands out ceil(K-tiles / split) K-tiles of 64 rows per
    slab, in order): a finish pass that lost its LAST slab must not hide behind a slab of zeros."""
    tall = -(-rows // 64)
    return (split - 1) * -(-tall // split) < tall


def rnd(gen, *shape, scale=1.0):
    return torch.randn(*shape, generator=gen) * scale


def ok(code, L=None):
    assert code == 0, (code, L.mf_last_error_string().decode() if L is not None and hasattr(L, "mf_last_error_string") else "")


# ------------------------------------------------- the launchers' rules, restated (csrc/gemm_bf16.hip: nt_plan, tn_plan)
# ``big`` / ``forced`` / ``half_max`` / ``tn_pp``: the MF_NT_BIG / MF_NT_SPLITK / MF_NT_HALF_MAX / MF_TN_PP knobs (None,
# 0, 255, None = not set).
def nt_tile(M, N, groups=1, table=False, dgrad_rows=0, S=1, big=None, half_max=255):
    """nt_plan's tile restated: the 256-row ping-pong form from 224 tiles of 256 x 256 on (N >= 160, no group table, a
    data gradient only with 256 | Do^3) and for every split of K, else 64-row tiles up to 255 tiles of 128 x 128 (never
    for the data gradient).  MF_NT_BIG: 0 never the 256-row form, 2 wherever its structure allows."""
    full = -(-M // 128) * -(-N // 128) * groups
    tiles = -(-M // 256) * -(-N // 256) * groups
    can_big = not table and not (dgrad_rows and dgrad_rows % 256)
    use_big = (tiles >= 224 and N >= 160 and can_big) or S > 1
    if big == 2:
        use_big = can_big
    elif big is not None:
        use_big = use_big and big == 1
    if use_big:
        return 256
    return 64 if full <= half_max and not dgrad_rows else 128


def nt_splitk(M, N, Kred, big=None, forced=0):
    """nt_plan's split restated: 16 .. 159 tiles of 256 x 256 at N >= 192 split K over 256 / tiles workgroups, each >= 16
    K-tiles of 64.  MF_NT_SPLITK forces a split that has a K-tile each; MF_NT_BIG=0 forbids the form a split runs on."""
    if N < 192 or N % 8 or big == 0:
        return 1
    tiles, T = -(-M // 256) * -(-N // 256), -(-Kred // 64)
    if forced > 0:
        return forced if forced <= T else 1
    if tiles >= 160 or tiles < 16:
        return 1
    S = 256 // tiles
    while S > 1 and T // S < 16:
        S -= 1
    return S


def tn_use_pp(Ni, Nj, rows, groups, ranges=False, big=None, tn_pp=None):
    """tn_plan's form restated: results of >= 192 x 192 whose reduction leaves every workgroup of a chip-filling split
    >= 48 K-tiles of 64 rows.  MF_TN_PP=0 / MF_NT_BIG=0: never; MF_NT_BIG=2: wherever there is no range table."""
    if tn_pp == 0 or big == 0 or ranges:
        return False
    if big == 2:
        return True
    if Ni < 192 or Nj < 192:
        return False
    tiles = -(-Ni // 256) * -(-Nj // 256) * groups
    fill = 1 if tiles >= 256 else -(-256 // tiles)
    return -(-rows // 64) >= 48 * fill


def deep_finish(split, slab_floats):
    return split >= 32 and slab_floats <= 65536


def wgrad_finish(split, slab_floats, conv=False):
    """tn_plan's finish restated: 0 none (an unsplit linear result), 1 k_wgrad_finish, 2 k_wgrad_finish_deep,
    3 k_wgrad_finish_conv (a convolution's slab of >= 2^20 floats)."""
    if conv and slab_floats >= 1 << 20:
        return 3
    if not conv and split == 1:
        return 0
    return 2 if deep_finish(split, slab_floats) else 1


# ... and the library's own answer (mf_gemm_bf16_nt_plan / mf_gemm_bf16_tn_plan: host arithmetic, no launch)
MODE_ROWS, MODE_CONV, MODE_DGRAD, MODE_CONV2_SPLIT, MODE_CONV3_SPLIT, MODE_ROWS_SPLIT = range(6)


def nt_plan(L, mode, M, N, K, groups=1, table=False, dgrad_rows=0, may_split=False, have_ws=False):
    """-> (tile, S)"""
    tile, S = ctypes.c_int32(-1), ctypes.c_int32(-1)
    ok(L.mf_gemm_bf16_nt_plan(mode, M, N, K, groups, int(table), dgrad_rows, int(may_split), int(have_ws),
                              ctypes.byref(tile), ctypes.byref(S)), L)
    return tile.value, S.value


def tn_plan(L, Ni, Nj, rows, groups=1, ldc=None, ranges=False, conv=False, split=0):
    """-> (form: 128 / 256, default split, finish kernel of ``split`` slabs: wgrad_finish's numbers)"""
    form, dsplit, finish = ctypes.c_int32(-1), ctypes.c_int32(-1), ctypes.c_int32(-1)
    ok(L.mf_gemm_bf16_tn_plan(Ni, Nj, Nj if ldc is None else ldc, rows, groups, int(ranges), int(conv), split,
                              ctypes.byref(form), ctypes.byref(dsplit), ctypes.byref(finish)), L)
    return form.value, dsplit.value, finish.value


# ---------------------------------------------------------------------------------------------------------- NT rows
def linear_case(L, dev, st, M, N, K, groups=1, relu=1, lda_pad=0, ldo_pad=0, expect_tile=None, seed=1,
                forms=((0, 0), (1, 0), (1, 1)), what="linear"):
    """out = act(A W^T + b), ``groups`` column blocks of wider matrices side by side; forms = (out_f32, accumulate)."""
    gen = torch.Generator().manual_seed(seed)
    lda, ldo = groups * K + lda_pad, groups * N + ldo_pad
    A = rnd(gen, M, lda).to(BF)
    W = rnd(gen, groups, N, K, scale=K ** -0.5).to(BF)
    b = rnd(gen, groups, N)
    Ad, Wd, bd = A.to(dev), W.to(dev), b.to(dev)
    for out_f32, acc in forms:
        base = rnd(gen, M, ldo) if acc else torch.full((M, ldo), SENT)
        out = base.clone().to(torch.float32 if out_f32 else BF).to(dev)   # (clone: on the CPU .to() aliases)
        act = 0 if acc else relu
        ok(L.mf_linear_bf16(p(Ad), K, lda, p(Wd), N * K, K, None if acc else p(bd), N, p(out), N, ldo, M, N, K, groups,
                            act, out_f32, acc, st()), L)
        if expect_tile is not None:
            assert L.mf_gemm_bf16_last_tile() == expect_tile, (L.mf_gemm_bf16_last_tile(), expect_tile)
        out = out.cpu()
        for g in range(groups):
            ref, S = BB.linear_ref(A[:, g * K:(g + 1) * K], W[g], None if acc else b[g])
            if acc:
                ref, S = ref + base[:, g * N:(g + 1) * N].double(), S + base[:, g * N:(g + 1) * N].double().abs()
            ref = F.relu(ref) if act else ref
            BB.assert_within(out[:, g * N:(g + 1) * N], ref, S, K + 1, f"{what} M{M} N{N} K{K} g{g} f32={out_f32} acc={acc}")
        if ldo_pad:  # nothing written past the last block
            assert torch.equal(out[:, groups * N:], base.to(out.dtype)[:, groups * N:])


def tiles_case(L, dev, st, table, N, K, n_groups, out_f32=0, lda_pad=8, ldo_pad=8, seed=2, what="tiles"):
    """mf_linear_bf16_tiles: ``table`` [M / 64] holds the weight group of every 64-row block, -1 = empty (left alone)."""
    gen = torch.Generator().manual_seed(seed)
    M = 64 * len(table)
    lda, ldo = K + lda_pad, N + ldo_pad
    A = rnd(gen, M, lda).to(BF)
    W = rnd(gen, n_groups, N, K, scale=K ** -0.5).to(BF)
    tg = torch.tensor(table, dtype=torch.int32)
    out = torch.full((M, ldo), SENT, dtype=torch.float32 if out_f32 else BF)
    Ad, Wd, tgd, od = A.to(dev), W.to(dev), tg.to(dev), out.to(dev)
    ok(L.mf_linear_bf16_tiles(p(Ad), lda, p(Wd), N * K, K, p(tgd), p(od), ldo, M, N, K, out_f32, st()), L)
    tile = L.mf_gemm_bf16_last_tile()
    assert tile in (64, 128)       # (the table form never takes the 256-row tile)
    got = od.cpu()
    assert torch.equal(got[:, N:], out[:, N:])
    for blk, g in enumerate(table):
        rows = slice(64 * blk, 64 * blk + 64)
        if g < 0:
            assert torch.equal(got[rows], out[rows]), f"empty block {blk} written"
            continue
        ref, S = BB.linear_ref(A[rows, :K], W[g])
        BB.assert_within(got[rows, :N], ref, S, K, f"{what} block {blk} group {g} N{N} K{K}")
    return tile


def ranges_case(L, dev, st, bounds, N, K, seed=3, what="ranges"):
    """mf_linear_wgrad_bf16_ranges: dW[g] = dY[rows of range g]^T A[rows of range g]; an empty range gives zeros."""
    gen = torch.Generator().manual_seed(seed)
    groups, M = len(bounds) - 1, bounds[-1]
    ldy, lda, ldc = N + 8, K + 16, K + 4
    dY, A = rnd(gen, M, ldy).to(BF), rnd(gen, M, lda).to(BF)
    dW = torch.full((groups, N, ldc), SENT)
    rng = torch.tensor(bounds, dtype=torch.int32)
    dYd, Ad, dWd, rd = dY.to(dev), A.to(dev), dW.to(dev), rng.to(dev)
    ok(L.mf_linear_wgrad_bf16_ranges(p(dYd), ldy, p(Ad), lda, p(dWd), N * ldc, ldc, p(rd), groups, N, K, st()), L)
    got = dWd.cpu()
    assert torch.equal(got[:, :, K:], dW[:, :, K:])
    for g in range(groups):
        rows = slice(bounds[g], bounds[g + 1])
        ref, S = BB.wgrad_ref(dY[rows, :N], A[rows, :K])
        BB.assert_within(got[g, :, :K], ref, S, max(bounds[g + 1] - bounds[g], 1), f"{what} range {g} rows {rows.start}:{rows.stop}")


def linear_wgrad_case(L, dev, st, M, N, K, groups, splits, seed=4, what="linear wgrad"):
    gen = torch.Generator().manual_seed(seed)
    ldy, lda, ldc = groups * N + 8, groups * K + 8, K
    dY, A = rnd(gen, M, ldy).to(BF), rnd(gen, M, lda).to(BF)
    dYd, Ad = dY.to(dev), A.to(dev)
    refs = [BB.wgrad_ref(dY[:, g * N:(g + 1) * N], A[:, g * K:(g + 1) * K]) for g in range(groups)]
    for split in splits:
        assert full_slabs(M, split), (M, split)
        dW = torch.full((groups, N, ldc), SENT, device=dev)
        ws = torch.empty(max(split, 1) * groups * N * ldc, device=dev)
        ok(L.mf_linear_wgrad_bf16(p(dYd), N, ldy, p(Ad), K, lda, p(dW), N * ldc, ldc, p(ws), M, N, K, groups, split, st()), L)
        got = dW.cpu()
        for g in range(groups):
            BB.assert_within(got[g], refs[g][0], refs[g][1], M + split, f"{what} M{M} N{N} K{K} g{g} split {split}")


# ---------------------------------------------------------------------------------------------- general-geometry conv
def conv_case(L, dev, st, B, Cin, Cout, D, geom, splits=(1,), ldo_pad=0, c_off=0, expect_tile=None, expect_ws=None,
              dgrad=True, repeat=0, seed=5, what="conv"):
    """mf_conv3d_bf16_pack / _fwd_ws / _wgrad and, for stride 1 with an input grid that is a power of two, the data
    gradient as the forward convolution of dy with the flipped / transposed operand.  ``c_off``: the output is a
    column block at that offset of a grid of pitch Cout + ldo_pad."""
    ks, stride, pad, dil = geom
    gen = torch.Generator().manual_seed(seed)
    taps, Do = ks ** 3, BB.conv_out_size(D, ks, stride, pad, dil)
    x = F.relu(rnd(gen, B, D ** 3, Cin)).to(BF)                    # (activations: half of them zero)
    W = rnd(gen, Cout, Cin, ks, ks, ks, scale=(Cin * taps) ** -0.5)
    bias = rnd(gen, Cout)
    dy = rnd(gen, B, Do ** 3, Cout).to(BF)
    Wb = W.to(BF)
    do_dx = dgrad and stride == 1 and D & (D - 1) == 0
    r = BB.conv_ref(x, Wb, bias, D, geom, dz_cl=dy, want_dx=do_dx)
    xd, Wd, bd, dyd = x.to(dev), W.to(dev), bias.to(dev), dy.to(dev)
    wt = torch.empty(Cout, taps, Cin, dtype=BF, device=dev)
    wf = torch.empty(Cin, taps, Cout, dtype=BF, device=dev) if do_dx else None
    ok(L.mf_conv3d_bf16_pack(p(Wd), Cout, Cin, Cin, 0, ks, p(wt), None, p(wf), st()), L)
    assert torch.equal(wt.cpu(), Wb.reshape(Cout, Cin, taps).permute(0, 2, 1))
    nws = L.mf_conv3d_bf16_fwd_workspace_bytes(B, Cin, Cout, D, ks, stride, pad, dil)
    if expect_ws is not None:
        assert nws == expect_ws, (nws, expect_ws)
    ws = torch.empty(max(nws, 16), dtype=torch.uint8, device=dev)
    ldo = Cout + ldo_pad
    Kf = taps * Cin + 1 + (nws // (B * Do ** 3 * Cout * 4) if nws else 0)
    first = None
    for relu, out_f32 in ((1, 0), (0, 1)):
        out = torch.full((B, Do ** 3, ldo), SENT, dtype=torch.float32 if out_f32 else BF, device=dev)
        for it in range(1 + (repeat if not out_f32 else 0)):
            ok(L.mf_conv3d_bf16_fwd_ws(p(xd), p(wt), p(bd), out.data_ptr() + c_off * out.element_size(), p(ws), nws, B,
                                       Cin, Cout, D, ks, stride, pad, dil, relu, out_f32, ldo, st()), L)
            if expect_tile is not None:
                assert L.mf_gemm_bf16_last_tile() == expect_tile, (L.mf_gemm_bf16_last_tile(), expect_tile)
            if repeat and not out_f32:   # every launch of a deterministic kernel gives the same bits
                if first is None:
                    first = out.clone()
                else:
                    assert torch.equal(out, first), f"{what}: launch {it} differs"
        got = out.cpu()
        ref = F.relu(r["y"]) if relu else r["y"]
        BB.assert_within(got[:, :, c_off:c_off + Cout], ref, r["Sy"], Kf, f"{what} fwd f32={out_f32}")
        rest = torch.cat((got[:, :, :c_off], got[:, :, c_off + Cout:]), 2)
        assert rest.numel() == 0 or float((rest.float() - SENT).abs().max()) == 0.0
    for split in splits:
        assert full_slabs(B * Do ** 3, split), (B * Do ** 3, split)
        dW = torch.full((Cout, Cin, ks, ks, ks), SENT, device=dev)
        wsw = torch.empty(L.mf_conv3d_bf16_wgrad_workspace_bytes(Cin, Cout, ks, split) // 4, device=dev)
        ok(L.mf_conv3d_bf16_wgrad(p(dyd), p(xd), p(dW), p(wsw), B, Cin, Cout, D, ks, stride, pad, dil, Cin, 0, split, st()), L)
        BB.assert_within(dW.cpu(), r["dw"], r["Sdw"], B * Do ** 3 + split, f"{what} wgrad split {split}")
    if do_dx:
        for out_f32 in (0, 1):
            dx = torch.full((B, D ** 3, Cin), SENT, dtype=torch.float32 if out_f32 else BF, device=dev)
            ok(L.mf_conv3d_bf16_fwd(p(dyd), p(wf), None, p(dx), B, Cout, Cin, Do, ks, 1, dil * (ks - 1) - pad, dil, 0,
                                    out_f32, Cin, st()), L)
            BB.assert_within(dx.cpu(), r["dx"], r["Sdx"], taps * Cout, f"{what} dgrad (flipped operand) f32={out_f32}")


def conv_refusal_case(L, dev, st):
    """Geometries the validator refuses return the error code and leave the output untouched."""
    x = torch.zeros(1, 12 ** 3, 16, dtype=BF, device=dev)
    wt = torch.zeros(16, 64, 16, dtype=BF, device=dev)
    out = torch.full((1, 12 ** 3, 16), SENT, dtype=BF, device=dev)
    for (Cin, Cout, D, ks, stride, pad, dil) in ((8, 8, 12, 3, 1, 1, 1),     # Do = 12: not a power of two
                                                  (8, 8, 9, 3, 1, 0, 1),      # Do = 7
                                                  (12, 8, 8, 3, 1, 1, 1),     # Cin % 8
                                                  (8, 12, 8, 3, 1, 1, 1),     # Cout % 8
                                                  (8, 8, 8, 5, 1, 2, 1),      # kernel 5
                                                  (8, 8, 8, 3, 3, 1, 1)):     # stride 3
        assert L.mf_conv3d_bf16_fwd(p(x), p(wt), None, p(out), 1, Cin, Cout, D, ks, stride, pad, dil, 0, 0, Cout, st()) != 0
        assert L.mf_conv3d_bf16_fwd_workspace_bytes(1, Cin, Cout, D, ks, stride, pad, dil) == 0
        dW = torch.full((Cout, Cin, ks, ks, ks), SENT, device=dev)
        ws = torch.empty(Cout * Cin * ks ** 3, device=dev)
        assert L.mf_conv3d_bf16_wgrad(p(out), p(x), p(dW), p(ws), 1, Cin, Cout, D, ks, stride, pad, dil, Cin, 0, 1, st()) != 0
        assert float((dW.cpu() - SENT).abs().max()) == 0.0
    assert float((out.float().cpu() - SENT).abs().max()) == 0.0


# --------------------------------------------------------------------------------------------------- k4 / s2 / p1 dgrad
def dgrad_k4s2_case(L, dev, st, B, Cin, Cout, D, expect_tile=None, seed=6, what="dgrad k4s2"):
    gen = torch.Generator().manual_seed(seed)
    Do = D // 2
    W = rnd(gen, Cout, Cin, 4, 4, 4, scale=(8 * Cout) ** -0.5)
    dy = rnd(gen, B, Do ** 3, Cout).to(BF)
    xz = torch.zeros(B, D ** 3, Cin)
    r = BB.conv_ref(xz, W.to(BF), None, D, (4, 2, 1, 1), dz_cl=dy)
    Wd, dyd = W.to(dev), dy.to(dev)
    wt = torch.empty(Cout, 64, Cin, dtype=BF, device=dev)
    wd = torch.empty(8, Cin, 8, Cout, dtype=BF, device=dev)
    ok(L.mf_conv3d_bf16_pack(p(Wd), Cout, Cin, Cin, 0, 4, p(wt), p(wd), None, st()), L)
    gen2 = torch.Generator().manual_seed(seed + 100)
    base = rnd(gen2, B, D ** 3, Cin)
    for out_f32, acc in ((0, 0), (1, 0), (1, 1)):
        dx = (base.clone() if acc else torch.full((B, D ** 3, Cin), SENT)).to(torch.float32 if out_f32 else BF).to(dev)
        ok(L.mf_conv3d_k4s2_bf16_dgrad(p(dyd), p(wd), p(dx), B, Cin, Cout, D, out_f32, acc, st()), L)
        if expect_tile is not None:
            assert L.mf_gemm_bf16_last_tile() == expect_tile, (L.mf_gemm_bf16_last_tile(), expect_tile)
        ref, S = (r["dx"] + base.double(), r["Sdx"] + base.double().abs()) if acc else (r["dx"], r["Sdx"])
        BB.assert_within(dx.cpu(), ref, S, 8 * Cout + acc, f"{what} B{B} {Cout}->{Cin} D{D} f32={out_f32} acc={acc}")


def dgrad_k4s2_refusal(L, dev, st):
    """D = 8: (D/2)^3 = 64 rows per parity class, below the 128-row tile -> the error code, dx untouched."""
    dy = torch.zeros(1, 64, 16, dtype=BF, device=dev)
    wd = torch.zeros(8, 16, 8, 16, dtype=BF, device=dev)
    dx = torch.full((1, 512, 16), SENT, dtype=BF, device=dev)
    assert L.mf_conv3d_k4s2_bf16_dgrad(p(dy), p(wd), p(dx), 1, 16, 16, 8, 0, 0, st()) != 0
    assert float((dx.float().cpu() - SENT).abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------------ narrow kernel
def narrow_tpw(B, D):
    """Tiles of 32 voxels one wave walks: mf_conv3d_k3_narrow_bf16's rule restated (doubles while every one of the
    workgroups' 4 waves would still leave >= 2048 workgroups at twice the count)."""
    tiles = (B * D ** 3 + 31) // 32
    tpw = 1
    while tpw < 8 and tiles // (4 * tpw * 2) >= 2048:
        tpw *= 2
    return tpw


def narrow_case(L, dev, st, B, CI, CO, D, dil, relu=1, w_cin=None, transpose=False, repeat=0, seed=7, what="narrow"):
    """mf_conv3d_k3_narrow_bf16 on x [B, D^3, CI] -> [B, D^3, CO].  Forward: layer CI -> CO with weight
    [CO, w_cin, 3, 3, 3] (input channels at or beyond w_cin read as zeros whatever x holds there), bias, ReLU.
    ``transpose``: the data gradient of the layer CO -> CI (x is that layer's output gradient), no bias / ReLU."""
    gen = torch.Generator().manual_seed(seed)
    w_cin = w_cin or (CO if transpose else CI)
    x = rnd(gen, B, D ** 3, CI).to(BF)
    geom = (3, 1, dil, dil)
    if not transpose:
        W = rnd(gen, CO, w_cin, 3, 3, 3, scale=(27 * w_cin) ** -0.5)
        bias = rnd(gen, CO)
        Wfull = torch.zeros(CO, CI, 3, 3, 3)
        Wfull[:, :w_cin] = W.to(BF).float()
        r = BB.conv_ref(x, Wfull, bias, D, geom)
        ref, S, Kred = (F.relu(r["y"]) if relu else r["y"]), r["Sy"], 27 * CI + 1
        pack_args = (CO, CI, w_cin, 0, 0)
    else:
        W = rnd(gen, CI, w_cin, 3, 3, 3, scale=(27 * CI) ** -0.5)   # layer CO -> CI: [Cout = CI][w_cin <= CO]
        bias, relu = None, 0
        Wfull = torch.zeros(CI, CO, 3, 3, 3)
        Wfull[:, :w_cin] = W.to(BF).float()
        r = BB.conv_ref(torch.zeros(B, D ** 3, CO), Wfull, None, D, geom, dz_cl=x)
        ref, S, Kred = r["dx"], r["Sdx"], 27 * CI
        pack_args = (CI, CO, w_cin, 0, 1)
    xd, Wd = x.to(dev), W.to(dev)
    bd = bias.to(dev) if bias is not None else None
    wp = torch.full((int(L.mf_conv3d_k3_narrow_bf16_pack_elems(CI)),), SENT, dtype=BF, device=dev)
    ok(L.mf_conv3d_k3_narrow_bf16_pack(p(Wd), *pack_args, p(wp), st()), L)
    V = B * D ** 3
    out = torch.full((V + 64, CO), SENT, dtype=BF, device=dev)   # 64 rows beyond the last voxel: a partial tile's lanes
    first = None
    for it in range(1 + repeat):
        ok(L.mf_conv3d_k3_narrow_bf16(p(xd), p(wp), p(bd), p(out), B, CI, CO, D, dil, relu, st()), L)
        if repeat:
            if first is None:
                first = out.clone()
            else:
                assert torch.equal(out, first), f"{what}: launch {it} differs"
    got = out.cpu()
    assert float((got[V:].float() - SENT).abs().max()) == 0.0, "rows beyond the last voxel written"
    BB.assert_within(got[:V].reshape(B, D ** 3, CO), ref, S, Kred,
                     f"{what} B{B} {CI}->{CO} D{D} dil{dil} w_cin{w_cin}{' transposed' if transpose else ''}")


def narrow_refusal_case(L, dev, st):
    x = torch.zeros(1, 512, 16, dtype=BF, device=dev)
    wp = torch.zeros(int(L.mf_conv3d_k3_narrow_bf16_pack_elems(16)), dtype=BF, device=dev)
    out = torch.full((512, 16), SENT, dtype=BF, device=dev)
    for CI, CO, D, dil in ((12, 8, 8, 1), (8, 6, 8, 1), (8, 20, 8, 1), (8, 8, 6, 1), (8, 8, 8, 0)):
        assert L.mf_conv3d_k3_narrow_bf16(p(x), p(wp), None, p(out), 1, CI, CO, D, dil, 0, st()) != 0
    assert float((out.float().cpu() - SENT).abs().max()) == 0.0


# --------------------------------------------------------------------------------------------------- bf16_ops.Conv3d
def op_conv3d_case(K, dev, B, Cin, Cout, D, geom, w_cin=None, need_dx=True, seed=8, what="Conv3d"):
    """bf16_ops.Conv3d forward (bias + ReLU) and backward: the reference gradients take the OPERATOR's ReLU mask
    (asserted to differ from the reference's only within the bound), so values and gradients obey the same bound."""
    ks, stride, pad, dil = geom
    torch.manual_seed(seed)
    w_cin = w_cin or Cin
    conv = torch.nn.Conv3d(w_cin, Cout, ks, stride, padding=pad, dilation=dil).to(dev)
    x = torch.randn(B, D ** 3, Cin).to(BF).to(dev).requires_grad_(need_dx)
    out = K.conv3d(x, conv, D)
    Do = BB.conv_out_size(D, ks, stride, pad, dil)
    assert out.shape == (B, Do ** 3, Cout) and out.dtype == BF
    g = torch.randn(out.shape).to(BF)
    out.backward(g.to(dev))
    taps = ks ** 3
    Wfull = torch.zeros(Cout, Cin, ks, ks, ks)
    keep = min(Cin, w_cin)
    Wfull[:, :keep] = conv.weight.detach().cpu().to(BF).float()[:, :keep]
    bias = conv.bias.detach().cpu()
    r0 = BB.conv_ref(x, Wfull, bias, D, geom)
    BB.assert_within(out, F.relu(r0["y"]), r0["Sy"], taps * Cin + 1, f"{what} {Cin}->{Cout} {geom} D{D} fwd")
    mask = BB.relu_mask_agrees(out, r0["y"], r0["Sy"], taps * Cin + 1, f"{what} {Cin}->{Cout} {geom} D{D}")
    dz = g.double() * mask
    r = BB.conv_ref(x, Wfull, None, D, geom, dz_cl=dz, want_dx=need_dx)
    L = K._lib.lib()
    split = int(L.mf_conv3d_bf16_wgrad_default_split(B, Cin, -(-Cout // 8) * 8, Do, ks))
    M = B * Do ** 3
    assert conv.weight.grad.shape == conv.weight.shape
    BB.assert_within(conv.weight.grad[:, :keep], r["dw"][:, :keep], r["Sdw"][:, :keep], M + split,
                     f"{what} {Cin}->{Cout} {geom} D{D} wgrad (split {split})")
    BB.assert_within(conv.bias.grad, dz.reshape(-1, Cout).sum(0), dz.abs().reshape(-1, Cout).sum(0), M,
                     f"{what} {Cin}->{Cout} {geom} D{D} bias grad")
    if need_dx:
        Kd = 8 * Cout if tuple(geom) == (4, 2, 1, 1) else taps * Cout
        BB.assert_within(x.grad, r["dx"], r["Sdx"], Kd, f"{what} {Cin}->{Cout} {geom} D{D} dgrad")
