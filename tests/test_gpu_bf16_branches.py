"""Every launcher branch of csrc/gemm_bf16.hip on the MI355X, each case asserting the branch it is for RAN, every
output element against the float64 CPU reference on the same bf16-rounded operands under the derived per-element
bound of tests/bf16_bound.py (no max-norm or percentage gates).  The case bodies are tests/bf16_cases.py, shared
with the emulator tests.

Which branch runs is read from outside where the library shows it -- ``mf_gemm_bf16_last_tile()`` (the 64 / 128 /
256-row NT tile that RAN), ``mf_conv3d_bf16_fwd_workspace_bytes`` (split-K and its S), ``mf_*_wgrad_default_split``,
``mf_gemm_bf16_tn_plan`` (the TN engine's 128 x 128 against its ping-pong form, and the finish kernel: plain, deep --
split >= 32 and a slab of <= 65536 floats -- or the convolution's transpose), a call recorder on
``mf_conv3d_k3_narrow_bf16``.  The launchers' rules are restated in tests/bf16_cases.py (held against the library's
answers over every threshold by tests/test_emul_gemm_bf16_plan.py); the shapes here sit on both sides of each rule.
NOT observable from outside, restated only: the narrow kernel's tiles per wave.

    branch                                   test                                              shape
    NT rows, 64-row tile                     test_linear_rows_tile_by_size[..64]               1000 x 136 x 200 x 3 groups; 300 x 24 x 8
    NT rows, 128-row tile by size            test_linear_rows_tile_by_size[..128]              40010 x 120 x 72; 20001 x 136 x 40 x 2 groups
    NT rows, 256-row ping-pong by size       test_linear_rows_tile_by_size[..256]              15001 x 1000 x 136
    NT rows, group table (64 / 128, -1)      test_linear_tiles_table_and_wgrad_ranges          640 and 38400 rows, 3 / 4 groups
    TN rows, row ranges (empty, unequal)     test_linear_tiles_table_and_wgrad_ranges          4 and 5 ranges up to 13568 rows
    NT conv forward 64 / 128 / 256           test_conv_forward_tile_by_size                    16^3 x 16 -> 72; 2 x 64^3 x 8 -> 64; -> 192
    NT conv forward, split-K by size S = 8   test_conv_forward_split_k_by_size_s8              32^3 x 128 -> 256 (3 launches, same bits)
    NT conv data gradient k4s2 128 / 256     test_conv_k4s2_dgrad_tile_by_size                 16^3 16 -> 24; 2 x 32^3 16 -> 160
    validators (Do, Cin % 8, D = 8 dgrad)    test_refusals_return_the_error_code_...           --
    TN linear 128 x 128 / ping-pong          test_linear_wgrad_both_tn_forms                   196544 / 196608 rows, 4 x 200 x 200
    k_wgrad_finish_deep by default split     test_linear_wgrad_deep_finish_by_default_split    65536 x 64 x 72
                                             test_conv_wgrad_deep_finish_by_default_split      2 x 64^3, k3 s2, 8 -> 16
    TN conv 128 x 128 / ping-pong            test_conv_wgrad_both_tn_forms                     11 / 12 x 32^3, 32 -> 512
    general geometry (conv_geom)             test_general_geometry                             k3 s2 p1; k4 s1 p3 d2; D 10 -> 8; D 9 -> 8
    narrow kernel, channels x dilation       test_narrow_kernel_channels_and_dilations         2 x 8^3, {8,16} -> {4,8,12,16}, dil 1 / 2 / 8
    narrow kernel, partial tile, w_cin < CI  test_narrow_kernel_partial_tiles_and_...          3 / 5 x 2^3; 2 x 16^3 w_cin 1
    narrow kernel, 2 / 4 / 8 tiles per wave  test_narrow_kernel_tiles_per_wave                 16 / 32 / 64 x 32^3
    Conv3d operator on narrow layers         test_conv3d_operator_narrow_layers                8 -> 12, 16 -> 4, 8 -> 8, 16 -> 16
"""
import pytest
import torch

import bf16_cases as C

pytestmark = pytest.mark.gpu

import morefusion_amd as mf  # noqa: E402
from morefusion_amd.contrib.singleview_3d.models import bf16_ops as K  # noqa: E402

DEV = "cuda"


@pytest.fixture()
def L(monkeypatch):
    for v in ("MF_NT_BIG", "MF_NT_SPLITK", "MF_TN_PP", "MF_NT_HALF_MAX", "MF_NARROW_CONV"):   # the launchers' own choice
        monkeypatch.delenv(v, raising=False)
    return mf._lib.lib()


def st():
    return mf._lib.stream_ptr()


nt_tile, nt_splitk, tn_use_pp, deep_finish = C.nt_tile, C.nt_splitk, C.tn_use_pp, C.deep_finish   # (the rules restated)


# ---------------------------------------------------------------------------------------------------------- NT rows
@pytest.mark.parametrize("M,N,K,groups,tile", [(1000, 136, 200, 3, 64), (300, 24, 8, 1, 64), (40010, 120, 72, 1, 128),
                                                (20001, 136, 40, 2, 128), (15001, 1000, 136, 1, 256)])
def test_linear_rows_tile_by_size(L, M, N, K, groups, tile):
    """mf_linear_bf16 on the 64-, 128- and 256-row tile CHOSEN BY SIZE: M and N off the tile, K = 8 and K off the
    K-tile of 64, row pitches beyond the data, groups side by side, bf16 / fp32 / accumulating outputs."""
    assert nt_tile(M, N, groups) == tile
    C.linear_case(L, DEV, st, M, N, K, groups=groups, lda_pad=8, ldo_pad=3, expect_tile=tile, what=f"rows tile {tile}")


def test_linear_tiles_table_and_wgrad_ranges(L):
    """mf_linear_bf16_tiles on both tile heights it can take (a table long enough for the 128-row tile), empty blocks
    in the middle and at the end left untouched; mf_linear_wgrad_bf16_ranges with an empty range and unequal ones."""
    assert C.tiles_case(L, DEV, st, [2, 2, -1, -1, 0, 0, 1, 1, -1, -1], N=72, K=40, n_groups=3, what="tiles 64") == 64
    table = ([0, 0] * 60 + [-1, -1] * 20 + [3, 3] * 100 + [1, 1] * 90 + [2, 2] * 20 + [-1, -1] * 10)
    assert nt_tile(64 * len(table), 136, table=True) == 128
    assert C.tiles_case(L, DEV, st, table, N=136, K=72, n_groups=4, out_f32=1, what="tiles 128") == 128
    C.ranges_case(L, DEV, st, [0, 128, 128, 192, 448], N=24, K=136, what="ranges")
    C.ranges_case(L, DEV, st, [0, 0, 6400, 6464, 6464, 20032], N=264, K=200, what="ranges big")


# ------------------------------------------------------------------------------------------------------ NT conv fwd
@pytest.mark.parametrize("B,Cin,Cout,D,geom,tile", [(1, 16, 72, 16, (4, 2, 1, 1), 64), (2, 8, 64, 64, (4, 2, 1, 1), 128),
                                                     (2, 8, 192, 64, (4, 2, 1, 1), 256)])
def test_conv_forward_tile_by_size(L, B, Cin, Cout, D, geom, tile):
    """mf_conv3d_bf16_fwd on the 64 / 128 / 256-row tile by size, written as a column block (c_off 8) of a wider grid."""
    Do = C.BB.conv_out_size(D, *geom)
    assert nt_tile(B * Do ** 3, Cout) == tile and nt_splitk(B * Do ** 3, Cout, 64 * Cin) == 1
    C.conv_case(L, DEV, st, B, Cin, Cout, D, geom, splits=(1,), ldo_pad=16, c_off=8, expect_tile=tile, expect_ws=0,
                what=f"conv fwd tile {tile}")


def test_conv_forward_split_k_by_size_s8(L):
    """Split-K chosen by size at S = 8 (16 tiles of 256 x 256, 128 K-tiles; the network's conv4 takes S = 4): the
    workspace size implies S; three launches give the same bits."""
    B, Cin, Cout, D = 1, 128, 256, 32
    M = B * 16 ** 3
    assert nt_splitk(M, Cout, 64 * Cin) == 8
    C.conv_case(L, DEV, st, B, Cin, Cout, D, (4, 2, 1, 1), splits=(1,), ldo_pad=8, c_off=8, expect_tile=256,
                expect_ws=8 * M * Cout * 4, repeat=2, what="conv fwd split-K 8")


# ------------------------------------------------------------------------------------------------------- k4s2 dgrad
@pytest.mark.parametrize("B,Cin,Cout,D,tile", [(1, 24, 16, 16, 128), (2, 160, 16, 32, 256)])
def test_conv_k4s2_dgrad_tile_by_size(L, B, Cin, Cout, D, tile):
    """The parity-class data gradient (never the 64-row tile): 128-row by size (one object, Cin < 160) and the 256-row
    form by size; bf16, fp32 and accumulating outputs."""
    assert nt_tile(B * D ** 3, Cin, dgrad_rows=(D // 2) ** 3) == tile
    C.dgrad_k4s2_case(L, DEV, st, B, Cin, Cout, D, expect_tile=tile, what=f"dgrad tile {tile}")


def test_refusals_return_the_error_code_and_leave_outputs_untouched(L):
    C.dgrad_k4s2_refusal(L, DEV, st)
    C.conv_refusal_case(L, DEV, st)
    C.narrow_refusal_case(L, DEV, st)


# --------------------------------------------------------------------------------------------------------------- TN
@pytest.mark.parametrize("M,pp", [(196608, True), (196608 - 64, False)], ids=["ping_pong", "tile128"])
def test_linear_wgrad_both_tn_forms(L, M, pp):
    """mf_linear_wgrad_bf16, four groups of 200 x 200 (off the 128 / 256 tiles): 3072 K-tiles is exactly where
    ``tn_use_pp`` turns to the ping-pong form, one K-tile less stays on the 128 x 128 form.  Split 1, 3 and the
    launcher's own."""
    N = Kc = 200
    assert tn_use_pp(N, Kc, M, 4) == pp
    split = int(L.mf_linear_wgrad_bf16_default_split(M, N, Kc, 4))
    assert split >= 1 and not deep_finish(split, 4 * N * Kc)     # (k_wgrad_finish)
    assert C.tn_plan(L, N, Kc, M, 4) == (256 if pp else 128, split, C.wgrad_finish(split, 4 * N * Kc))   # (the library's answer)
    C.linear_wgrad_case(L, DEV, st, M, N, Kc, 4, splits=sorted({1, 3, split}), what=f"TN linear {'pp' if pp else '128'}")


def test_linear_wgrad_deep_finish_by_default_split(L):
    """A small result with a long reduction: the cost model's own split is >= 32 and the slab <= 65536 floats ->
    k_wgrad_finish_deep; one slab short of 32 takes k_wgrad_finish."""
    M, N, Kc = 65536, 64, 72
    split = int(L.mf_linear_wgrad_bf16_default_split(M, N, Kc, 1))
    assert deep_finish(split, N * Kc) and not deep_finish(31, N * Kc) and not tn_use_pp(N, Kc, M, 1)
    assert C.tn_plan(L, N, Kc, M) == (128, split, 2) and C.tn_plan(L, N, Kc, M, split=31) == (128, split, 1)
    C.linear_wgrad_case(L, DEV, st, M, N, Kc, 1, splits=(31, split), what="TN linear deep finish")


@pytest.mark.parametrize("B,pp", [(12, True), (11, False)], ids=["ping_pong", "tile128"])
def test_conv_wgrad_both_tn_forms(L, B, pp):
    """mf_conv3d_bf16_wgrad 32 -> 512 (k4 s2, 32^3): 16 tiles of 256 x 256 need 768 K-tiles for the ping-pong form --
    12 objects have them, 11 do not.  Split 1 and the launcher's own (k_wgrad_finish_conv: a slab of 2^20 floats)."""
    Cin, Cout, D = 32, 512, 32
    assert tn_use_pp(Cout, 64 * Cin, B * 16 ** 3, 1) == pp
    split = int(L.mf_conv3d_bf16_wgrad_default_split(B, Cin, Cout, 16, 4))
    assert C.tn_plan(L, Cout, 64 * Cin, B * 16 ** 3, conv=True) == (256 if pp else 128, split, 3)   # (k_wgrad_finish_conv)
    C.conv_case(L, DEV, st, B, Cin, Cout, D, (4, 2, 1, 1), splits=sorted({1, split}), expect_tile=256,
                what=f"TN conv {'pp' if pp else '128'}")


# ------------------------------------------------------------------------------------------------- general geometry
@pytest.mark.parametrize("Cin,Cout,D,geom", [(16, 24, 16, (3, 2, 1, 1)), (16, 24, 8, (4, 1, 3, 2)), (16, 24, 10, (3, 1, 0, 1)),
                                             (8, 16, 9, (4, 1, 1, 1))], ids=["k3s2p1", "k4s1p3d2", "k3s1p0_D10", "k4s1p1_D9"])
def test_general_geometry(L, Cin, Cout, D, geom):
    """Forward, weight gradient (split 1, 3 and 32 -- k_wgrad_finish and, with one K-tile of 64 rows in each of the 32
    slabs of four 8^3 outputs, k_wgrad_finish_deep) and, for the stride-1 layer on a power-of-two grid, the data
    gradient through the flipped operand."""
    assert deep_finish(32, Cout * geom[0] ** 3 * Cin) and not deep_finish(3, Cout * geom[0] ** 3 * Cin)
    rows = 4 * C.BB.conv_out_size(D, *geom) ** 3
    assert [C.tn_plan(L, Cout, geom[0] ** 3 * Cin, rows, conv=True, split=s)[2] for s in (1, 3, 32)] == [1, 1, 2]
    C.conv_case(L, DEV, st, 4, Cin, Cout, D, geom, splits=(1, 3, 32), ldo_pad=8, c_off=8, what=f"conv {geom} D{D}")


def test_conv_wgrad_deep_finish_by_default_split(L):
    """k3 s2 p1 on 2 x 64^3 -> 32^3, 8 -> 16: 1024 K-tiles for one small tile -- the launcher's own split reaches the
    deep finish."""
    B, Cin, Cout, D, geom = 2, 8, 16, 64, (3, 2, 1, 1)
    split = int(L.mf_conv3d_bf16_wgrad_default_split(B, Cin, Cout, 32, 3))
    assert deep_finish(split, Cout * 27 * Cin)
    assert C.tn_plan(L, Cout, 27 * Cin, B * 32 ** 3, conv=True) == (128, split, 2)
    C.conv_case(L, DEV, st, B, Cin, Cout, D, geom, splits=(split,), what="conv wgrad deep finish by size")


@pytest.mark.parametrize("D,geom", [(10, (3, 1, 0, 1)), (9, (4, 1, 1, 1))], ids=["k3p0_D10", "k4p1_D9"])
def test_conv3d_operator_refuses_input_gradient_when_input_grid_is_not_a_power_of_two(L, D, geom):
    C.op_conv3d_case(K, DEV, 2, 8, 16, D, geom, need_dx=False, what="Conv3d")
    conv = torch.nn.Conv3d(8, 16, geom[0], geom[1], padding=geom[2], dilation=geom[3]).cuda()
    x = torch.randn(1, D ** 3, 8, device=DEV).to(torch.bfloat16).requires_grad_(True)
    out = K.conv3d(x, conv, D)
    with pytest.raises(RuntimeError, match="output size a power of two"):
        out.backward(torch.ones_like(out))


# ---------------------------------------------------------------------------------------------------- narrow kernel
@pytest.mark.parametrize("CI", [8, 16])
@pytest.mark.parametrize("CO", [4, 8, 12, 16])
def test_narrow_kernel_channels_and_dilations(L, CI, CO):
    """k_conv_k3_narrow_bf16 directly: read channels x written channels, dilation 1, 2 and 8 = D (every tap but the
    centre is padding), forward (bias + ReLU) and the data gradient through the transposed pack."""
    for dil in (1, 2, 8):
        C.narrow_case(L, DEV, st, 2, CI, CO, 8, dil, what="narrow")
        C.narrow_case(L, DEV, st, 2, CI, CO, 8, dil, transpose=True, what="narrow")


def test_narrow_kernel_partial_tiles_and_one_real_input_channel(L):
    """D = 2: 24 voxels (one partial tile of 32) and 40 (a full and a partial one); w_cin = 1 of 8 travelling channels."""
    for B, CI, CO in ((3, 8, 4), (5, 16, 16), (3, 16, 12), (5, 8, 8)):
        C.narrow_case(L, DEV, st, B, CI, CO, 2, 1, what="narrow partial")
        C.narrow_case(L, DEV, st, B, CI, CO, 2, 1, transpose=True, what="narrow partial")
    C.narrow_case(L, DEV, st, 2, 8, 8, 16, 1, w_cin=1, what="narrow w_cin 1")


@pytest.mark.parametrize("B,CI,CO,dil,transpose,tpw,repeat", [(16, 8, 12, 1, False, 2, 0), (32, 16, 4, 2, True, 4, 0),
                                                             (64, 16, 16, 2, False, 8, 2)], ids=["tpw2", "tpw4", "tpw8"])
def test_narrow_kernel_tiles_per_wave(L, B, CI, CO, dil, transpose, tpw, repeat):
    """16 / 32 / 64 objects of 32^3: a wave walks 2 / 4 / 8 tiles (the launcher's rule restated: C.narrow_tpw; not
    observable from outside).  Every voxel of every object is compared; three launches at 8 give the same bits."""
    assert C.narrow_tpw(B, 32) == tpw and C.narrow_tpw(2, 32) == 1
    C.narrow_case(L, DEV, st, B, CI, CO, 32, dil, transpose=transpose, repeat=repeat, what=f"narrow tpw {tpw}")


@pytest.mark.parametrize("Cin,Cout,D,dil", [(8, 12, 16, 1), (16, 4, 16, 2), (8, 8, 8, 1), (16, 16, 8, 2)])
def test_conv3d_operator_narrow_layers(L, monkeypatch, Cin, Cout, D, dil):
    """bf16_ops.Conv3d on narrow layers with the input gradient wanted, 4 and 12 written channels included (their
    output gradient travels zero-padded to 8 / 16 channels): forward and data gradient on the narrow kernel
    (recorded), weight gradient on the TN engine."""
    calls = []
    real = L.mf_conv3d_k3_narrow_bf16
    monkeypatch.setattr(L, "mf_conv3d_k3_narrow_bf16", lambda *a: (calls.append(a[5:9]), real(*a))[1], raising=False)
    C.op_conv3d_case(K, DEV, 2, Cin, Cout, D, (3, 1, dil, dil), what="Conv3d narrow")
    assert calls == [(Cin, Cout, D, dil), (-(-Cout // 8) * 8, Cin, D, dil)]
