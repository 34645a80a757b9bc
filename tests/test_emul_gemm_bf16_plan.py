"""The launch plans of csrc/gemm_bf16.hip (nt_plan / tn_plan) without a GPU: the host-emulated build answers
``mf_gemm_bf16_nt_plan`` / ``mf_gemm_bf16_tn_plan`` with the very functions the launchers use, and every answer is held
against the rules restated in tests/bf16_cases.py -- the restatements tests/test_gpu_bf16_branches.py asserts
``mf_gemm_bf16_last_tile()`` against on the MI355X.  The grid has both neighbours of every threshold (224 tiles of
256 x 256, N 160, 255 tiles of 128 x 128, N 192, 16 .. 159 tiles and 16 K-tiles per split, 192 x 192 and 48 x fill
K-tiles, split 32, slabs of 65536 and 2^20 floats), with and without a group table, data gradients with 256 | Do^3 and
not, one and three groups, under every setting of the MF_NT_BIG / MF_NT_SPLITK / MF_TN_PP / MF_NT_HALF_MAX knobs.
Arithmetic only: nothing is launched.  Also here: MF_PP_DBG must not reach a default build's kernels."""
import itertools

import pytest

import bf16_cases as C
from host_emul import emul

pytestmark = pytest.mark.skipif(not emul.available(), reason="g++ not available")

KNOBS = ("MF_NT_BIG", "MF_NT_SPLITK", "MF_TN_PP", "MF_NT_HALF_MAX", "MF_PP_DBG")
# (MF_NT_BIG, MF_NT_SPLITK, MF_TN_PP, MF_NT_HALF_MAX); None = not set.  A forced split of 3 lies within the K-tile
# count of every K below but the smallest (one K-tile), 300 beyond all of them.  The first setting is the default, so
# the non-default MF_NT_HALF_MAX at the end is set after the library has been called.
SETTINGS = [(None, None, None, None), (0, None, None, None), (1, None, None, None), (2, None, None, None),
            (None, 3, None, None), (None, 300, None, None), (2, 3, None, None), (2, 300, None, None),
            (None, None, 0, None), (2, None, 0, None), (None, None, None, 100)]

NT_M = sorted({1, 128 * 100, 128 * 100 + 1, 128 * 255, 128 * 255 + 1} |
              {256 * t + d for t in (15, 16, 159, 160, 223, 224, 255, 256) for d in (0, 1)})
NT_N = (128, 159, 160, 191, 192, 196, 256, 264)            # (196: not a multiple of 8 -- never split)
NT_K = (24, 64 * 255, 64 * 255 + 24, 64 * 256 + 8)          # 1, 255, 256 and 257 K-tiles; multiples of 24 = 3 Kp


def nt_points():
    """(mode, M, N, K, groups, table, dgrad_rows, may_split, have_ws)"""
    for M, N in itertools.product(NT_M, NT_N):
        for groups, table in itertools.product((1, 3), (False, True)):
            yield (C.MODE_ROWS, M, N, NT_K[1], groups, table, 0, False, False)
        for groups, rows in itertools.product((1, 3), (512, 640)):   # Do^3 a multiple of 256, and of 128 only
            yield (C.MODE_DGRAD, M, N, NT_K[1], groups, False, rows, False, False)
        for K, have_ws in itertools.product(NT_K, (False, True)):
            yield (C.MODE_ROWS_SPLIT, M, N, K, 1, False, 0, True, have_ws)


def tn_points():
    """(Ni, Nj, ldc, rows, groups, ranges, conv, split)"""
    shapes = [(191, 192, 1), (192, 191, 1), (192, 192, 1), (192, 192, 3), (512, 512, 1), (4096, 4096, 1), (4096, 4104, 1),
              (64, 1024, 1), (8, 8192, 1), (1024, 1024, 1), (1016, 1024, 1)]
    for Ni, Nj, groups in shapes:
        tiles = -(-Ni // 256) * -(-Nj // 256) * groups
        edge = 48 * (1 if tiles >= 256 else -(-256 // tiles))   # 1, 3, 4 and >= 256 result tiles: 48 x fill K-tiles
        for ktiles in (1, 47, 48, edge - 1, edge, 4 * edge):
            for rows in (64 * ktiles - 63, 64 * ktiles):
                for ranges, conv in ((False, False), (False, True), (True, False)):
                    for split in (0, 1, 31, 32):
                        yield (Ni, Nj, Nj, rows, groups, ranges, conv, split)
    for ldc, split in itertools.product((65536, 65537), (31, 32)):   # a slab of 65536 / 65537 floats
        yield (1, 8, ldc, 64 * 100, 1, False, False, split)
        yield (1, ldc, ldc, 64 * 100, 1, False, True, split)
    for Ni in (1023, 1024):                                            # a convolution's slab of 2^20 floats, and below
        yield (Ni, 1024, 1024, 64 * 100, 1, False, True, 4)


@pytest.fixture(scope="module")
def L():
    return emul.build(["gemm_bf16.hip"])


def set_knobs(monkeypatch, setting):
    for name, value in zip(KNOBS, tuple(setting) + (None,)):
        if value is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, str(value))


def test_plans_equal_the_restated_rules_on_both_sides_of_every_threshold(L, monkeypatch):
    nt, tn = list(nt_points()), list(tn_points())
    for big, forced, tn_pp, half_max in SETTINGS:
        set_knobs(monkeypatch, (big, forced, tn_pp, half_max))
        for pt in nt:
            mode, M, N, K, groups, table, dgrad_rows, may_split, have_ws = pt
            S = C.nt_splitk(M, N, K, big=big, forced=forced or 0) if may_split and have_ws else 1
            tile = C.nt_tile(M, N, groups, table, dgrad_rows, S=S, big=big, half_max=255 if half_max is None else half_max)
            assert C.nt_plan(L, *pt) == (tile, S), (pt, big, forced, half_max)
            if may_split and have_ws:   # the size every *_workspace_bytes function answers (one of them: any M, N, K)
                assert L.mf_linear_split_workspace_bytes(M, N, K // 3) == (S * M * N * 4 if S > 1 and N % 8 == 0 else 0), pt
        for pt in tn:
            Ni, Nj, ldc, rows, groups, ranges, conv, split = pt
            pp = C.tn_use_pp(Ni, Nj, rows, groups, ranges=ranges, big=big, tn_pp=tn_pp)
            form, default, finish = C.tn_plan(L, Ni, Nj, rows, groups, ldc, ranges, conv, split)
            assert form == (256 if pp else 128), (pt, big, tn_pp)
            assert finish == C.wgrad_finish(split or default, Ni * ldc * groups, conv), (pt, big, tn_pp)
            if not pp:   # (the exported cost model is the 128 x 128 form's)
                assert default == L.mf_wgrad_split(-(-Ni // 128) * -(-Nj // 128) * groups, -(-rows // 64), Ni * Nj * 4 * groups)
            if not ranges:
                assert default == L.mf_linear_wgrad_bf16_default_split(rows, Ni, Nj, groups), (pt, big, tn_pp)
    assert len(nt) * len(SETTINGS) > 20000 and len(tn) * len(SETTINGS) > 10000   # (the grid did not shrink to nothing)


CONV3 = [(1, 128, 256, 32, 4, 2, 1, 1), (2, 128, 256, 32, 4, 2, 1, 1), (1, 32, 192, 64, 4, 2, 1, 1), (1, 64, 192, 16, 3, 1, 1, 1),
         (16, 256, 512, 16, 4, 2, 1, 1), (1, 8, 184, 32, 4, 2, 1, 1)]
CONV2 = [(1, 512, 512, 64, 3, 1, 1, 1), (1, 128, 256, 64, 1, 1, 0, 1), (2, 64, 192, 128, 3, 2, 1, 1), (1, 1024, 2048, 32, 3, 1, 2, 2),
         (1, 8, 64, 64, 3, 1, 1, 1)]


def test_workspace_sizes_and_default_splits_are_the_plans(L, monkeypatch):
    """Every *_workspace_bytes function answers S * M * N * 4 of the plan (0 at S = 1), every *_default_split the plan's
    split, under every knob setting."""
    split_k = 0
    for setting in SETTINGS:
        set_knobs(monkeypatch, setting)

        def want(mode, M, N, K):
            S = C.nt_plan(L, mode, M, N, K, may_split=True, have_ws=True)[1]
            return S * M * N * 4 if S > 1 else 0

        for B, Cin, Cout, D, ks, stride, pad, dil in CONV3:
            Do = C.BB.conv_out_size(D, ks, stride, pad, dil)
            ws = L.mf_conv3d_bf16_fwd_workspace_bytes(B, Cin, Cout, D, ks, stride, pad, dil)
            assert ws == want(C.MODE_CONV, B * Do ** 3, Cout, ks ** 3 * Cin)
            split_k += ws > 0
            if (ks, stride, pad, dil) == (4, 2, 1, 1):
                assert L.mf_conv3d_k4s2_split_workspace_bytes(B, Cin, Cout, D) == want(C.MODE_CONV3_SPLIT, B * Do ** 3, Cout, 64 * 3 * Cin)
            default = C.tn_plan(L, Cout, ks ** 3 * Cin, B * Do ** 3, conv=True)[1]
            assert L.mf_conv3d_bf16_wgrad_default_split(B, Cin, Cout, Do, ks) == default
            if (ks, stride, pad, dil) == (4, 2, 1, 1):
                assert L.mf_conv3d_k4s2_bf16_wgrad_default_split(B, Cin, Cout, D) == default
        for B, Cin, Cout, D, ks, stride, pad, dil in CONV2:
            Do = (D + 2 * pad - dil * (ks - 1) - 1) // stride + 1
            ws = L.mf_conv2d_split_workspace_bytes(B, Cin, Cout, D, ks, stride, pad, dil)
            assert ws == want(C.MODE_CONV2_SPLIT, B * Do * Do, Cout, ks * ks * 3 * Cin)
            split_k += ws > 0
        for M, N, Kp in ((4096, 256, 2048), (4096, 248, 2048), (16 * 1000, 1920, 328), (300, 1000, 8)):
            assert L.mf_linear_split_workspace_bytes(M, N, Kp) == want(C.MODE_ROWS_SPLIT, M, N, 3 * Kp)
            assert L.mf_linear_wgrad_bf16_default_split(M, N, Kp, 3) == C.tn_plan(L, N, Kp, M, groups=3)[1]
    assert split_k >= 20   # (the shapes do split)


def test_plan_queries_refuse_malformed_questions(L):
    import ctypes
    out = [ctypes.byref(ctypes.c_int32()) for _ in range(3)]
    assert L.mf_gemm_bf16_nt_plan(6, 100, 128, 64, 1, 0, 0, 0, 0, *out[:2]) < 0
    assert L.mf_gemm_bf16_nt_plan(0, 100, 128, 64, 1, 0, 0, 0, 0, None, out[0]) < 0
    assert L.mf_gemm_bf16_tn_plan(64, 64, 56, 100, 1, 0, 0, 0, *out) < 0


def test_pp_dbg_in_the_environment_does_not_reach_a_default_build(L, monkeypatch):
    """MF_PP_DBG=1 skips the ping-pong kernel's operand requests after K-tile 0 (a timing ablation): only a build with
    -DMF_PP_ABLATE may read it.  One 256-row tile, K = 136 (three K-tiles), every element under its bound."""
    set_knobs(monkeypatch, (2, None, None, None))
    monkeypatch.setenv("MF_PP_DBG", "1")
    C.linear_case(L, "cpu", lambda: None, 200, 136, 136, expect_tile=256, forms=((1, 0),), what="MF_PP_DBG=1, default build")
