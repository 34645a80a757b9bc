"""The sparse conv3 of the bf16 training path on the CPU, stage by stage and bit for bit: the kernel text of
csrc/sparseconv_bf16.hip and of the compact-row voxelization (csrc/voxelize.hip) on the emulated library, CPU tensors
as device memory, every C-ABI entry point called directly on the REFERENCE's tables (tests/sparseconv_bf16_cases.py;
tests/test_gpu_sparseconv_bf16.py runs the same cases on the MI355X).

    stage                                         test                                   shapes
    index, one index workgroup                    test_index_one_workgroup               B2 D8, B1 D6 (Vo = 27); n = 0
    index, class padding (128 / 129 / 1 / 0)      test_index_class_padding               B3 D16: 6 index workgroups
    index, prefix carry over 32-workgroup chunks  test_index_prefix_carry                B3 D32: 48 index workgroups
    mean rows fwd / bwd, compact and dense        test_mean_rows                         C 2 / 130 / 144, piles of 70 and 64
    pack / unpack_dw / pack_cols, refusals        test_pack_unpack_pack_cols             Cout 8 Cs 8 of 24 at 8; 16 / 16
    reduce                                        test_reduce                            3 tables x Cout 256 / 512; 264 refused
    gather_dy                                     test_gather_dy                         3 tables x Cout 8 / 256 / 520
    col2im                                        test_col2im                            B2, D 6 / 8, Cin 8 / 16; 12 refused
    the operator end to end, per element          test_sparse_conv3_wiring_per_element   B2 D8 16 + 8 -> 256
"""
import pytest

import sparseconv_bf16_cases as S
from host_emul import emul

pytestmark = pytest.mark.skipif(not emul.available(), reason="g++ not available")

DEV = "cpu"
TABLES = {"faces_B2_D8": lambda: S.points_faces(2, 8) + (2, 8), "faces_B1_D6": lambda: S.points_faces(1, 6) + (1, 6),
          "padding_B3_D16": S.points_class_padding}


@pytest.fixture(scope="module")
def L():
    return emul.build(["gemm_bf16.hip", "sparseconv_bf16.hip", "voxelize.hip"])


def st():
    return None


@pytest.mark.parametrize("B,D", [(2, 8), (1, 6)])
def test_index_one_workgroup(L, B, D):
    pts, bi = S.points_faces(B, D)
    T = S.index_case(L, DEV, st, pts, bi, B, D, f"index B{B} D{D}")
    S.assert_faces_cover(T, pts, bi, B, D)
    S.index_empty_case(L, DEV, st, B, D)


def test_index_class_padding(L):
    pts, bi, B, D = S.points_class_padding()
    S.assert_padding_covers(S.index_case(L, DEV, st, pts, bi, B, D, "index class padding"))


def test_index_prefix_carry(L):
    pts, bi, B, D = S.points_prefix_carry()
    S.assert_carry_covers(S.index_case(L, DEV, st, pts, bi, B, D, "index prefix carry"), D)


@pytest.mark.parametrize("C", [2, 130, 144])
def test_mean_rows(L, C):
    pts, bi = S.points_faces(2, 8, piles=(70, 64))
    S.mean_rows_case(L, DEV, st, pts, bi, 2, 8, C)


@pytest.mark.parametrize("Cout,Cs,w_cin,c_off", [(8, 8, 24, 8), (16, 16, 16, 0)])
def test_pack_unpack_pack_cols(L, Cout, Cs, w_cin, c_off):
    S.pack_case(L, DEV, st, Cout, Cs, w_cin, c_off)
    S.pack_refusal_case(L, DEV, st)


@pytest.mark.parametrize("Cout", [256, 512])
@pytest.mark.parametrize("tables", sorted(TABLES))
def test_reduce(L, tables, Cout):
    pts, bi, B, D = TABLES[tables]()
    S.reduce_case(L, DEV, st, pts, bi, B, D, Cout)


def test_reduce_refuses_cout_264(L):
    S.reduce_refusal_case(L, DEV, st)


@pytest.mark.parametrize("Cout", [8, 256, 520])
@pytest.mark.parametrize("tables", sorted(TABLES))
def test_gather_dy(L, tables, Cout):
    pts, bi, B, D = TABLES[tables]()
    S.gather_case(L, DEV, st, pts, bi, B, D, Cout)


@pytest.mark.parametrize("Cin", [8, 16])
@pytest.mark.parametrize("D", [6, 8])
def test_col2im(L, D, Cin):
    S.col2im_case(L, DEV, st, 2, D, Cin)
    S.col2im_refusal_case(L, DEV, st)


def test_sparse_conv3_wiring_per_element(L, monkeypatch):
    from morefusion_amd.contrib.singleview_3d.models import bf16_ops
    emul.patch_lib(L, monkeypatch)
    ratios = S.wiring_case(bf16_ops, DEV, what="emul SparseConv3")
    assert len(ratios) == 12, ratios     # out, 8 classes of dW, dW occupancy, dfeat, docc
