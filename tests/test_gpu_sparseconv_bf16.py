"""The sparse conv3 of the bf16 training path on the MI355X, stage by stage and bit for bit: every C-ABI entry point
of csrc/sparseconv_bf16.hip and the compact-row / dense bf16 voxelization of csrc/voxelize.hip called directly on the
REFERENCE's tables, every table element and every value's bit pattern equal to the numpy references of
tests/sparseconv_bf16_cases.py (shared with tests/test_emul_sparseconv_bf16.py, which lists the stages and shapes);
then bf16_ops.SparseConv3 end to end, per element under derived bounds."""
import pytest

import sparseconv_bf16_cases as S

pytestmark = pytest.mark.gpu

import morefusion_amd as mf  # noqa: E402
from morefusion_amd.contrib.singleview_3d.models import bf16_ops as K  # noqa: E402

DEV = "cuda"
TABLES = {"faces_B2_D8": lambda: S.points_faces(2, 8) + (2, 8), "faces_B1_D6": lambda: S.points_faces(1, 6) + (1, 6),
          "padding_B3_D16": S.points_class_padding}


@pytest.fixture()
def L():
    return mf._lib.lib()


def st():
    return mf._lib.stream_ptr()


@pytest.mark.parametrize("B,D", [(2, 8), (1, 6)])
def test_index_one_workgroup(L, B, D):
    """One index workgroup of 2048 voxels (D = 6: Vo = 27 is no multiple of 64): coordinates on .5, -0.4, NaN, batch
    indices outside, several points in a voxel; and n = 0."""
    pts, bi = S.points_faces(B, D)
    T = S.index_case(L, DEV, st, pts, bi, B, D, f"index B{B} D{D}")
    S.assert_faces_cover(T, pts, bi, B, D)
    S.index_empty_case(L, DEV, st, B, D)


def test_index_class_padding(L):
    """Classes of exactly 128, 129, 1 and 0 occupied voxels: the next class starts at + 128, + 256, + 128, + 0."""
    pts, bi, B, D = S.points_class_padding()
    S.assert_padding_covers(S.index_case(L, DEV, st, pts, bi, B, D, "index class padding"))


def test_index_prefix_carry(L):
    """48 index workgroups: k_scb_offsets scans them in chunks of 32 and carries the first chunk's total."""
    pts, bi, B, D = S.points_prefix_carry()
    S.assert_carry_covers(S.index_case(L, DEV, st, pts, bi, B, D, "index prefix carry"), D)


@pytest.mark.parametrize("C", [2, 130, 144])
def test_mean_rows(L, C):
    """Mean rows forward / backward through the reference's row map and chains (in a random order), a voxel of 70
    points (the selection path) and one of 64; C = 130: a lane's second trip.  Then the dense form."""
    pts, bi = S.points_faces(2, 8, piles=(70, 64))
    S.mean_rows_case(L, DEV, st, pts, bi, 2, 8, C)


@pytest.mark.parametrize("Cout,Cs,w_cin,c_off", [(8, 8, 24, 8), (16, 16, 16, 0)])
def test_pack_unpack_pack_cols(L, Cout, Cs, w_cin, c_off):
    S.pack_case(L, DEV, st, Cout, Cs, w_cin, c_off)
    S.pack_refusal_case(L, DEV, st)


@pytest.mark.parametrize("Cout", [256, 512])
@pytest.mark.parametrize("tables", sorted(TABLES))
def test_reduce(L, tables, Cout):
    """dense / bias present or NULL x ReLU on / off; NaN in every row of C nothing may read.  Cout = 512: the channel
    loop's second trip."""
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


def test_sparse_conv3_wiring_per_element(L):
    """bf16_ops.SparseConv3 end to end: every element of out, dW (both channel ranges), dfeat and docc under the
    bounds derived in sparseconv_bf16_cases.wiring_case; the worst ratios are printed."""
    ratios = S.wiring_case(K, DEV, what="gpu SparseConv3")
    assert len(ratios) == 12, ratios     # out, 8 classes of dW, dW occupancy, dfeat, docc
