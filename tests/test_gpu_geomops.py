"""The first-generation geometry kernels on the MI355X (csrc/occgrid_knn.hip: k_occgrid_fwd / _bwd, k_nn, k_icp,
k_icp_step; csrc/tdf.hip: k_tdf_fwd<3> / <0>, k_tdf_bwd, k_pocc_wraw / _grids): the cases of tests/geomops_cases.py
(its docstrings say which case reaches which branch and which reference rule is pinned) against the float32 mirror, bit
for bit, and the float64 references and a-priori bounds of tests/geomops_ref.py -- the same bodies as
tests/test_emul_geomops.py, where LDS and global atomics run one at a time; here they race.  The ulp figures of the
device's sqrtf and divide behind the bounds are ASSUMED (2 ulp), not measured.

Worst |got - ref| / bound per kernel, measured on one run, shows slack only (the bounds are derived in geomops_ref.py,
never fitted):

    k_occgrid_fwd 0.257   k_occgrid_bwd 0.254   k_nn 0.579   k_icp 0.250   mf_icp_refine (losses) 0.050
    k_tdf_fwd 0.281       k_tdf_bwd 0.325       k_pocc_wraw / k_pocc_grids 0.188
"""
import pytest

import geomops_cases as C
import geomops_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    R.report()


@pytest.mark.parametrize("dims", C.OCC_DIMS)
@pytest.mark.parametrize("P", C.OCC_PS)
def test_occupancy_grid_every_element_within_its_bound(P, dims):
    C.check_occgrid(DEV, C.occ_case(P, dims), f"P={P} dims={dims}")


@pytest.mark.parametrize("thr", C.EXACT_THRS)
def test_occupancy_grid_backward_edges_in_exact_numbers(thr):
    C.check_occgrid_exact(DEV, thr)


def test_occupancy_grid_one_point_nearest_to_hundreds_of_voxels():
    C.check_occgrid_one_point_many_voxels(DEV)


def test_occupancy_grid_nan_point_and_no_point():
    C.check_occgrid_nan_and_empty(DEV)


@pytest.mark.parametrize("Q", C.NN_QS)
@pytest.mark.parametrize("Rn", C.NN_RS)
def test_nn_indices_and_distances(Rn, Q):
    C.check_nn(DEV, Rn, Q)


def test_nn_nan_query_and_nan_reference():
    C.check_nn_nan(DEV)


@pytest.mark.parametrize("Tn", C.ICP_TS)
@pytest.mark.parametrize("S", C.ICP_SS)
def test_icp_loss_and_gradient_within_their_bounds(S, Tn):
    C.check_icp(DEV, S, Tn)


@pytest.mark.parametrize("lo,hi", C.ICP_TIE_PAIRS)
def test_icp_equidistant_sources_lowest_index_wins(lo, hi):
    C.check_icp_equidistant(DEV, lo, hi)


def test_icp_threshold_edge_and_nan_source():
    C.check_icp_thresh_edge_and_nan(DEV)


@pytest.mark.parametrize("L", C.REFINE_LS)
def test_icp_refine_batches_steps_and_losses(L):
    C.check_refine(DEV, L)


@pytest.mark.parametrize("ks", C.TDF_KS)
@pytest.mark.parametrize("P", C.TDF_PS)
def test_tdf_chunk_paths_and_kernel_sizes(P, ks):
    C.check_tdf_chunks(DEV, P, ks)


@pytest.mark.parametrize("dims", C.TDF_TILE_DIMS)
def test_tdf_partial_last_y_tile(dims):
    C.check_tdf_partial_tile(DEV, dims)


def test_tdf_truncation_edge_voxel_centre_and_no_point():
    C.check_tdf_edges(DEV)


def test_tdf_backward_one_point_owning_343_voxels():
    C.check_tdf_one_point_many_voxels(DEV)


def test_tdf_z_4096_runs_and_4097_is_refused():
    """Buffers of 4096 and 4097 voxels really exist; the refusal returns before any launch."""
    C.check_tdf_z_limit(DEV)


@pytest.mark.parametrize("dims", C.POCC_DIMS)
def test_pseudo_occupancy_grids(dims):
    C.check_pocc(DEV, dims)


def test_pseudo_occupancy_all_weights_negative_gives_nan_grids():
    C.check_pocc(DEV, (5, 13, 1), negative=True)
