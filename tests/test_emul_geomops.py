"""The first-generation geometry kernels' TEXT (csrc/occgrid_knn.hip, csrc/tdf.hip) on the host emulator: the cases of
tests/geomops_cases.py (its docstrings say which case reaches which branch and which reference rule is pinned) against
the float32 mirror, bit for bit, and the float64 references and a-priori bounds of tests/geomops_ref.py.  The same
bodies run on the MI355X in tests/test_gpu_geomops.py; the ``P * K`` refusal runs here only (its P is not backed by
memory)."""
import numpy as np
import pytest

import geomops_cases as C
import geomops_ref as R
from host_emul import emul

pytestmark = pytest.mark.skipif(not emul.available(), reason="g++ not available")

DEV = "cpu"


@pytest.fixture(scope="module")
def geom_lib():
    return emul.build(["occgrid_knn.hip", "tdf.hip"])


@pytest.fixture(autouse=True)
def _emulated(geom_lib, monkeypatch):
    emul.patch_lib(geom_lib, monkeypatch)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    R.report()


# ---- the references stand on their own feet -----------------------------------------------------------------------------
def test_reference_gradients_agree_with_central_differences():
    """geomops_ref.occgrid_bwd / tdf_bwd / icp against central differences of their own float64 forwards."""
    c = C.occ_case(1023, (4, 8, 8))
    args = (c["pitch"], c["origin"], c["dims"], c["thr"])
    (_, dmin), _ = R.occgrid(c["points"], *args)
    gp, _ = R.occgrid_bwd(c["ggrid"], c["points"], *args, dmin.astype(np.float32))
    hit = np.flatnonzero(np.abs(gp).sum(axis=1) > 0)
    assert len(hit) > 3

    def occ_value(pts):
        _, _, d, _ = R._occ_geometry(pts, c["pitch"], c["origin"], c["dims"])
        return (np.clip(c["thr"] - d.min(axis=1), 0, 1) * c["ggrid"].reshape(-1).astype(np.float64)).sum()
    # the float64 forward on float64 points: voxel_coords casts to float32, so difference its formula directly
    for p in hit[:3]:
        for i in range(3):
            v = []
            for sgn in (1, -1):
                q, _ = R.voxel_coords(c["points"], c["pitch"], c["origin"])
                q[p, i] += sgn * 1e-6 / c["pitch"]
                d = np.sqrt(((R._voxels(c["dims"])[:, None, :] - q[None]) ** 2).sum(-1)).min(axis=1)
                v.append((np.clip(c["thr"] - d, 0, 1) * c["ggrid"].reshape(-1).astype(np.float64)).sum())
            np.testing.assert_allclose(gp[p, i], (v[0] - v[1]) / 2e-6, rtol=1e-5, atol=1e-6)
    ci = C.icp_case(33, 9)
    ref = R.icp(ci["source"], ci["target"], ci["Rt"], C.ICP_THRESH)
    for j in (0, 4, 8, 9, 11):
        v = []
        for sgn in (1, -1):
            Rt = ci["Rt"].astype(np.float64).copy()
            Rt[j] += sgn * 1e-7
            img = ci["source"].astype(np.float64) @ Rt[:9].reshape(3, 3).T + Rt[9:]
            k = ref["match"]
            d = img[k[k >= 0]] - ci["target"][k >= 0].astype(np.float64)
            v.append((d * d).sum())
        np.testing.assert_allclose(ref["out"][4 + j], (v[0] - v[1]) / 2e-7, rtol=1e-5, atol=1e-9)


# ---- occupancy_grid_3d ------------------------------------------------------------------------------------------------------
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


# ---- nn -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Q", C.NN_QS)
@pytest.mark.parametrize("Rn", C.NN_RS)
def test_nn_indices_and_distances(Rn, Q):
    C.check_nn(DEV, Rn, Q)


def test_nn_nan_query_and_nan_reference():
    C.check_nn_nan(DEV)


# ---- ICP ------------------------------------------------------------------------------------------------------------------------
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


# ---- truncated distance function --------------------------------------------------------------------------------------------------
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
    C.check_tdf_z_limit(DEV)


def test_tdf_refuses_candidate_ids_beyond_32_bits(geom_lib):
    """P * K >= 2^32 - 1 returns before any launch: the point buffer holds three rows, P says 159 072 863 (x 27)."""
    pts = np.zeros((3, 3), np.float32)
    tdf, flat = np.full((4, 4, 4), C.SENT, np.float32), np.full((4, 4, 4), C.ISENT, np.int32)
    P = -(-(2 ** 32 - 1) // 27)
    rc = geom_lib.mf_truncated_distance_function_fwd(pts.ctypes.data, P, 1.0, 0.0, 0.0, 0.0, 4, 4, 4, 1.5,
                                                     tdf.ctypes.data, flat.ctypes.data, None)
    assert rc != 0 and (tdf == C.SENT).all() and (flat == C.ISENT).all()
    assert geom_lib.mf_truncated_distance_function_fwd(pts.ctypes.data, 3, 1.0, 0.0, 0.0, 0.0, 4, 4, 4, 1.5,
                                                       tdf.ctypes.data, flat.ctypes.data, None) == 0


# ---- pseudo occupancy ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", C.POCC_DIMS)
def test_pseudo_occupancy_grids(dims):
    C.check_pocc(DEV, dims)


def test_pseudo_occupancy_all_weights_negative_gives_nan_grids():
    C.check_pocc(DEV, (5, 13, 1), negative=True)
