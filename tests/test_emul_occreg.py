"""csrc/occreg.hip through the host emulator (tests/host_emul), bitwise against the NumPy mirror tests/occreg_ref.py,
and the mirror itself against the dense formulation (oracle/oracle_np.py): the pruning is exact, the per-point
gradients are within the float32 summation bound of a float64 evaluation.  No GPU."""
import numpy as np
import pytest

import occreg_cases as C
import occreg_ref as R
from host_emul import emul
from oracle import oracle_np as O

needs_gxx = pytest.mark.skipif(not emul.available(), reason="g++ not available")


class EmulBackend:
    def __init__(self):
        self.lib = emul.build(["occreg.hip"])

    to_dev = staticmethod(lambda a: a)
    to_np = staticmethod(lambda a: a)
    ptr = staticmethod(emul.ptr)


@pytest.fixture(scope="module")
def be():
    return EmulBackend()


@pytest.mark.parametrize("index", C.FINITE + (C.NAN_OBJECT,))
def test_mirror_grid_equals_the_dense_formulation_bit_for_bit(index):
    """m of the pruned scatter == oracle_np.occupancy_grid_3d (every voxel against every point) of the moved points."""
    o = C.batch_objects()[index]
    occ, unocc = C.occ_unocc(o)
    _, _, _, aux = C.mirror_loss_grad(o, aux=True)
    # (the dense formulation is fed the grid coordinates themselves, pitch 1 at origin 0: (pf - 0) / 1 == pf)
    dense = O.occupancy_grid_3d(aux["pf"], pitch=np.float32(1.0), origin=np.zeros(3, np.float32), dims=occ.shape,
                                threshold=o["thr"])
    assert C.same_bits(aux["m"], dense)
    assert (int((dense > 0).sum()) == 0) == (index == C.NAN_OBJECT)


@pytest.mark.parametrize("index", C.FINITE)
def test_mirror_point_gradients_within_the_float32_bound_of_float64(index):
    """|g - g64| <= (n + 2) 2^-23 sum|term| per point and component, n = voxels that select the point."""
    o = C.batch_objects()[index]
    _, _, _, aux = C.mirror_loss_grad(o, aux=True)
    g64 = R.point_gradients_f64(aux, o["pitch"])
    bound = (aux["n"][:, None] + 2) * 2.0 ** -23 * aux["absum"]
    err = np.abs(aux["g"].astype(np.float64) - g64)
    print("max error / bound", float((err / np.maximum(bound, 1e-300)).max()), "selected", int(aux["n"].sum()))
    assert np.isfinite(aux["g"]).all() and aux["n"].sum() > 0
    assert (err <= bound).all()


def test_mirror_micro_cases_against_the_dense_backward():
    """Ties, the reference's known answer, the NaN of a point on a voxel centre: the mirror's point gradients against
    oracle_np.occupancy_grid_3d_backward fed with the mirror's d loss / d m."""
    for k, o in enumerate((C.micro_tie(), C.micro_known_answer(), C.micro_on_centre())):
        occ, unocc = C.occ_unocc(o)
        _, _, _, aux = C.mirror_loss_grad(o, aux=True)
        A, Sm, Bq, So = aux["sums"]
        gm = (unocc * np.float32(1 / Sm) - np.float32((A / Sm) / Sm)) - occ * np.float32(1 / So)
        with np.errstate(all="ignore"):
            dense = O.occupancy_grid_3d_backward(gm.astype(np.float32), aux["pf"], pitch=np.float32(1.0),
                                                 origin=np.zeros(3, np.float32), dims=occ.shape, threshold=o["thr"])
        dense = dense / o["pitch"]
        if k == 2:
            assert np.isnan(aux["g"][0]).all() and np.isnan(dense[0]).all()
            np.testing.assert_allclose(aux["g"][1], dense[1], rtol=1e-5, atol=1e-7)
        else:
            np.testing.assert_allclose(aux["g"], dense, rtol=1e-5, atol=1e-7)
    assert int((C.mirror_loss_grad(C.micro_known_answer(), aux=True)[3]["m"] > 0).sum()) == 6


@needs_gxx
def test_loss_grad_bitwise_vs_mirror(be):
    C.check_loss_grad_bitwise(be)


@needs_gxx
@pytest.mark.parametrize("n_iter", [1, 2, 7])
def test_refine_bitwise_vs_mirror(be, n_iter):
    C.check_refine_bitwise(be, n_iter)


@needs_gxx
def test_refine_across_launches_bitwise_vs_mirror(be):
    C.check_refine_across_launches(be)


@needs_gxx
def test_micro_cases(be):
    C.check_micro_cases(be)


@needs_gxx
def test_loss_grad_vs_executed_reference(be):
    C.check_against_executed_reference(be)
