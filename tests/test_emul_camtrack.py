"""csrc/camtrack.hip (with csrc/pickorder.hip for the normals) through the host emulator behind the product's Python
layer (contrib.camera_tracking; torch CPU tensors as device memory): the cases (a) .. (d) of tests/camtrack_cases.py,
every pyramid level, vertex and normal map, every iteration's statistics and the final pose bitwise equal to the
NumPy mirror (tests/camtrack_ref.py)."""
import numpy as np
import pytest

import camtrack_cases as C
import camtrack_ref as R
from host_emul import emul

pytestmark = pytest.mark.skipif(not emul.available(), reason="g++ not available")


@pytest.fixture()
def product(monkeypatch):
    L = emul.build(["camtrack.hip", "pickorder.hip"])
    emul.patch_lib(L, monkeypatch)


def test_a_odd_coarse_level_and_ragged_workgroups(product):
    case = C.make_case("a")
    got, exp = C.run_product(case, "cpu"), C.run_mirror(case)
    C.assert_equal(got, exp)
    assert exp["cur"][1]["depth"].shape == (1, 15, 20)
    assert exp["status"].tolist() == [R.TRACKING] and (exp["stats"][0, :, 0] >= 20).all()
    assert not np.array_equal(exp["pose"], C.initial_pose(case))  # it moved


def test_b_a_lost_alignment_leaves_its_neighbour_alone(product):
    case = C.make_case("b")
    got, exp = C.run_product(case, "cpu"), C.run_mirror(case)
    C.assert_equal(got, exp)
    assert got["status"].tolist() == [R.TRACKING, R.LOST_PAIRS]
    assert np.array_equal(got["pose"][1], C.initial_pose(case)[1])
    assert np.allclose(got["T"][1], case["T_ref"][1], rtol=0, atol=1e-15)
    assert not got["stats"][1].any() and (got["stats"][0, :, 0] > 0).all()
    alone = {k: (v[:1] if isinstance(v, np.ndarray) and k != "K" else v) for k, v in case.items()}
    one = C.run_product(alone, "cpu")
    for k in ("pose", "T", "stats", "status"):
        assert np.array_equal(one[k][0], got[k][0]), k


def test_c_min_pairs_out_of_reach_is_lost_at_iteration_0(product):
    case = C.make_case("c")
    got, exp = C.run_product(case, "cpu"), C.run_mirror(case)
    C.assert_equal(got, exp)
    assert got["status"].tolist() == [R.LOST_PAIRS]
    assert got["stats"][0, 0, 0] > 0 and got["stats"][0, 0, 2] == 0 and not got["stats"][0, 1:].any()
    assert np.array_equal(got["pose"], C.initial_pose(case))


def test_d_levels_with_zero_iterations_are_skipped(product):
    case = C.make_case("d")
    got, exp = C.run_product(case, "cpu"), C.run_mirror(case)
    C.assert_equal(got, exp)
    assert got["stats"].shape == (1, 3, 3) and got["status"].tolist() == [R.TRACKING]
    assert exp["cur"][2]["depth"].shape == (1, 12, 17)
    # level 0 has 50 * 70 pixels: the pair counts are those of the finest level, not of a coarser one
    assert (got["stats"][0, :, 0] > 12 * 17 + 25 * 35).all()
