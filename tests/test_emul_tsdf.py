"""csrc/tsdf.hip through the host emulator behind the product's Python layer (contrib.TsdfVolume; torch CPU tensors as
device memory): the cases (a) .. (e) of tests/tsdf_cases.py -- the volume's bytes after every integrate, depth and end
code of every ray-cast -- bitwise equal to the NumPy mirror (tests/tsdf_ref.py), and the mirror's outputs show that
the cases take every branch."""
import numpy as np
import pytest

import tsdf_cases as C
import tsdf_ref as R
from host_emul import emul

pytestmark = pytest.mark.skipif(not emul.available(), reason="g++ not available")


@pytest.fixture()
def product(monkeypatch):
    emul.patch_lib(emul.build(["tsdf.hip"]), monkeypatch)


@pytest.fixture(scope="module")
def mirror():
    return {name: C.run_mirror(C.make_case(name)) for name in "abcde"}


def test_the_cases_take_every_branch(mirror):
    """Every ray end code, and both outcomes of every requirement of integrate (a voxel that reaches UPDATED passed
    all of them), occur in the mirror's results; so do both sides of the two clamps."""
    codes, outcomes = C.coverage([r for res in mirror.values() for r in res])
    assert codes == {R.HIT, R.LEFT, R.BACKFACE, R.MISS, R.CAP}
    assert outcomes == {-1, R.BEHIND, R.OUTSIDE, R.HOLE, R.OCCLUDED, R.UPDATED}
    first = mirror["a"][0]["volume"]
    touched = first[..., 1] > 0
    assert (first[..., 0][touched] == 1).any() and (first[..., 0][touched] < 1).any()  # f clamped to 1, and not
    assert (first[..., 0][touched] < 0).any() and not touched.all()


def test_a_odd_volume_two_integrates_and_a_raycast(product, mirror):
    C.assert_equal(C.run_product(C.make_case("a"), "cpu"), mirror["a"])
    assert mirror["a"][1]["volume"][..., 1].max() == 2
    assert (mirror["a"][2]["code"] == R.HIT).sum() > 300


def test_b_axis_parallel_rays_inside_and_outside_the_slab(product, mirror):
    case, exp = C.make_case("b"), mirror["b"]
    C.assert_equal(C.run_product(case, "cpu"), exp)
    inside, outside, within = exp[1], exp[2], exp[3]
    assert inside["code"][12, 16] == R.HIT and abs(inside["depth"][12, 16] - 0.81) < 0.02  # the sphere's front
    assert (outside["code"][:, 16] == R.MISS).all()  # d_x = 0 with the camera's x outside the slab
    assert (outside["code"] == R.HIT).any()
    assert (within["code"] == R.HIT).all() and (within["depth"] > 0).all()  # the camera inside the volume


def test_c_the_weight_caps_and_the_third_update_still_moves(product, mirror):
    exp = mirror["c"]
    C.assert_equal(C.run_product(C.make_case("c"), "cpu"), exp)
    assert exp[1]["volume"][..., 1].max() == 2 and exp[2]["volume"][..., 1].max() == 2
    assert (exp[2]["volume"][..., 0] != exp[1]["volume"][..., 0]).sum() > 100


def test_d_holes_voxels_behind_and_the_skip_word(product, mirror):
    exp = mirror["d"]
    C.assert_equal(C.run_product(C.make_case("d"), "cpu"), exp)
    assert exp[1]["volume"].tobytes() == exp[0]["volume"].tobytes() and (exp[1]["outcome"] == -1).all()
    assert exp[2]["volume"].tobytes() != exp[1]["volume"].tobytes()
    assert (exp[0]["outcome"] == R.HOLE).sum() > 50 and (exp[2]["outcome"] == R.BEHIND).sum() > 500


def test_e_back_faces_a_fresh_volume_and_the_step_cap(product, mirror):
    exp = mirror["e"]
    C.assert_equal(C.run_product(C.make_case("e"), "cpu"), exp)
    fresh, behind, capped = exp[0], exp[2], exp[3]
    assert not fresh["depth"].any() and set(np.unique(fresh["code"])) <= {R.LEFT, R.MISS}
    assert (behind["code"] == R.BACKFACE).sum() > 300 and not behind["depth"].any()
    assert (capped["code"] == R.CAP).all() and not capped["depth"].any()
