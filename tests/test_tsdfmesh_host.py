"""The TSDF mesh without a device: what the NumPy mirror (tests/tsdfmesh_ref.py, written from include/mfhip.h "TSDF
mesh") gives for the cases of tests/tsdfmesh_cases.py has the properties the contract promises -- the product is pinned
to the mirror bit for bit elsewhere (tests/test_emul_tsdfmesh.py, tests/test_gpu_tsdfmesh.py) -- and geometry.save_obj
writes what geometry.load_obj reads."""
import math

import numpy as np
import pytest

import tsdfmesh_cases as C
import tsdfmesh_ref as R
from morefusion_amd import geometry


@pytest.fixture(scope="module")
def mirror():
    return {name: C.run_mirror(C.make_case(name)) for name in C.NAMES}


def test_a_fused_volume_gives_an_open_mesh_and_a_higher_min_weight_fewer_faces(mirror):
    one, two = mirror["a"], C.run_mirror(C.make_case("a"), min_weight=2.0)
    assert len(one["faces"]) > 500 and 0 < len(two["faces"]) < len(one["faces"])
    assert not R.edge_pairing(one["faces"])[0]  # unobserved regions: the surface has a boundary
    weight = C.make_case("a")["volume"][..., 1]
    assert (weight == 0).any() and (weight == 1).any() and (weight == 2).any()


def test_b_sphere_is_closed_oriented_and_as_accurate_as_linear_interpolation_allows(mirror):
    """The four checks.  (1) every undirected edge lies in exactly two faces, with opposite directions; (2) V - E + F
    = 2; (3) the signed volume is positive and within the shell of check (4) of 4/3 pi R^3; (4) | |v - c| - R | <=
    L^2 / (8 (R - L)) with L = sqrt(3) pitch: along an edge (at most L long) the distance to the centre has a second
    derivative of at most 1 / (distance to the centre) <= 1 / (R - L), so its linear interpolant is off by at most
    L^2 / 8 times that; the stored float32 values add 2^-24 truncations each, and the crossing moves by at most the
    value error over the slope (>= 1 / L per L of edge, so a factor L / pitch <= 2), both ends: 4 * 2^-24 truncation.
    And every normal points away from the centre."""
    m, h = mirror["b"], C.SPHERE["pitch"]
    v, f, c = m["vertices"], m["faces"], C.sphere_centre()
    closed, n_edges = R.edge_pairing(f)
    assert closed
    assert len(v) - n_edges + len(f) == 2
    Rad, L = C.SPHERE["radius"] * h, math.sqrt(3.0) * h
    bound = L * L / (8.0 * (Rad - L)) + 4.0 * 2.0 ** -24 * C.SPHERE["truncation"] * h
    radial = np.abs(np.linalg.norm(v - c, axis=1) - Rad)
    assert radial.max() <= bound, (radial.max(), bound)
    volume = R.signed_volume(v - c, f)
    assert volume > 0
    assert 4.0 / 3.0 * math.pi * (Rad - bound) ** 3 <= volume <= 4.0 / 3.0 * math.pi * (Rad + bound) ** 3
    assert (np.einsum("ij,ij->i", m["normals"], v - c) > 0).all()
    assert np.allclose(np.linalg.norm(m["normals"], axis=1), 1.0, rtol=0, atol=1e-15)
    assert 100 < len(v) < 400 and not ((m["r"] == 0) | (m["r"] == 1)).any()


def test_c_every_corner_pattern_has_the_faces_of_the_tetrahedron_rules_and_only_observed_cells_have_any(mirror):
    m = mirror["c"]
    per_cell = m["faces_per_cell"]
    for pattern in range(256):
        assert per_cell.get((0, 0, 3 * pattern), 0) == R.expected_cell_faces(pattern), pattern
    assert set(per_cell) <= {(0, 0, 3 * p) for p in range(256)}
    # corner 0 lies in all six tetrahedra, corner code 1 = (0, 0, 1) in the two that walk z first
    assert R.expected_cell_faces(0) == R.expected_cell_faces(255) == 0
    assert R.expected_cell_faces(1) == 6 and R.expected_cell_faces(2) == 2
    assert max(per_cell.values()) == 12 and sum(per_cell.values()) == len(m["faces"])
    # no vertex on an edge that only unobserved cells contain: both ends of every vertex's edge lie in the layers
    # 3 p and 3 p + 1 of one pattern
    k, dz = m["owner"][:, 2], np.asarray(R.DIRS)[m["owner"][:, 3]][:, 2]
    assert ((k % 3) + dz <= 1).all()
    assert ((m["r"] > 0) & (m["r"] < 1)).all() and len(np.unique(m["r"])) > 8  # interpolated, not midpoints


def test_d_long_rows_carry_vertices_past_a_workgroup(mirror):
    m = mirror["d"]
    i = m["owner"][:, 0]
    assert (i < 64).any() and ((i >= 64) & (i < 256)).any() and (i >= 256).any()
    assert (m["cell"][:, 0] >= 256).any() and (m["cell"][:, 0] == 255).any()  # a cell across the chunk border


def test_e_zeros_are_inside_degenerate_faces_stay_and_the_gradient_takes_its_branches(mirror):
    """An exact 0.0 and a -0.0 are inside: their edges have r = 0 (owner) or r = 1 (other end), several vertices
    coincide and the triangles between them are kept.  The gradient's central and both one-sided branches occur; the
    fourth ("neither neighbour usable") cannot occur at an end of a vertex's edge: the observed cell that contains
    the edge contains, for each axis, a neighbour of each of its corners along that axis.  Zero normals occur (the
    alternating tsdf makes every central difference along x zero)."""
    case, m = C.make_case("e"), mirror["e"]
    F = case["volume"][..., 0]
    assert F[1, 1, 2] == 0 and not np.signbit(F[1, 1, 2]) and F[2, 2, 4] == 0 and np.signbit(F[2, 2, 4])
    assert (m["r"] == 0).any() and (m["r"] == 1).any()
    p = m["vertices"][m["faces"]]
    area2 = np.linalg.norm(np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]), axis=1)
    assert (area2 == 0).any() and (area2 > 0).any()
    assert sum(m["faces_per_cell"].values()) == len(m["faces"])
    assert m["branches"] == {R.CENTRAL, R.FORWARD, R.BACKWARD}
    zero = ~m["normals"].any(axis=1)
    assert zero.any() and not zero.all()
    # the unobserved point takes its cells out: no face in a cell that has it as a corner
    assert not any(i in (3, 4) and j == 0 and k == 0 for i, j, k in m["faces_per_cell"])


def test_f_no_surface_no_mesh(mirror):
    for name in ("f_fresh", "f_positive"):
        m = mirror[name]
        assert m["vertices"].shape == (0, 3) and m["faces"].shape == (0, 3) and m["normals"].shape == (0, 3)


def test_g_save_obj_round_trips_through_load_obj(mirror, tmp_path):
    m = mirror["b"]
    path = str(tmp_path / "sphere.obj")
    geometry.save_obj(path, m["vertices"], m["faces"])
    v, f = geometry.load_obj(path)
    assert f.dtype == np.int32 and np.array_equal(f, m["faces"])
    assert np.array_equal(v, m["vertices"])  # 17 significant digits: every float64 survives the text
    import torch
    geometry.save_obj(path, torch.from_numpy(m["vertices"]), torch.from_numpy(m["faces"]))
    v2, f2 = geometry.load_obj(path)
    assert np.array_equal(v2, v) and np.array_equal(f2, f)
    with pytest.raises(ValueError):
        geometry.save_obj(path, m["vertices"][:5], m["faces"])
    geometry.save_obj(path, np.zeros((0, 3)), np.zeros((0, 3), np.int32))
    v0, f0 = geometry.load_obj(path)
    assert v0.shape == (0, 3) and f0.shape == (0, 3)
