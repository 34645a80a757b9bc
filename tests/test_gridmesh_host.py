"""Grid meshes without a GPU and without the kernels: the reference's two morphology calls are identities (scipy), the
properties of the mirror tests/gridmesh_ref.py that make its meshes closed oriented 2-manifolds (none depends on a case
table being right), the mirror's label branches, the C ABI's host-side refusals and the Python interface's argument
checks."""
import numpy as np
import pytest

import gridmesh_cases as C
import gridmesh_ref as M


def test_grey_opening_and_dilation_of_size_one_are_identities():
    """voxel_grids_to_mesh_markers.py:92-93: size=(1,1,1) leaves the matrix as it is, so the product skips both."""
    import scipy.ndimage
    g = np.random.RandomState(3).uniform(0, 1, (9, 8, 7)).astype(np.float32)
    g[g < 0.5] = 0
    opened = scipy.ndimage.grey_opening(g, size=(1, 1, 1))
    assert opened.dtype == g.dtype and np.array_equal(opened, g)
    assert np.array_equal(scipy.ndimage.grey_dilation(opened, size=(1, 1, 1)), g)


def _properties(grid, pitch=0.5):
    v, f, cases = M.mesh(grid, pitch, (0.1, -0.2, 0.3), return_cases=True)
    assert M.half_edges_closed(f)  # closed, manifold, consistently oriented
    n_comp = M.components(f, len(v))
    chi = M.euler(f, len(v))
    vol = M.volume(v, f)
    n_occ, n_surf = int((np.nan_to_num(grid) > 0).sum()), M.surface_cells(grid)
    assert vol > 0
    assert (n_occ - n_surf) * pitch ** 3 <= vol <= (n_occ + n_surf) * pitch ** 3
    assert M.volume(M.humphrey(v, f), f) > 0
    return len(v), len(f), n_comp, chi, vol, cases


def test_single_voxel_is_the_half_scale_star():
    """A lattice point of the Kuhn subdivision has 14 edges and its star is 24 tetrahedra of volume 1/6, each cut at half
    scale (1/8 of its volume): 14 vertices, 24 faces, volume 24 / 6 / 8 = 1/2 cell -- the mirror confirms the issue's
    derivation."""
    nv, nf, n_comp, chi, vol, _ = _properties(C.one_voxel(), 0.5)
    assert (nv, nf, n_comp, chi) == (14, 24, 1, 2)
    assert abs(vol - 0.5 ** 3 / 2) < 1e-13  # 24 float64 triple products of coordinates below 1: a few 1e-16 each


def test_diagonal_pairs_the_subdivision_is_anisotropic():
    """(1,1,1) is an edge of the subdivision: the two voxels join into one surface.  (1,-1,1) is not: two surfaces."""
    assert np.count_nonzero(C.diagonal_pair((1, 1, 1))) == np.count_nonzero(C.diagonal_pair((1, -1, 1))) == 2
    nv, nf, n_comp, chi, _, _ = _properties(C.diagonal_pair((1, 1, 1)))
    assert (n_comp, chi) == (1, 2) and nv < 28
    nv, nf, n_comp, chi, _, _ = _properties(C.diagonal_pair((1, -1, 1)))
    assert (nv, nf, n_comp, chi) == (28, 48, 2, 4)


def test_voxels_in_the_first_and_last_cell_of_every_axis():
    nv, nf, n_comp, chi, vol, _ = _properties(C.corners(), 1.0)
    assert (nv, nf, n_comp, chi) == (8 * 14, 8 * 24, 8, 16) and abs(vol - 4.0) < 1e-11  # 192 terms below 100


def test_random_grid_meets_every_case_of_every_tetrahedron():
    """V - E + F = 2 (components - handles) on a closed orientable surface: it equals 2 x components, as the issue
    states it, only where no component has a handle (the shapes above, the full grid).  A random grid at density 0.5 has
    tunnels, so here the assertion is the general one: even, and at most 2 x components."""
    g = C.random_grid()
    assert g.shape == (5, 7, 6) and 0.4 < np.mean(np.nan_to_num(g) > 0) < 0.6
    nv, nf, n_comp, chi, _, cases = _properties(g)
    assert (cases[:, 1:15] > 0).all(), "change RANDOM_SEED: a case of a tetrahedron does not occur"
    assert chi % 2 == 0 and chi <= 2 * n_comp


def test_full_grid_checkerboard_and_the_degenerate_grids():
    grids, pitch, origin, ref = C.big_batch()
    (v_e, f_e), (v_1, f_1), (v_f, f_f), (v_c, f_c) = ref
    assert len(v_e) == 0 and len(f_e) == 0
    assert (len(v_1), len(f_1)) == (14, 24)
    assert M.half_edges_closed(f_f) and M.components(f_f, len(v_f)) == 1 and M.euler(f_f, len(v_f)) == 2
    assert abs(M.volume(v_f, f_f) / float(pitch[2]) ** 3 - 32 ** 3) < 6 * 32 * 32
    assert M.half_edges_closed(f_c) and M.euler(f_c, len(v_c)) % 2 == 0
    # the vertex maximum: every axis edge that touches an occupied cell is active (31 x 32 x 32 inner ones per axis and
    # one for each of the 2 x 32 x 32 / 2 occupied boundary cells), no face diagonal is, body diagonals come on top
    assert len(v_c) > 3 * 32 ** 3 + 32 ** 3 > len(v_f)
    d = np.abs(v_c[f_c[:, 0]] - v_c[f_c[:, 1]]) / float(pitch[3])
    assert d.max() < 1.0 + 1e-9
    rows, deg = M.neighbours(f_c, len(v_c))
    assert 3 <= deg.min() and deg.max() <= 12  # MF_GRIDMESH_MAX_NEIGHBOURS


def test_label_scene_takes_every_branch():
    _, depth, _, label, counts = C.label_scene()
    assert counts["drawn"] - counts["behind"] >= 20 and counts["behind"] >= 20 and counts["nan_kept"] >= 20
    assert int((label == -2).sum()) - counts["behind"] >= 20  # nothing drawn
    assert set(np.unique(label)) == {-2, 3, 5, 8}
    assert np.isnan(depth).any()


def test_abi_refuses_over_cap_input():
    from morefusion_amd import _lib
    L = _lib.lib()
    assert L.mf_gridmesh_workspace_bytes(4, 1000) > L.mf_gridmesh_workspace_bytes(4, 0) > 0
    assert L.mf_gridmesh_workspace_bytes(4097, 0) < 0 and L.mf_gridmesh_workspace_bytes(-1, 0) < 0
    assert L.mf_gridmesh_workspace_bytes(1, (1 << 30) + 1) < 0
    assert L.mf_gridmesh_count(None, None, None, 4097, None, None, None) < 0
    assert L.mf_gridmesh_emit(None, None, None, None, None, 1, None, None, (1 << 30) + 1, 0, None, None, None) < 0
    assert L.mf_gridmesh_adjacency(None, None, 0, 1, 1, None, None, None) < 0
    assert L.mf_gridmesh_smooth(None, None, None, 1, 0.1, 0.5, -1, None, None) < 0
    assert L.mf_gridmesh_label(None, None, None, 0, 5, None, None) < 0
    assert L.mf_occserver_map_grids(None, 0, None, None, None, 1, 32, None, None, None) < 0


def test_interface_argument_checks():
    import torch
    from morefusion_amd import contrib, geometry
    with pytest.raises(ValueError, match="1..32"):
        geometry.voxel_grids_to_meshes([np.zeros((33, 2, 2), np.float32)], [0.1], [[0, 0, 0]], device="cpu")
    with pytest.raises(ValueError, match="differ in length"):
        geometry.voxel_grids_to_meshes([np.zeros((2, 2, 2), np.float32)], [0.1, 0.2], [[0, 0, 0]], device="cpu")
    assert geometry.voxel_grids_to_meshes(np.zeros((0, 4, 4, 4), np.float32), [], np.zeros((0, 3)), device="cpu") == []
    server = contrib.OctomapServer(device="cpu")
    with pytest.raises(ValueError, match="server"):
        contrib.InstanceTracker(server.mapping, render="mesh")
    with pytest.raises(ValueError, match="server"):
        contrib.InstanceTracker(server.mapping, render="mesh", server=contrib.OctomapServer(device="cpu"))
    with pytest.raises(ValueError, match="raycast"):
        contrib.InstanceTracker(server.mapping, render="opengl")
    assert contrib.InstanceTracker(server.mapping).render == "raycast"
    out = server.grids_in_map_frame()
    assert out["instance_ids"] == [] and tuple(out["grid"].shape) == (0, 32, 32, 32) and out["grid"].dtype == torch.float32


def test_design_names_the_unpinned_parities():
    import os
    from conftest import ROOT
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    section = text[text.index("Grid meshes"):]
    assert "trimesh / scikit-image parity unpinned" in section and "filter_humphrey" in section
