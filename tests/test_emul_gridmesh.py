"""csrc/gridmesh.hip (with render.hip, occserver.hip, occmap.hip, occtrack.hip) through the host emulator behind
geometry.voxel_grids_to_meshes, contrib.render_voxel_grids, OctomapServer.grids_in_map_frame and
InstanceTracker(render="mesh") (torch CPU tensors as device memory), bit for bit against the mirror tests/gridmesh_ref.py
on the grids of tests/gridmesh_cases.py."""
import numpy as np
import pytest

import gridmesh_cases as C
import gridmesh_ref as M
import occserver_cases as OC
from host_emul import emul

pytestmark = pytest.mark.skipif(not emul.available(), reason="g++ not available")

H, W, N_OBJECTS, RESOLUTION = 48, 64, 3, 0.02


@pytest.fixture()
def product(monkeypatch):
    emul.patch_lib(emul.build(["occmap.hip", "occserver.hip", "occtrack.hip", "render.hip", "gridmesh.hip"]), monkeypatch)


def test_small_grids_vertices_faces_offsets(product):
    C.check_extraction(C.small_batch(), "cpu")


@pytest.mark.parametrize("iterations", [0, 1, 10])
def test_small_grids_smoothed(product, iterations):
    C.check_smoothing(C.small_batch(), "cpu", iterations)


def test_empty_unit_full_and_checkerboard(product):
    plan = C.check_extraction(C.big_batch(), "cpu")
    assert plan.n_vertices > 160000 and plan.v_off[1] == 0 and plan.v_off[2] == 14
    C.check_smoothing(C.big_batch(), "cpu", 1)


def test_same_dims_batch_as_one_array(product):
    """[B, X, Y, Z] in one array, tensors for pitch and origin."""
    import torch
    from morefusion_amd import geometry
    grids = np.stack([C.blobs(s, 8) for s in (4, 5)])
    pitch, origin = np.array([0.01, 0.02], np.float32), np.array([[0, 0, 0], [1, 1, 1]], np.float64)
    got = geometry.voxel_grids_to_meshes(torch.from_numpy(grids), torch.from_numpy(pitch), torch.from_numpy(origin))
    C.assert_meshes_equal(C.to_numpy(got), M.voxel_grids_to_meshes(grids, pitch, origin))


def test_label_of_three_meshes(product):
    C.check_label("cpu")


def test_grids_in_map_frame_after_sequence_a(product):
    frames = OC.make_frames(0, H, W, N_OBJECTS)
    server, ref = OC.run_sequence(frames, OC.make_pitch_of(W), "cpu", RESOLUTION)
    C.check_map_grids(server, ref)


def test_tracker_mesh_route_matches_the_raycast_route(product):
    C.check_tracker_routes("cpu", 96, 128, N_OBJECTS, RESOLUTION)
