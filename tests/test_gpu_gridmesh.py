"""csrc/gridmesh.hip on the MI355X through geometry.voxel_grids_to_meshes, contrib.render_voxel_grids,
OctomapServer.grids_in_map_frame and InstanceTracker(render="mesh"), bit for bit against the mirror
tests/gridmesh_ref.py on the grids of tests/gridmesh_cases.py; 8 grids of one 480 x 640 frame run to run identical; the
online example with --render-service end to end (its own process and time limit)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import gridmesh_cases as C
import occserver_cases as OC
from conftest import ROOT

pytestmark = pytest.mark.gpu


def test_small_grids_vertices_faces_offsets():
    C.check_extraction(C.small_batch(), "cuda")


@pytest.mark.parametrize("iterations", [0, 1, 10])
def test_small_grids_smoothed(iterations):
    C.check_smoothing(C.small_batch(), "cuda", iterations)


def test_empty_unit_full_and_checkerboard():
    plan = C.check_extraction(C.big_batch(), "cuda")
    assert plan.n_vertices > 160000 and plan.v_off[1] == 0 and plan.v_off[2] == 14


@pytest.mark.parametrize("iterations", [1, 10])
def test_empty_unit_full_and_checkerboard_smoothed(iterations):
    C.check_smoothing(C.big_batch(), "cuda", iterations)


def test_label_of_three_meshes():
    C.check_label("cuda")


def test_grids_in_map_frame_after_sequence_a():
    frames = OC.make_frames(0, 121, 163, 5)
    server, ref = OC.run_sequence(frames, OC.make_pitch_of(163), "cuda", 0.01)
    C.check_map_grids(server, ref)


def test_tracker_mesh_route_matches_the_raycast_route():
    C.check_tracker_routes("cuda", 120, 160, 3, 0.01)


def test_full_frame_run_to_run_identity():
    from morefusion_amd import geometry, synthetic
    from morefusion_amd.contrib import OctomapServer, render_voxel_grids
    seq = synthetic.make_tracking_sequence(1, 1, 480, 640, n_objects=8)[0]
    f = OC.make_frames(1, 480, 640, 8, n_frames=1)[0]
    pitch_of = lambda c: synthetic.CLASS_PITCH[int(c)]  # noqa: E731
    depth = torch.as_tensor(seq["depth"]).cuda()
    snaps = []
    for _ in range(2):
        server = OctomapServer()
        OC.insert(server, f, pitch_of, to=lambda x: torch.as_tensor(x).cuda())
        grids = server.grids_in_map_frame()
        meshes = geometry.voxel_grids_to_meshes(grids["grid"], grids["pitch"], grids["origin"])
        label = render_voxel_grids(grids, depth, seq["K"], f["T_sensor_to_map"], 480, 640)
        torch.cuda.synchronize()
        snap = {k: v.cpu().numpy() for k, v in grids.items() if isinstance(v, torch.Tensor)}
        snap["ids"], snap["label"] = np.asarray(grids["instance_ids"]), label.cpu().numpy()
        for b, (v, fc) in enumerate(meshes):
            snap[f"v{b}"], snap[f"f{b}"] = v.cpu().numpy(), fc.cpu().numpy()
        snaps.append(snap)
    a, b = snaps
    assert a.keys() == b.keys() and len(a["ids"]) == 8
    for k in a:
        assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), k
    assert all(len(a[f"f{i}"]) > 0 for i in range(8)) and len(set(np.unique(a["label"]).tolist()) - {-2}) >= 6


def test_online_example_with_the_render_service():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "online_pose_refinement.py"), "--frames", "2",
                        "--render-service"], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    assert "frame 1 (mesh)" in p.stdout and re.search(r"refined (\d+) objects in (\d+) steps", p.stdout), p.stdout[-2000:]
