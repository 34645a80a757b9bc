"""The map server on the MI355X (csrc/occserver.hip through contrib.OctomapServer) against the mirror
(tests/occserver_ref.py) bit for bit: sequences A and B of tests/occserver_cases.py at 121 x 163 (odd in both
directions: the last stride-2 pixel is the last pixel) with 5 objects; one 480 x 640 frame inserted and published twice
from fresh servers, run to run identical; NumPy and device inputs; the online example end to end (its own process and
time limit)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import occserver_cases as C
import occserver_ref as S
from conftest import ROOT

pytestmark = pytest.mark.gpu

H, W, N_OBJECTS, RESOLUTION = 121, 163, 5, 0.01


@pytest.fixture(scope="module")
def frames():
    return C.make_frames(0, H, W, N_OBJECTS)


def test_sequence_a_three_poses_bitwise(frames):
    C.run_sequence(frames, C.make_pitch_of(W), "cuda", RESOLUTION)


def test_sequence_b_clamped_cells_and_published_grids(frames):
    server, ref = C.run_clamped(frames[0], C.make_pitch_of(W), "cuda", RESOLUTION)
    C.check_clean(server)
    for ground in (True, False):
        for free in (True, False):
            C.check_publish(server, ref, frames[1]["T_sensor_to_map"], ground, free)


def _snapshot(server, T):
    out = server.publish_grids(T)
    torch.cuda.synchronize()
    snap = {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in out.items()}
    for i in server.mapping.instance_ids:
        snap[f"lo{i}"], snap[f"logodds{i}"] = server.mapping.dense_logodds(i)
    for i, c in server.centers.items():
        snap[f"center{i}"], snap[f"bbx{i}"] = c, np.stack(server.bbx[i])
    return snap


def _same(a, b):
    assert a.keys() == b.keys()
    for k, v in a.items():
        if isinstance(v, np.ndarray):
            assert v.dtype == b[k].dtype and np.array_equal(v, b[k], equal_nan=v.dtype.kind == "f"), k
        else:
            assert v == b[k], k


def test_full_frame_run_to_run_identity():
    from morefusion_amd import synthetic
    from morefusion_amd.contrib import OctomapServer
    f = C.make_frames(1, 480, 640, 8, n_frames=1)[0]
    pitch_of = lambda c: synthetic.CLASS_PITCH[int(c)]  # noqa: E731
    snaps = []
    for _ in range(2):
        server = OctomapServer()
        C.insert(server, f, pitch_of, to=lambda x: torch.as_tensor(x).cuda())
        snaps.append(_snapshot(server, f["T_sensor_to_map"]))
        C.check_clean(server)
    _same(*snaps)
    assert len(snaps[0]["instance_ids"]) >= 6 and (snaps[0]["grid_target"] > 0).any() and snaps[0]["grid_nontarget_empty"].any()


def test_numpy_and_device_inputs_agree(frames):
    from morefusion_amd.contrib import OctomapServer
    pitch_of = C.make_pitch_of(W)
    snaps = []
    for to in (None, lambda x: torch.as_tensor(x).cuda()):
        server = OctomapServer()
        for f in frames[:2]:
            C.insert(server, f, pitch_of, to=to)
        snaps.append(_snapshot(server, frames[1]["T_sensor_to_map"]))
    _same(*snaps)
    label = torch.as_tensor(frames[0]["label"]).cuda().clone()
    label[5, 7] = 77  # an odd pixel of a device label: found by the kernel
    with pytest.raises(KeyError, match="77"):
        OctomapServer().insert_scan(torch.as_tensor(frames[0]["pts_map"]).cuda(), label, frames[0]["classes"], pitch_of)


def test_online_example_end_to_end():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "online_pose_refinement.py"), "--frames", "2"],
                       cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    assert re.search(r"refined (\d+) objects in (\d+) steps", p.stdout), p.stdout[-2000:]
    poses = re.findall(r"instance (\d+): before t = \[([^\]]*)\] q = \[([^\]]*)\], after t = \[([^\]]*)\] q = \[([^\]]*)\]", p.stdout)
    assert len(poses) == int(re.search(r"refined (\d+) objects", p.stdout).group(1)) >= 1
    for row in poses:
        values = np.array([float(v) for part in row[1:] for v in part.split(",")])
        assert values.shape == (14,) and np.isfinite(values).all()
