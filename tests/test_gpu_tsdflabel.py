"""TSDF labels on the MI355X (csrc/tsdflabel.hip through contrib.InstanceTsdfVolume / contrib.ModelTracker) against the
NumPy mirror (tests/tsdflabel_ref.py), bit for bit: the cases (a) .. (e) of tests/tsdflabel_cases.py; run-to-run identity
of the atomically summed statistics; ModelTracker.track(depth, label) over the 120 x 160 four-frame sequence -- the poses
of track(depth) on a plain volume; the published grids through the consumer of OctomapServer.publish_grids' output (ICC
refinement); and the online example with its grids from the model (its own process and time limit)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import camtrack_cases as CC
import tsdf_cases as TC
import tsdflabel_cases as C
from conftest import ROOT
from morefusion_amd.contrib import InstanceTsdfVolume, ModelTracker, TsdfVolume

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", C.CASES)
def test_kernel_cases_bitwise_vs_mirror(name):
    case = C.make_case(name)
    C.assert_equal(C.run_product(case, "cuda"), C.run_mirror(case))


def _fused():
    vol = InstanceTsdfVolume(**C.VOLUME)
    for k in range(3):
        depth, label, T = C.frame(k)
        vol.integrate(depth, C.K, T, label=label)
    return vol


def test_volume_bytes_are_the_plain_integrates_and_statistics_repeat():
    vol, plain = _fused(), TsdfVolume(**C.VOLUME)
    for k in range(3):
        depth, _, T = C.frame(k)
        plain.integrate(depth, C.K, T)
    assert vol.volume.cpu().numpy().tobytes() == plain.volume.cpu().numpy().tobytes()
    tables = [vol.instance_table(C.IDS_64).cpu().numpy() for _ in range(3)]
    assert tables[0][:, 0].max() > 1000 and tables[0].tobytes() == tables[1].tobytes() == tables[2].tobytes()


def test_labels_do_not_move_the_camera():
    """Four 120 x 160 frames: track(depth, label) into an InstanceTsdfVolume and track(depth) into a TsdfVolume give the
    same poses, statistics and volume, bit for bit; the labels arrive."""
    frames = TC.model_sequence(CC.ACCURACY_SEEDS[0])
    H, W = CC.ACCURACY_SHAPE
    vol, plain_volume = InstanceTsdfVolume(**TC.MODEL_VOLUME), TsdfVolume(**TC.MODEL_VOLUME)
    trk, plain = ModelTracker(frames[0]["K"], H, W, vol), ModelTracker(frames[0]["K"], H, W, plain_volume)
    with pytest.raises(TypeError, match="InstanceTsdfVolume"):
        plain.track(frames[0]["depth"], frames[0]["label_detected"])
    for k, f in enumerate(frames):
        label = np.where(f["label_detected"] >= 0, f["label_detected"] + 1, -1).astype(np.int32)
        depth = torch.as_tensor(f["depth"]).cuda()
        got = trk.track(depth, torch.as_tensor(label).cuda() if k % 2 else label)
        exp = plain.track(depth)
        assert got.is_cuda and np.array_equal(got.cpu().numpy(), exp.cpu().numpy()), k
        if k:
            assert not trk.lost
    assert np.array_equal(trk.stats, plain.stats)
    assert vol.volume.cpu().numpy().tobytes() == plain_volume.volume.cpu().numpy().tobytes()
    labels = vol.labels.cpu().numpy()
    assert labels[..., 1].max() == 4 and (labels[..., 0] == -1).sum() > 10000 and (labels[..., 0] >= 1).sum() > 1000


def test_published_grids_feed_the_collision_refinement():
    """The dict has OctomapServer.publish_grids' keys, dtypes and shapes, and IterativeCollisionCheckLink takes it the
    way examples/online_pose_refinement.py hands the server's over."""
    import morefusion_amd as mf
    vol = _fused()
    T = C.frame_pose(1)
    grids = vol.publish_grids(T, [1, 3, 9], pitch={1: 0.0075, 3: 0.007, 9: 0.01}, class_ids={1: 4, 3: 11, 9: 2},
                              ground_z=0.0)
    assert grids["instance_ids"] == [1, 3] and grids["class_ids"] == [4, 11]
    expected = dict(pitch=(torch.float32, (2,)), origin=(torch.float64, (2, 3)),
                    grid_target=(torch.float32, (2, 32, 32, 32)), grid_noentry=(torch.float32, (2, 32, 32, 32)),
                    grid_nontarget_empty=(torch.bool, (2, 32, 32, 32)))
    assert set(grids) == set(expected) | {"instance_ids", "class_ids"}
    for key, (dtype, shape) in expected.items():
        assert grids[key].is_cuda and grids[key].dtype == dtype and tuple(grids[key].shape) == shape, key
    assert grids["grid_target"].sum() > 100 and grids["grid_noentry"].sum() > 1000
    assert torch.equal(grids["grid_nontarget_empty"], grids["grid_noentry"] != 0)
    rs = np.random.RandomState(0)
    points = [mf.synthetic.make_primitive("sphere", float(p), rs)[0].astype(np.float32) for p in grids["pitch"].cpu()]
    sdf = [torch.as_tensor(mf.synthetic.synthetic_sdf(p).astype(np.float32)).cuda() for p in points]
    T_init = np.stack([np.eye(4)] * 2)
    centre = grids["origin"].cpu().numpy() + 15.5 * grids["pitch"].cpu().numpy().astype(np.float64)[:, None]
    T_init[:, :3, 3] = centre + 0.01
    link = mf.contrib.IterativeCollisionCheckLink(T_init, sdf_offset=0.01).to_gpu()
    n_steps = link.refine_until_converged([torch.as_tensor(p).cuda() for p in points], sdf, grids["pitch"],
                                          grids["origin"].float(), grids["grid_target"], grids["grid_noentry"], sync=True)
    assert 1 <= int(n_steps[0]) <= 30
    assert torch.isfinite(link.translation).all() and torch.isfinite(link.quaternion).all()


def test_online_example_with_the_grids_from_the_model():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "online_pose_refinement.py"), "--frames", "2",
                        "--track-model", "--grids-from-model"], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    assert "(model)" in p.stdout and re.search(r"refined (\d+) objects in (\d+) steps", p.stdout), p.stdout[-2000:]
