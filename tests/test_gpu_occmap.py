"""Occupancy mapping on the MI355X (csrc/occmap.hip through contrib.MultiInstanceOctreeMapping): a full
480 x 640 frame with real geometry (8 objects on a table, wall + table as background labels) against the
restatement (tests/occmap_ref.py) bit for bit, run-to-run identity, the network booleans, update(), NumPy vs
device inputs, and the ``--occupancy`` frame example end to end (its own process and time limit)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import occmap_ref as R
from conftest import ROOT

pytestmark = pytest.mark.gpu

from morefusion_amd import geometry, synthetic  # noqa: E402
from morefusion_amd.contrib import MultiInstanceOctreeMapping  # noqa: E402
from morefusion_amd.data_formats import grids_for_network  # noqa: E402


def pitch_of(c):
    return synthetic.CLASS_PITCH[int(c)]


@pytest.fixture(scope="module")
def frame():
    f = synthetic.make_occupancy_frame(0)
    K = f["K"]
    f["pcd"] = geometry.pointcloud_from_depth(f["depth"], K[0, 0], K[1, 1], K[0, 2], K[1, 2])
    f["pitch"] = np.array([pitch_of(c) for c in f["class_ids"]])
    f["origin"] = np.stack([np.nanmedian(f["pcd"][f["label"] == i], axis=0) for i in f["instance_ids"]]) \
        - 15.5 * f["pitch"][:, None]
    return f


@pytest.fixture(scope="module")
def ref(frame):
    return R.build_octomap(frame["pcd"], frame["label"], frame["instance_ids"], frame["class_ids"], pitch_of)


def _map(frame, on_device=True):
    m = MultiInstanceOctreeMapping()
    pcd = torch.as_tensor(frame["pcd"]).cuda() if on_device else frame["pcd"]
    label = torch.as_tensor(frame["label"]).cuda() if on_device else frame["label"]
    m.integrate_frame(pcd, label, frame["instance_ids"], frame["class_ids"], pitch_of)
    return m


def _grids(m, frame, **kw):
    return m.get_target_grids_batch(frame["instance_ids"], torch.as_tensor(frame["pitch"]).cuda(),
                                    torch.as_tensor(frame["origin"]).cuda(), **kw)


def test_full_frame_grids_bitwise_vs_restatement_and_run_to_run(frame, ref):
    m1, m2 = _map(frame), _map(frame)
    g1, g2 = _grids(m1, frame), _grids(m2, frame)
    torch.cuda.synchronize()
    assert int(m1._overflow[0]) == 0
    for a, b in zip(g1, g2):
        assert torch.equal(a, b)
    for iid in m1.instance_ids:
        assert np.array_equal(m1.dense_logodds(iid)[1], m2.dense_logodds(iid)[1], equal_nan=True)
    seen = np.zeros(3, bool)
    for b, (tid, p, o) in enumerate(zip(frame["instance_ids"], frame["pitch"], frame["origin"])):
        exp = ref.get_target_grids(tid, dimensions=(32, 32, 32), pitch=p, origin=o)
        for got, e in zip(g1, exp):
            assert np.array_equal(got[b].cpu().numpy(), e), tid
        assert (exp[0] > 0).any() and (exp[2] > 0).any(), tid
        seen |= [(e > 0).any() for e in exp]
    assert seen.all()  # target, non-target and empty space all occur


def test_network_inputs_match_grids_for_network(frame):
    gt, gn, ge, nt, nte = _grids(_map(frame), frame, network_inputs=True)
    assert nt.dtype == torch.bool and nte.dtype == torch.bool
    for b in range(len(frame["instance_ids"])):
        t_ref, nte_ref = grids_for_network(gt[b].cpu().numpy(), gn[b].cpu().numpy(), ge[b].cpu().numpy(), train=False)
        assert np.array_equal(nt[b].cpu().numpy(), t_ref) and np.array_equal(nte[b].cpu().numpy(), nte_ref)
    assert nte.any()


def test_update_matches_restatement(frame):
    ids, label, pcd = frame["instance_ids"], frame["label"], frame["pcd"]
    m = _map(frame)
    r = R.build_octomap(pcd, label, ids, frame["class_ids"], pitch_of)
    rs = np.random.RandomState(0)
    for iid in (ids[2], 0):
        pts = pcd[(label == (iid if iid else 1))]
        pts = pts[~np.isnan(pts).any(axis=1)]
        occ = pts[rs.choice(len(pts), 300)] + rs.uniform(-0.03, 0.03, (300, 3))  # duplicates, some out of the box
        m.update(iid, torch.as_tensor(occ).cuda())
        r.update(iid, occ)
        lo, lg = m.dense_logodds(iid)
        known = ~np.isnan(lg)
        got = dict(zip(R.pack(np.argwhere(known) + lo).tolist(), lg[known].tolist()))
        exp = r.octrees[iid].values
        assert set(got) == set(exp) and all(np.float32(got[k]) == exp[k] for k in exp)
    assert int(m._overflow[0]) == 0


def test_numpy_and_device_inputs_agree(frame):
    md, mh = _map(frame, on_device=True), _map(frame, on_device=False)
    gd = _grids(md, frame)
    gh = mh.get_target_grids_batch(frame["instance_ids"], frame["pitch"], frame["origin"])
    assert all(isinstance(g, np.ndarray) for g in gh)
    for a, b in zip(gd, gh):
        assert np.array_equal(a.cpu().numpy(), b)
    one = mh.get_target_grids(frame["instance_ids"][0], dimensions=(32, 32, 32), pitch=frame["pitch"][0],
                              origin=frame["origin"][0])
    for a, b in zip(one, gh):
        assert np.array_equal(a, b[0])


def test_occupancy_frame_example_end_to_end():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "singleview_3d_from_frame.py"), "--occupancy"],
                       cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    n = int(re.search(r"grid_nontarget_empty (\d+) voxels", p.stdout).group(1))
    assert n > 0
    l0, l1 = map(float, re.search(r"ICC loss (\S+) -> (\S+) in", p.stdout).groups())
    assert np.isfinite(l0) and np.isfinite(l1)
    trans = re.findall(r"translation \[([^\]]*)\]", p.stdout)
    assert len(trans) == 8 and all(np.isfinite(np.array(t.split(), float)).all() for t in trans)
