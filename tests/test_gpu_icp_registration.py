"""ICP registration on the MI355X (csrc/icpreg.hip through contrib.ICPRegistration / icp_registration_batch):
the three real fixtures and a 16-object batch bit for bit against the mirror restatement (tests/icpreg_ref.py),
run-to-run identity, NumPy vs device inputs, the active mask, register_iterative's history,
extra.open3d.voxel_down_sample, pose recovery on synthetic observations, and the predict -> refine seam of the
frame example (in process, and ``--icp`` end to end in its own process and time limit)."""
import importlib.util
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import icpreg_ref as R
from conftest import ROOT

pytestmark = pytest.mark.gpu

import morefusion_amd as morefusion  # noqa: E402
from morefusion_amd import synthetic  # noqa: E402
from morefusion_amd.contrib import ICPRegistration, icp_registration_batch  # noqa: E402

FIXTURES = [os.path.join(ROOT, "tests", "golden", f"fixture_pose_refinement_0000000{i}.npz") for i in range(3)]


def _np(x):
    return x.cpu().numpy()


def _equal(out, b, ref, hist=True):
    assert np.array_equal(_np(out[0][b]), ref["transform"])
    assert float(out[1][b]) == ref["fitness"] and float(out[2][b]) == ref["inlier_rmse"]
    assert int(out[3][b]) == ref["n_iter"]
    if hist:
        for g, e in zip(out[4], ref["history"]):
            assert np.array_equal(_np(g[b]), e)


@pytest.mark.parametrize("path", FIXTURES)
def test_fixture_bitwise_vs_mirror(path):
    depth, cad, init = R.fixture_inputs(path)
    ref = R.register(depth, cad, init)
    out = icp_registration_batch([torch.as_tensor(depth).cuda()], [torch.as_tensor(cad).cuda()],
                                 torch.as_tensor(init)[None].cuda(), return_history=True)
    _equal(out, 0, ref)
    got = ICPRegistration(depth, cad, init).register()  # NumPy in, NumPy out
    assert isinstance(got, np.ndarray) and got.dtype == np.float64 and np.array_equal(got, ref["transform"])


def test_batch16_bitwise_run_to_run_numpy_vs_device():
    depth, cad, init, _ = synthetic.make_icp_batch(16, seed=5, n_cad=1500)
    kw = dict(iteration=40, voxel_size=0.008, return_history=True)
    a = icp_registration_batch([torch.as_tensor(d).cuda() for d in depth], [torch.as_tensor(c).cuda() for c in cad],
                               torch.as_tensor(init).cuda(), **kw)
    b = icp_registration_batch(depth, cad, init, **kw)
    c = icp_registration_batch(depth, cad, init, **kw)
    torch.cuda.synchronize()
    for x, y, z in zip(a[:4] + tuple(a[4]), b[:4] + tuple(b[4]), c[:4] + tuple(c[4])):
        assert torch.equal(x, y) and torch.equal(y, z)
    for k in range(16):
        _equal(a, k, R.register(depth[k], cad[k], init[k], iteration=40, voxel_size=0.008))


def test_active_mask_and_shared_cached_target():
    depth, cad, init, _ = synthetic.make_icp_batch(4, seed=6, n_cad=1500)
    active = torch.tensor([True, False, True, False], device="cuda")
    out = icp_registration_batch(depth, [cad[0]] * 4, init, iteration=20, active=active, cad_keys=["c"] * 4)
    again = icp_registration_batch(depth, [cad[0]] * 4, init, iteration=20, active=active, cad_keys=["c"] * 4)
    for k in (0, 2):
        ref = R.register(depth[k], cad[0], init[k], iteration=20)
        _equal(out, k, ref, hist=False)
        _equal(again, k, ref, hist=False)
    for k in (1, 3):
        assert np.array_equal(_np(out[0][k]), init[k]) and int(out[3][k]) == 0


def test_register_iterative_history_bitwise(capsys):
    depth, cad, init = R.fixture_inputs(FIXTURES[1])
    ref = R.register_iterative(depth, cad, init, iteration=6)
    steps = list(ICPRegistration(depth, cad, init).register_iterative(iteration=6))
    assert len(steps) == 7 and steps[0] is init
    for k in range(1, 7):
        assert np.array_equal(steps[k], ref["history"][0][k])
    lines = capsys.readouterr().out.strip().splitlines()
    assert lines[0] == f"[00000000] fitness={ref['history'][1][1]:.2g} inlier_rmse={ref['history'][2][1]:.2g}"
    assert len(lines) == 6


def test_voxel_down_sample_matches_restatement():
    depth, cad, _ = R.fixture_inputs(FIXTURES[2])
    pts = np.concatenate([cad, np.full((3, 3), np.nan)])
    got = morefusion.extra.open3d.voxel_down_sample(pts, 0.004)
    assert isinstance(got, np.ndarray) and got.dtype == np.float64
    assert np.array_equal(got, R.voxel_down_sample(pts, 0.004))
    got_t = morefusion.extra.open3d.voxel_down_sample(torch.as_tensor(pts).cuda(), 0.004)
    assert got_t.is_cuda and np.array_equal(_np(got_t), got)


def _err(A, B):
    Rr = A[:3, :3].T @ B[:3, :3]
    return np.degrees(np.arccos(np.clip((np.trace(Rr) - 1) / 2, -1, 1))), np.linalg.norm(A[:3, 3] - B[:3, 3])


def test_pose_recovery():
    # seed 0: the restatement brings every object from <= 3.7 deg / 7.6 mm to <= 2.3 deg / 1.3 mm
    depth, cad, init, gt = synthetic.make_icp_batch(8, seed=0, n_cad=3000)
    T, fit, rmse, n_iter = icp_registration_batch(depth, cad, init, voxel_size=0.01)
    for k in range(8):
        ang0, tr0 = _err(init[k], gt[k])
        ang, tr = _err(_np(T[k]), gt[k])
        assert ang <= 2.5 and tr <= 0.0015, (k, ang, tr)
        assert tr < tr0
        assert float(fit[k]) > 0.95 and 0 < int(n_iter[k]) < 100


def _example():
    spec = importlib.util.spec_from_file_location("frame_example", os.path.join(ROOT, "examples",
                                                                                "singleview_3d_from_frame.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_seam_history_starts_at_argmax_transformation_matrix():
    ex = _example()
    torch.manual_seed(0)
    n, P, S = 3, 5, 32
    q = torch.nn.functional.normalize(torch.randn(n, P, 4, device="cuda"), dim=-1)
    t = torch.randn(n, P, 3, device="cuda") * 0.05 + torch.tensor([0, 0, 0.5], device="cuda")
    conf = torch.rand(n, P, device="cuda")
    pcd = torch.randn(n, S, S, 3, device="cuda") * 0.03 + torch.tensor([0, 0, 0.5], device="cuda")
    pcd[:, :8] = float("nan")
    class_id = torch.tensor([2, 5, 2], dtype=torch.int32, device="cuda")
    out = ex.refine_icp(pcd, q, t, conf, class_id, np.arange(n), threshold=0.0, iteration=5)
    best = conf.argmax(dim=1)
    T = morefusion.functions.transformation_matrix(q[torch.arange(n), best], t[torch.arange(n), best]).double()
    assert torch.equal(out["history"][0][:, 0], T)
    assert torch.equal(out["init"].double(), T)


def test_frame_example_icp_end_to_end():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "singleview_3d_from_frame.py"), "--icp"],
                       cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    rows = re.findall(r"icp instance \d+ \(confidence [\d.]+\): fitness ([\d.]+) inlier_rmse ([\d.]+) iterations (\d+)",
                      p.stdout)
    assert len(rows) > 0, p.stdout[-2000:]
