"""The ICP registration restatements (tests/icpreg_ref.py) on the CPU: open3d's voxel_down_sample rules,
Eigen's umeyama (exact recovery, the reflection case), the empty-correspondence result, the convergence
stop, register vs register_iterative, and the mirror against the independent restatement on the three
real fixtures (the reference's ICP driver input)."""
import os

import numpy as np
import pytest

import icpreg_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURES = [os.path.join(GOLDEN, f"fixture_pose_refinement_0000000{i}.npz") for i in range(3)]


def _rot(ax, ang):
    c, s = np.cos(ang), np.sin(ang)
    i, j = [(1, 2), (2, 0), (0, 1)][ax]
    m = np.eye(3)
    m[i, i], m[i, j], m[j, i], m[j, j] = c, -s, s, c
    return m


def test_voxel_down_sample_rules():
    v = 0.5
    # min = 0 -> vmin = -0.25: voxel boundaries at 0.25 + k * 0.5 (exact in binary)
    pts = np.array([
        [0.0, 0.0, 0.0],
        [0.25, 0.0, 0.0],     # exactly on a boundary: the upper voxel (floor)
        [0.2, 0.0, 0.0],      # same voxel as the first
        [np.nan, 1.0, 1.0],   # dropped
        [1.0, 1.0, np.nan],   # dropped
        [0.1, 0.0, 0.0],      # same voxel as the first (third member)
        [0.0, 0.75, 0.0],     # voxel (0, 2, 0)
        [0.0, 0.0, 0.3],      # voxel (0, 0, 1)
    ])
    got = R.voxel_down_sample(pts, v)
    exp = np.array([
        [(0.0 + 0.2) + 0.1, 0.0, 0.0],
        [0.0, 0.0, 0.3],
        [0.0, 0.75, 0.0],
        [0.25, 0.0, 0.0],
    ])
    exp[0] /= 3.0
    assert np.array_equal(got, exp)  # (i, j, k) order: (0,0,0), (0,0,1), (0,2,0), (1,0,0)
    assert np.array_equal(R.voxel_down_sample_independent(pts, v), got)
    assert R.voxel_down_sample(np.full((3, 3), np.nan), v).shape == (0, 3)


def test_voxel_down_sample_input_order_sum():
    rs = np.random.RandomState(0)
    p = rs.uniform(0, 0.05, (500, 3))
    got = R.voxel_down_sample(p, 0.01)
    assert np.array_equal(got, R.voxel_down_sample_independent(p, 0.01))


def test_umeyama_exact_recovery_and_reflection():
    rs = np.random.RandomState(1)
    s = rs.uniform(-0.1, 0.1, (50, 3))
    Rm = _rot(0, 0.3) @ _rot(1, -0.7) @ _rot(2, 1.1)
    t = s @ Rm.T + [0.05, -0.02, 0.4]
    ms, mt = s.mean(0), t.mean(0)
    sig = ((t - mt).T @ (s - ms) / len(s)).reshape(9)
    upd = R.umeyama(sig, ms, mt)
    assert np.abs(upd[:3, :3] - Rm).max() <= 1e-12
    assert np.abs(upd[:3, 3] - [0.05, -0.02, 0.4]).max() <= 1e-12
    # a mirrored target: the best rotation, never a reflection
    tm = s * [1, 1, -1]
    ms, mt = s.mean(0), tm.mean(0)
    sig = ((tm - mt).T @ (s - ms) / len(s)).reshape(9)
    upd = R.umeyama(sig, ms, mt)
    assert abs(np.linalg.det(upd[:3, :3]) - 1) < 1e-12
    assert np.abs(upd - R.umeyama_independent(s, tm)).max() < 1e-9
    # planar correspondences (rank 2) still give the exact rotation
    sp = s * [1, 1, 0]
    tp = sp @ Rm.T
    ms, mt = sp.mean(0), tp.mean(0)
    upd = R.umeyama(((tp - mt).T @ (sp - ms) / len(sp)).reshape(9), ms, mt)
    assert np.abs(upd[:3, :3] - Rm).max() <= 1e-12


def test_inverse_and_product():
    T = np.eye(4)
    T[:3, :3] = _rot(1, 0.4) @ _rot(2, -1.3)
    T[:3, 3] = [0.1, 0.2, 0.5]
    assert np.abs(R.inv4(T) - np.linalg.inv(T)).max() < 1e-15
    assert np.abs(R.mul4(T, R.inv4(T)) - np.eye(4)).max() < 1e-15


def test_no_correspondences_identity_zero_zero():
    src = np.random.RandomState(2).uniform(0, 0.05, (40, 3))
    cad = src + 1.0  # far beyond 2 * voxel_size
    out = R.register(src, cad, np.eye(4), iteration=10, voxel_size=0.01)
    assert out["fitness"] == 0.0 and out["inlier_rmse"] == 0.0
    assert out["n_iter"] == 1  # identity update, unchanged result: converged
    assert np.array_equal(out["transform"], np.eye(4))


def test_convergence_stop_and_modes():
    depth, cad, init = R.fixture_inputs(FIXTURES[2])
    full = R.register(depth, cad, init, iteration=100, voxel_size=0.01)
    n = full["n_iter"]
    assert 1 < n < 100
    _, f, r = full["history"]
    assert abs(f[n] - f[n - 1]) < 1e-6 and abs(r[n] - r[n - 1]) < 1e-6
    assert not (abs(f[n - 1] - f[n - 2]) < 1e-6 and abs(r[n - 1] - r[n - 2]) < 1e-6)
    assert np.array_equal(full["history"][0][0], init) and np.array_equal(full["history"][0][-1], full["transform"])
    short = R.register(depth, cad, init, iteration=3, voxel_size=0.01)
    assert short["n_iter"] == 3 and np.array_equal(short["transform"], full["history"][0][3])
    # register_iterative: no convergence test, re-transforms the source at every step
    it = R.register_iterative(depth, cad, init, iteration=n + 3, voxel_size=0.01)
    assert it["n_iter"] == n + 3
    assert np.array_equal(it["history"][0][0], init)
    one = R.register(depth, cad, init, iteration=1, voxel_size=0.01)
    assert np.array_equal(it["history"][0][1], one["transform"])  # step 1 = one update from init
    assert np.abs(it["transform"] - full["transform"]).max() < 1e-4


@pytest.mark.parametrize("path", FIXTURES)
def test_mirror_vs_independent_on_fixtures(path):
    depth, cad, init = R.fixture_inputs(path)
    m = R.register(depth, cad, init)
    ind = R.register_independent(depth, cad, init)
    assert np.abs(m["transform"] - ind["transform"]).max() <= 1e-9
    assert m["n_iter"] == ind["n_iter"]
    assert abs(m["fitness"] - ind["fitness"]) < 1e-12 and abs(m["inlier_rmse"] - ind["inlier_rmse"]) < 1e-12
