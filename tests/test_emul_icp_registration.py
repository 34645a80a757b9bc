"""csrc/icpreg.hip through the host emulator (tests/host_emul) behind the product's Python layer
(contrib/icp_registration.py, torch CPU tensors as device memory): fixture 0 and a 3-object synthetic
batch, bitwise equal to the mirror restatement (tests/icpreg_ref.py) -- down-sampled points, transforms,
fitness, inlier_rmse, iteration counts and the per-iteration history, in both register modes."""
import os

import numpy as np
import pytest
import torch

import icpreg_ref as R
from host_emul import emul

pytestmark = pytest.mark.skipif(not emul.available(), reason="g++ not available")

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture()
def M(monkeypatch):
    from morefusion_amd.contrib import icp_registration as mod
    L = emul.build(["icpreg.hip"])
    emul.patch_lib(L, monkeypatch)
    mod.clear_cache()
    yield mod
    mod.clear_cache()


def synthetic_batch(n, seed=0):
    from morefusion_amd import synthetic
    return synthetic.make_icp_batch(n, seed)[:3]


def _check(got, ref, hist=True):
    T, fit, rmse, n_iter = got[:4]
    assert np.array_equal(T.numpy(), ref["transform"])
    assert float(fit) == ref["fitness"] and float(rmse) == ref["inlier_rmse"] and int(n_iter) == ref["n_iter"]
    if hist:
        for g, e in zip(got[4], ref["history"]):
            assert np.array_equal(g.numpy(), e)


def test_fixture0_bitwise_vs_mirror(M):
    depth, cad, init = R.fixture_inputs(os.path.join(GOLDEN, "fixture_pose_refinement_00000000.npz"))
    ref = R.register(depth, cad, init, iteration=30, voxel_size=0.01)
    out = M.icp_registration_batch([depth], [cad], init[None], iteration=30, voxel_size=0.01, return_history=True,
                                   device="cpu")
    _check([o[0] for o in out[:4]] + [[h[0] for h in out[4]]], ref)
    ds, off, cnt = M.voxel_down_sample_batch([depth, cad], 0.01, device="cpu")
    assert np.array_equal(ds[off[0]:off[0] + int(cnt[0])].numpy(), ref["source"])
    assert np.array_equal(ds[off[1]:off[1] + int(cnt[1])].numpy(), ref["target"])
    assert ref["n_iter"] > 1 and ref["fitness"] > 0.5
    got = M.ICPRegistration(depth, cad, init, device="cpu").register(iteration=30)
    assert isinstance(got, np.ndarray) and np.array_equal(got, ref["transform"])
    ref_it = R.register_iterative(depth, cad, init, iteration=3)
    steps = list(M.ICPRegistration(depth, cad, init, device="cpu").register_iterative(iteration=3))
    assert steps[0] is init and all(np.array_equal(a, b) for a, b in zip(steps[1:], ref_it["history"][0][1:]))


def test_synthetic_batch_both_modes_bitwise_vs_mirror(M):
    depth, cad, init = synthetic_batch(3)
    out = M.icp_registration_batch(depth, cad, torch.from_numpy(init), iteration=12, voxel_size=0.008,
                                   return_history=True, device="cpu")
    for b in range(3):
        ref = R.register(depth[b], cad[b], init[b], iteration=12, voxel_size=0.008)
        _check([o[b] for o in out[:4]] + [[h[b] for h in out[4]]], ref)
    it = M.icp_registration_batch(depth, cad, init, iteration=4, voxel_size=0.008, return_history=True,
                                  iterative=True, device="cpu")
    for b in range(3):
        ref = R.register_iterative(depth[b], cad[b], init[b], iteration=4, voxel_size=0.008)
        _check([o[b] for o in it[:4]] + [[h[b] for h in it[4]]], ref)


def test_cached_targets_and_active_mask(M):
    depth, cad, init = synthetic_batch(3, seed=1)
    ref = [R.register(depth[b], cad[0], init[b], iteration=10, voxel_size=0.008) for b in range(3)]
    for _ in range(2):  # second call: the target comes from the cache
        out = M.icp_registration_batch(depth, [cad[0]] * 3, init, iteration=10, voxel_size=0.008, cad_keys=[4, 4, 4],
                                       active=[True, False, True], device="cpu")
        for b in (0, 2):
            _check([o[b] for o in out], ref[b], hist=False)
        assert np.array_equal(out[0][1].numpy(), init[1]) and int(out[3][1]) == 0
    assert len(M._CACHE) == 1
