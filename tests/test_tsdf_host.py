"""TSDF fusion without a GPU: the argument validation of contrib.TsdfVolume and contrib.ModelTracker, a known answer
of the NumPy mirror (tests/tsdf_ref.py), the accuracy of the mirror's ModelTracker on synthetic sequences -- the
condition the device inherits by being bitwise equal to it -- and ModelTracker on the host emulator against the
mirror's."""
import numpy as np
import pytest
import torch

import camtrack_cases as CC
import camtrack_ref as CR
import tsdf_cases as C
import tsdf_ref as R
from host_emul import emul
from morefusion_amd.contrib import ModelTracker, TsdfVolume

K = np.array([[50.0, 0, 20], [0, 50.0, 16], [0, 0, 1]])


def test_tsdf_volume_validates_its_arguments():
    ok = dict(dims=(8, 8, 8), pitch=0.1, origin=(0, 0, 0), device="cpu")
    for change, match in ((dict(dims=(8, 8)), "dims"), (dict(dims=(8, 1, 8)), "dims"),
                          (dict(dims=(2048, 1024, 1024)), "2\\^31"), (dict(pitch=0.0), "pitch"),
                          (dict(pitch=float("nan")), "pitch"), (dict(origin=(0, 0)), "origin"),
                          (dict(truncation=-1.0), "truncation"), (dict(max_weight=0.0), "max_weight")):
        with pytest.raises(ValueError, match=match):
            TsdfVolume(**dict(ok, **change))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        TsdfVolume(**ok)


@pytest.fixture()
def product(monkeypatch):
    if not emul.available():
        pytest.skip("g++ not available")
    emul.patch_lib(emul.build(["tsdf.hip", "camtrack.hip", "pickorder.hip"]), monkeypatch)


def test_integrate_and_raycast_validate_their_arguments(product):
    vol = TsdfVolume((8, 8, 8), 0.1, (0, 0, 0.5), device="cpu")
    assert vol.truncation == 0.4 and vol.max_weight == 64.0
    assert vol.volume.shape == (8, 8, 8, 2) and (vol.tsdf == 1).all() and not vol.weight.any()
    d, T = np.ones((32, 40), np.float32), np.eye(4)
    with pytest.raises(ValueError, match="3 x 3"):
        vol.integrate(d, np.eye(4), T)
    with pytest.raises(ValueError, match="fx and fy must be > 0"):
        vol.integrate(d, np.diag([-50.0, 50.0, 1.0]), T)
    with pytest.raises(TypeError, match="float image"):
        vol.integrate(d.astype(np.int32), K, T)
    with pytest.raises(ValueError, match="one \\[H, W\\] image"):
        vol.integrate(np.ones((2, 32, 40), np.float32), K, T)
    with pytest.raises(ValueError, match="T_sensor_to_map"):
        vol.integrate(d, K, np.eye(3))
    with pytest.raises(TypeError, match="skip_if"):
        vol.integrate(d, K, T, skip_if=torch.zeros(1, dtype=torch.int64))
    with pytest.raises(TypeError, match="skip_if"):
        vol.integrate(d, K, T, skip_if=np.zeros(1, np.int32))
    assert not vol.weight.any()  # nothing above reached the kernel
    with pytest.raises(ValueError, match="height x width"):
        vol.raycast(K, T, 0, 40)
    with pytest.raises(ValueError, match="step"):
        vol.raycast(K, T, 32, 40, step=0.0)
    with pytest.raises(ValueError, match="min_depth"):
        vol.raycast(K, T, 32, 40, min_depth=2.0, max_depth=1.0)
    with pytest.raises(ValueError, match="samples per ray"):
        vol.raycast(K, T, 32, 40, step=1e-6)
    with pytest.raises(ValueError, match="T_sensor_to_map"):
        vol.raycast(K, np.eye(3), 32, 40)
    vol.integrate(d, K, T)
    assert vol.weight.any() and vol.reset() is vol and not vol.weight.any() and (vol.tsdf == 1).all()
    assert vol.raycast(K, T, 32, 40).shape == (32, 40) and vol.max_steps(0.2) == int(0.7 * 3 ** 0.5 / 0.2) + 2


def test_model_tracker_validates_its_arguments(product):
    vol = TsdfVolume((8, 8, 8), 0.1, (0, 0, 0.5), device="cpu")
    with pytest.raises(TypeError, match="TsdfVolume"):
        ModelTracker(K, 32, 40, None)
    with pytest.raises(TypeError, match="reference is fixed"):
        ModelTracker(K, 32, 40, vol, reference="previous")
    with pytest.raises(TypeError, match="device is fixed"):
        ModelTracker(K, 32, 40, vol, device="cpu")
    with pytest.raises(ValueError, match="at least 8 x 8"):
        ModelTracker(K, 30, 40, vol)
    with pytest.raises(ValueError, match="T_first"):
        ModelTracker(K, 32, 40, vol, levels=2, iterations=(1, 1), T_first=np.eye(3))
    with pytest.raises(ValueError, match="fx and fy must be > 0"):
        ModelTracker(np.diag([50.0, -50.0, 1.0]), 32, 40, vol, levels=2, iterations=(1, 1))
    trk = ModelTracker(K, 32, 40, vol, levels=2, iterations=(1, 1))
    with pytest.raises(ValueError, match="32 x 40"):
        trk.track(np.ones((32, 41), np.float32))
    with pytest.raises(RuntimeError, match="no alignment yet"):
        trk.status


def test_mirror_returns_a_fronto_parallel_plane_to_a_micrometre():
    """One plane at depth D seen from the identity, integrated once and ray-cast from the same pose: along every ray
    the fused field is the linear function (D - s) / truncation of the depth s, trilinear interpolation is exact for a
    field that is linear in z, so the zero crossing is D -- to 1e-6 m (float32 storage of the field: 6e-8 of the
    truncation per voxel) on every pixel whose ray meets the plane inside the box of voxel centres."""
    D, H, W = 0.8125, 24, 32
    vol = R.Volume((13, 9, 17), 0.04, (-0.24, -0.16, 0.5))  # inside the frustum: every voxel in front of D is seen
    Kc = np.array([[30.0, 0, 15.5], [0, 30.0, 11.5], [0, 0, 1]])
    vol.integrate(np.full((H, W), D, np.float32), Kc, np.eye(4))
    depth, code = vol.raycast(Kc, np.eye(4), H, W)
    v, u = np.mgrid[:H, :W]
    x, y = D * (u - 15.5) / 30.0, D * (v - 11.5) / 30.0
    margin = 0.04  # one voxel inside the box: the crossing's 8 corners and those of the sample before it exist
    inside = (np.abs(x) < 0.24 - margin) & (np.abs(y) < 0.16 - margin)
    assert inside.sum() > 100
    assert (code[inside] == R.HIT).all()
    assert np.abs(depth[inside].astype(np.float64) - D).max() <= 1e-6


@pytest.mark.parametrize("seed", CC.ACCURACY_SEEDS)
def test_mirror_tracks_against_the_model_from_the_identity(seed):
    """On every frame the translation and the rotation error are at most a quarter of the identity pose's (the
    camera tracker's own condition) and at most twice what was recorded for the mirror in tsdf_cases.py."""
    frames = C.model_sequence(seed)
    poses, trk = C.track_model_mirror(frames)
    assert np.array_equal(poses[0], np.eye(4)) and trk.status[0] == CR.TRACKING
    errors = CC.sequence_errors(frames, poses)
    print(f"seed {seed}: (t_err, r_err, identity's t_err, r_err) = {errors}")
    assert len(errors) == len(C.MODEL_ERRORS[seed]) == C.MODEL_FRAMES - 1
    for (t_err, r_err, t_id, r_id), (t_rec, r_rec) in zip(errors, C.MODEL_ERRORS[seed]):
        assert t_err <= t_id / 4 and r_err <= r_id / 4
        assert t_err <= 2 * t_rec and r_err <= 2 * r_rec


SMALL_VOLUME = dict(dims=(41, 24, 31), pitch=0.04, origin=(-0.8, -0.62, 0.3))
KNOBS = dict(levels=2, iterations=(3, 2), min_pairs=20)


def test_model_tracker_matches_the_mirror_and_a_loss_leaves_the_model_alone(product):
    frames = CC.sequence(4, 3, 30, 40)
    anchor = np.array([[1.0, 0, 0, 0.0], [0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]])
    vol = TsdfVolume(device="cpu", **SMALL_VOLUME)
    trk = ModelTracker(frames[0]["K"], 30, 40, vol, T_first=anchor, **KNOBS)
    ref = R.ModelTracker(frames[0]["K"], 30, 40, R.Volume(**SMALL_VOLUME), T_first=anchor, **KNOBS)
    for k, f in enumerate(frames):
        got = trk.track(torch.as_tensor(f["depth"]) if k % 2 else f["depth"])
        assert isinstance(got, torch.Tensor) and got.dtype == torch.float64 and got.shape == (4, 4)
        assert np.array_equal(got.numpy(), ref.track(f["depth"])), k
        assert np.array_equal(vol.volume.numpy(), ref.volume.volume), k
        if k:
            assert trk.status == ref.status[0] == CR.TRACKING and not trk.lost
            assert np.array_equal(trk.stats, ref.stats[0])
    assert vol.weight.max() == 3
    # a tracker that cannot find its pairs: lost, the pose the last one, every byte of the model as before
    lost = ModelTracker(frames[0]["K"], 30, 40, vol, **dict(KNOBS, min_pairs=30 * 40 + 1))
    lost._T_last = got
    before = vol.volume.numpy().copy()
    T = lost.track(frames[2]["depth"])
    assert lost.lost and np.allclose(T.numpy(), got.numpy(), rtol=0, atol=1e-15)
    assert vol.volume.numpy().tobytes() == before.tobytes()
