"""TSDF labels without a GPU: the mirror's results over the cases take every branch of the contract; what the fused
labels mean (the mirror's label image from a held-out pose against the analytic label render); the argument validation
of contrib.InstanceTsdfVolume and of ModelTracker.track(depth, label); and ModelTracker with labels on the host
emulator -- the poses are those of the plain tracker."""
import numpy as np
import pytest
import torch

import camtrack_cases as CC
import tsdflabel_cases as C
import tsdflabel_ref as LR
from host_emul import emul
from morefusion_amd.contrib import InstanceTsdfVolume, ModelTracker, TsdfVolume

# the agreement measured on the mirror for sequence (a): 269 of 273 pixels (DESIGN.md "TSDF labels")
LABEL_AGREEMENT = 0.9853


@pytest.fixture(scope="module")
def mirror():
    return {name: C.run_mirror(C.make_case(name)) for name in C.CASES}


def test_the_cases_take_every_branch(mirror):
    """Every vote outcome (claim, agree, saturate, decrement, release, and each kind of no-vote: not updated, far in
    front of the surface, -2, 0, below -2, skip word), every publish outcome (ground, outside, under-weight, target,
    other instance, background, unowned, free, in between), non-empty and empty statistics rows."""
    results = [r for res in mirror.values() for r in res]
    votes, outcomes = C.coverage(results)
    assert votes == {-1, LR.NOT_UPDATED, LR.FAR, LR.UNCERTAIN, LR.ZERO, LR.BELOW, LR.CLAIM, LR.AGREE, LR.SATURATE,
                     LR.DECREMENT, LR.RELEASE}
    assert outcomes == {LR.GROUND, LR.OUTSIDE, LR.UNDER_WEIGHT, LR.TARGET, LR.OTHER, LR.BACKGROUND, LR.UNOWNED, LR.FREE,
                        LR.BETWEEN}
    counts = np.concatenate([r["table"][:, 0] for r in results if "table" in r])
    assert (counts > 0).any() and (counts == 0).any()
    # both sides of min_count in the label image and in the statistics, and a publication that dropped an id
    a = mirror["a"]
    assert (a[7]["label_image"] != a[8]["label_image"]).any() and (a[5]["table"][:2, 0] < a[4]["table"][:2, 0]).all()
    assert a[-1]["instance_ids"].tolist() == [1, 3]
    for r in results:  # target and no-entry never overlap; the mask is the no-entry grid
        if "outcome" in r:
            assert not (r["grid_target"] * r["grid_noentry"]).any()
            assert np.array_equal(r["grid_nontarget_empty"], r["grid_noentry"] != 0)


def test_statistics_are_the_spheres(mirror):
    """After sequence (a): the centre of each sphere's solid voxels is within two voxels of the sphere's centre in x and
    y and inside the sphere in z (the camera sees its upper half only), and the bounds hold the centre."""
    stats = mirror["a"][4]
    for row, (_, centre, radius) in zip(range(2), C.SPHERES):
        assert np.abs(stats["center"][row][:2] - centre[:2]).max() < 2 * C.VOLUME["pitch"]
        assert centre[2] < stats["center"][row][2] < centre[2] + radius
        assert (stats["bbx_min"][row] <= stats["center"][row]).all() and (stats["center"][row] <= stats["bbx_max"][row]).all()
    assert np.isnan(stats["center"][2:]).all() and (stats["count"][2:] == 0).all()


def test_fused_labels_agree_with_the_analytic_label_render():
    """Sequence (a) fused into the mirror volume, ray-cast from a held-out pose: over the pixels where both the render
    of the model and the analytic render see a surface, the fused label is the analytic one -- everywhere but on the
    spheres' silhouettes, where a 2 cm voxel holds both sides.  Floor: the recorded agreement minus 0.02."""
    case = C.make_case("a")
    vol = LR.InstanceVolume(**case["volume"])
    for op in case["ops"]:
        if op[0] == "integrate":
            vol.integrate(op[1], C.K, op[2], label=op[3])
    depth, _ = vol.raycast(C.K, C.HELD_OUT, C.H, C.W)
    got = vol.label_image(depth, C.K, C.HELD_OUT)
    exp_depth, exp = C.render(C.HELD_OUT)
    both = (depth > 0) & (exp_depth > 0)
    agreement = float((got[both] == exp[both]).mean())
    print(f"label agreement {agreement:.4f} over {int(both.sum())} pixels")
    assert both.sum() > 250 and set(np.unique(exp[both])) == {-1, 1, 3}
    assert agreement >= LABEL_AGREEMENT - 0.02
    # away from the silhouettes (the analytic label's 3 x 3 neighbourhood is uniform) there is no error at all
    pad = np.pad(exp, 1, mode="edge")
    flat = np.all([pad[1 + dy:C.H + 1 + dy, 1 + dx:C.W + 1 + dx] == exp for dy in (-1, 0, 1) for dx in (-1, 0, 1)], 0)
    assert (both & flat).sum() > 150 and (got[both & flat] == exp[both & flat]).all()


def test_instance_tsdf_volume_validates_its_arguments():
    ok = dict(dims=(8, 8, 8), pitch=0.1, origin=(0, 0, 0), device="cpu")
    for max_count in (0, -1, 1.5):
        with pytest.raises(ValueError, match="max_count"):
            InstanceTsdfVolume(**dict(ok, max_count=max_count))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        InstanceTsdfVolume(**ok)


@pytest.fixture()
def product(monkeypatch):
    if not emul.available():
        pytest.skip("g++ not available")
    emul.patch_lib(emul.build(["tsdf.hip", "tsdflabel.hip", "camtrack.hip", "pickorder.hip"]), monkeypatch)


K = np.array([[50.0, 0, 20], [0, 50.0, 16], [0, 0, 1]])


def test_methods_validate_their_arguments(product):
    vol = InstanceTsdfVolume((8, 8, 8), 0.1, (0, 0, 0.5), device="cpu")
    assert vol.max_count == 64 and vol.labels.shape == (8, 8, 8, 2) and vol.labels.dtype == torch.int32
    assert not vol.labels.any()
    d, T, lab = np.ones((32, 40), np.float32), np.eye(4), np.ones((32, 40), np.int32)
    with pytest.raises(TypeError, match="integer image"):
        vol.integrate(d, K, T, label=lab.astype(np.float32))
    with pytest.raises(ValueError, match="like the depth"):
        vol.integrate(d, K, T, label=lab[:, :39])
    with pytest.raises(TypeError, match="skip_if"):
        vol.integrate(d, K, T, label=lab, skip_if=np.zeros(1, np.int32))
    with pytest.raises(ValueError, match="one \\[H, W\\] image"):
        vol.integrate(np.ones((2, 32, 40), np.float32), K, T, label=lab)
    with pytest.raises(ValueError, match="min_count"):
        vol.label_image(d, K, T, min_count=0)
    assert not vol.labels.any() and not vol.weight.any()  # nothing above reached a kernel
    for ids, match in (([], "between 1 and 64"), (list(range(1, 66)), "between 1 and 64"), ([3, 1], "ascending"),
                       ([1, 1], "ascending"), ([0, 1], ">= 1"), ([-2, 1], ">= 1")):
        with pytest.raises(ValueError, match=match):
            vol.instance_stats(ids)
    with pytest.raises(ValueError, match="min_weight"):
        vol.instance_stats([1], min_weight=0.0)
    with pytest.raises(ValueError, match="ids >= 1"):
        vol.publish_grids(T, [-1, 1], [0.01, 0.01])
    with pytest.raises(ValueError, match="pitches"):
        vol.publish_grids(T, [1, 2], [0.01])
    with pytest.raises(ValueError, match="each > 0"):
        vol.publish_grids(T, [1], [0.0])
    with pytest.raises(ValueError, match="dim"):
        vol.publish_grids(T, [1], [0.01], dim=0)
    with pytest.raises(ValueError, match="centers"):
        vol.publish_grids(T, [1], [0.01], centers=np.zeros((2, 3)))
    with pytest.raises(ValueError, match="\\[4, 4\\]"):
        vol.publish_grids(np.eye(3), [1], [0.01])
    # an int64 label tensor goes in; reset clears both tensors; nothing seen: every id is dropped
    vol.integrate(d, K, T, label=torch.ones((32, 40), dtype=torch.int64))
    assert vol.labels.any() and vol.weight.any()
    assert vol.reset() is vol and not vol.labels.any() and not vol.weight.any() and (vol.tsdf == 1).all()
    out = vol.publish_grids(T, [1, 2], {1: 0.01, 2: 0.02})
    assert out["instance_ids"] == [] and out["grid_target"].shape == (0, 32, 32, 32)
    assert out["grid_nontarget_empty"].dtype == torch.bool and out["origin"].dtype == torch.float64


SMALL_VOLUME = dict(dims=(41, 24, 31), pitch=0.04, origin=(-0.8, -0.62, 0.3))
KNOBS = dict(levels=2, iterations=(3, 2), min_pairs=20)


def test_model_tracker_with_labels_finds_the_plain_trackers_poses(product):
    frames = CC.sequence(4, 3, 30, 40)
    labels = [np.where(f["label_detected"] >= 0, f["label_detected"] + 1, -1).astype(np.int32) for f in frames]
    plain_volume = TsdfVolume(device="cpu", **SMALL_VOLUME)
    with pytest.raises(TypeError, match="InstanceTsdfVolume"):
        ModelTracker(frames[0]["K"], 30, 40, plain_volume, **KNOBS).track(frames[0]["depth"], labels[0])
    assert not plain_volume.weight.any()
    plain = ModelTracker(frames[0]["K"], 30, 40, plain_volume, **KNOBS)
    vol = InstanceTsdfVolume(device="cpu", **SMALL_VOLUME)
    trk = ModelTracker(frames[0]["K"], 30, 40, vol, **KNOBS)
    seen = []
    for k, f in enumerate(frames):
        label = labels[k] if k % 2 else (lambda T, k=k: seen.append(T.clone()) or torch.as_tensor(labels[k]))
        got = trk.track(f["depth"], label)
        assert np.array_equal(got.numpy(), plain.track(f["depth"]).numpy()), k
        assert np.array_equal(vol.volume.numpy(), plain_volume.volume.numpy()), k
    assert len(seen) == 2 and np.array_equal(seen[1].numpy(), got.numpy())  # the callable got the pose just found
    assert vol.labels[..., 1].max() == 3 and (vol.labels[..., 0] == -1).any() and (vol.labels[..., 0] >= 1).any()
    # a lost alignment leaves the labels alone too
    lost = ModelTracker(frames[0]["K"], 30, 40, vol, **dict(KNOBS, min_pairs=30 * 40 + 1))
    lost._T_last = got
    before = vol.labels.numpy().copy()
    lost.track(frames[2]["depth"], labels[2])
    assert lost.lost and vol.labels.numpy().tobytes() == before.tobytes()
