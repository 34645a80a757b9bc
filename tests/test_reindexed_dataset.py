"""datasets.reindex and RGBDPoseEstimationDatasetReIndexedBase: three synthetic.make_cad_frame frames written as
the reference's npz tree and read back, plain and augmented (host emulator, 64 x 64 crops); on the MI355X the
augmented minibatch goes through transform_example into one Model loss with gradients."""
import json
import os

import numpy as np
import pytest
import torch

import render_cases as C
import morefusion_amd as mf
from host_emul import emul


class Frames(C.CadFrameDataset):
    def __init__(self, H, W, device, image_size, n_frames=3):
        super().__init__(H, W, device)
        self._image_size = image_size
        self._ids = [f"scene/{i:06d}" for i in range(n_frames)]


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


def _check_dataset(dev, H, W, S, tmp_path):
    base = Frames(H, W, dev, S)
    assert len(base) == 3
    root = tmp_path / "reindexed"
    meta = mf.datasets.reindex(root, [base])
    want = {i: base.get_example(i) for i in range(3)}
    files = sorted(os.path.relpath(os.path.join(dp, f), root) for dp, _, fs in os.walk(root) for f in fs)
    assert files == sorted(["meta.json"] + [f"scene/{i:06d}/{k:08d}.npz" for i in range(3) for k in range(len(want[i]))])
    on_disk = json.load(open(root / "meta.json"))
    assert on_disk == meta and list(on_disk) == [f"scene/{i:06d}/{k:08d}" for i in range(3) for k in range(len(want[i]))]
    assert all(set(m) == {"class_id", "visibility"} and isinstance(m["class_id"], int) for m in on_disk.values())
    ds = mf.datasets.RGBDPoseEstimationDatasetReIndexedBase(root, device=dev)
    flat = [e for i in range(3) for e in want[i]]
    assert len(ds) == len(flat) == 9
    for k, e in enumerate(flat):
        got = ds.get_example(k)
        assert set(got) == set(e) - {"visibility"}
        assert all(_same(np.asarray(got[key]), np.asarray(e[key])) for key in got), k
    assert ds.get_indices_from_image_id("scene/000001") == [3, 4, 5]
    only = int(flat[0]["class_id"])
    sub = mf.datasets.RGBDPoseEstimationDatasetReIndexedBase(root, class_ids=[only], device=dev)
    assert len(sub) == sum(int(e["class_id"]) == only for e in flat) and 0 < len(sub) < len(flat)
    assert all(int(sub.get_example(k)["class_id"]) == only for k in range(len(sub)))
    assert sub.get_indices_from_image_id("scene/000002") == [
        sub._ids.index(i) for i in ds._image_id_to_instance_ids["scene/000002"] if i in sub._ids]
    with pytest.raises(IOError):
        mf.datasets.RGBDPoseEstimationDatasetReIndexedBase(tmp_path / "absent", device=dev)
    # augmentation: one augment_rgbd call over the stacked minibatch, same seed -> same arrays
    aug = mf.datasets.RGBDPoseEstimationDatasetReIndexedBase(root, augmentation=True, device=dev, random_state=5)
    idx = [0, 4, 8, 2]
    got = aug.get_examples(idx)
    rgb = torch.from_numpy(np.stack([flat[i]["rgb"] for i in idx])).to(dev)
    pcd = torch.from_numpy(np.stack([flat[i]["pcd"] for i in idx])).to(dev)
    r, p, keep = mf.datasets.augment_rgbd(rgb, pcd, random_state=5)
    assert bool(keep.all())
    for k, i in enumerate(idx):
        assert _same(got[k]["rgb"], r[k].cpu().numpy()) and _same(got[k]["pcd"], p[k].cpu().numpy())
        assert got[k]["pcd"].dtype == np.float64 and "visibility" not in got[k]
        assert not _same(got[k]["rgb"], flat[i]["rgb"])
        assert _same(got[k]["grid_target"], flat[i]["grid_target"])
    return aug, flat


@pytest.mark.skipif(not emul.available(), reason="g++ not available")
def test_reindex_and_read_back(monkeypatch, tmp_path):
    emul.patch_lib(emul.build(["render.hip", "meshsdf.hip", "occmap.hip", "preprocess.hip", "augment.hip"]), monkeypatch)
    _check_dataset("cpu", 120, 160, 64, tmp_path)


@pytest.mark.gpu
def test_augmented_minibatch_trains(tmp_path):
    from morefusion_amd.chainer_compat import cuda, dataset
    from morefusion_amd.contrib.singleview_3d.models import Model
    aug, flat = _check_dataset("cuda", 480, 640, 256, tmp_path)
    examples = aug.get_examples(list(range(len(aug))))
    before = sum(int((~np.isnan(e["pcd"]).any(-1)).sum()) for e in flat)
    after = sum(int((~np.isnan(e["pcd"]).any(-1)).sum()) for e in examples)
    print(f"valid points: {before} before, {after} after augmentation")
    assert 0 < after
    rs = np.random.RandomState(0)
    batch = dataset.concat_examples([mf.synthetic.transform_example(e, train=True, random_state=rs) for e in examples])
    torch.manual_seed(0)
    model = Model(n_fg_class=21, with_occupancy=True, models=aug_models()).cuda().train()
    keys = ("class_id", "rgb", "pcd", "quaternion_true", "translation_true", "pitch", "origin", "grid_nontarget_empty")
    loss = model(**{k: cuda.to_gpu(batch[k]) for k in keys})
    assert np.isfinite(float(loss))
    loss.backward()
    grads = [p.grad for p in model.parameters() if p.grad is not None]
    assert grads and all(bool(torch.isfinite(g).all()) for g in grads)


def aug_models():
    return C.CadFrameDataset._shared[next(d for d in C.CadFrameDataset._shared if str(d) != "cpu")]
