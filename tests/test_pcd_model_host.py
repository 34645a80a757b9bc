"""Host-side contracts of the point-cloud baseline network (contrib/singleview_pcd): checkpoint naming, refused
losses, and the point selection it shares with the 3-D model."""
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN


def test_parameter_paths_match_the_reference_link_tree_and_round_trip(tmp_path):
    import morefusion_amd as mf
    from morefusion_amd import serializers
    from morefusion_amd.contrib.singleview_pcd.models import Model
    ref = json.load(open(os.path.join(GOLDEN, "ref_pcd_chainer_param_paths.json")))["params"]
    torch.manual_seed(1)
    model = Model(n_fg_class=21)
    mine = {key: list(t.shape) for _, key, t in serializers._entries(model)}
    mine = {k: ([] if k.endswith("prelu/W") else v) for k, v in mine.items()}  # Chainer's PReLU slope is a scalar
    assert mine == ref
    assert {"posenet_extractor/conv1_pcd/W", "conv1_rot/W", "conv4_conf/b"} <= set(ref)
    assert ref["conv1_rot/W"] == [640, 1408, 1] and ref["posenet_extractor/conv1_pcd/W"] == [64, 3, 1]
    # a snapshot in the reference's naming (written array by array, not through save_npz) loads and reproduces the state
    state = {k: v.clone() for k, v in model.state_dict().items()}
    arrays = {key: (t.detach().numpy().reshape(()) if key.endswith("prelu/W") else t.detach().numpy())
              for _, key, t in serializers._entries(model)}
    assert set(arrays) == set(ref)
    np.savez(tmp_path / "snapshot.npz", **{"updater/model:main/" + k: v for k, v in arrays.items()})
    torch.manual_seed(2)
    other = Model(n_fg_class=21)
    assert not torch.equal(other.conv1_rot.weight, model.conv1_rot.weight)
    left = serializers.load_npz(tmp_path / "snapshot.npz", other, path="updater/model:main/")
    assert left == []
    for k, v in other.state_dict().items():
        assert torch.equal(v, state[k]), k
    # ... and save_npz writes exactly those keys
    serializers.save_npz(tmp_path / "mine.npz", model)
    with np.load(tmp_path / "mine.npz") as z:
        assert set(z.files) == set(ref)
    assert mf.contrib.singleview_pcd.models.Model is Model
    import morefusion
    assert morefusion.contrib.singleview_pcd.models.Model is Model


@pytest.mark.parametrize("loss", ["add/add_s+occupancy", "add+occupancy", "overlap", ""])
def test_unknown_losses_are_refused(loss):
    from morefusion_amd.contrib.singleview_pcd.models import Model
    with pytest.raises(ValueError, match="unknown loss"):
        Model(n_fg_class=2, loss=loss)


def test_known_losses_and_defaults():
    from morefusion_amd.contrib.singleview_pcd.models import Model
    assert Model(n_fg_class=2)._loss == "add/add_s" and Model(n_fg_class=2, loss="add")._loss == "add"
    m = Model(n_fg_class=2, centerize_pcd=False)
    assert m._n_point == 1000 and m._lambda_confidence == 0.015 and not m._centerize_pcd and m.pcd_kernels


def test_shared_point_selection_is_what_the_3d_model_had():
    """The mix-in returns, for the 3-D model and for the baseline, what ``Model._keep_indices`` of the 3-D model
    returned before it was factored out: the reference's RandomState(1234) subsample / pad, restated here."""
    from morefusion_amd.contrib.point_selection import PointSelection
    from morefusion_amd.contrib.singleview_3d.models import Model as Model3D
    from morefusion_amd.contrib.singleview_pcd.models import Model as ModelPcd
    assert issubclass(Model3D, PointSelection) and issubclass(ModelPcd, PointSelection)
    assert Model3D._keep_indices is ModelPcd._keep_indices is PointSelection._keep_indices
    assert Model3D._eval_keep_cache is PointSelection._eval_keep_cache
    m3, mp = Model3D(n_fg_class=2).eval(), ModelPcd(n_fg_class=2).eval()
    for n in (1, 7, 999, 1000, 1001, 8797):
        rs = np.random.RandomState(1234)
        want = rs.permutation(n)[:1000] if n >= 1000 else np.r_[np.arange(n), rs.randint(0, n, 1000 - n)]
        for m in (m3, mp):
            got = m._keep_indices(n)
            assert got.dtype == np.int64 and np.array_equal(got, want), n
    for m in (m3, mp):
        with pytest.raises(ValueError, match="no valid point"):
            m._keep_indices(0)
    order = torch.arange(2000, dtype=torch.int32).flip(0)[None].repeat(2, 1)
    assert torch.equal(m3._subsample(order, np.array([1500, 3])), mp._subsample(order, np.array([1500, 3])))
    m3.train()
    np.random.seed(3)
    a = m3._keep_indices(1500)
    np.random.seed(3)
    assert np.array_equal(a, np.random.permutation(1500)[:1000])  # training: the global NumPy RNG, not memoised


def test_predict_refuses_cpu_tensors_and_crops_without_points():
    from morefusion_amd.contrib.singleview_pcd.models import Model
    m = Model(n_fg_class=2).eval()
    rgb = torch.zeros((1, 16, 16, 3), dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.predict(class_id=torch.tensor([1]), rgb=rgb, pcd=torch.zeros((1, 16, 16, 3)))
