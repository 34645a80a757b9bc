"""The evaluation loop end to end on the MI355X (contrib/singleview_3d/evaluate.py, Model.evaluate(on_device=True)):
the seam between the network's pose and the refiners, and the metric of every row.  Small synthetic inputs: three
objects of ``synthetic.make_singleview_examples`` through ``transform_example``, random weights with a fixed seed, CAD
stand-ins from ``synthetic.make_primitive`` / ``synthetic_sdf``.  Free-running refinement trajectories are NOT compared
with the oracle from different start poses (ill-conditioned); the refiners are pinned in their own tests."""
import numpy as np
import pytest
import torch

import morefusion_amd as mf
from morefusion_amd.contrib.singleview_3d import METHODS, evaluate_batch
from morefusion_amd.contrib.singleview_3d.evaluate import argmax_pose, icc_scene
from morefusion_amd.contrib.singleview_3d.models import Model, PitchTableModels
from morefusion_amd.functions.geometry.transformation_matrix import transformation_matrix_batch
from morefusion_amd.synthetic import CLASS_IDS_SYMMETRIC, CLASS_PITCH

pytestmark = pytest.mark.gpu
ATOL = 1e-12  # the device metric against the host function (tests/posemetric_cases.py HOST_ATOL has the reasoning)
SEED = 8      # classes 10, 13, 16: one asymmetric, two symmetric


class StandInModels(PitchTableModels):
    """``YCBVideoModels`` stand-in: a solid primitive per class on a lattice of the class's pitch, its signed distance
    from ``synthetic_sdf`` with a few NaN entries (the reference's sdf files have them; the loop drops them)."""

    def __init__(self, class_ids):
        rs = np.random.RandomState(3)
        self._sdf = {}
        for k, cid in enumerate(sorted(set(class_ids))):
            points, _ = mf.synthetic.make_primitive(("box", "cylinder", "sphere")[k % 3], CLASS_PITCH[cid], rs)
            sdf = mf.synthetic.synthetic_sdf(points)
            sdf[rs.permutation(len(sdf))[:5]] = np.nan
            self._sdf[cid] = (points, sdf)
        super().__init__({cid: p for cid, (p, _) in self._sdf.items()})

    def get_sdf(self, class_id):
        return self._sdf[int(class_id)]


@pytest.fixture(scope="module")
def joint():
    torch.manual_seed(0)
    examples = [mf.synthetic.transform_example(e) for e in mf.synthetic.make_singleview_examples(3, seed=SEED)]
    batch = {k: np.stack([e[k] for e in examples]) for k in examples[0]}
    models = StandInModels(batch["class_id"].tolist())
    model = Model(n_fg_class=21, with_occupancy=True, models=models).cuda().eval()
    recorded = []
    predict = model.predict

    def recording_predict(**kw):  # what evaluate_batch consumed is what the seam is compared with
        recorded.append(predict(**kw))
        return recorded[-1]

    model.predict = recording_predict
    try:
        rows, transforms = evaluate_batch(model, batch, models, frame_index=7)
    finally:
        del model.predict
    assert len(recorded) == 1
    quaternion, translation = argmax_pose(recorded[0][0].float(), recorded[0][1].float(), recorded[0][2])
    return dict(model=model, models=models, batch=batch, rows=rows, transforms=transforms, quaternion=quaternion,
                translation=translation)


def test_model_evaluate_on_device_equals_host(joint):
    kw = dict(class_id=torch.as_tensor(joint["batch"]["class_id"]),
              quaternion_true=torch.as_tensor(joint["batch"]["quaternion_true"]).cuda(),
              translation_true=torch.as_tensor(joint["batch"]["translation_true"]).cuda(),
              quaternion_pred=joint["quaternion"], translation_pred=joint["translation"])
    host, device = joint["model"].evaluate(**kw), joint["model"].evaluate(on_device=True, **kw)
    assert list(host) == list(device) == ["add", "add_s", "add_or_add_s"]
    for k in host:
        print(k, host[k], device[k], abs(host[k] - device[k]))
        assert abs(host[k] - device[k]) <= ATOL and host[k] > 0
    host = joint["model"].evaluate(per_instance=True, **kw)
    device = joint["model"].evaluate(per_instance=True, on_device=True, **kw)
    strip = lambda rep: [k.rsplit("/", 1)[0] for k in rep]  # noqa: E731  ({metric}/{class_id:04d}/{uuid})
    assert strip(host) == strip(device) and len(host) == 9
    np.testing.assert_allclose(list(device.values()), list(host.values()), rtol=0, atol=ATOL)


def test_seam_network_pose_to_refiners(joint):
    from oracle import oracle_c as OC
    q, t, T = joint["quaternion"], joint["translation"], joint["transforms"]
    assert tuple(T) == ("true",) + METHODS
    # the network's arg-max pose IS the "morefusion" transform: wxyz order, no renormalisation in between
    assert torch.equal(T["morefusion"], transformation_matrix_batch(q, t))
    np.testing.assert_allclose(T["morefusion"].cpu().numpy(), mf.functions.transformation_matrix(q, t).cpu().numpy(),
                               rtol=0, atol=1e-6)
    # ICC by hand from those device poses, the same arguments: the same kernels, the same bits
    class_ids = joint["batch"]["class_id"].tolist()
    scene = icc_scene({k: torch.as_tensor(v).cuda() for k, v in joint["batch"].items()}, joint["models"], class_ids)
    scenes = mf.contrib.IccScenes([scene])
    q_icc, t_icc = q.clone(), t.clone()
    scenes.refine(q_icc, t_icc, torch.zeros((3, 7), device="cuda"), torch.zeros((3, 7), device="cuda"), 30,
                  alpha_q=0.01, alpha_t=0.001)
    assert torch.equal(T["morefusion+icc"], transformation_matrix_batch(q_icc, t_icc))
    assert not torch.equal(T["morefusion+icc"], T["morefusion"])
    # the loss ICC starts from, at the network's pose in metric units, against the C oracle (the bound of
    # tests/test_gpu_icc.py for this comparison)
    loss, _, _ = scenes.loss_grad(q, t)
    b = joint["batch"]
    loss_o = OC.icc_loss_grad(scene["points"], scene["sdf"], b["pitch"], b["origin"],
                              b["grid_target"].astype(np.float32), b["grid_nontarget_empty"].astype(np.float32),
                              q.cpu().numpy(), t.cpu().numpy())[0]
    print("ICC loss at iteration 0:", float(loss[0]), "oracle:", loss_o)
    np.testing.assert_allclose(float(loss[0]), loss_o, rtol=2e-5, atol=1e-6)


def test_every_row_equals_the_host_metric(joint):
    rows, T = joint["rows"], joint["transforms"]
    class_ids = joint["batch"]["class_id"].tolist()
    assert len(rows) == len(METHODS) * 3
    assert [r["method"] for r in rows] == [m for m in METHODS for _ in range(3)]
    true = T["true"].cpu().numpy()
    for r in rows:
        assert list(r) == ["frame_index", "batch_index", "class_id", "add_or_add_s", "add_s", "method"]
        i = r["batch_index"]
        assert r["frame_index"] == 7 and r["class_id"] == class_ids[i]
        add, add_s = mf.metrics.average_distance([joint["models"].get_pcd(r["class_id"])], [true[i]],
                                                 [T[r["method"]][i].cpu().numpy()])
        symmetric = r["class_id"] in CLASS_IDS_SYMMETRIC
        print(r["method"], r["class_id"], r["add_or_add_s"], r["add_s"], add[0], add_s[0])
        assert abs(r["add_s"] - add_s[0]) <= ATOL
        assert abs(r["add_or_add_s"] - (add_s[0] if symmetric else add[0])) <= ATOL
        assert (r["add_or_add_s"] == r["add_s"]) == symmetric  # (a random pose is never as near as its neighbour)


def test_symmetry_flags_with_the_truth_as_prediction(joint):
    b = joint["batch"]
    assert {c in CLASS_IDS_SYMMETRIC for c in b["class_id"].tolist()} == {True, False}
    model = joint["model"]
    model.predict = lambda **kw: (torch.as_tensor(b["quaternion_true"]).cuda()[:, None, :],
                                  torch.as_tensor(b["translation_true"]).cuda()[:, None, :],
                                  torch.ones((3, 1), device="cuda"))
    try:
        rows, T = evaluate_batch(model, b, joint["models"], methods=("morefusion",))
    finally:
        del model.predict
    assert torch.equal(T["morefusion"], T["true"])
    assert [r["add_or_add_s"] for r in rows] == [0.0, 0.0, 0.0] and [r["add_s"] for r in rows] == [0.0, 0.0, 0.0]
