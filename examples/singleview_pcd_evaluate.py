#!/usr/bin/env python
"""singleview_pcd evaluation -- counterpart of the reference's examples/ycb_video/singleview_pcd/evaluate.py for one
batch: model.predict, the arg-max-confidence pose per object, and ADD / ADD-S against the ground truth through the
device metric (``metrics.average_distance_device``, float64: the poses never leave the GPU).  Synthetic examples and
synthetic CAD clouds; ``--model snapshot.npz`` loads a Chainer checkpoint of the reference."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import morefusion_amd as morefusion  # noqa: E402
from morefusion_amd.contrib.singleview_3d.evaluate import argmax_pose  # noqa: E402
from morefusion_amd.contrib.singleview_3d.models import PitchTableModels  # noqa: E402
from morefusion_amd.contrib.singleview_pcd.models import Model  # noqa: E402


def main(batch_size=2, checkpoint=None):
    torch.manual_seed(0)
    rs = np.random.RandomState(0)
    pcds = {c: rs.uniform(-0.05, 0.05, (800, 3)) for c in morefusion.synthetic.CLASS_PITCH}
    model = Model(n_fg_class=21, models=PitchTableModels(pcds))
    if checkpoint:
        morefusion.serializers.load_npz(checkpoint, model)
    model = model.cuda().eval()
    examples = morefusion.synthetic.make_singleview_batch(batch_size, seed=0)
    b = {k: torch.as_tensor(examples[k]).cuda() for k in ("class_id", "rgb", "pcd", "quaternion_true", "translation_true")}
    with torch.no_grad():
        quaternion, translation, confidence = model.predict(class_id=b["class_id"], rgb=b["rgb"], pcd=b["pcd"])
        quaternion, translation = argmax_pose(quaternion, translation, confidence)
        report = model.evaluate(class_id=b["class_id"], quaternion_true=b["quaternion_true"],
                                translation_true=b["translation_true"], quaternion_pred=quaternion,
                                translation_pred=translation, per_instance=True, on_device=True)
    for i, cid in enumerate(b["class_id"].tolist()):
        print(f"class {cid:2d} quaternion {quaternion[i].cpu().numpy().round(4)} translation {translation[i].cpu().numpy().round(4)}")
    for key in sorted(report):
        kind, cid, _ = key.split("/")
        print(f"class {int(cid):2d} {kind:13s} {report[key]:.5f} m")


if __name__ == "__main__":
    parser = argparse.ArgumentParser()
    parser.add_argument("--model", help="chainer .npz checkpoint of the reference's singleview_pcd model")
    parser.add_argument("--batch-size", type=int, default=2)
    args = parser.parse_args()
    main(args.batch_size, args.model)
