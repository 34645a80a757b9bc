#!/usr/bin/env python
"""singleview_3d evaluation -- counterpart of the reference's examples/ycb_video/singleview_3d/evaluate.py: per frame
predict, take the most confident pose, refine it with ICP and / or ICC, score ADD / ADD-S of every (object, method)
against the ground truth, write ``evaluate.csv`` and print the ADD(-S) AUC per method.

Everything between the inputs and the two metric vectors runs on the device
(``morefusion_amd.contrib.singleview_3d.evaluate_batch``).  Frames are synthetic
(``synthetic.make_singleview_examples`` + ``transform_example``) or the instances of a re-indexed dataset directory
(``--dataset``, grouped by image).  ``--model snapshot.npz`` loads a Chainer checkpoint of the reference, ``--random``
keeps the random initialisation.  The YCB CAD models are a download, so solid primitives of each class's size stand in
for them (``get_pcd`` / ``get_sdf``)."""
import argparse
import csv
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import morefusion_amd as morefusion  # noqa: E402
from morefusion_amd.contrib.singleview_3d import METHODS, evaluate_batch  # noqa: E402
from morefusion_amd.contrib.singleview_3d.models import Model, PitchTableModels  # noqa: E402

COLUMNS = ("frame_index", "batch_index", "class_id", "add_or_add_s", "add_s", "method")


class PrimitiveModels(PitchTableModels):
    """A solid primitive per class on a lattice of the class's voxel pitch, with its signed distance."""

    def __init__(self):
        rs = np.random.RandomState(0)
        self._sdf = {}
        for cid, pitch in morefusion.synthetic.CLASS_PITCH.items():
            self._sdf[cid] = morefusion.synthetic.make_primitive(("box", "cylinder", "sphere")[cid % 3], pitch, rs)
        super().__init__({cid: points for cid, (points, _) in self._sdf.items()})

    def get_sdf(self, class_id):
        return self._sdf[int(class_id)]


def synthetic_frames(n_frames, n_objects):
    for frame in range(n_frames):
        yield morefusion.synthetic.make_singleview_examples(n_objects, seed=frame)


def dataset_frames(root_dir, n_frames):
    dataset = morefusion.datasets.RGBDPoseEstimationDatasetReIndexedBase(root_dir)
    for frame, image_id in enumerate(dataset._image_id_to_instance_ids):
        if frame == n_frames:
            return
        indices = dataset.get_indices_from_image_id(image_id)
        if indices:
            yield dataset.get_examples(indices)


def main(args):
    torch.manual_seed(0)
    models = PrimitiveModels()
    model = Model(n_fg_class=21, with_occupancy=True, models=models)
    if args.model:
        morefusion.serializers.load_npz(args.model, model)
    model = model.cuda().eval()
    frames = dataset_frames(args.dataset, args.frames) if args.dataset else synthetic_frames(args.frames, args.objects)
    rows = []
    for frame_index, examples in enumerate(frames):
        examples = [morefusion.synthetic.transform_example(e) for e in examples]
        batch = {k: np.stack([e[k] for e in examples]) for k in examples[0]}
        rows += evaluate_batch(model, batch, models, methods=args.methods, frame_index=frame_index)[0]
    os.makedirs(args.log_dir, exist_ok=True)
    path = os.path.join(args.log_dir, "evaluate.csv")
    with open(path, "w", newline="") as f:
        writer = csv.writer(f)
        writer.writerow(("",) + COLUMNS)  # (the leading index column of pandas.DataFrame.to_csv)
        for k, row in enumerate(rows):
            writer.writerow([k] + [row[c] for c in COLUMNS])
    print(f"{len(rows)} rows -> {path}")
    for method in args.methods:
        errors = np.array([r["add_or_add_s"] for r in rows if r["method"] == method])
        print(f"{method:>20}: ADD(-S) AUC {morefusion.metrics.ycb_video_add_auc(errors):.4f}, "
              f"mean {errors.mean():.4f} m over {errors.size} objects")


if __name__ == "__main__":
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    group = parser.add_mutually_exclusive_group(required=True)
    group.add_argument("--model", help="chainer .npz checkpoint (snapshot_model_best_auc.npz)")
    group.add_argument("--random", action="store_true", help="random weights")
    parser.add_argument("--dataset", help="a re-indexed dataset directory (default: synthetic frames)")
    parser.add_argument("--frames", type=int, default=4)
    parser.add_argument("--objects", type=int, default=3, help="objects per synthetic frame")
    parser.add_argument("--methods", nargs="+", default=list(METHODS), choices=METHODS)
    parser.add_argument("--log-dir", default="logs/singleview_3d_evaluate")
    main(parser.parse_args())
