#!/usr/bin/env python
"""Frames -> re-indexed npz tree -> augmented minibatch -> one training loss: the data path of the reference's
``train.py`` (re-indexed datasets with ``augmentation=True``) on the device.

Frames are rendered from the three meshes under tests/golden/ (``synthetic.make_cad_frame``), ``datasets.reindex``
writes them in the reference's layout into a temporary directory, ``RGBDPoseEstimationDatasetReIndexedBase(...,
augmentation=True).get_examples`` loads a minibatch and augments it in one call (csrc/augment.hip), then
``transform_example(train=True)`` and ``concat_examples`` make the network's batch and ``Model`` returns the loss."""
import argparse
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import morefusion_amd as morefusion  # noqa: E402
from morefusion_amd.chainer_compat import cuda, dataset  # noqa: E402
from morefusion_amd.contrib.singleview_3d.models import Model  # noqa: E402


class CadFrames(morefusion.datasets.RGBDPoseEstimationDatasetBase):

    def __init__(self, models, meshes_by_class, n_frames, n_objects):
        super().__init__(models)
        self._meshes, self._n_objects = meshes_by_class, n_objects
        self._ids = [f"cad_frames/{i:06d}" for i in range(n_frames)]

    def get_frame(self, index):
        return morefusion.synthetic.make_cad_frame(self._meshes, seed=index, n_objects=self._n_objects)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=3)
    ap.add_argument("--objects", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    meshes = {}
    for class_id, name in ((2, "003_cracker_box"), (3, "004_sugar_box"), (9, "010_potted_meat_can")):
        d = np.load(os.path.join(ROOT, "tests", "golden", f"ycb_mesh_{name}.npz"))
        meshes[class_id] = (d["vertices"], d["faces"])
    models = morefusion.datasets.MeshModels(meshes)
    valid = lambda examples: sum(int((~np.isnan(e["pcd"]).any(-1)).sum()) for e in examples)  # noqa: E731
    with tempfile.TemporaryDirectory() as root:
        morefusion.datasets.reindex(root, [CadFrames(models, meshes, args.frames, args.objects)])
        plain = morefusion.datasets.RGBDPoseEstimationDatasetReIndexedBase(root)
        augmented = morefusion.datasets.RGBDPoseEstimationDatasetReIndexedBase(root, augmentation=True,
                                                                               random_state=args.seed)
        indices = list(range(len(plain)))
        before, examples = plain.get_examples(indices), augmented.get_examples(indices)
    print(f"{len(examples)} examples, valid points: {valid(before)} before, {valid(examples)} after augmentation")
    rs = np.random.RandomState(args.seed)
    batch = dataset.concat_examples([morefusion.synthetic.transform_example(e, train=True, random_state=rs)
                                     for e in examples])
    torch.manual_seed(0)
    model = Model(n_fg_class=21, with_occupancy=True, models=models).cuda().eval()
    keys = ("class_id", "rgb", "pcd", "quaternion_true", "translation_true", "pitch", "origin", "grid_nontarget_empty")
    with torch.no_grad():
        loss = model(**{k: cuda.to_gpu(batch[k]) for k in keys})
    print(f"loss {float(loss):.6f}")
    assert np.isfinite(float(loss))
    return float(loss)


if __name__ == "__main__":
    main()
