#!/usr/bin/env python
"""Frame with ground-truth poses in -> training examples out -> one loss evaluation: the reference's
``RGBDPoseEstimationDatasetBase.get_example`` (datasets/rgbd_pose_estimation/base.py:78-197) on the device.

A frame is rendered from triangle meshes at known poses (``synthetic.make_cad_frame``: CAD models on a table in
front of a wall, drawn by csrc/render.hip); ``get_example`` turns it into the reference's per-object example
dicts (crops, occupancy grids, visibility from one render launch, ``grid_*_full`` from one full-grid launch);
``synthetic.transform_example`` and ``concat_examples`` make the network's batch; ``Model`` returns the pose loss.
Meshes: ``--cad-dir`` (a YCB-Video model directory, <NNN_name>/textured_simple.obj) or the three meshes under
tests/golden/."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import morefusion_amd as morefusion  # noqa: E402
from morefusion_amd.chainer_compat import cuda, dataset  # noqa: E402
from morefusion_amd.contrib.singleview_3d.models import Model  # noqa: E402


class CadFrames(morefusion.datasets.RGBDPoseEstimationDatasetBase):

    def __init__(self, models, meshes_by_class, n_objects):
        super().__init__(models)
        self._meshes, self._n_objects = meshes_by_class, n_objects

    def get_frame(self, index):
        return morefusion.synthetic.make_cad_frame(self._meshes, seed=index, n_objects=self._n_objects)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cad-dir", help="YCB-Video model directory; default: the meshes under tests/golden/")
    ap.add_argument("--frame", type=int, default=0)
    ap.add_argument("--objects", type=int, default=3)
    args = ap.parse_args()
    if args.cad_dir:
        ycb = morefusion.datasets.YCBVideoModels(args.cad_dir)
        meshes = {c: tuple(ycb.get_cad(c)) for c in range(1, len(ycb.class_names))}
        models = morefusion.datasets.MeshModels(meshes)
    else:
        meshes = {}
        for class_id, name in ((2, "003_cracker_box"), (3, "004_sugar_box"), (9, "010_potted_meat_can")):
            d = np.load(os.path.join(ROOT, "tests", "golden", f"ycb_mesh_{name}.npz"))
            meshes[class_id] = (d["vertices"], d["faces"])
        models = morefusion.datasets.MeshModels(meshes)
    ds = CadFrames(models, meshes, args.objects)
    examples = ds.get_example(args.frame)
    for ex in examples:
        print(f"class {int(ex['class_id'])}: visibility {ex['visibility']:.3f}, pitch {ex['pitch']:.5f}, "
              f"grid_target {int((ex['grid_target'] > 0.5).sum())} voxels, grid_target_full "
              f"{int(ex['grid_target_full'].sum())}, others in its grid {int((ex['grid_nontarget_full'] > 0).sum())}")
    batch = dataset.concat_examples([morefusion.synthetic.transform_example(e) for e in examples])
    torch.manual_seed(0)
    model = Model(n_fg_class=21, with_occupancy=True, models=models).cuda().eval()
    keys = ("class_id", "rgb", "pcd", "quaternion_true", "translation_true", "pitch", "origin", "grid_nontarget_empty")
    with torch.no_grad():
        loss = model(**{k: cuda.to_gpu(batch[k]) for k in keys})
    print(f"{len(examples)} examples, loss {float(loss):.6f}")
    return examples, float(loss)


if __name__ == "__main__":
    main()
