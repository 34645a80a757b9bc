#!/usr/bin/env python
"""RGB-D frame in -> refined poses out: the callback of the reference's ROS node
(ros/src/morefusion_ros/nodes/singleview_3d_pose_estimation.py:113-256) without ROS:
instance crops (HIP, no host loop) -> grid placement -> Model.predict -> arg-max confidence
-> 4x4 transforms.  Synthetic frame, random weights unless ``--model snapshot.npz``.

``--occupancy``: the frame path with the scene's occupancy (base.py:28-46, 153-163): a frame with real
geometry (synthetic.make_occupancy_frame), full-frame back-projection uploaded to the device ->
MultiInstanceOctreeMapping.integrate_frame -> per-object grids at the network's origin / class pitch ->
Model.predict with the real grid_nontarget_empty -> ICC refinement (IccScenes) on grid_target /
grid_nontarget_empty.

``--icp``: the node's ICP refinement (singleview_3d_pose_estimation.py:236-262) on top of either path: the
arg-max pose's transformation_matrix as the init, every kept instance's valid crop points against a CAD
stand-in cloud (synthetic.make_primitive of the class pitch), objects below ``--confidence`` skipped through
``active`` -- one contrib.icp_registration_batch call, no host loop over objects."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import morefusion_amd as morefusion  # noqa: E402
from morefusion_amd.contrib.singleview_3d.models import Model  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", help="chainer .npz checkpoint of the reference")
    ap.add_argument("--occupancy", action="store_true",
                    help="map the frame's occupancy, feed it to the network and refine the poses with ICC")
    ap.add_argument("--icc-iters", type=int, default=30)
    ap.add_argument("--icp", action="store_true", help="refine the arg-max poses with ICPRegistration (batched)")
    ap.add_argument("--confidence", type=float, default=0.0, help="--icp: objects below this confidence are skipped")
    ap.add_argument("--cad-dir", help="YCB-Video model directory (<NNN_name>/textured*.obj): real CAD clouds for --icp "
                    "and real (points, sdf) for --occupancy's ICC in place of the primitive stand-ins")
    args = ap.parse_args()
    if args.occupancy:
        return main_occupancy(args)

    frame = morefusion.synthetic.make_rgbd_frame(0)
    class_of_instance = dict(zip(frame["instance_ids"].tolist(), [2, 5, 9, 12, 15, 16, 19, 21]))
    to_gpu = lambda x: torch.as_tensor(x).cuda()  # noqa: E731
    crops = morefusion.geometry.instance_crops(
        to_gpu(frame["rgb"]), to_gpu(frame["depth"]), frame["K"], to_gpu(frame["label"]),
        frame["instance_ids"], image_size=256, min_valid=50)
    keep = crops["keep"].cpu().numpy()  # the node's `continue` for inactive / tiny instances
    instance_ids = frame["instance_ids"][keep]
    class_id = torch.tensor([class_of_instance[i] for i in instance_ids.tolist()], dtype=torch.int32).cuda()
    rgb, pcd = crops["rgb"][crops["keep"]], crops["pcd"][crops["keep"]]

    torch.manual_seed(0)
    model = Model(n_fg_class=21, with_occupancy=True)
    if args.model:
        morefusion.serializers.load_npz(args.model, model)
    model = model.cuda().eval()
    grid_nontarget_empty = torch.zeros((len(instance_ids), 32, 32, 32), dtype=torch.bool, device="cuda")
    with torch.no_grad():  # pitch from the class table, origin = median - 15.5 pitch (model.py:195-207)
        quaternion, translation, confidence = model.predict(
            class_id=class_id, rgb=rgb, pcd=pcd, grid_nontarget_empty=grid_nontarget_empty)
    best = confidence.argmax(dim=1)
    ar = torch.arange(len(instance_ids), device=best.device)
    T = morefusion.functions.transformation_matrix(quaternion[ar, best], translation[ar, best])
    for ins, cls, t in zip(instance_ids, class_id.tolist(), T.cpu().numpy()):
        print(f"instance {ins} (class {cls}): translation {np.round(t[:3, 3], 4)}")
    if args.icp:
        return refine_icp(pcd, quaternion, translation, confidence, class_id, instance_ids, args.confidence,
                          cad_cloud=cad_from_dir(args.cad_dir) if args.cad_dir else cad_standin)


def main_occupancy(args):
    from morefusion_amd.contrib.singleview_3d.models.model import PitchTableModels

    frame = morefusion.synthetic.make_occupancy_frame(0)
    K = frame["K"]
    to_gpu = lambda x: torch.as_tensor(x).cuda()  # noqa: E731
    crops = morefusion.geometry.instance_crops(
        to_gpu(frame["rgb"]), to_gpu(frame["depth"]), K, to_gpu(frame["label"]),
        frame["instance_ids"], image_size=256, min_valid=50)
    keep = crops["keep"].cpu().numpy()
    instance_ids = frame["instance_ids"][keep]
    class_of_instance = dict(zip(frame["instance_ids"].tolist(), frame["class_ids"].tolist()))
    class_id = torch.tensor([class_of_instance[i] for i in instance_ids.tolist()], dtype=torch.int32).cuda()
    rgb, pcd = crops["rgb"][crops["keep"]], crops["pcd"][crops["keep"]]

    # the scene's occupancy: full-frame points (host back-projection, uploaded once) -> one map per instance
    models = PitchTableModels()
    pcd_full = morefusion.geometry.pointcloud_from_depth(frame["depth"], K[0, 0], K[1, 1], K[0, 2], K[1, 2])
    mapping = morefusion.contrib.MultiInstanceOctreeMapping()
    mapping.integrate_frame(to_gpu(pcd_full.astype(np.float32)), frame["label"], frame["instance_ids"],
                            frame["class_ids"], lambda c: models.get_voxel_pitch(32, c))
    # grids where the network places them: class pitch, origin = median of the crop's points - 15.5 pitch
    pitch = torch.tensor([models.get_voxel_pitch(32, int(c)) for c in class_id.tolist()],
                         dtype=torch.float32, device="cuda")
    origin = morefusion.geometry.grid_origin(pcd.float(), pitch, dim=32)
    grid_target, _, _, target_bool, grid_nontarget_empty = mapping.get_target_grids_batch(
        instance_ids, pitch, origin, network_inputs=True)

    torch.manual_seed(0)
    model = Model(n_fg_class=21, with_occupancy=True)
    if args.model:
        morefusion.serializers.load_npz(args.model, model)
    model = model.cuda().eval()
    with torch.no_grad():
        quaternion, translation, confidence = model.predict(
            class_id=class_id, rgb=rgb, pcd=pcd, pitch=pitch, origin=origin,
            grid_nontarget_empty=grid_nontarget_empty)
    best = confidence.argmax(dim=1)
    ar = torch.arange(len(instance_ids), device=best.device)
    q = quaternion[ar, best].float().contiguous()
    t = translation[ar, best].float().contiguous()

    # ICC on the mapped grids; stand-in CAD points / SDFs (solid primitives of the class pitch), or with --cad-dir the
    # CAD models' solid points and signed distances (YCBVideoModels.get_sdf)
    rs = np.random.RandomState(0)
    points, sdf = [], []
    if args.cad_dir:
        ycb = morefusion.datasets.YCBVideoModels(args.cad_dir)
        for p, d in ycb.get_sdf_batch(class_id.tolist()):
            points.append(to_gpu(p.astype(np.float32)))
            sdf.append(to_gpu(d.astype(np.float32)))
    for k, c in enumerate(class_id.tolist()[len(points):]):
        p, d = morefusion.synthetic.make_primitive("sphere" if k % 2 == 0 else "box", models.get_voxel_pitch(32, c), rs)
        points.append(to_gpu(p))
        sdf.append(to_gpu(d))
    scenes = morefusion.contrib.IccScenes([dict(points=points, sdf=sdf, pitch=pitch, origin=origin,
                                                grid_target=grid_target, grid_nontarget_empty=grid_nontarget_empty)],
                                         sdf_offset=0.02)
    adam_m = torch.zeros((len(instance_ids), 7), dtype=torch.float32, device="cuda")
    adam_v = torch.zeros_like(adam_m)
    losses = torch.empty((args.icc_iters, 1), dtype=torch.float32, device="cuda")
    scenes.refine(q, t, adam_m, adam_v, args.icc_iters, losses=losses)
    T = morefusion.functions.transformation_matrix(q, t)
    print(f"occupancy: grid_nontarget_empty {int(grid_nontarget_empty.sum())} voxels, "
          f"grid_target {int(target_bool.sum())} voxels over {len(instance_ids)} objects")
    print(f"ICC loss {float(losses[0, 0]):.6f} -> {float(losses[-1, 0]):.6f} in {args.icc_iters} iterations")
    for ins, cls, tr in zip(instance_ids, class_id.tolist(), T.cpu().numpy()):
        print(f"instance {ins} (class {cls}): translation {np.round(tr[:3, 3], 4)}")
    if args.icp:
        refine_icp(pcd, quaternion, translation, confidence, class_id, instance_ids, args.confidence,
                   cad_cloud=cad_from_dir(args.cad_dir) if args.cad_dir else cad_standin)
    return dict(grid_nontarget_empty=grid_nontarget_empty, losses=losses, transform=T)


def cad_standin(class_id):
    """A CAD stand-in cloud per class: the surface layer of a solid primitive of the class pitch."""
    from morefusion_amd.contrib.singleview_3d.models.model import PitchTableModels
    pitch = PitchTableModels().get_voxel_pitch(32, int(class_id))
    p, d = morefusion.synthetic.make_primitive("box" if int(class_id) % 2 else "sphere", pitch,
                                               np.random.RandomState(int(class_id)))
    return p[d < pitch]


def cad_from_dir(root):
    """--cad-dir: the class's points.xyz when present, else its solid points (YCBVideoModels.get_sdf)."""
    ycb = morefusion.datasets.YCBVideoModels(root)

    def cad(class_id):
        if ycb.get_pcd_file(class_id).exists():
            return ycb.get_pcd(class_id)
        return ycb.get_sdf(class_id)[0]
    return cad


def refine_icp(pcd, quaternion, translation, confidence, class_id, instance_ids, threshold, iteration=100,
               cad_cloud=None):
    """The node's ICP step for every kept instance in one batch: arg-max pose -> transformation_matrix (init) ->
    icp_registration_batch(crop points [n, S, S, 3] with NaN holes, CAD clouds (``cad_cloud(class_id)``, default the
    stand-ins), active = confidence >= threshold)."""
    cad_cloud = cad_cloud or cad_standin
    best = confidence.argmax(dim=1)
    ar = torch.arange(len(instance_ids), device=best.device)
    T = morefusion.functions.transformation_matrix(quaternion[ar, best], translation[ar, best])
    conf = confidence[ar, best]
    classes = class_id.tolist()
    transform, fitness, rmse, n_iter, hist = morefusion.contrib.icp_registration_batch(
        pcd, [cad_cloud(c) for c in classes], T.double(), iteration=iteration, voxel_size=0.01,
        active=conf >= threshold, return_history=True, cad_keys=classes)
    for ins, c, f, r, n, ok in zip(instance_ids, conf.tolist(), fitness.tolist(), rmse.tolist(), n_iter.tolist(),
                                   (conf >= threshold).tolist()):
        state = f"fitness {f:.4f} inlier_rmse {r:.6f} iterations {n}" if ok else "skipped"
        print(f"icp instance {ins} (confidence {c:.3f}): {state}")
    return dict(init=T, transform=transform, fitness=fitness, inlier_rmse=rmse, n_iter=n_iter, history=hist)


if __name__ == "__main__":
    main()
