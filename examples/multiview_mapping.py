"""Multi-view object mapping: N synthetic RGB-D frames of one scene from a moving camera, the detector's instance ids
shuffled in every frame -> InstanceTracker (render the maps, match the detections: stable ids) ->
integrate_tracked_frame (one occupancy map per stable id) -> target grids -> Model.predict -> ObjectMapping (an
object is spawned once three of its poses agree).  Prints the id table of every frame.

    python examples/multiview_mapping.py [--frames 3] [--model <chainer .npz checkpoint>]
                                       [--track-camera | --track-model [--save-mesh PATH] [--skip-empty] [--color]]

--track-camera: the sensor pose is CameraTracker.track(depth) (dense depth alignment, frame to frame, anchored at frame
0's pose) instead of the sequence's ground truth; its error against the ground truth is printed per frame.
--track-model: the same through ModelTracker: every frame is aligned to a ray-cast of the TSDF volume that the earlier
frames were fused into (1 cm voxels over the scene), frame to model instead of frame to frame.
--skip-empty (with --track-model): ModelTracker takes its reference from TsdfVolume.render, the ray-cast that skips free
and unseen space through a block summary of the volume (the same bytes, so the same poses).
--save-mesh PATH (with --track-model): after the last frame the fused model is written as a Wavefront OBJ
(TsdfVolume.extract_mesh, geometry.save_obj).
--color (with --track-model): the volume is built with colors=True and ModelTracker.track(depth, color=rgb) fuses every
frame's RGB image next to its depth; with --save-mesh the OBJ carries a colour per vertex (``v x y z r g b``).
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import morefusion_amd as morefusion  # noqa: E402
from morefusion_amd.contrib.instance_tracking import transform_points  # noqa: E402
from morefusion_amd.contrib.singleview_3d.models import Model  # noqa: E402
from morefusion_amd.contrib.singleview_3d.models.model import PitchTableModels  # noqa: E402

# the synthetic objects are 30 .. 100 pixels across: the reference's vetoes (40 / 80 / 60) scaled to them
THRESHOLDS = dict(min_mask=20, min_bbox=30, min_side=24)
# --track-model: a 1 cm volume over the synthetic scene (x -0.8 .. 0.8, y -0.62 .. 0.3, z 0.3 .. 1.5)
MODEL_VOLUME = dict(dims=(161, 93, 121), pitch=0.01, origin=(-0.8, -0.62, 0.3))


def track_camera(camera, depth, T_true, k, **fused):
    """CameraTracker's (or ModelTracker's) pose of the frame, and its error against the ground truth on stdout."""
    T = camera.track(depth, **fused).cpu().numpy()
    D = np.linalg.inv(T_true) @ T
    angle = np.degrees(np.arccos(np.clip((np.trace(D[:3, :3]) - 1) / 2, -1, 1)))
    state = "" if k == 0 else (" LOST" if camera.lost else f" ({int(camera.stats[-1, 0])} pairs)")
    print(f"frame {k}: tracked camera off by {np.linalg.norm(T[:3, 3] - T_true[:3, 3]) * 1e3:.3f} mm, "
          f"{angle:.4f} deg{state}")
    return T


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=3)
    ap.add_argument("--model", help="chainer .npz checkpoint of the reference")
    ap.add_argument("--track-camera", action="store_true", help="estimate the sensor pose from the depth images")
    ap.add_argument("--track-model", action="store_true",
                    help="estimate the sensor pose by aligning every frame to the fused TSDF model")
    ap.add_argument("--save-mesh", metavar="PATH", help="with --track-model: write the fused model as an OBJ")
    ap.add_argument("--skip-empty", action="store_true",
                    help="with --track-model: render the model with empty-space skipping (TsdfVolume.render)")
    ap.add_argument("--color", action="store_true",
                    help="with --track-model: fuse the frames' RGB into the model; --save-mesh writes vertex colours")
    args = ap.parse_args()
    if args.track_camera and args.track_model:
        ap.error("--track-camera or --track-model, not both")
    if args.save_mesh and not args.track_model:
        ap.error("--save-mesh needs --track-model")
    if args.skip_empty and not args.track_model:
        ap.error("--skip-empty needs --track-model")
    if args.color and not args.track_model:
        ap.error("--color needs --track-model")
    frames = morefusion.synthetic.make_tracking_sequence(0, args.frames)
    models = PitchTableModels()
    pitch_of = lambda c: models.get_voxel_pitch(32, int(c))  # noqa: E731
    to_gpu = lambda x: torch.as_tensor(x).cuda()  # noqa: E731
    rs = np.random.RandomState(0)
    cad = {}  # stand-in model clouds for the voter: a sphere / a box of the class's size

    def points_of(c):
        if c not in cad:
            cad[c] = morefusion.synthetic.make_primitive("sphere" if c % 2 else "box", pitch_of(c), rs)[0]
        return cad[c]

    torch.manual_seed(0)
    model = Model(n_fg_class=21, with_occupancy=True)
    if args.model:
        morefusion.serializers.load_npz(args.model, model)
    model = model.cuda().eval()
    mapping = morefusion.contrib.MultiInstanceOctreeMapping()
    tracker = morefusion.contrib.InstanceTracker(mapping, thresholds=THRESHOLDS)
    voter = morefusion.contrib.ObjectMapping(points_of, lambda c: c in morefusion.synthetic.CLASS_IDS_SYMMETRIC)
    ids_of_object = {}
    camera = None
    if args.track_camera:
        height, width = frames[0]["depth"].shape
        camera = morefusion.contrib.CameraTracker(frames[0]["K"], height, width, T_first=frames[0]["T_sensor_to_map"])
    if args.track_model:
        height, width = frames[0]["depth"].shape
        camera = morefusion.contrib.ModelTracker(frames[0]["K"], height, width,
                                                 morefusion.contrib.TsdfVolume(colors=args.color, **MODEL_VOLUME),
                                                 T_first=frames[0]["T_sensor_to_map"], skip_empty=args.skip_empty)
    for k, f in enumerate(frames):
        K, T = f["K"], f["T_sensor_to_map"]
        if camera is not None:
            T = track_camera(camera, to_gpu(f["depth"]), T, k, **(dict(color=to_gpu(f["rgb"])) if args.color else {}))
        pcd = morefusion.geometry.pointcloud_from_depth(f["depth"], K[0, 0], K[1, 1], K[0, 2], K[1, 2])
        tracked, merged, class_of, _ = tracker.track(to_gpu(pcd.astype(np.float32)), to_gpu(f["label_detected"]),
                                                     f["class_ids_by_detection"], K, T)
        mapping.integrate_tracked_frame(tracker.pts_map, tracked, class_of, pitch_of, origin=T[:3, 3])
        table = {d: int(t) for d, t in zip(tracker.last["det_ids"], tracker.last["remap_host"][:-1])}
        print(f"frame {k}: ids {{{', '.join(f'{d}->{t}' for d, t in table.items())}}}")
        for d, t in table.items():
            if t >= 0:
                ids_of_object.setdefault(f["object_of_detection"][d], set()).add(t)
        # the pose stage works on the tracked label: crops -> map-frame points -> the map's grids -> the network
        ids = np.array(sorted(t for t in set(table.values()) if t >= 0), np.int32)
        crops = morefusion.geometry.instance_crops(to_gpu(f["rgb"]), to_gpu(f["depth"]), K, tracked, ids,
                                                   image_size=256, min_valid=50)
        keep = crops["keep"].cpu().numpy()
        ids = ids[keep]
        if len(ids) == 0:
            continue
        rgb, crop_pcd = crops["rgb"][crops["keep"]], crops["pcd"][crops["keep"]]
        crop_pcd = transform_points(crop_pcd, T).reshape(crop_pcd.shape)
        class_id = torch.tensor([class_of[int(i)] for i in ids], dtype=torch.int32).cuda()
        pitch = torch.tensor([pitch_of(c) for c in class_id.tolist()], dtype=torch.float32, device="cuda")
        origin = morefusion.geometry.grid_origin(crop_pcd.float(), pitch, dim=32)
        grid_nontarget_empty = mapping.get_target_grids_batch(ids, pitch, origin, network_inputs=True)[4]
        with torch.no_grad():
            quaternion, translation, confidence = model.predict(
                class_id=class_id, rgb=rgb, pcd=crop_pcd, pitch=pitch, origin=origin,
                grid_nontarget_empty=grid_nontarget_empty)
        best = confidence.argmax(dim=1)
        ar = torch.arange(len(ids), device=best.device)
        T_cad2map = morefusion.functions.transformation_matrix(quaternion[ar, best], translation[ar, best]).cpu().numpy()
        for i, c, pose in zip(ids.tolist(), class_id.tolist(), T_cad2map):
            voter.append_pose(i, c, pose)
        print(f"frame {k}: {len(ids)} poses, spawned objects {voter.validate()}")
    if args.save_mesh:
        vertices, faces, *colors = camera.volume.extract_mesh(colors=args.color)
        morefusion.geometry.save_obj(args.save_mesh, vertices, faces, *colors)
        coloured = f", {int((colors[0][:, 3] == 255).sum())} of them coloured" if args.color else ""
        print(f"fused model: {len(vertices)} vertices{coloured}, {len(faces)} faces -> {args.save_mesh}")
    stable = sum(len(t) == 1 for t in ids_of_object.values())
    print(f"stable ids: {stable} of {len(ids_of_object)} objects")


if __name__ == "__main__":
    main()
