"""The online path of the reference's ROS nodes on one synthetic sequence: RGB-D frames from a moving camera ->
InstanceTracker (stable ids) -> OctomapServer.insert_scan (one shared free set in the background map, hit-only instance
maps) -> OctomapServer.publish_grids (the grids of every instance in the SENSOR frame) -> Model.predict with the
server's pitch, origin and grid_nontarget_empty -> IterativeCollisionCheckLink.refine_until_converged on the float
grid_target / grid_noentry, as collision_based_pose_refinement.py passes them.  The network is untrained unless
--model is given and the CAD clouds / signed distances are stand-ins, as in the other examples; the poses are printed
before and after the refinement.

    python examples/online_pose_refinement.py [--frames 3] [--model <chainer .npz checkpoint>] [--render-service]
                                              [--track-camera | --track-model [--save-mesh PATH]
                                               [--grids-from-model] [--skip-empty] [--color]]

--render-service: the tracker matches against the reference's render-service route (use_render_service,
OctomapServer.cpp:126-135) -- OctomapServer.grids_in_map_frame meshed and rasterised (contrib.render_voxel_grids) --
instead of the per-pixel ray-cast.
--track-camera: the sensor pose handed to the tracker and the server is CameraTracker.track(depth) (dense depth
alignment, frame to frame, anchored at frame 0's pose) instead of the sequence's ground truth; its error against the
ground truth is printed per frame.
--track-model: the same through ModelTracker: every frame is aligned to a ray-cast of the TSDF volume that the earlier
frames were fused into (1 cm voxels over the scene), frame to model instead of frame to frame.
--grids-from-model (with --track-model): the volume is an InstanceTsdfVolume, ModelTracker.track(depth, label) fuses the
tracked labels of every frame next to its depth, and the grids of the pose stage are InstanceTsdfVolume.publish_grids
(the fused model, the same dict) instead of OctomapServer.publish_grids.  The server is still filled: the instance
tracker matches its detections against the server's maps.
--skip-empty (with --track-model): ModelTracker takes its reference from TsdfVolume.render, the ray-cast that skips free
and unseen space through a block summary of the volume (the same bytes, so the same poses); with --grids-from-model the
instance ids the fused model shows from the frame's pose are printed too, depth and labels from that one render launch.
--save-mesh PATH (with --track-model): after the last frame the fused model is written as a Wavefront OBJ
(TsdfVolume.extract_mesh, geometry.save_obj).
--color (with --track-model): the volume is built with colors=True and ModelTracker.track(depth, color=rgb) fuses every
frame's RGB image next to its depth (and labels); with --save-mesh the OBJ carries a colour per vertex.
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import morefusion_amd as morefusion  # noqa: E402
from morefusion_amd.contrib.singleview_3d.models import Model  # noqa: E402
from morefusion_amd.contrib.singleview_3d.models.model import PitchTableModels  # noqa: E402

# the synthetic objects are 30 .. 100 pixels across: the reference's vetoes (40 / 80 / 60) scaled to them
THRESHOLDS = dict(min_mask=20, min_bbox=30, min_side=24)
# --track-model: a 1 cm volume over the synthetic scene (x -0.8 .. 0.8, y -0.62 .. 0.3, z 0.3 .. 1.5) in the ground frame
MODEL_VOLUME = dict(dims=(161, 121, 93), pitch=0.01, origin=(-0.8, 0.3, -0.1))
# the synthetic scene has its table top at y = 0.2 with y pointing down: the server's map frame has it at z = 0, z up
TO_GROUND = np.array([[1, 0, 0, 0], [0, 0, 1, 0], [0, -1, 0, 0.2], [0, 0, 0, 1]], np.float64)


def track_camera(camera, depth, T_true, k, **labels):
    """CameraTracker's (or ModelTracker's) pose of the frame, and its error against the ground truth on stdout."""
    T = camera.track(depth, **labels).cpu().numpy()
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
    ap.add_argument("--render-service", action="store_true", help="render the maps as meshes (render_voxel_grids.py)")
    ap.add_argument("--track-camera", action="store_true", help="estimate the sensor pose from the depth images")
    ap.add_argument("--track-model", action="store_true",
                    help="estimate the sensor pose by aligning every frame to the fused TSDF model")
    ap.add_argument("--save-mesh", metavar="PATH", help="with --track-model: write the fused model as an OBJ")
    ap.add_argument("--grids-from-model", action="store_true",
                    help="with --track-model: fuse the tracked labels into the TSDF volume and take the pose stage's "
                         "grids from it (InstanceTsdfVolume.publish_grids) instead of from the map server")
    ap.add_argument("--skip-empty", action="store_true",
                    help="with --track-model: render the model with empty-space skipping (TsdfVolume.render)")
    ap.add_argument("--color", action="store_true",
                    help="with --track-model: fuse the frames' RGB into the model; --save-mesh writes vertex colours")
    args = ap.parse_args()
    if args.track_camera and args.track_model:
        ap.error("--track-camera or --track-model, not both")
    if args.save_mesh and not args.track_model:
        ap.error("--save-mesh needs --track-model")
    if args.grids_from_model and not args.track_model:
        ap.error("--grids-from-model needs --track-model")
    if args.skip_empty and not args.track_model:
        ap.error("--skip-empty needs --track-model")
    if args.color and not args.track_model:
        ap.error("--color needs --track-model")
    frames = morefusion.synthetic.make_tracking_sequence(0, args.frames)
    models = PitchTableModels()
    pitch_of = lambda c: models.get_voxel_pitch(32, int(c))  # noqa: E731
    to_gpu = lambda x: torch.as_tensor(x).cuda()  # noqa: E731
    rs = np.random.RandomState(0)
    cad = {}  # stand-in model clouds and signed distances: a sphere / a box of the class's size

    def cad_of(c):
        if c not in cad:
            points = morefusion.synthetic.make_primitive("sphere" if c % 2 else "box", pitch_of(c), rs)[0]
            cad[c] = (points.astype(np.float32), morefusion.synthetic.synthetic_sdf(points).astype(np.float32))
        return cad[c]

    torch.manual_seed(0)
    model = Model(n_fg_class=21, with_occupancy=True)
    if args.model:
        morefusion.serializers.load_npz(args.model, model)
    model = model.cuda().eval()
    server = morefusion.contrib.OctomapServer()
    if args.render_service:
        tracker = morefusion.contrib.InstanceTracker(server.mapping, thresholds=THRESHOLDS, render="mesh", server=server)
    else:
        tracker = morefusion.contrib.InstanceTracker(server.mapping, thresholds=THRESHOLDS)
    camera = None
    if args.track_camera:
        height, width = frames[0]["depth"].shape
        camera = morefusion.contrib.CameraTracker(frames[0]["K"], height, width,
                                                  T_first=TO_GROUND @ frames[0]["T_sensor_to_map"])
    if args.track_model:
        height, width = frames[0]["depth"].shape
        volume = (morefusion.contrib.InstanceTsdfVolume if args.grids_from_model else morefusion.contrib.TsdfVolume)
        camera = morefusion.contrib.ModelTracker(frames[0]["K"], height, width,
                                                 volume(colors=args.color, **MODEL_VOLUME),
                                                 T_first=TO_GROUND @ frames[0]["T_sensor_to_map"],
                                                 skip_empty=args.skip_empty)
    classes = {}  # instance id -> class id, over the frames so far
    for k, f in enumerate(frames):
        K, T = f["K"], TO_GROUND @ f["T_sensor_to_map"]
        pcd = morefusion.geometry.pointcloud_from_depth(f["depth"], K[0, 0], K[1, 1], K[0, 2], K[1, 2])
        fused = dict(color=to_gpu(f["rgb"])) if args.color else {}

        def track_instances(T):
            return tracker.track(to_gpu(pcd.astype(np.float32)), to_gpu(f["label_detected"]),
                                 f["class_ids_by_detection"], K, T,
                                 depth=to_gpu(f["depth"]) if args.render_service else None)

        if args.grids_from_model:
            found = []  # the labels need the frame's pose: ModelTracker asks for them once it has aligned the frame

            def label_at(T_device):
                found.append(track_instances(T_device.cpu().numpy()))
                return found[0][0]

            T = track_camera(camera, to_gpu(f["depth"]), T, k, label=label_at, **fused)
            tracked, _, class_of, _ = found[0]
        else:
            if camera is not None:
                T = track_camera(camera, to_gpu(f["depth"]), T, k, **fused)
            tracked, _, class_of, _ = track_instances(T)
        classes.update({int(i): int(c) for i, c in class_of.items()})
        server.insert_scan(tracker.pts_map.reshape(pcd.shape), tracked, class_of, pitch_of, origin=T[:3, 3])
        if args.grids_from_model:
            ids = sorted(classes)
            grids = camera.volume.publish_grids(T, ids, pitch={i: pitch_of(classes[i]) for i in ids}, class_ids=classes,
                                                ground_z=0.0 if server.ground_as_noentry else None,
                                                free_as_noentry=server.free_as_noentry)
            if args.skip_empty:  # depth and labels of the model from one launch
                _, model_label = camera.volume.render(K, T, height, width, labels=True)
                print(f"frame {k}: the model's render shows ids {sorted(set(model_label.unique().tolist()) - {0, -1})}")
        else:
            grids = server.publish_grids(T)
        source = "model" if args.grids_from_model else tracker.render
        print(f"frame {k} ({source}): maps {server.mapping.instance_ids}, published {grids['instance_ids']}")
    if args.save_mesh:
        vertices, faces, *colors = camera.volume.extract_mesh(colors=args.color)
        morefusion.geometry.save_obj(args.save_mesh, vertices, faces, *colors)
        coloured = f", {int((colors[0][:, 3] == 255).sum())} of them coloured" if args.color else ""
        print(f"fused model: {len(vertices)} vertices{coloured}, {len(faces)} faces -> {args.save_mesh}")
    # the pose stage of the last frame, in the sensor frame: crops -> the server's grids -> the network
    published = grids["instance_ids"]
    crops = morefusion.geometry.instance_crops(to_gpu(f["rgb"]), to_gpu(f["depth"]), K, tracked,
                                               np.array(published, np.int32), image_size=256, min_valid=50)
    keep = crops["keep"]
    if int(keep.sum()) == 0:
        print("no instance with enough valid pixels in the last frame")
        return
    ids = [i for i, ok in zip(published, keep.cpu().tolist()) if ok]
    class_id = torch.tensor(grids["class_ids"], dtype=torch.int32).cuda()[keep]
    pitch, origin = grids["pitch"][keep], grids["origin"][keep].float()
    with torch.no_grad():
        quaternion, translation, confidence = model.predict(
            class_id=class_id, rgb=crops["rgb"][keep], pcd=crops["pcd"][keep], pitch=pitch, origin=origin,
            grid_nontarget_empty=grids["grid_nontarget_empty"][keep])
    best = confidence.argmax(dim=1)
    ar = torch.arange(len(ids), device=best.device)
    T_init = morefusion.functions.transformation_matrix(quaternion[ar, best], translation[ar, best]).cpu().numpy()
    # collision_based_pose_refinement.py:86-98: the float grids as the server publishes them
    points = [to_gpu(cad_of(c)[0]) for c in class_id.tolist()]
    sdf = [to_gpu(cad_of(c)[1]) for c in class_id.tolist()]
    link = morefusion.contrib.IterativeCollisionCheckLink(T_init, sdf_offset=0.01).to_gpu()
    n_steps = link.refine_until_converged(points, sdf, pitch, origin, grids["grid_target"][keep],
                                          grids["grid_noentry"][keep], sync=True)
    T_refined = morefusion.functions.transformation_matrix(link.quaternion, link.translation).detach().cpu().numpy()
    print(f"refined {len(ids)} objects in {int(n_steps[0])} steps (of at most 30)")
    for i, a, b in zip(ids, T_init, T_refined):
        q0, q1 = morefusion.geometry.quaternion_from_matrix(a), morefusion.geometry.quaternion_from_matrix(b)
        print(f"instance {i}: before t = {np.round(a[:3, 3], 4).tolist()} q = {np.round(q0, 4).tolist()}, "
              f"after t = {np.round(b[:3, 3], 4).tolist()} q = {np.round(q1, 4).tolist()}")


if __name__ == "__main__":
    main()
