#!/usr/bin/env python
"""ICC driver -- this repository's counterpart of the reference's
examples/ycb_video/pose_refinement/check_iterative_collision_check_link.py:14-79
(same argument marshalling, hyper-parameters and iteration count; no viewer).

Inputs: the three real fixture instances the reference ships (tests/golden/) plus
synthetic primitives; their SDF values are synthetic (the YCB SDFs are a download), or with
--cad-dir DIR the fixture objects' (points, sdf) come from YCBVideoModels(DIR).get_sdf (the CAD meshes'
solid points and signed distances, computed on the device).
  --mode step   : the reference's loop (loss.backward(); optimizer.update(); zerograds())
  --mode fused  : link.refine() -- the whole loop as one hipGraph on the device
  --until-converged : the loop of the reference's ROS node (collision_based_pose_refinement.py:178-207: at most 30
                  iterations, left once its LossObserver validates), decided on the device per scene
                  (link.refine_until_converged()), next to the fixed 30-iteration loop from the same start
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import morefusion_amd as morefusion  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["step", "fused"], default="fused")
    ap.add_argument("--objects", type=int, default=8)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--cad-dir", help="YCB-Video model directory (<NNN_name>/textured*.obj): the fixture objects' "
                    "points and SDF from the CAD meshes instead of the synthetic stand-in")
    ap.add_argument("--until-converged", action="store_true",
                    help="the ROS node's loop (<= 30 iterations, stops once the loss has converged) beside the fixed 30")
    args = ap.parse_args()

    gold = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")
    fixtures = [dict(np.load(os.path.join(gold, f"fixture_pose_refinement_0000000{i}.npz"))) for i in range(3)]
    data = morefusion.synthetic.make_icc_scene(args.objects, seed=0, fixtures=fixtures)
    if args.cad_dir:  # the scene's first objects are the fixtures, in order
        n_fix = min(len(fixtures), args.objects)
        ycb = morefusion.datasets.YCBVideoModels(args.cad_dir)
        for k, (p, d) in enumerate(ycb.get_sdf_batch([int(f["class_id"]) for f in fixtures[:n_fix]])):
            data["points"][k], data["sdf"][k] = p.astype(np.float32), d.astype(np.float32)
            print(f"object {k}: class {ycb.class_names[int(fixtures[k]['class_id'])]}, {len(p)} CAD points, "
                  f"sdf {d.min():.4f} .. {d.max():.4f}")

    to_gpu = lambda x: torch.as_tensor(np.ascontiguousarray(x)).cuda()  # noqa: E731
    points = [to_gpu(p) for p in data["points"]]
    sdf = [to_gpu(s) for s in data["sdf"]]
    pitch, origin = to_gpu(data["pitch"]), to_gpu(data["origin"])
    grid_target = to_gpu(data["grid_target"])
    grid_nontarget_empty = to_gpu(data["grid_nontarget_empty"])

    if args.until_converged:
        inputs = (points, sdf, pitch, origin, grid_target, grid_nontarget_empty)
        fixed = morefusion.contrib.IterativeCollisionCheckLink(data["transform_init"], sdf_offset=0.02).to_gpu()
        losses_f, _ = fixed.refine(*inputs, n_iter=30, return_history=True)
        link = morefusion.contrib.IterativeCollisionCheckLink(data["transform_init"], sdf_offset=0.02).to_gpu()
        n_steps, losses_c, _ = link.refine_until_converged(*inputs, sync=True, return_history=True)
        n = int(n_steps[0])
        T_f = morefusion.functions.transformation_matrix(fixed.quaternion, fixed.translation).detach()
        T_c = morefusion.functions.transformation_matrix(link.quaternion, link.translation).detach()
        print(f"scene 0: {n} steps until converged (of at most 30); last loss {float(losses_c[n - 1]):.5f}, "
              f"fixed 30 iterations: {float(losses_f[-1]):.5f}")
        # ADD of the converged pose against the fixed loop's, per object: mean distance of the model points
        for k, p in enumerate(points):
            a = p @ T_c[k, :3, :3].T + T_c[k, :3, 3]
            b = p @ T_f[k, :3, :3].T + T_f[k, :3, 3]
            print(f"  object {k}: ADD against the fixed 30-iteration pose {float((a - b).norm(dim=1).mean()) * 1e3:.3f} mm")
        return

    link = morefusion.contrib.IterativeCollisionCheckLink(data["transform_init"], sdf_offset=0.02)
    link.to_gpu()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    if args.mode == "step":
        optimizer = morefusion.optimizers.Adam(alpha=0.01)
        optimizer.setup(link)
        link.translation.update_rule.hyperparam.alpha *= 0.1
        losses = []
        for i in range(args.iters):
            loss = link(points, sdf, pitch, origin, grid_target, grid_nontarget_empty)
            loss.backward()
            optimizer.update()
            link.zerograds()
            losses.append(float(loss.detach()))
    else:
        losses, _ = link.refine(points, sdf, pitch, origin, grid_target, grid_nontarget_empty,
                                n_iter=args.iters, return_history=True)
        losses = losses.cpu().tolist()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    transform = morefusion.functions.transformation_matrix(link.quaternion, link.translation)
    print(f"{args.mode}: {args.objects} objects x {args.iters} iterations in {dt * 1e3:.1f} ms "
          f"(first call includes graph capture); loss {losses[0]:.4f} -> {losses[-1]:.4f}")
    print("refined transform[0]:\n", transform[0].detach().cpu().numpy())


if __name__ == "__main__":
    main()
