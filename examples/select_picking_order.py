#!/usr/bin/env python
"""Posed objects in -> which to pick first to reach a target, and where to grasp each: the reference's
``select_picking_order`` node (ros/src/morefusion_ros/nodes/select_picking_order.py) without ROS.

A table scene is posed by ``synthetic.make_cad_frame`` (the YCB meshes under tests/golden/, or ``--cad-dir``: a
YCB-Video model directory); ``contrib.SelectPickingOrder`` renders the objects together and each one alone in one
launch (csrc/render.hip), measures who hides whom and derives a grasp pose per object (csrc/pickorder.hip), and
``get_picking_order`` peels the occlusion graph until the target is free."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import morefusion_amd as morefusion  # noqa: E402

GOLDEN = {2: "003_cracker_box", 3: "004_sugar_box", 9: "010_potted_meat_can"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cad-dir", help="YCB-Video model directory; default: the meshes under tests/golden/")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--objects", type=int, default=6)
    ap.add_argument("--target", type=int, help="target class id; default: the class of the farthest object")
    ap.add_argument("--min-ratio", type=float, default=0.1)
    args = ap.parse_args()
    if args.cad_dir:
        ycb = morefusion.datasets.YCBVideoModels(args.cad_dir)
        meshes = {c: tuple(ycb.get_cad(c)) for c in range(1, len(ycb.class_names))}
    else:
        meshes = {}
        for c, name in GOLDEN.items():
            d = np.load(os.path.join(ROOT, "tests", "golden", f"ycb_mesh_{name}.npz"))
            meshes[c] = (d["vertices"], d["faces"])
    frame = morefusion.synthetic.make_cad_frame(meshes, seed=args.seed, n_objects=args.objects)
    H, W = frame["depth"].shape
    Ts = frame["Ts_cad2cam"].copy()
    Ts[:, 0, 3] *= 0.45  # the frame spreads the objects along the table: push them together so that they overlap
    target = int(frame["class_ids"][np.argmax(Ts[:, 2, 3])]) if args.target is None else args.target
    picker = morefusion.contrib.SelectPickingOrder(meshes, target_class_id=target, min_ratio=args.min_ratio)
    res = picker(frame["class_ids"], frame["instance_ids"], Ts, frame["K"], H, W)
    an = res["analysis"]
    print(f"{args.objects} objects at {H} x {W}, target class {target}")
    for k, (i, c) in enumerate(zip(frame["instance_ids"], frame["class_ids"])):
        hidden = {int(frame["instance_ids"][j]): round(float(an["ratio"][k, j]), 3)
                  for j in range(len(Ts)) if an["ratio"][k, j] > 0}
        print(f"  instance {i} (class {c}): {an['whole'][k]} px alone, {an['occluded_by'][k, k]} visible, "
              f"occluded by {hidden or 'nothing'}")
    print("edges (i is occluded by j: hidden pixels):", {k: v for k, v in sorted(res["edges"].items())})
    print("picking order:", res["order"])
    for i in res["order"]:
        t, q = res["translation"][i], res["quaternion"][i]
        print(f"  grasp instance {i}: translation ({t[0]:+.4f}, {t[1]:+.4f}, {t[2]:+.4f}) m, "
              f"quaternion wxyz ({q[0]:+.4f}, {q[1]:+.4f}, {q[2]:+.4f}, {q[3]:+.4f}) in the camera frame")


if __name__ == "__main__":
    main()
