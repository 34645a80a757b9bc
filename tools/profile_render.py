#!/usr/bin/env python
"""Event timings of the render stages (csrc/render.hip): medians of 20 launches after warm-up.
Case A: 8 YCB-sized objects, a table and a wall in one 480 x 640 composite.  Case B: 21 single-object renders,
one 480 x 640 image each (what get_example asks for on a full frame).  Prints CSV rows
case,stage,median_us,min_us for profiles/render_kernel_table.csv."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import morefusion_amd as mf  # noqa: E402
from morefusion_amd.geometry.render import RenderPlan  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")


def meshes():
    out = []
    for name in ("003_cracker_box", "004_sugar_box", "010_potted_meat_can"):
        d = np.load(os.path.join(GOLDEN, f"ycb_mesh_{name}.npz"))
        out.append((d["vertices"], d["faces"]))
    return out


def time_stage(fn, before=None, n=20, warm=5):
    ts = []
    for k in range(warm + n):
        if before:
            before()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        if k >= warm:
            ts.append(a.elapsed_time(b) * 1e3)
    return float(np.median(ts)), float(np.min(ts))


def main():
    H, W = 480, 640
    K = np.array([[619.4, 0, 319.7], [0, 618.9, 240.7], [0, 0, 1]])
    ycb = meshes()
    rs = np.random.RandomState(0)
    quad = mf.synthetic.quad_mesh
    wall = quad((-3, -3, 1.4), (3, -3, 1.4), (3, 3, 1.4), (-3, 3, 1.4))
    table = quad((-1.5, 0.2, 0.2), (1.5, 0.2, 0.2), (1.5, 0.2, 1.4), (-1.5, 0.2, 1.4))

    def pose(i, n):
        T = np.eye(4)
        T[:3, :3] = mf.synthetic.random_rotation(rs)
        T[:3, 3] = (-0.35 + 0.7 * (i + 0.5) / n, 0.05, rs.uniform(0.6, 0.9))
        return T
    cases = {
        "composite8": RenderPlan([wall, table] + ycb, np.stack([np.eye(4), np.eye(4)] + [pose(i, 8) for i in range(8)]),
                                 K, H, W, mesh_index=[0, 1] + [2 + i % 3 for i in range(8)]),
        "single21": RenderPlan(ycb, np.stack([pose(i % 7, 7) for i in range(21)]), K, H, W,
                               targets=list(range(21)), mesh_index=[i % 3 for i in range(21)]),
    }
    print("case,stage,median_us,min_us")
    for name, plan in cases.items():
        plan.run()
        torch.cuda.synchronize()
        rows = [("setup", plan.setup, None), ("raster", plan.raster, plan.setup), ("resolve", plan.resolve, None),
                ("all", plan.run, None)]
        for stage, fn, before in rows:
            med, lo = time_stage(fn, before)
            print(f"{name},{stage},{med:.1f},{lo:.1f}")
        print(f"# {name}: {plan.total} face records, {plan.n_targets} x {H} x {W} px, "
              f"covered {int(plan.out['count'].sum())} px", flush=True)


if __name__ == "__main__":
    main()
