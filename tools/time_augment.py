#!/usr/bin/env python
"""Time datasets.augment_rgbd and its three stages at n = 16, 256 x 256 on the GPU: medians of 20 launches after
warm-up, by events; for context the NumPy mirror (tests/augment_ref.py) on the same inputs, once.  Writes
profiles/augment_rgbd.json (or the path given as the first argument)."""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import morefusion_amd as mf  # noqa: E402
from morefusion_amd.datasets import augmentation as A  # noqa: E402


def median_ms(fn, reps=20, warmup=5):
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times))


def main():
    import augment_cases as C
    import augment_ref as R
    n, S = 16, 256
    rgb_h, pcd_h = C.crops("cuda", S, n)
    rgb, pcd = torch.from_numpy(rgb_h).cuda(), torch.from_numpy(pcd_h).cuda()
    rs = np.random.RandomState(0)
    params = A.draw_params(n, rs)
    prm = A._table(params, n, rgb.device)
    ws = A._workspace(n, S, rgb.device)
    m = A.augment_mask(rgb, pcd, prm, 1, workspace=ws)
    out = {"n": n, "S": S, "reps": 20, "unit": "ms (median)", "pcd_dtype": "float64",
           "augment_rgbd": median_ms(lambda: mf.datasets.augment_rgbd(rgb, pcd, 0)),
           "mask_stage": median_ms(lambda: A.augment_mask(rgb, pcd, prm, 1, workspace=ws)),
           "colour_stage": median_ms(lambda: A.augment_rgb(m["rgb"], prm, workspace=ws)),
           "point_stage": median_ms(lambda: A.augment_pcd(m["pcd"], prm, 1))}
    t0 = time.perf_counter()
    R.augment_rgbd(rgb_h, pcd_h, params, 1)
    out["numpy_mirror_once"] = (time.perf_counter() - t0) * 1e3
    print(json.dumps(out))
    dst = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "augment_rgbd.json")
    with open(dst, "w") as f:
        json.dump(out, f, indent=1)

if __name__ == "__main__":
    main()
