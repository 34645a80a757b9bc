"""Time mf_camtrack_prepare and mf_camtrack_align at 480 x 640 (3 levels, iterations 10 / 5 / 4) for B = 1 and 8 with
device events: 50 calls per window, the smallest and the largest of 5 windows after warm-up, one JSON line (DESIGN.md
"Camera tracking").

    python tools/time_camtrack.py [--out timing.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from morefusion_amd import synthetic  # noqa: E402
from morefusion_amd.contrib import camera_tracking as CT  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", help="also write the JSON line to this file")
args = ap.parse_args()
assert torch.cuda.is_available(), "needs the MI355X"
frames = synthetic.make_tracking_sequence(0, 2)
K = frames[0]["K"]
out = {}
for B in (1, 8):
    cur = torch.as_tensor(np.stack([frames[1]["depth"]] * B)).cuda()
    ref = torch.as_tensor(np.stack([frames[0]["depth"]] * B)).cuda()
    T = torch.as_tensor(np.stack([np.eye(4)] * B)).cuda()
    intr = CT._intrinsics(K)
    pc, pr = (CT.DepthPyramid(B, 480, 640, 3, intr, "cuda") for _ in range(2))
    al = CT._Aligner(B, 480, 640, 3, intr, (10, 5, 4), 0.1, np.cos(np.radians(20.0)), 100, "cuda")

    def timed(fn, reps):
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ts = []
        for _ in range(5):
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1) / reps)
        return min(ts), max(ts)

    pr.fill(ref, 0.05)
    out[f"B{B}_prepare_ms"] = timed(lambda: pc.fill(cur, 0.05), 50)
    out[f"B{B}_align_19it_ms"] = timed(lambda: al.run(pc, pr, T, T), 50)
    out[f"B{B}_status"] = al.status.cpu().tolist()
print(json.dumps(out))
if args.out:
    with open(args.out, "w") as fh:
        json.dump(out, fh)
