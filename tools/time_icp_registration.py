"""ICP registration batches on the device (contrib.icp_registration_batch, csrc/icpreg.hip): the three real
fixtures (one batch each) and 8- / 16-object synthetic batches (synthetic.make_icp_batch), REPS times after a
warm-up, wall time per batch with the extents readback included (CUDA events) and the iteration counts;
``--ref`` adds the mirror restatement's CPU time (tests/icpreg_ref.py) for the same problems.  Run under
``rocprofv3 --kernel-trace --stats`` for the kernel table (DESIGN.md "ICP registration")."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from morefusion_amd import synthetic  # noqa: E402
from morefusion_amd.contrib import icp_registration_batch  # noqa: E402


def cases():
    import icpreg_ref as R
    for i in range(3):
        d, c, t = R.fixture_inputs(os.path.join(ROOT, "tests", "golden", f"fixture_pose_refinement_0000000{i}.npz"))
        yield f"fixture_{i}", [d], [c], t[None]
    for n in (8, 16):
        d, c, t, _ = synthetic.make_icp_batch(n, seed=0, n_cad=3000)
        yield f"synthetic_{n}", d, c, t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--ref", action="store_true")
    args = ap.parse_args()
    rows = []
    for name, depth, cad, init in cases():
        depth_d = [torch.as_tensor(x).cuda() for x in depth]
        cad_d = [torch.as_tensor(x).cuda() for x in cad]
        init_d = torch.as_tensor(init).cuda()
        out = icp_registration_batch(depth_d, cad_d, init_d)  # warm-up
        torch.cuda.synchronize()
        times = []
        for _ in range(args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = icp_registration_batch(depth_d, cad_d, init_d)
            e1.record()
            torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1))
        row = dict(case=name, objects=len(depth), points=int(sum(len(x) for x in depth)),
                   n_iter=out[3].cpu().tolist(), ms_median=float(np.median(times)), ms_min=float(np.min(times)))
        if args.ref:
            import icpreg_ref as R
            t0 = time.perf_counter()
            for d, c, t in zip(depth, cad, init):
                R.register(d, c, t)
            row["ref_cpu_ms"] = 1e3 * (time.perf_counter() - t0)
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


if __name__ == "__main__":
    main()
