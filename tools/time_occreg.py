"""Time 100 iterations of OccupancyRegistration: the host loop (``OccupancyRegistration.register``, one object after
the other) against ONE ``contrib.occupancy_registration_batch`` call, for B = 1 and 8 objects on 16^3 grids with 300
points and 32^3 grids with 1000 points.  Every configuration runs in a fresh process: 10 warm-up calls, then the
median of 30, each timed with a pair of events on the current stream, the host waiting on the closing event.
``kernel_ms_per_iteration``: the batch call's median / 100 -- the call is one ``mf_occreg_refine`` launch plus a few
small tensor operations, so this bounds the kernel's time per iteration from above.

    python tools/time_occreg.py [--out profiles/occreg_timing.json]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ITER, WARMUP, REPS = 100, 10, 30
CONFIGS = [(dim, P, B) for dim, P in ((16, 300), (32, 1000)) for B in (1, 8)]


def objects(dim, P, B, seed=0):
    import numpy as np
    rs = np.random.RandomState(seed)
    pitch, out = 0.01, []
    for _ in range(B):
        origin = np.full(3, -0.5 * pitch * dim, np.float32)
        occ = np.zeros((dim,) * 3, np.float32)
        lo, hi = dim // 4, dim - dim // 4
        occ[lo:hi, lo:hi, lo:hi] = 1  # a solid block; free space around it
        vox = rs.uniform(lo, hi - 1, (P, 3))
        T = np.eye(4, dtype=np.float32)
        T[:3, 3] = rs.uniform(-pitch, pitch, 3)
        out.append(dict(points=(origin + pitch * vox).astype(np.float32), grid=np.stack([occ, 1 - occ]), pitch=pitch,
                        origin=origin, T=T))
    return out


def timed(fn):
    import numpy as np
    import torch
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(np.min(ms)), float(np.max(ms))


def child(mode, dim, P, B):
    import numpy as np
    import torch

    import morefusion_amd as mf
    objs = objects(dim, P, B)
    res = dict(mode=mode, dim=dim, points=P, objects=B, iterations=ITER)
    if mode == "host":
        dev = [dict(o, points=torch.as_tensor(o["points"]).cuda(), grid=torch.as_tensor(o["grid"]).cuda()) for o in objs]

        def run():
            for o in dev:
                mf.contrib.OccupancyRegistration(o["points"], o["grid"], pitch=o["pitch"], origin=tuple(o["origin"]),
                                                 threshold=2, transform_init=o["T"], alpha=0.01).register(ITER)
        med, lo, hi = timed(run)
    else:
        kw = dict(points_source=[torch.as_tensor(o["points"]).cuda() for o in objs],
                  grids_target=torch.as_tensor(np.stack([o["grid"] for o in objs])).cuda(),
                  pitch=[o["pitch"] for o in objs], origin=np.stack([o["origin"] for o in objs]), threshold=2,
                  transforms_init=np.stack([o["T"] for o in objs]), iteration=ITER, alpha=0.01)
        med, lo, hi = timed(lambda: mf.contrib.occupancy_registration_batch(**kw))
        res["kernel_ms_per_iteration"] = med / ITER  # the call is ONE launch (+ a few small tensor ops): an upper bound
    res.update(median_ms=med, min_ms=lo, max_ms=hi, per_object_ms=med / B)
    print("RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "occreg_timing.json"))
    ap.add_argument("--child", nargs=4)
    args = ap.parse_args()
    if args.child:
        return child(args.child[0], *(int(x) for x in args.child[1:]))
    rows = []
    for dim, P, B in CONFIGS:
        for mode in ("host", "batch"):
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", mode, str(dim), str(P), str(B)],
                               capture_output=True, text=True, timeout=300)
            if p.returncode != 0:
                sys.stderr.write(p.stdout + p.stderr)
                raise SystemExit(f"{mode} {dim} {P} {B}: exit {p.returncode}")  # nothing more is started
            row = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
            print(row, flush=True)
            rows.append(row)
    for dim, P, B in CONFIGS:
        h = next(r for r in rows if (r["mode"], r["dim"], r["objects"]) == ("host", dim, B))
        b = next(r for r in rows if (r["mode"], r["dim"], r["objects"]) == ("batch", dim, B))
        print(f"{dim}^3 x {P} points, B = {B}: host loop {h['per_object_ms']:.2f} ms / object, batch "
              f"{b['per_object_ms']:.3f} ms / object ({h['median_ms'] / b['median_ms']:.1f} x), kernel "
              f"<= {b['kernel_ms_per_iteration'] * 1000:.1f} us / iteration")
    with open(args.out, "w") as f:
        json.dump(dict(method=f"fresh process per row, {WARMUP} warm-up calls, median of {REPS}, event pairs, "
                       f"{ITER} iterations per call", rows=rows), f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
