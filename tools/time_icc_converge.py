"""Time ``IccScenes.refine_until_converged(max_iter=30)`` against the fixed ``refine(30)``: wall time per scene of one
call (one hipGraph launch each), for 1 scene and 8 scenes of 8 objects, with observer thresholds under which all
scenes converge early (threshold inf: every scene stops after n_passed_threshold + 1 = 4 steps), none converges
(threshold 0), the node's constants, and -- 8 scenes -- about half of the scenes converge early (window 1, 1 pass,
a threshold between the scenes' |delta| at iteration 8; the step counts that came out are reported).  10 warm-up calls, then the
median of 30, each timed with a pair of events on the current stream.

    python tools/time_icc_converge.py [--out profiles/icc_converge_timing.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
WARMUP, REPS, MAX_ITER = 10, 30, 30


def timed(fn):
    import numpy as np
    import torch
    ms = []
    for k in range(WARMUP + REPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        if k >= WARMUP:
            ms.append(e0.elapsed_time(e1))
    return float(np.median(ms))


def main():
    import numpy as np
    import torch
    import morefusion_amd as mf
    from morefusion_amd.contrib import IccScenes
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    rows = []
    for n_scenes in (1, 8):
        scenes = [mf.synthetic.make_icc_scene(8, seed=s) for s in range(n_scenes)]
        S = IccScenes([dict(points=sc["points"], sdf=sc["sdf"], pitch=sc["pitch"], origin=sc["origin"],
                            grid_target=sc["grid_target"], grid_nontarget_empty=sc["grid_nontarget_empty"])
                       for sc in scenes], sdf_offset=0.02)
        q0 = torch.from_numpy(np.concatenate([np.stack([mf.geometry.quaternion_from_matrix(T) for T in sc["transform_init"]])
                                              for sc in scenes]).astype(np.float32)).cuda()
        t0 = torch.from_numpy(np.concatenate([sc["transform_init"][:, :3, 3] for sc in scenes]).astype(np.float32)).cuda()
        q, t = q0.clone(), t0.clone()
        m, v = torch.zeros((q.shape[0], 7), device="cuda"), torch.zeros((q.shape[0], 7), device="cuda")
        losses = torch.zeros((MAX_ITER, n_scenes), device="cuda")

        def reset():
            q.copy_(q0); t.copy_(t0); m.zero_(); v.zero_()

        def fixed():
            reset()
            S.refine(q, t, m, v, MAX_ITER)

        ms_fixed = timed(fixed)
        reset()
        S.refine(q, t, m, v, MAX_ITER, losses=losses)
        d = (losses[1:] - losses[:-1]).abs().double()
        # "half": a threshold between the scenes' delta levels at iteration 8, window 1, 1 pass
        lvl = d[7].sort().values
        half_thr = float((lvl[(n_scenes - 1) // 2] * 1.0000001).item()) if n_scenes > 1 else None
        cases = [("all_converge_early", dict(max_delta_threshold=float("inf"))),
                 ("none_converges", dict(max_delta_threshold=0.0)),
                 ("node_constants", dict())]
        if half_thr is not None:
            cases.append(("about_half_converge", dict(max_delta_threshold=half_thr, window=1, n_passed_threshold=1)))
        for name, kw in cases:
            out = {}

            def conv():
                reset()
                out["n"] = S.refine_until_converged(q, t, m, v, max_iter=MAX_ITER, **kw)

            ms = timed(conv)
            rows.append(dict(scenes=n_scenes, objects=int(q.shape[0]), case=name, observer=kw,
                             n_steps=out["n"].cpu().tolist(), ms_converge=ms, ms_fixed_30=ms_fixed,
                             ms_per_scene_converge=ms / n_scenes, ms_per_scene_fixed_30=ms_fixed / n_scenes))
            print(json.dumps(rows[-1]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(dict(max_iter=MAX_ITER, warmup=WARMUP, reps=REPS, work_skipping=True, rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
