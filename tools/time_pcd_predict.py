#!/usr/bin/env python
"""Timing of the point-cloud baseline network's inference (contrib/singleview_pcd) on one GPU, one process.

Method: every figure is the median of ``--iters`` device times taken with a pair of CUDA events around one call, after
``--warmup`` untimed calls (weight packs, workspaces and MIOpen's solver choices settle there); the host waits for the
closing event of each call, so no call overlaps the next.  At B = 1 and B = 8 (``--batches``):
  * the stages of the kernel path (models/pcdnet.py), each alone on the activations the stage before it left;
  * the whole ``predict`` on the kernel path against the stock-torch formulation of the same model (``pcd_kernels``);
  * heads layer 1 folded (M = B GEMM + K = 384 GEMM + bias / ReLU / split) against unfolded: one mf_linear_split_fwd
    with K = 1408 on rows that hold the pooled vector repeated over the points -- built here only, and building them
    is timed apart.
Writes profiles/pcd_predict_timing.json and profiles/pcd_predict_kernels.csv."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import morefusion_amd as mf  # noqa: E402
from morefusion_amd import _lib  # noqa: E402
from morefusion_amd.contrib.singleview_pcd.models import Model  # noqa: E402
from morefusion_amd.geometry.instance_crops import valid_points_median  # noqa: E402
from morefusion_amd.contrib.singleview_pcd.models.pcdnet import PcdNetKernels  # noqa: E402


def timed(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(np.min(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    args = ap.parse_args()
    torch.manual_seed(0)
    model = Model(n_fg_class=21).cuda().eval()
    L = _lib.lib()
    result = {"device": torch.cuda.get_device_name(0), "warmup": args.warmup, "iters": args.iters,
              "statistic": "median of per-call CUDA-event times, ms (min in brackets in the csv)", "batches": {}}
    rows_csv = ["batch,what,median_ms,min_ms"]
    with torch.no_grad():
        for B in args.batches:
            b = mf.synthetic.make_singleview_batch(B, seed=5)
            inp = {k: torch.as_tensor(b[k]).cuda() for k in ("class_id", "rgb", "pcd")}
            P = model._n_point
            M = B * P
            r = {}
            model.pcd_kernels = True
            r["predict, kernel path"] = timed(lambda: model.predict(**inp), args.warmup, args.iters)
            model.pcd_kernels = False
            r["predict, torch formulation"] = timed(lambda: model.predict(**inp), args.warmup, args.iters)
            model.pcd_kernels = True
            # the stages, on the activations of a real call
            pcd = inp["pcd"].float()
            pix = model._select_points(pcd)
            center = valid_points_median(pcd).contiguous()
            feats = model.resnet_extractor(inp["rgb"].permute(0, 3, 1, 2))
            rows = model.pspnet_extractor.forward_sampled_rows(feats, pix)
            K = PcdNetKernels(model)
            p, ws = K.packs(), K.workspace(B, P, rows.device)
            pixf = pix.reshape(-1).contiguous()
            r["2-D backbone + sampled PSPNet tail"] = timed(
                lambda: model.pspnet_extractor.forward_sampled_rows(model.resnet_extractor(inp["rgb"].permute(0, 3, 1, 2)), pix),
                args.warmup, args.iters)
            stages = (("stem", lambda: K.stem(ws, p, rows, pcd, pixf, center, B, P)),
                      ("conv2 x2, conv3, conv4", lambda: K.extractor(ws, p, M)),
                      ("pool", lambda: K.pool(ws, B, P)),
                      ("heads layer 1, folded", lambda: K.heads1(ws, p, B, P)),
                      ("heads layers 2-4", lambda: K.heads234(ws, p, M)),
                      ("epilogue", lambda: K.epilogue(ws, p, inp["class_id"], center, B, P)))
            for name, fn in stages:
                r[name] = timed(fn, args.warmup, args.iters)
            r["point MLP + heads, all stages in sequence"] = timed(
                lambda: K.pose(inp["class_id"], rows, pcd, pix, center), args.warmup, args.iters)

            # heads layer 1 unfolded: K = 1408 on materialised rows (hi 1408 | lo 1408)
            names = ("rot", "trans", "conf")
            w1 = torch.cat([getattr(model, f"conv1_{k}").weight.detach().float().squeeze(-1) for k in names]).contiguous()
            b1 = torch.cat([getattr(model, f"conv1_{k}").bias.detach().float() for k in names]).contiguous()
            wp = K._split_pack(w1, 1408)
            full = torch.empty((M, 2 * 1408), dtype=torch.bfloat16, device="cuda")
            h1u = torch.empty((M, 2 * 1920), dtype=torch.bfloat16, device="cuda")

            def materialise():
                full[:, 0:384] = ws["xs"][:, 0:384]
                full[:, 1408:1408 + 384] = ws["xs"][:, 384:768]
                hi = ws["pooled"].to(torch.bfloat16)
                lo = (ws["pooled"] - hi.float()).to(torch.bfloat16)
                full[:, 384:1408] = hi.repeat_interleave(P, dim=0)
                full[:, 1408 + 384:] = lo.repeat_interleave(P, dim=0)

            nbytes = L.mf_linear_split_workspace_bytes(M, 1920, 1408)
            sk = torch.empty((max(nbytes, 16),), dtype=torch.uint8, device="cuda")

            def unfolded():
                _lib.check(L.mf_linear_split_fwd(full.data_ptr(), 2 * 1408, wp.data_ptr(), b1.data_ptr(), 1, None, 0,
                                                 h1u.data_ptr(), 2 * 1920, 1920, sk.data_ptr(), nbytes, M, 1920, 1408,
                                                 _lib.stream_ptr()), "mf_linear_split_fwd")
            r["heads layer 1, unfolded: building the 1408-wide rows"] = timed(materialise, args.warmup, args.iters)
            r["heads layer 1, unfolded: GEMM K = 1408"] = timed(unfolded, args.warmup, args.iters)
            # the two forms compute the same layer
            K.heads1(ws, p, B, P)
            folded = torch.cat([ws["h1"][:, 1280 * g:1280 * g + 640].float() + ws["h1"][:, 1280 * g + 640:1280 * (g + 1)].float()
                                for g in range(3)], dim=1)
            unf = h1u[:, :1920].float() + h1u[:, 1920:].float()
            r_diff = float((folded - unf).abs().max())
            result["batches"][str(B)] = {k: {"median_ms": v[0], "min_ms": v[1]} for k, v in r.items()}
            result["batches"][str(B)]["folded vs unfolded, max |difference|"] = r_diff
            for k, v in r.items():
                rows_csv.append(f"{B},{k},{v[0]:.4f},{v[1]:.4f}")
                print(f"B={B:2d} {k:58s} {v[0]:8.3f} ms (min {v[1]:.3f})")
            print(f"B={B:2d} folded vs unfolded heads layer 1: max |difference| {r_diff:.3e}")
    os.makedirs(args.out, exist_ok=True)
    json.dump(result, open(os.path.join(args.out, "pcd_predict_timing.json"), "w"), indent=1)
    open(os.path.join(args.out, "pcd_predict_kernels.csv"), "w").write("\n".join(rows_csv) + "\n")


if __name__ == "__main__":
    main()
