"""Per-layer time of the 2-D backbone's in-scope convolutions: MIOpen fp32 (the layer as the stock path runs it) vs the
split-bf16 GEMM (ops2d.conv_split, epilogue included), 1 and 8 objects, and Model.predict with the split path on / off.
CUDA-event medians over --reps launches after a warm-up.  -> one JSON line per measurement.

--front: the front end instead -- res2 / res3's layers alone (MIOpen on the NCHW map it gets, the split GEMM with its
epilogue), the stem pool and the layer GROUP with its glue (pool + res2 + res3 as the stock modules run them against
maxpool_split + the split blocks), at --batches objects -> --csv (profiles/frontend_split_layers.csv)."""
import argparse
import json
import statistics

import torch
import torch.nn as nn
import torch.nn.functional as F

import morefusion_amd as mf
from morefusion_amd.contrib.singleview_3d.models import Model
from morefusion_amd.models import backbone2d, ops2d

LAYERS = {  # name: (Cin, Cout, ks, dil, map side, bias, act, calls per predict)
    "res4.0.conv1": (128, 256, 3, 1, 32, False, 1, 1),
    "res4.0.conv2": (256, 256, 3, 1, 32, False, 1, 1),        # the first block of a stage is not dilated
    "res4.1.conv1/conv2": (256, 256, 3, 2, 32, False, 1, 2),
    "res4.residual": (128, 256, 1, 1, 32, False, 0, 1),
    "res5.0.conv1": (256, 512, 3, 1, 32, False, 1, 1),
    "res5.0.conv2": (512, 512, 3, 1, 32, False, 1, 1),
    "res5.1.conv1/conv2": (512, 512, 3, 4, 32, False, 1, 2),
    "res5.residual": (256, 512, 1, 1, 32, False, 0, 1),
    "psp.bottleneck": (2560, 1024, 1, 1, 32, True, 1, 1),
    "up1.conv": (1024, 256, 3, 1, 64, True, 2, 1),
    "up2.conv": (256, 64, 3, 1, 128, True, 2, 1),
}


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts)


FRONT_LAYERS = {  # name: (Cin, Cout, ks, stride, input side, act, calls per predict)
    "res2.conv 3x3 64->64": (64, 64, 3, 1, 64, 1, 4),
    "res3.0.conv1 3x3 s2 64->128": (64, 128, 3, 2, 64, 1, 1),
    "res3 3x3 128->128": (128, 128, 3, 1, 32, 1, 3),
    "res3.residual 1x1 s2 64->128": (64, 128, 1, 2, 64, 0, 1),
}


def front(args):
    rows = []

    def emit(**kw):
        rows.append(kw)
        print(json.dumps(kw), flush=True)

    with torch.no_grad():
        res = backbone2d.ResNet18().cuda().eval()
        for B in [int(b) for b in args.batches.split(",")]:
            for name, (Cin, Cout, ks, stride, D, act, calls) in FRONT_LAYERS.items():
                conv = nn.Conv2d(Cin, Cout, ks, stride, padding=ks // 2, bias=False).cuda().eval()
                x = torch.randn(B, Cin, D, D, device="cuda")
                xs = ops2d.to_split(x)
                emit(B=B, what=name, calls=calls, stock_ms=round(timed(lambda: conv(x), args.reps), 4),
                     new_ms=round(timed(lambda: ops2d.conv_split(xs, conv, act=act, out32=False, outs=True), args.reps), 4))
            c1 = torch.randn(B, 64, 128, 128, device="cuda")  # conv1's output, NCHW as MIOpen leaves it

            def stock_front():
                return res.res3(res.res2(F.max_pool2d(c1, 3, 2, 1)))

            def split_front():
                x32, xs = ops2d.maxpool_split(c1)
                return backbone2d.ResNet18._blocks_split(list(res.res2) + list(res.res3), xs, x32)

            emit(B=B, what="stem pool alone", calls=1, stock_ms=round(timed(lambda: F.max_pool2d(c1, 3, 2, 1), args.reps), 4),
                 new_ms=round(timed(lambda: ops2d.maxpool_split(c1), args.reps), 4))
            emit(B=B, what="group: pool + res2 + res3 with glue", calls=1, stock_ms=round(timed(stock_front, args.reps), 4),
                 new_ms=round(timed(split_front, args.reps), 4))
    if args.csv:
        with open(args.csv, "w") as f:
            f.write("objects,what,calls_per_predict,stock_ms,new_ms\n")
            for r in rows:
                f.write(f"{r['B']},{r['what']},{r['calls']},{r['stock_ms']},{r['new_ms']}\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--front", action="store_true", help="the front end (stem pool, res2 / res3) instead")
    ap.add_argument("--csv", default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no-predict", action="store_true")
    ap.add_argument("--batches", default="1,8")
    args = ap.parse_args()
    torch.backends.cudnn.benchmark = False
    if args.front:
        return front(args)
    slope = torch.tensor([0.25], device="cuda")
    with torch.no_grad():
        for B in [int(b) for b in args.batches.split(",")]:
            for name, (Cin, Cout, ks, dil, D, has_bias, act, calls) in LAYERS.items():
                conv = nn.Conv2d(Cin, Cout, ks, 1, padding=dil * (ks // 2), dilation=dil, bias=has_bias).cuda().eval()
                x = torch.randn(B, Cin, D, D, device="cuda")
                xs = ops2d.to_split(x)
                t_miopen = timed(lambda: conv(x), args.reps)
                t_split = timed(lambda: ops2d.conv_split(xs, conv, act=act, slope=slope, outs=act == 1), args.reps)
                gflop = 2.0 * B * D * D * Cout * Cin * ks * ks / 1e9
                print(json.dumps(dict(B=B, layer=name, calls=calls, miopen_ms=round(t_miopen, 4),
                                      split_ms=round(t_split, 4), gflop=round(gflop, 2),
                                      split_tflops=round(gflop / t_split, 1))), flush=True)
        if not args.no_predict:
            model = Model(n_fg_class=21, with_occupancy=True).cuda().eval()
            for B in (1, 8):
                b = mf.synthetic.make_singleview_batch(B, seed=7)
                inp = {k: torch.as_tensor(b[k]).cuda() for k in
                       ("class_id", "rgb", "pcd", "pitch", "origin", "grid_nontarget_empty")}
                for split in (False, True, False, True):
                    backbone2d.ResNet18.split_bf16 = backbone2d.PSPNetExtractor.split_bf16 = split
                    t = timed(lambda: model.predict(**inp), args.reps)
                    print(json.dumps(dict(B=B, what="predict", split=split, ms=round(t, 3))), flush=True)
            backbone2d.ResNet18.split_bf16 = backbone2d.PSPNetExtractor.split_bf16 = True


if __name__ == "__main__":
    main()
