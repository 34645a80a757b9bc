"""Per-layer time of the PSP decoder's up-sampling blocks in their two forms, 1 and 8 objects:
  old  resize-and-split of the fp32 map (ops2d.upsample_split) + 3 x 3 split-bf16 GEMM at the high resolution
  new  1 x 1 tap GEMM Cin -> 9 Cout at the low resolution (ops2d.conv_taps_split) + tap-sum resize (upsample_tapsum)
and, for reference, the stock form (resize kernel + MIOpen convolution + PReLU) that up2 runs below
SPLIT_MIN_BATCH["up2"].  CUDA-event medians over --reps launches after a warm-up -> CSV on stdout or --out."""
import argparse
import statistics
import sys

import torch

from morefusion_amd.models import backbone2d, ops2d

LAYERS = {"up1": (1024, 256, 32), "up2": (256, 64, 64)}  # name: (Cin, Cout, low-resolution side)


def timed(fn, reps):
    for _ in range(3):
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--batches", default="1,8")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    torch.backends.cudnn.benchmark = False
    out = open(args.out, "w") if args.out else sys.stdout
    print("B,layer,form,piece,ms", file=out, flush=True)
    with torch.no_grad():
        for B in [int(b) for b in args.batches.split(",")]:
            for name, (Cin, Cout, D) in LAYERS.items():
                up = backbone2d.PSPUpsample(Cin, Cout).cuda().eval()
                conv, slope, bias = up.conv, up.prelu.weight.detach(), up.conv.bias.detach()
                x32 = torch.relu(torch.randn(B, D, D, Cin, device="cuda"))       # channels-last fp32: the old form's input
                xs = ops2d.to_split(x32.permute(0, 3, 1, 2))                      # split form: the new form's input
                us = ops2d.upsample_split(x32, 2 * D, 2 * D)
                z = ops2d.conv_taps_split(xs, conv)
                # the outputs each form writes in the pipeline: up1 -> split (new) / fp32 (old), up2 -> fp32
                o32, osplit = (name == "up2"), (name == "up1")
                pieces = {
                    ("old", "resize_split"): lambda: ops2d.upsample_split(x32, 2 * D, 2 * D),
                    ("old", "conv3x3"): lambda: ops2d.conv_split(us, conv, act=2, slope=slope),
                    ("old", "total"): lambda: ops2d.conv_split(ops2d.upsample_split(x32, 2 * D, 2 * D), conv, act=2,
                                                               slope=slope),
                    ("new", "tap_gemm"): lambda: ops2d.conv_taps_split(xs, conv),
                    ("new", "tapsum"): lambda: ops2d.upsample_tapsum(z, bias, act=2, slope=slope, out32=o32, outs=osplit),
                    ("new", "total"): lambda: ops2d.upsample_tapsum(ops2d.conv_taps_split(xs, conv), bias, act=2,
                                                                    slope=slope, out32=o32, outs=osplit),
                    ("stock", "total"): lambda: up(x32.permute(0, 3, 1, 2)),
                }
                for (form, piece), fn in pieces.items():
                    print(f"{B},{name},{form},{piece},{timed(fn, args.reps):.4f}", file=out, flush=True)


if __name__ == "__main__":
    main()
