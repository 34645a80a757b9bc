"""Per-layer time of the volumetric part's layers on the fp32-MFMA kernels vs the split-bf16 GEMMs (epilogue and split-K
finish pass included), at --batches objects, and the volumetric part / Model.predict with the split path on / off.
CUDA-event medians over --reps launches after a warm-up.  -> CSV on stdout (profiles/volumetric_split_bf16_layers.csv,
DESIGN.md 8.4: the basis of volumetric_cl.SPLIT_MIN_BATCH).
--conv3-occ: conv3's 16 occupancy channels instead -- the layer (split-K finish included) and the occupancy branch that
feeds it in both forms, and the layer under the other plans the knobs allow (profiles/volumetric_split2_layers.csv)."""
import argparse
import os
import statistics

import torch

import morefusion_amd as mf
from morefusion_amd import _lib
from morefusion_amd.contrib.singleview_3d.models import Model, volumetric_cl
from morefusion_amd.contrib.singleview_3d.models.volumetric_cl import ChannelsLastVolumetric, F_COLS, F_LD

KEYS = ("class_id", "rgb", "pcd", "pitch", "origin", "grid_nontarget_empty")


def timed(fn, reps):
    fn()
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


def split(x):
    hi = x.to(torch.bfloat16)
    return torch.cat([hi, (x - hi.float()).to(torch.bfloat16)], dim=-1).contiguous()


def conv3_occ(model, vol, L, args):
    """B,what,fp32_ms,split_ms,tile,S,gflop,split_tflops_fp32_equivalent; ``what`` = conv3_occ (the default plan),
    conv3_occ@<knobs> (the same layer under a forced plan), occupancy_convs (the producer: fp32 store / split store)."""
    plans = [("", {}), ("@tile256_S1", {"MF_NT_BIG": "2", "MF_NT_SPLITK": "1"}),
             ("@tile256_S3", {"MF_NT_BIG": "2", "MF_NT_SPLITK": "3"}), ("@tile128", {"MF_NT_BIG": "0"})]
    print("B,what,fp32_ms,split_ms,tile,S,gflop,split_tflops_fp32_equivalent")
    for B in [int(b) for b in args.batches.split(",")]:
        grid = (torch.rand(B, 32, 32, 32, device="cuda") < 0.4).float()
        t32 = timed(lambda: vol.occupancy(grid), args.reps)
        ts = timed(lambda: vol.occupancy(grid, split=True), args.reps)
        print(f"{B},occupancy_convs,{t32:.4f},{ts:.4f},,,,", flush=True)
        h = vol.occupancy(grid).clone()
        hs = vol.occupancy(grid, split=True)
        kw = dict(cin=16, c_off=144, relu=False, bias=False)
        t32 = timed(lambda: vol.conv_k4s2("conv3_occ", model.conv3, h, B, 32, **kw), args.reps)
        g = 2.0 * B * 16 ** 3 * 256 * 64 * 16 / 1e9
        for tag, env in plans:
            os.environ.update(env)
            try:
                ts = timed(lambda: vol.conv_k4s2_split("conv3_occ", model.conv3, hs, B, 32, **kw), args.reps)
                tile = L.mf_gemm_bf16_last_tile()
                S = L.mf_conv3d_k4s2_split_workspace_bytes(B, 16, 256, 32) // (B * 16 ** 3 * 256 * 4) or 1
            finally:
                for k in env:
                    del os.environ[k]
            print(f"{B},conv3_occ{tag},{t32:.4f},{ts:.4f},{tile},{S},{g:.2f},{g / ts:.1f}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--batches", default="1,2,4,8")
    ap.add_argument("--no-predict", action="store_true")
    ap.add_argument("--conv3-occ", action="store_true")
    args = ap.parse_args()
    torch.backends.cudnn.benchmark = False
    torch.manual_seed(0)
    model = Model(n_fg_class=21, with_occupancy=True).cuda().eval()
    vol = ChannelsLastVolumetric(model)
    L = _lib.lib()
    if args.conv3_occ:
        with torch.no_grad():
            conv3_occ(model, vol, L, args)
        return
    print("B,what,fp32_ms,split_ms,gflop,split_tflops_fp32_equivalent")
    with torch.no_grad():
        for B in [int(b) for b in args.batches.split(",")]:
            n = B * 1000
            h3 = torch.relu(torch.randn(B, 16 ** 3, 256, device="cuda"))
            h3s = split(h3)
            t32 = timed(lambda: vol.conv_k4s2("conv4", model.conv4, h3, B, 16, cin=256), args.reps)
            ts = timed(lambda: vol.conv_k4s2_split("conv4", model.conv4, h3s, B, 16, cin=256), args.reps)
            g = 2.0 * B * 512 * 512 * 64 * 256 / 1e9
            print(f"{B},conv4,{t32:.4f},{ts:.4f},{g:.2f},{g / ts:.1f}", flush=True)
            feat = torch.zeros(n, F_LD, device="cuda")
            feat[:, :F_COLS].normal_()
            fs = torch.zeros(n, 2 * F_LD, dtype=torch.bfloat16, device="cuda")
            vol._split_cols(feat, 0, F_COLS, fs)
            h1 = torch.empty(n, 1920, device="cuda")
            ChannelsLastVolumetric.split_bf16 = False
            vol.heads(feat, B, 1000)   # builds the fp32 pack
            ChannelsLastVolumetric.split_bf16 = True
            w1, b1 = vol._packs["gemm_heads1"][1]
            t32 = timed(lambda: _lib.check(L.mf_linear_fwd(feat.data_ptr(), 0, F_LD, w1.data_ptr(), 0, F_LD, b1.data_ptr(), 0,
                                                           h1.data_ptr(), 0, 1920, n, 1920, 1920, F_LD, 1, 1,
                                                           _lib.stream_ptr()), "mf_linear_fwd"), args.reps)
            ts = timed(lambda: vol.heads1_split(fs, h1), args.reps)
            g = 2.0 * n * 1920 * F_COLS / 1e9
            print(f"{B},heads1,{t32:.4f},{ts:.4f},{g:.2f},{g / ts:.1f}", flush=True)
            tsp = timed(lambda: vol._split_cols(feat, 0, 216, fs), args.reps)
            print(f"{B},split_mlp_columns,,{tsp:.4f},,", flush=True)
            if args.no_predict:
                continue
            b = mf.synthetic.make_singleview_batch(B, seed=7)
            inp = {k: torch.as_tensor(b[k]).cuda() for k in KEYS}
            pix = model._select_points(inp["pcd"])
            values, points = model._backbone_features(inp["rgb"], inp["pcd"], pix)
            pa = (inp["class_id"], values, points, inp["pitch"].float(), inp["origin"].float(), inp["grid_nontarget_empty"])
            saved = dict(volumetric_cl.SPLIT_MIN_BATCH)
            for k in saved:   # (force the split path at this batch: the table is what is being measured)
                volumetric_cl.SPLIT_MIN_BATCH[k] = 1
            res = {}
            for what, fn in (("volumetric_part", lambda: model._pose_from_features(*pa)), ("predict", lambda: model.predict(**inp))):
                for on in (False, True, False, True):
                    ChannelsLastVolumetric.split_bf16 = on
                    res.setdefault((what, on), []).append(timed(fn, args.reps))
                print(f"{B},{what},{min(res[(what, False)]):.4f},{min(res[(what, True)]):.4f},,", flush=True)
            ChannelsLastVolumetric.split_bf16 = True
            volumetric_cl.SPLIT_MIN_BATCH.update(saved)


if __name__ == "__main__":
    main()
