"""Attribute the 2-D backbone's convolution launches of a bench kernel sequence (tools/kernel_stats.py MF_SEQ output of
the steady steps) to layers, from launch order -> per-layer mean kernel time per step (CSV on stdout).

MIOpen path: a predict launches 27 convolutions (igemm / CK grouped-conv kernels) in module order, listed in LAYERS.
Split path: the 2-D split GEMMs (k_gemm_nt_bf16*<3...>), their split-K finish, the split / resize-split kernels are
summed as one group; the convolutions still on MIOpen are attributed in order to the layers the dispatch left there.
usage: python tools/attribute_convs.py SEQ.csv STEPS [off|on]"""
import collections
import sys

LAYERS = (["conv1"] + [f"res2.{b}.conv{i}" for b in (0, 1) for i in (1, 2)]
          + [n for s in (3, 4, 5) for n in (f"res{s}.0.conv1", f"res{s}.0.conv2", f"res{s}.0.residual",
                                            f"res{s}.1.conv1", f"res{s}.1.conv2")]
          + [f"psp.branch{i}" for i in range(4)] + ["psp.bottleneck", "up1.conv", "up2.conv"])
IN_SCOPE = {n for n in LAYERS if n.startswith(("res4", "res5")) or n in ("psp.bottleneck", "up1.conv", "up2.conv")}
SPLIT = ("k_gemm_nt_bf16_pp<3>", "k_gemm_nt_bf16<3,", "k_splitk_finish_conv2", "k_split_bf16", "k_up_fwd_split",
         "k_conv2_pack_split")


def main():
    path, steps, mode = sys.argv[1], int(sys.argv[2]), (sys.argv[3] if len(sys.argv) > 3 else "off")
    rows = [line.rstrip("\n").split(",", 3) for line in open(path)]
    convs = [(float(r[2]), r[3]) for r in rows if "igemm" in r[3] or "grouped_conv" in r[3]]
    split = sum(float(r[2]) for r in rows if any(s in r[3] for s in SPLIT))
    left = LAYERS if mode == "off" else [n for n in LAYERS if n not in IN_SCOPE]
    if len(convs) != len(left) * steps:
        sys.exit(f"{len(convs)} convolution launches, expected {len(left)} x {steps}")
    per = collections.OrderedDict((n, 0.0) for n in left)
    for i, (us, _) in enumerate(convs):
        per[left[i % len(left)]] += us
    print("layer,us_per_step,in_scope")
    for n, us in per.items():
        print(f"{n},{us / steps:.1f},{int(n in IN_SCOPE)}")
    if mode == "on":
        print(f"split-bf16 kernels (all in-scope layers),{split / steps:.1f},1")
    ins = sum(us for n, us in per.items() if n in IN_SCOPE) + (split if mode == "on" else 0.0)
    print(f"total in-scope,{ins / steps:.1f},1")


if __name__ == "__main__":
    main()
