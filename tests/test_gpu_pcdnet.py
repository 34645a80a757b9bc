"""The point-cloud baseline network's hand-written path on the MI355X: the kernel checks of tests/test_emul_pcdnet.py
(tests/pcdnet_cases.py) on the device, every GEMM layer of the chain against float64 within the split-bf16 contract
|y - y_fp64| <= 2^-15 (|x| . |w|)_fp64 per element (reference and bound from the fp32 inputs the layer received), the
folded heads' first layer against the unfolded 1408-channel layer, and ``predict`` on the kernel path against
``predict`` with the kernel path switched off (2e-4, the project's gate for the split path against the stock path)."""
import functools

import numpy as np
import pytest
import torch

import bf16_bound as BB
import pcdnet_cases as C

pytestmark = pytest.mark.gpu
DEV = "cuda"
CONTRACT = 2.0 ** -15


def test_stem_bitwise_vs_mirror_and_within_fp32_bound():
    C.check_stem(DEV)


def test_pool_fixed_order_and_run_to_run():
    C.check_pool(DEV)


def test_bias_relu_split_bitwise():
    C.check_bias_relu_split(DEV)


def test_epilogue_reference_rounding_order():
    C.check_epilogue(DEV)


def test_launcher_refusals():
    C.check_refusals(DEV)


def _val(split, c0, K):
    """bf16 split rows [M, ld] -> the fp32 values they carry, float64 [M, K]: hi at c0, lo K columns further."""
    return split[:, c0:c0 + K].double() + split[:, c0 + K:c0 + 2 * K].double()


def _within(got, x, w, b, relu, what):
    """got [M,N] against float64 x w^T + b on the inputs the layer received, bound 2^-15 (|x| |w|^T + |b|)."""
    ref, S = BB.linear_ref(x, w, b)
    if relu:
        ref = ref.clamp(min=0)
    err = (got.double().cpu() - ref).abs()
    bound = CONTRACT * S
    ratio = float((err / bound.clamp(min=1e-300)).max())
    BB.RATIOS[what] = max(BB.RATIOS.get(what, 0.0), ratio)
    print(f"PCDNET layer {what}: worst |got - ref| / bound = {ratio:.4f} (max err {float(err.max()):.3e})")
    assert bool(torch.isfinite(got).all()) and ratio <= 1.0, (what, ratio)


@functools.lru_cache(maxsize=None)
def _chain():
    """B = 2, P = 1000, n_fg = 21 on random activations: every stage run once, the workspace copied to the host."""
    from morefusion_amd.contrib.singleview_pcd.models import Model
    from morefusion_amd.contrib.singleview_pcd.models.pcdnet import PcdNetKernels
    B, P = 2, 1000
    torch.manual_seed(3)
    model = Model(n_fg_class=C.N_FG).eval().to(DEV)
    with torch.no_grad():
        for p in model.parameters():   # weights and biases of a size that leaves the ReLUs half open
            p.copy_(torch.randn_like(p) * (0.5 if p.ndim == 1 else (2.0 / p.shape[1]) ** 0.5))
        K = PcdNetKernels(model)
        rows = torch.randn((B * P, 32), device=DEV)
        pcd = torch.rand((B, 40, 40, 3), device=DEV) * 0.4 + torch.tensor([-0.2, -0.2, 0.4], device=DEV)
        pix = torch.randint(0, 1600, (B, P), device=DEV)
        center = pcd.reshape(B, -1, 3).median(dim=1).values.contiguous()
        cid = torch.tensor([C.N_FG, 3], device=DEV)
        p, ws = K.packs(), K.workspace(B, P, DEV)
        K.stem(ws, p, rows, pcd, pix.reshape(-1).contiguous(), center, B, P)
        K.extractor(ws, p, B * P)
        K.pool(ws, B, P)
        K.heads1(ws, p, B, P)
        K.heads234(ws, p, B * P)
        out = K.epilogue(ws, p, cid, center, B, P)
        torch.cuda.synchronize()
        host = {k: v.detach().cpu() for k, v in ws.items() if k not in ("raw", "splitk")}
    return model.cpu(), host, [o.cpu() for o in out], B, P


def test_layer_chain_within_split_bf16_contract():
    model, ws, _, B, P = _chain()
    e = model.posenet_extractor
    w = lambda c: c.weight.detach().squeeze(-1)  # noqa: E731
    xs, f1 = ws["xs"], ws["f1"]
    _within(xs[:, 128:256].double() + xs[:, 512:640].double(), _val(f1, 0, 64), w(e.conv2_rgb), e.conv2_rgb.bias, True,
            "conv2_rgb")
    _within(xs[:, 256:384].double() + xs[:, 640:768].double(), _val(f1, 128, 64), w(e.conv2_pcd), e.conv2_pcd.bias,
            True, "conv2_pcd")
    x384 = _val(xs, 0, 384)
    _within(_val(ws["h3"], 0, 512), x384[:, 128:], w(e.conv3), e.conv3.bias, True, "conv3")
    _within(ws["h4"], _val(ws["h3"], 0, 512), w(e.conv4), e.conv4.bias, True, "conv4")
    w1 = torch.cat([w(getattr(model, f"conv1_{k}")) for k in ("rot", "trans", "conf")])
    b1 = torch.cat([getattr(model, f"conv1_{k}").bias.detach() for k in ("rot", "trans", "conf")])
    _within(ws["gbias"], ws["pooled"], w1[:, 384:], b1, False, "heads1 global")
    _within(ws["y"], x384, w1[:, :384], None, False, "heads1 per point")
    np4 = C.NP4
    for g, k in enumerate(("rot", "trans", "conf")):
        c2, c3, c4 = (getattr(model, f"conv{i}_{k}") for i in (2, 3, 4))
        _within(_val(ws["h2"], 512 * g, 256), _val(ws["h1"], 1280 * g, 640), w(c2), c2.bias, True, f"heads2 {k}")
        _within(_val(ws["h3h"], 256 * g, 128), _val(ws["h2"], 512 * g, 256), w(c3), c3.bias, True, f"heads3 {k}")
        n = c4.out_channels
        _within(ws["o"][:, np4 * g:np4 * g + n], _val(ws["h3h"], 256 * g, 128), w(c4), c4.bias, False, f"heads4 {k}")
        assert not ws["o"][:, np4 * g + n:np4 * (g + 1)].any()  # the padding columns: zero weights, zero bias


def test_pool_of_the_chain_is_the_fixed_order_mean():
    import pcdnet_ref as PR
    _, ws, _, B, P = _chain()
    C.same_bits(ws["pooled"].numpy(), PR.pool(ws["h4"].numpy(), B, P), "pool of conv4's output")


def test_folded_heads1_equals_the_unfolded_1408_channel_layer():
    """h1 = relu(W[:, :384] x + (W[:, 384:] pooled + b)) as computed (GEMM K = 384, one M = B GEMM, bias + ReLU + split)
    against float64 relu(W [x | mean_p h4] + b) over all 1408 channels, from the layer's own inputs (the split rows xs
    and conv4's fp32 output), bound 2^-15 (|x| . |w|) over all 1408 channels."""
    model, ws, _, B, P = _chain()
    names = ("rot", "trans", "conf")
    w1 = torch.cat([getattr(model, f"conv1_{k}").weight.detach().squeeze(-1) for k in names])
    b1 = torch.cat([getattr(model, f"conv1_{k}").bias.detach() for k in names])
    pooled = ws["h4"].double().reshape(B, P, -1).mean(dim=1)
    feat = torch.cat([_val(ws["xs"], 0, 384), pooled.repeat_interleave(P, dim=0)], dim=1)  # [M, 1408]
    got = torch.cat([_val(ws["h1"], 1280 * g, 640) for g in range(3)], dim=1)
    _within(got, feat, w1, b1, True, "heads1 folded vs unfolded")


def test_chain_outputs_are_finite_poses():
    _, _, (rot, trans, conf), B, P = _chain()
    assert rot.shape == (B, P, 4) and trans.shape == (B, P, 3) and conf.shape == (B, P)
    assert bool(torch.isfinite(rot).all() and torch.isfinite(trans).all() and ((conf > 0) & (conf < 1)).all())
    assert float((rot.norm(dim=2) - 1).abs().max()) < 1e-3


@pytest.mark.parametrize("B", [2, 1])
def test_predict_kernel_path_vs_torch_formulation(B):
    import morefusion_amd as mf
    from morefusion_amd.contrib.singleview_pcd.models import Model
    torch.manual_seed(0)
    model = Model(n_fg_class=21).eval().to(DEV)
    b = mf.synthetic.make_singleview_batch(B, seed=5)
    inp = {k: torch.as_tensor(b[k]).to(DEV) for k in ("class_id", "rgb", "pcd")}
    with torch.no_grad():
        pix = model._select_points(inp["pcd"])
        pts = torch.gather(inp["pcd"].reshape(B, -1, 3), 1, pix[:, :, None].expand(B, -1, 3))
        model.predict(**inp)
        got = model.predict(**inp)
        assert model._pcd_kernels_op is not None
        model.pcd_kernels = False
        model.predict(**inp)
        ref = model.predict(**inp)
    for name, g, r in (("quaternion", got[0], ref[0]), ("offset", got[1] - pts, ref[1] - pts), ("confidence", got[2], ref[2])):
        d = float((g - r).abs().max())
        print(f"PCDNET predict kernel path vs torch formulation B={B} {name}: max |diff| = {d:.3e}")
        assert d <= 2e-4, (name, d)
    with torch.no_grad(), pytest.raises(ValueError, match="no valid point"):
        model.predict(class_id=inp["class_id"], rgb=inp["rgb"], pcd=torch.full_like(inp["pcd"], float("nan")))
