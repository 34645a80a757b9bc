"""The 2-D backbone's split-bf16 convolutions on the MI355X (csrc/gemm_bf16.hip mf_conv2d_split_fwd).

* every in-scope layer at its real shape, 1 and 8 objects: |y - y_fp64| <= 2^-15 conv(|x|, |w|)_fp64 elementwise (the
  precision contract gives ~3 * 2^-18 per product plus fp32 accumulation);
* ``Model.predict`` on the split path against the MIOpen path (``split_bf16 = False``), same weights and inputs;
* ``Model.predict_graphed`` replays the split path on new frames as the eager path computes them."""
import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import morefusion_amd as mf  # noqa: E402
from morefusion_amd.contrib.singleview_3d.models import Model  # noqa: E402
from morefusion_amd.models import backbone2d, ops2d  # noqa: E402

KEYS = ("class_id", "rgb", "pcd", "pitch", "origin", "grid_nontarget_empty")

LAYERS = {  # name: (Cin, Cout, ks, dil, map side, bias, act)
    "res4.conv1": (128, 256, 3, 1, 32, False, 1),
    "res4.conv2_dil2": (256, 256, 3, 2, 32, False, 1),
    "res4.residual": (128, 256, 1, 1, 32, False, 0),
    "res5.conv1": (256, 512, 3, 1, 32, False, 1),
    "res5.conv2_dil4": (512, 512, 3, 4, 32, False, 1),
    "res5.residual": (256, 512, 1, 1, 32, False, 0),
    "psp.bottleneck": (2560, 1024, 1, 1, 32, True, 1),
    "up1.conv": (1024, 256, 3, 1, 64, True, 2),
    "up2.conv": (256, 64, 3, 1, 128, True, 2),
}


@pytest.mark.parametrize("B", [1, 8])
@pytest.mark.parametrize("name", list(LAYERS))
def test_layer_error_bound(name, B):
    Cin, Cout, ks, dil, D, has_bias, act = LAYERS[name]
    torch.manual_seed(0)
    conv = nn.Conv2d(Cin, Cout, ks, 1, padding=dil * (ks // 2), dilation=dil, bias=has_bias).cuda().eval()
    x = torch.randn(B, Cin, D, D, device="cuda")
    slope = torch.tensor([0.25], device="cuda")
    with torch.no_grad():
        y, ys = ops2d.conv_split(ops2d.to_split(x), conv, act=act, slope=slope, outs=True)
        x64, w64 = x.double(), conv.weight.double()
        ref = F.conv2d(x64, w64, None, 1, conv.padding, conv.dilation)
        bound = F.conv2d(x64.abs(), w64.abs(), None, 1, conv.padding, conv.dilation)
        if has_bias:
            ref = ref + conv.bias.double()[None, :, None, None]
    pre = ref.permute(0, 2, 3, 1)
    want = F.relu(pre) if act == 1 else torch.where(pre > 0, pre, 0.25 * pre) if act == 2 else pre
    lim = 2.0 ** -15 * bound.permute(0, 2, 3, 1) + 1e-30
    err = (y.double() - want).abs()
    # (ReLU / PReLU are 1-Lipschitz: the bound of the pre-activation holds after them)
    assert bool((err <= lim).all()), (name, B, float((err / lim).max()))
    # the split output is the split of the fp32 output
    hi = ys[..., :Cout].float()
    lo = ys[..., Cout:].float()
    assert torch.equal(hi, y.to(torch.bfloat16).float())
    assert torch.equal(lo, (y - hi).to(torch.bfloat16).float())


def _predict(model, inputs, split, graphed=False):
    saved = backbone2d.ResNet18.split_bf16, backbone2d.PSPNetExtractor.split_bf16
    backbone2d.ResNet18.split_bf16 = backbone2d.PSPNetExtractor.split_bf16 = split
    try:
        with torch.no_grad():
            f = model.predict_graphed if graphed else model.predict
            f(**inputs)
            return tuple(x.cpu() for x in f(**inputs))
    finally:
        backbone2d.ResNet18.split_bf16, backbone2d.PSPNetExtractor.split_bf16 = saved


def _add(points, qa, ta, qb, tb):
    from oracle import oracle_np as O
    Ta = O.transformation_matrix(qa.astype(np.float64)[None], ta.astype(np.float64)[None])[0]
    Tb = O.transformation_matrix(qb.astype(np.float64)[None], tb.astype(np.float64)[None])[0]
    return float(np.linalg.norm((points @ Ta[:3, :3].T + Ta[:3, 3]) - (points @ Tb[:3, :3].T + Tb[:3, 3]), axis=1).mean())


@pytest.mark.parametrize("weights,batch", [("random", 1), ("random", 8), ("ref_predict", None), ("ref_predict", 8)])
def test_predict_split_vs_miopen(weights, batch):
    """Random weights, and the weights / inputs of tests/golden/ref_predict.npz (its own batch, and 8 objects: the
    split path then covers res4 / res5 / up2 too)."""
    torch.backends.cudnn.benchmark = False
    seed = 7
    if weights == "ref_predict":
        from conftest import golden
        g = golden("ref_predict.npz")
        torch.manual_seed(int(g["weight_seed"]))
        seed = int(g["seed"])
        batch = int(g["batch_size"]) if batch is None else batch
    else:
        torch.manual_seed(0)
    model = Model(n_fg_class=21, with_occupancy=True).cuda().eval()
    b = mf.synthetic.make_singleview_batch(batch, seed=seed)
    inputs = {k: torch.as_tensor(b[k]).cuda() for k in KEYS}
    rot_s, trans_s, conf_s = _predict(model, inputs, True)
    rot_m, trans_m, conf_m = _predict(model, inputs, False)
    np.testing.assert_allclose(rot_s.numpy(), rot_m.numpy(), rtol=0, atol=2e-4)
    np.testing.assert_allclose(conf_s.numpy(), conf_m.numpy(), rtol=0, atol=2e-4)
    pitch = np.asarray(b["pitch"], np.float32).reshape(batch, 1, 1)
    np.testing.assert_allclose(trans_s.numpy() / pitch, trans_m.numpy() / pitch, rtol=0, atol=2e-4)
    cad = np.random.RandomState(0).uniform(-0.05, 0.05, (500, 3))
    for i in range(batch):
        j = int(conf_m[i].argmax())
        add = _add(cad, rot_s[i, j].numpy(), trans_s[i, j].numpy(), rot_m[i, j].numpy(), trans_m[i, j].numpy())
        assert add <= 1e-5, (i, add)


@pytest.mark.parametrize("batch", [1, 8])
def test_predict_graphed_split_replay_on_new_frames(batch):
    """At 8 objects every split layer group (res4 / res5 blocks with their residual epilogue, psp + up1, up2) is in
    the captured graph; at 1 object psp + up1."""
    assert backbone2d.ResNet18.split_bf16 and backbone2d.PSPNetExtractor.split_bf16
    assert batch >= backbone2d.SPLIT_MIN_BATCH["res4_res5"] or batch == 1
    torch.manual_seed(0)
    torch.backends.cudnn.benchmark = False
    model = Model(n_fg_class=21, with_occupancy=True).cuda().eval()
    frames = []
    for seed in (31, 32, 33):
        b = mf.synthetic.make_singleview_batch(batch, seed=seed)
        frames.append({k: torch.as_tensor(b[k]).cuda() for k in KEYS})
    with torch.no_grad():
        eager = [tuple(x.clone() for x in model.predict(**f)) for f in frames]
        eager = [tuple(x.clone() for x in model.predict(**f)) for f in frames]
        for i, f in enumerate(frames):
            got = model.predict_graphed(**f)
            for g, e in zip(got, eager[i]):
                np.testing.assert_allclose(g.cpu().numpy(), e.cpu().numpy(), rtol=0, atol=2e-5)
        assert len(model._graphed.entries) == 1


@pytest.mark.parametrize("H,W", [(256, 192), (240, 240)])
def test_other_geometry_falls_back_to_miopen(H, W):
    """A map the split GEMM cannot address -- not square (res3 side 32 x 24), or a side that is not a power of two
    (240: side 30) -- runs the MIOpen path whatever the switch says: the same result as with the switch off."""
    torch.manual_seed(0)
    torch.backends.cudnn.benchmark = False
    B = 8
    res, psp = backbone2d.ResNet18().cuda().eval(), backbone2d.PSPNetExtractor().cuda().eval()
    rgb = torch.rand(B, 3, H, W, device="cuda") * 255
    pix = torch.randint(0, H * W, (B, 100), device="cuda")
    outs = {}
    for split in (False, True):
        saved = backbone2d.ResNet18.split_bf16, backbone2d.PSPNetExtractor.split_bf16
        backbone2d.ResNet18.split_bf16 = backbone2d.PSPNetExtractor.split_bf16 = split
        try:
            with torch.no_grad():
                for _ in range(2):  # (MIOpen's solver choice settles on the first call of a shape)
                    feat = res(rgb)
                    rows = psp.forward_sampled_rows(feat, pix)
        finally:
            backbone2d.ResNet18.split_bf16, backbone2d.PSPNetExtractor.split_bf16 = saved
        outs[split] = (feat.float().cpu(), rows.cpu())
    assert outs[True][0].shape == (B, 512, H // 8, W // 8)
    for a, b in zip(outs[True], outs[False]):
        np.testing.assert_allclose(a.numpy(), b.numpy(), rtol=0, atol=1e-6 * float(b.abs().max()))
