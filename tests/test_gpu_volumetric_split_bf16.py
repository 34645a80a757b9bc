"""The volumetric part's split-bf16 layers on the MI355X (conv4 and heads layer 1 through csrc/gemm_bf16.hip's
mf_conv3d_k4s2_split_fwd / mf_linear_split_fwd; the precision contract is 8.1's).

* each split layer at its real shape, 1 and 8 objects: |y - y_fp64| <= 2^-15 conv(|x|, |w|)_fp64 elementwise (about
  3 * 2^-18 per product plus fp32 accumulation: the backbone's gate);
* split outputs (sparse conv3's reduce, the samplers, the GEMM epilogue) equal the split of the fp32 value bit for bit;
* two runs of conv4 at its largest split-K are ``torch.equal``;
* ``Model.predict`` with ``ChannelsLastVolumetric.split_bf16`` on against off, same weights and inputs: 2e-4 on rot,
  conf, trans / pitch, ADD between the two arg-max poses <= 1e-5 m (the backbone test's limits);
* ``Model.predict_graphed`` replays the split path on new frames as the eager path computes them;
* below the table's batch, and under autocast, the fp32 kernels run (the result of the switch-off path, bit for bit)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import morefusion_amd as mf  # noqa: E402
from morefusion_amd import _lib  # noqa: E402
from morefusion_amd.contrib.singleview_3d.models import Model, volumetric_cl  # noqa: E402
from morefusion_amd.contrib.singleview_3d.models.volumetric_cl import ChannelsLastVolumetric, F_COLS, F_LD  # noqa: E402

KEYS = ("class_id", "rgb", "pcd", "pitch", "origin", "grid_nontarget_empty")


def _split(x):
    """fp32 [..., C] -> bf16 [..., 2C] (hi | lo), torch restatement of the split"""
    hi = x.to(torch.bfloat16)
    lo = (x - hi.float()).to(torch.bfloat16)
    return torch.cat([hi, lo], dim=-1).contiguous()


def _vol(seed=0):
    torch.manual_seed(seed)
    model = Model(n_fg_class=21, with_occupancy=True).cuda().eval()
    return model, ChannelsLastVolumetric(model)


@pytest.mark.parametrize("B", [1, 8])
def test_conv4_error_bound_and_split_output(B):
    model, vol = _vol()
    conv = model.conv4
    torch.manual_seed(1)
    x = torch.relu(torch.randn(B, 256, 16, 16, 16, device="cuda"))
    x_cl = x.permute(0, 2, 3, 4, 1).reshape(B, 16 ** 3, 256).contiguous()
    ys = torch.empty(B, 8 ** 3, 1024, dtype=torch.bfloat16, device="cuda")
    with torch.no_grad():
        y = vol.conv_k4s2_split("conv4", conv, _split(x_cl), B, 16, cin=256, out_split=ys)
        x64, w64 = x.double(), conv.weight.double()
        ref = F.relu(F.conv3d(x64, w64, conv.bias.double(), 2, 1)).permute(0, 2, 3, 4, 1).reshape(B, 8 ** 3, 512)
        bound = F.conv3d(x64.abs(), w64.abs(), None, 2, 1).permute(0, 2, 3, 4, 1).reshape(B, 8 ** 3, 512)
    lim = 2.0 ** -15 * bound + 1e-30
    err = (y.double() - ref).abs()   # (ReLU is 1-Lipschitz: the bound of the pre-activation holds after it)
    print("conv4 B=%d max err / limit = %.4f" % (B, float((err / lim).max())))
    assert bool((err <= lim).all()), (B, float((err / lim).max()))
    assert torch.equal(ys, _split(y))


@pytest.mark.parametrize("B", [1, 8])
def test_heads1_error_bound(B):
    model, vol = _vol()
    n = B * 1000
    torch.manual_seed(2)
    feat = torch.zeros(n, F_LD, device="cuda")
    feat[:, :F_COLS] = torch.relu(torch.randn(n, F_COLS, device="cuda"))
    names = ("rot", "trans", "conf")
    with torch.no_grad():
        fs = torch.zeros(n, 2 * F_LD, dtype=torch.bfloat16, device="cuda")
        vol._split_cols(feat, 0, F_COLS, fs)
        assert torch.equal(fs[:, :F_LD], feat.to(torch.bfloat16))
        assert torch.equal(fs[:, F_LD:], (feat - feat.to(torch.bfloat16).float()).to(torch.bfloat16))
        h1 = torch.empty(n, 1920, device="cuda")
        vol.heads1_split(fs, h1)
        w = torch.cat([getattr(model, f"conv1_{k}").weight.squeeze(-1) for k in names]).double()
        b = torch.cat([getattr(model, f"conv1_{k}").bias for k in names]).double()
        x64 = feat[:, :F_COLS].double()
        ref = F.relu(x64 @ w.T + b)
        bound = x64.abs() @ w.abs().T
    lim = 2.0 ** -15 * bound + 1e-30
    err = (h1.double() - ref).abs()
    print("heads1 B=%d max err / limit = %.4f" % (B, float((err / lim).max())))
    assert bool((err <= lim).all()), (B, float((err / lim).max()))


def test_conv4_largest_split_is_deterministic():
    """8 objects: 32 tiles of 256 x 256, the reduction split 8 ways over fp32 slabs added in slab order."""
    model, vol = _vol()
    B = 8
    assert _lib.lib().mf_conv3d_k4s2_split_workspace_bytes(B, 256, 512, 16) == 8 * B * 512 * 512 * 4
    torch.manual_seed(3)
    xs = _split(torch.relu(torch.randn(B, 16 ** 3, 256, device="cuda")))
    with torch.no_grad():
        a = vol.conv_k4s2_split("conv4", model.conv4, xs, B, 16, cin=256).clone()
        b = vol.conv_k4s2_split("conv4", model.conv4, xs, B, 16, cin=256)
    assert torch.equal(a, b)


def _stage_inputs(model, B, seed=5):
    b = mf.synthetic.make_singleview_batch(B, seed=seed)
    inp = {k: torch.as_tensor(b[k]).cuda() for k in KEYS}
    pix = model._select_points(inp["pcd"])
    values, points = model._backbone_features(inp["rgb"], inp["pcd"], pix)
    return values, points, inp["pitch"].float(), inp["origin"].float(), inp["grid_nontarget_empty"]


def test_producers_write_the_split_of_their_fp32_values():
    """features() on the split path: Fs's point-MLP columns, h3's split form and both samplers' columns are the split
    of the fp32 values the fp32 path writes (h3 and its samples: the same kernels' fp32 form, bit for bit)."""
    model, vol = _vol()
    B = 8
    assert B >= max(volumetric_cl.SPLIT_MIN_BATCH.values())
    with torch.no_grad():
        args = _stage_inputs(model, B)
        feat, _ = vol.features(*args)
        fs = feat._mf_split.clone()
        h3s = vol._buf[("h3_split", (B, 16 ** 3, 512), str(feat.device), torch.bfloat16)].clone()
        ChannelsLastVolumetric.split_bf16 = False
        try:
            ref, _ = vol.features(*args)
        finally:
            ChannelsLastVolumetric.split_bf16 = True
        assert getattr(ref, "_mf_split", None) is None
    assert torch.equal(feat[:, :216], ref[:, :216])
    # columns 0..471: the same fp32 values on both paths (point MLP, samples of the fp32 h3)
    want = _split(ref[:, :472])
    assert torch.equal(fs[:, :472], want[:, :472]) and torch.equal(fs[:, F_LD:F_LD + 472], want[:, 472:])
    assert float(fs[:, F_COLS:F_LD].float().abs().max()) == 0 and float(fs[:, F_LD + F_COLS:].float().abs().max()) == 0
    # h3's split form against the fp32 h3 of the sparse conv3 (recomputed on the fp32 path)
    with torch.no_grad():
        h_occ = vol.occupancy(args[4])
        dense = vol.conv_k4s2("conv3_occ", model.conv3, h_occ, B, 32, cin=16, c_off=144, relu=False, bias=False)
        pts, _, _, bi = vol.prep(*args[:4])
        h3 = vol._sparse.from_points_cl(ref[:, 72:216], F_LD, pts, bi, B, dense, 32)
        assert torch.equal(h3s, _split(h3))
        # columns 472..983 sample the split path's own h4 (deterministic): the split of its fp32 samples
        h4 = vol.conv_k4s2_split("conv4", model.conv4, h3s, B, 16, cin=256)
        s4 = torch.empty(B * 1000, 512, device="cuda")
        vol.sample(h4, 8, pts * 0.25, bi, s4, 512)
    want4 = _split(s4)
    assert torch.equal(fs[:, 472:F_COLS], want4[:, :512]) and torch.equal(fs[:, F_LD + 472:F_LD + F_COLS], want4[:, 512:])


def _predict(model, inputs, split, graphed=False):
    saved = ChannelsLastVolumetric.split_bf16
    ChannelsLastVolumetric.split_bf16 = split
    try:
        with torch.no_grad():
            f = model.predict_graphed if graphed else model.predict
            f(**inputs)
            return tuple(x.cpu() for x in f(**inputs))
    finally:
        ChannelsLastVolumetric.split_bf16 = saved


def _add(points, qa, ta, qb, tb):
    from oracle import oracle_np as O
    Ta = O.transformation_matrix(qa.astype(np.float64)[None], ta.astype(np.float64)[None])[0]
    Tb = O.transformation_matrix(qb.astype(np.float64)[None], tb.astype(np.float64)[None])[0]
    return float(np.linalg.norm((points @ Ta[:3, :3].T + Ta[:3, 3]) - (points @ Tb[:3, :3].T + Tb[:3, 3]), axis=1).mean())


@pytest.mark.parametrize("weights,batch", [("random", 1), ("random", 8), ("ref_predict", None), ("ref_predict", 8)])
def test_predict_split_on_vs_off(weights, batch):
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
    pitch = np.asarray(b["pitch"], np.float32).reshape(batch, 1, 1)
    print("predict %s B=%d: rot %.3g conf %.3g trans/pitch %.3g" % (
        weights, batch, float((rot_s - rot_m).abs().max()), float((conf_s - conf_m).abs().max()),
        float(np.abs(trans_s.numpy() / pitch - trans_m.numpy() / pitch).max())))
    np.testing.assert_allclose(rot_s.numpy(), rot_m.numpy(), rtol=0, atol=2e-4)
    np.testing.assert_allclose(conf_s.numpy(), conf_m.numpy(), rtol=0, atol=2e-4)
    np.testing.assert_allclose(trans_s.numpy() / pitch, trans_m.numpy() / pitch, rtol=0, atol=2e-4)
    cad = np.random.RandomState(0).uniform(-0.05, 0.05, (500, 3))
    for i in range(batch):
        j = int(conf_m[i].argmax())
        add = _add(cad, rot_s[i, j].numpy(), trans_s[i, j].numpy(), rot_m[i, j].numpy(), trans_m[i, j].numpy())
        assert add <= 1e-5, (i, add)


@pytest.mark.parametrize("batch", [1, 8])
def test_predict_graphed_split_replay_on_new_frames(batch):
    assert ChannelsLastVolumetric.split_bf16
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


def test_small_batch_and_autocast_run_the_fp32_kernels():
    """Below SPLIT_MIN_BATCH the fp32-MFMA kernels run whatever the switch says: the switch-off result, bit for bit,
    and no split form is attached to F.  Under autocast the split path is never taken."""
    model, vol = _vol()
    B = min(volumetric_cl.SPLIT_MIN_BATCH.values()) - 1
    assert B >= 1
    with torch.no_grad():
        args = _stage_inputs(model, B)
        on, _ = vol.features(*args)
        assert getattr(on, "_mf_split", None) is None
        assert not vol._split_path("conv4", B) and not vol._split_path("heads1", B)
        heads_on = [t.clone() for t in vol.heads(on, B, 1000)]
        ChannelsLastVolumetric.split_bf16 = False
        try:
            off, _ = vol.features(*args)
            heads_off = vol.heads(off, B, 1000)
        finally:
            ChannelsLastVolumetric.split_bf16 = True
        assert torch.equal(on, off)
        for a, b in zip(heads_on, heads_off):
            assert torch.equal(a, b)
        args8 = _stage_inputs(model, 8)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            assert not vol._split_path("conv4", 8) and not vol._split_path("heads1", 8)
            f8, _ = vol.features(*args8)
            assert getattr(f8, "_mf_split", None) is None
        assert vol._split_path("conv4", 8) and vol._split_path("heads1", 8)
    with torch.enable_grad():
        assert not vol._split_path("conv4", 8)
