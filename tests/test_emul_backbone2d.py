"""csrc/backbone2d.hip on the CPU emulator through models/ops2d.py: bilinear resize with align_corners and the
single-slope PReLU of PSPNet's decoder (morefusion/models/dense_fusion/pspnet.py:18-22,50-57), forward and backward,
float32 and bfloat16, against torch's own operators + autograd."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from host_emul import emul

pytestmark = pytest.mark.skipif(not emul.available(), reason="g++ not available")


@pytest.fixture()
def ops(monkeypatch):
    from morefusion_amd.models import ops2d
    L = emul.build(["backbone2d.hip"])
    emul.patch_lib(L, monkeypatch)
    return ops2d


@pytest.mark.parametrize("dtype,tol", [(torch.float32, 2e-6), (torch.bfloat16, 2.0 ** -7)])
@pytest.mark.parametrize("shape,size", [((2, 16, 5, 7), (10, 14)), ((1, 8, 1, 1), (6, 6)), ((1, 8, 3, 2), (12, 12)),
                                        ((2, 8, 6, 6), (12, 12)), ((1, 64, 9, 11), (18, 22)), ((1, 64, 8, 8), (13, 16)),
                                        ((1, 64, 1, 1), (8, 8)), ((2, 64, 3, 2), (16, 16))])
@pytest.mark.parametrize("layout", ["channels_first", "channels_last"])
def test_bilinear_resize_forward_and_backward(ops, dtype, tol, shape, size, layout):
    torch.manual_seed(0)
    x = torch.randn(shape).to(dtype)
    if layout == "channels_last":
        x = x.contiguous(memory_format=torch.channels_last)
    xa = x.clone(memory_format=torch.preserve_format).requires_grad_(True)
    y = ops.upsample_bilinear(xa, size)
    if shape[2] * shape[3] > 1:   # (a 1 x 1 map is contiguous in both formats: either result layout is right)
        assert y.is_contiguous(memory_format=torch.channels_last if layout == "channels_last" else torch.contiguous_format)
    g = torch.randn(y.shape).to(dtype)
    y.backward(g)
    xr = x.float().requires_grad_(True)
    yr = F.interpolate(xr, size, mode="bilinear", align_corners=True)
    yr.backward(g.float())
    assert y.shape == yr.shape and y.dtype == dtype
    assert float((y.float() - yr).abs().max()) <= tol * max(1.0, float(yr.abs().max()))
    assert float((xa.grad.float() - xr.grad).abs().max()) <= max(tol, 2e-6) * max(1.0, float(xr.grad.abs().max()))


@pytest.mark.parametrize("dtype,tol", [(torch.float32, 1e-6), (torch.bfloat16, 2.0 ** -7)])
def test_single_slope_prelu_forward_and_backward(ops, dtype, tol):
    torch.manual_seed(1)
    x = torch.randn(2, 16, 9, 11).to(dtype)        # 3168 elements: one ragged workgroup
    slope = torch.tensor([0.25], requires_grad=True)
    xa = x.clone().requires_grad_(True)
    y = ops.prelu(xa, slope)
    g = torch.randn(y.shape).to(dtype)
    y.backward(g)
    xr = x.float().requires_grad_(True)
    sr = torch.tensor([0.25], requires_grad=True)
    yr = F.prelu(xr, sr)
    yr.backward(g.float())
    assert float((y.float() - yr).abs().max()) <= tol * float(yr.abs().max())
    assert float((xa.grad.float() - xr.grad).abs().max()) <= tol * float(xr.grad.abs().max())
    assert abs(float(slope.grad) - float(sr.grad)) <= 1e-4 * abs(float(sr.grad)) + 1e-5


@pytest.mark.parametrize("dtype,tol", [(torch.float32, 1e-6), (torch.bfloat16, 2.0 ** -7)])
@pytest.mark.parametrize("layout", ["channels_first", "channels_last"])
@pytest.mark.parametrize("residual,relu", [(False, True), (True, True), (False, False)])
def test_batchnorm_inference_add_relu_in_one_launch(ops, monkeypatch, dtype, tol, layout, residual, relu):
    """ops2d.bn_act (k_bn_act) vs torch's BatchNorm2d in eval mode (+ add) (+ ReLU): ResNet18Extractor's units
    (models/resnet.py:44; chainercv2 ResUnit)."""
    torch.manual_seed(4)
    B, C, H, W = 2, 16, 6, 4
    bn = torch.nn.BatchNorm2d(C).eval()
    with torch.no_grad():
        bn.running_mean.normal_()
        bn.running_var.uniform_(0.3, 2.0)
        bn.weight.normal_()
        bn.bias.normal_()
    fmt = torch.channels_last if layout == "channels_last" else torch.contiguous_format
    x = torch.randn(B, C, H, W).to(dtype).contiguous(memory_format=fmt)
    idn = torch.randn(B, C, H, W).to(dtype).contiguous(memory_format=fmt) if residual else None
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    with torch.no_grad():
        assert ops.bn_act_supported(x, bn)
        y = ops.bn_act(x, bn, identity=idn, relu=relu)
    monkeypatch.undo()
    with torch.no_grad():
        ref = bn(x.float())
        if residual:
            ref = ref + idn.float()
        if relu:
            ref = F.relu(ref)
    assert y.dtype == dtype and y.shape == x.shape and y.is_contiguous(memory_format=fmt)
    assert float((y.float() - ref).abs().max()) <= tol * max(1.0, float(ref.abs().max()))
    assert not ops.bn_act_supported(x, bn)            # a CPU tensor
    assert not ops.bn_act_supported(x, bn.train())    # training statistics


@pytest.mark.parametrize("dtype", [torch.uint8, torch.float32])
def test_rgb_normalisation_in_one_launch_is_bit_equal_to_the_composite(ops, dtype):
    """ops2d.normalize_rgb (k_rgb_norm) vs ``(rgb / 255 - mean) / std`` (models/resnet.py:33-36), same operation order."""
    from morefusion_amd.models.backbone2d import ResNet18Extractor as R
    torch.manual_seed(0)
    rgb = torch.randint(0, 256, (2, 5, 7, 3), dtype=torch.uint8).to(dtype)
    y = ops.normalize_rgb(rgb, R.mean_rgb, R.std_rgb)
    x = rgb.float().permute(0, 3, 1, 2)
    ref = (x / 255.0 - torch.tensor(R.mean_rgb).view(1, 3, 1, 1)) / torch.tensor(R.std_rgb).view(1, 3, 1, 1)
    assert y.shape == ref.shape and y.stride() == ref.stride()
    assert torch.equal(y, ref)


# ---------------------------------------------------------------------------------------------------------------------
# Per element against float64 references (tests/decoder2d_ref.py, tests/decoder2d_cases.py; the same cases run on the
# MI355X in tests/test_gpu_backbone2d.py), every case asserting its branch through mf_backbone2d_last_path().
# NOT run on the emulator: the two BatchNorm cases at C = 2048 with 4096 and 8193 pixels (ppt = 2 and 4 of
# k_bn_act_cl) -- 8 and 17 million elements through one fiber per lane; they run on the GPU only.
import decoder2d_cases as D  # noqa: E402
import decoder2d_ref as R  # noqa: E402


@pytest.fixture()
def L2d():
    return emul.build(["backbone2d.hip"])


def _st():
    return None


def test_resize_mirror_vs_torch_float64():
    """The float32 mirror of the index / weight arithmetic (decoder2d_ref.axis_taps) against torch's own bilinear
    resize in float64: they differ only by the float32 rounding of the source coordinate -- the allowance is derived
    in decoder2d_ref's docstring (|d weight| <= 2^-23 max(H, W) + 2^-24 per axis)."""
    gen = torch.Generator().manual_seed(0)
    for (B, C, H, W), (Ho, Wo) in D.RESIZE_MIRROR_SHAPES:
        x = torch.randn(B, C, H, W, generator=gen).double().requires_grad_(True)
        y = F.interpolate(x, (Ho, Wo), mode="bilinear", align_corners=True)
        g = torch.randn(y.shape, generator=gen).double()
        y.backward(g)
        fwd, _ = R.resize_fwd_ref(x, Ho, Wo)
        bwd, _ = R.resize_bwd_ref(g, H, W)
        tol_f, tol_b = R.mirror_allowance(H, W, Ho, Wo, float(x.detach().abs().max()), float(g.abs().max()))
        ef, eb = float((fwd - y.detach()).abs().max()), float((bwd - x.grad).abs().max())
        print(f"DECODER2D mirror {(B, C, H, W)}->{(Ho, Wo)}: fwd {ef:.3e} <= {tol_f:.3e}, bwd {eb:.3e} <= {tol_b:.3e}")
        assert ef <= tol_f and eb <= tol_b


@pytest.mark.parametrize("bf16", [0, 1], ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape,size,path", D.RESIZE_CL_CASES, ids=D.case_id)
def test_resize_channels_last_per_element(L2d, shape, size, path, bf16):
    """Every branch of mf_upsample_bilinear_cl_bwd (and the forward) per element; a ``tile`` shape runs the direct
    kernel in fp32 (the tile kernel is bf16 only)."""
    D.resize_cl_case(L2d, "cpu", _st, shape, size, bf16, path if bf16 or path != D.TILE else D.DIRECT, what="emul resize")


@pytest.mark.parametrize("bf16", [0, 1], ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape,size", D.RESIZE_CF_CASES, ids=D.case_id)
def test_resize_channels_first_per_element(L2d, shape, size, bf16):
    D.resize_cf_case(L2d, "cpu", _st, shape, size, bf16, what="emul resize cf")


def test_resize_refusals(L2d):
    D.resize_refusal_case(L2d, "cpu", _st)


@pytest.mark.parametrize("bf16", [0, 1], ids=["fp32", "bf16"])
@pytest.mark.parametrize("n,slope", D.PRELU_CASES, ids=D.case_id)
def test_prelu_backward_per_element(L2d, n, slope, bf16):
    D.prelu_bwd_case(L2d, "cpu", _st, n, slope, bf16, what="emul prelu")


@pytest.mark.parametrize("kw", D.BN_CASES, ids=D.case_id)
def test_batchnorm_branches_per_element(L2d, kw):
    D.bn_case(L2d, "cpu", _st, what="emul bn", **kw)
