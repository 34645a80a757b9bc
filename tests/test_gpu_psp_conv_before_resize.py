"""The decoder's conv-before-resize form on the MI355X: csrc/backbone2d.hip mf_upsample2x_tapsum_fwd,
ops2d.conv_taps_split / upsample_tapsum and the ``PSPNetExtractor.conv_before_resize`` switch.

* the tap-sum resize alone against the float64 masked-tap formula, corners / edges / interior apart;
* the layer pair (1 x 1 tap GEMM at the low resolution + tap-sum resize + PReLU) against the float64 resize -> conv,
  every element within 2^-15 conv(U |x|, |w|);
* ``forward_sampled_rows`` with the switch on and off: 2e-4 absolute (the predict gate); a 240-pixel crop falls back."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from morefusion_amd.models import backbone2d, ops2d  # noqa: E402
from psp_conv_before_resize_ref import check_layer_pair, check_tapsum  # noqa: E402


@pytest.mark.parametrize("side", [2, 4])
def test_tapsum_alone(side):
    check_tapsum(ops2d, "cuda", side)


@pytest.mark.parametrize("signed", [False, True])
@pytest.mark.parametrize("Cin,Cout", [(64, 64), (128, 32)])
@pytest.mark.parametrize("B", [1, 2])
def test_layer_pair(B, Cin, Cout, signed):
    """side 8 -> 16; 9 Cout = 576 / 288: not a multiple of the 128 / 256 tile widths, and (288) with a tile's tail"""
    check_layer_pair(ops2d, "cuda", B, Cin, Cout, signed)


def _rows(psp, feat, pix, on, counts=None):
    saved = backbone2d.PSPNetExtractor.conv_before_resize
    backbone2d.PSPNetExtractor.conv_before_resize = on
    real = ops2d.conv_taps_split

    def counted(*a, **k):
        if counts is not None:
            counts[on] = counts.get(on, 0) + 1
        return real(*a, **k)
    ops2d.conv_taps_split = counted
    try:
        with torch.no_grad():
            return psp.forward_sampled_rows(feat, pix).cpu()
    finally:
        ops2d.conv_taps_split = real
        backbone2d.PSPNetExtractor.conv_before_resize = saved


@pytest.fixture(scope="module")
def psp():
    torch.manual_seed(0)
    torch.backends.cudnn.benchmark = False
    return backbone2d.PSPNetExtractor().cuda().eval()


@pytest.mark.parametrize("B", [1, 4])
def test_switch_on_off_rows_agree(psp, B):
    g = torch.Generator().manual_seed(B)
    feat = torch.relu(torch.randn(B, 512, 32, 32, generator=g)).cuda()
    pix = torch.randint(0, 256 * 256, (B, 100), generator=g).cuda()
    _rows(psp, feat, pix, False)  # (MIOpen's solver choice for the stock layers settles on the first call of a shape)
    counts = {}
    off = _rows(psp, feat, pix, False, counts)
    on = _rows(psp, feat, pix, True, counts)
    assert counts.get(False, 0) == 0
    want = sum(B >= n for n in backbone2d.CONV_BEFORE_RESIZE_MIN_BATCH.values())
    assert counts.get(True, 0) == want, counts
    assert off.shape == on.shape == (B * 100, 32)
    err = float((on - off).abs().max())
    print(f"switch B {B}: max |on - off| = {err:.3e}")
    assert err <= 2e-4, err


def test_crop_240_falls_back(psp):
    """side 30 is no power of two: the MIOpen path whatever the switch says, the new operators never called"""
    g = torch.Generator().manual_seed(3)
    feat = torch.relu(torch.randn(2, 512, 30, 30, generator=g)).cuda()
    pix = torch.randint(0, 240 * 240, (2, 100), generator=g).cuda()
    counts = {}
    _rows(psp, feat, pix, False)  # (MIOpen's solver choice settles on the first call of a shape)
    off = _rows(psp, feat, pix, False, counts)
    on = _rows(psp, feat, pix, True, counts)
    assert counts == {}
    # (the same launches; MIOpen's own run-to-run differences get the allowance of test_gpu_backbone_split_bf16.py's
    # fall-back test)
    assert float((on - off).abs().max()) <= 1e-6 * float(off.abs().max())
