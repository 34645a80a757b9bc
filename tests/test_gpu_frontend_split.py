"""The 2-D front end of fp32 inference on the MI355X: the stem's max-pool into split form, res2 / res3
as split-bf16 layers, and the whole front with the new path on against off.  The dispatch is forced on whatever the batch table says."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from morefusion_amd.models import backbone2d, ops2d  # noqa: E402
import frontend_split_ref as R  # noqa: E402


@pytest.fixture
def forced(monkeypatch):
    """every group of the dispatch table from one object on"""
    monkeypatch.setattr(backbone2d, "SPLIT_MIN_BATCH", {k: 1 for k in backbone2d.SPLIT_MIN_BATCH})
    monkeypatch.setattr(backbone2d, "CONV_BEFORE_RESIZE_MIN_BATCH", {k: 1 for k in backbone2d.CONV_BEFORE_RESIZE_MIN_BATCH})


@pytest.mark.parametrize("channels_last", [False, True])
@pytest.mark.parametrize("side", [8, 16])
@pytest.mark.parametrize("kind", ["negative", "border"])
def test_maxpool(kind, side, channels_last):
    R.check_maxpool(ops2d, "cuda", kind, side, channels_last)


@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("name", list(R.FRONT_LAYERS))
def test_front_layer_error_bound(name, B):
    R.check_front_layer(ops2d, "cuda", name, B)


def _front(res, psp, rgb, on):
    saved = backbone2d.ResNet18.front_split
    backbone2d.ResNet18.front_split = on
    try:
        with torch.no_grad():
            for _ in range(2):  # (MIOpen's solver choice settles on the first call of a shape)
                feat = res(rgb)
                h32, _ = psp._psp_up1_split(feat)
    finally:
        backbone2d.ResNet18.front_split = saved
    return feat.float().cpu(), h32.cpu()


def test_whole_front_on_vs_off(forced, monkeypatch):
    """ResNet18.forward and _psp_up1_split at B = 4, image side 64: new path on against off within 2e-4 relative;
    the new operator is the one that ran"""
    torch.manual_seed(0)
    torch.backends.cudnn.benchmark = False
    calls = []
    for name in ("maxpool_split",):
        f = getattr(ops2d, name)
        monkeypatch.setattr(ops2d, name, lambda *a, _f=f, _n=name, **k: (calls.append(_n), _f(*a, **k))[1])
    res, psp = backbone2d.ResNet18().cuda().eval(), backbone2d.PSPNetExtractor().cuda().eval()
    rgb = torch.rand(4, 3, 64, 64, device="cuda") * 255
    off = _front(res, psp, rgb, False)
    assert not calls
    on = _front(res, psp, rgb, True)
    assert set(calls) == {"maxpool_split"}
    assert on[0].shape == (4, 512, 8, 8)
    for a, b in zip(on, off):
        lim = 2e-4 * float(b.abs().max())
        print(f"on vs off: max |diff| = {float((a - b).abs().max()):.3e}, limit {lim:.3e}")
        np.testing.assert_allclose(a.numpy(), b.numpy(), rtol=0, atol=lim)


def test_240_pixel_crop_still_takes_miopen(forced, monkeypatch):
    """conv1's side 120 and res5's side 30 are no powers of two: none of the new operators may run, and the result is
    the switch-off result"""
    torch.manual_seed(0)
    torch.backends.cudnn.benchmark = False

    def refuse(*a, **k):
        raise AssertionError("a split-path operator ran on a 240-pixel crop")

    for name in ("maxpool_split", "conv_split"):
        monkeypatch.setattr(ops2d, name, refuse)
    res, psp = backbone2d.ResNet18().cuda().eval(), backbone2d.PSPNetExtractor().cuda().eval()
    rgb = torch.rand(2, 3, 240, 240, device="cuda") * 255
    pix = torch.randint(0, 240 * 240, (2, 50), device="cuda")
    outs = {}
    for on in (False, True):
        saved = backbone2d.ResNet18.front_split
        backbone2d.ResNet18.front_split = on
        try:
            with torch.no_grad():
                for _ in range(2):
                    feat = res(rgb)
                    rows = psp.forward_sampled_rows(feat, pix)
        finally:
            backbone2d.ResNet18.front_split = saved
        outs[on] = (feat.float().cpu(), rows.cpu())
    assert outs[True][0].shape == (2, 512, 30, 30)
    for a, b in zip(outs[True], outs[False]):
        np.testing.assert_allclose(a.numpy(), b.numpy(), rtol=0, atol=1e-6 * float(b.abs().max()))
