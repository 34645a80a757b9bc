"""The identity behind the decoder's conv-before-resize form, in float64 on the CPU:

    conv3x3(U x)(p) = bias + sum_t m_t(p) (U (W_t x))(p + d_t)

U the x2 bilinear resize (align_corners), W_t tap t's [Cout, Cin] matrix applied at the LOW resolution, m_t the zero
padding of the convolution on the up-sampled map.  Pins the border mask and the tap order (t = ky 3 + kx, rows
t Cout + co) that the kernel and the weight pack follow."""
import pytest
import torch

from psp_conv_before_resize_ref import masked_tap_sum, regions, resize_conv, tap_maps

CIN, COUT = 3, 2


def _check(x, w, bias):
    want = resize_conv(x, w, bias)
    got = masked_tap_sum(tap_maps(x, w)) + bias[None, :, None, None]
    scale = float(want.abs().max())
    assert scale > 0
    for name, m in regions(want.shape[2], want.shape[3]).items():
        if bool(m.any()):
            err = float((got - want)[:, :, m].abs().max())
            assert err <= 1e-12 * scale, (name, err, scale)


@pytest.mark.parametrize("side", [2, 4])
def test_identity_random_signed(side):
    g = torch.Generator().manual_seed(side)
    x = torch.randn(2, CIN, side, side, generator=g, dtype=torch.float64)
    w = torch.randn(COUT, CIN, 3, 3, generator=g, dtype=torch.float64)
    bias = torch.randn(COUT, generator=g, dtype=torch.float64)
    _check(x, w, bias)


@pytest.mark.parametrize("side", [2, 4])
@pytest.mark.parametrize("corner", [(0, 0), (0, -1), (-1, 0), (-1, -1)])
def test_identity_single_corner_pixel(side, corner):
    """only a corner pixel is non-zero: every output it reaches sits at the border, where a wrong mask (taps clipped
    on the low-resolution map, or not clipped at all) changes the sum"""
    g = torch.Generator().manual_seed(11)
    x = torch.zeros(1, CIN, side, side, dtype=torch.float64)
    x[0, :, corner[0], corner[1]] = torch.randn(CIN, generator=g, dtype=torch.float64)
    w = torch.randn(COUT, CIN, 3, 3, generator=g, dtype=torch.float64)
    bias = torch.randn(COUT, generator=g, dtype=torch.float64)
    _check(x, w, bias)


def test_unmasked_sum_differs_at_the_border():
    """the mask matters: padding the LOW-resolution tap maps by replication (what an unmasked gather would read)
    changes border outputs and leaves the interior alone"""
    g = torch.Generator().manual_seed(5)
    x = torch.randn(1, CIN, 4, 4, generator=g, dtype=torch.float64)
    w = torch.randn(COUT, CIN, 3, 3, generator=g, dtype=torch.float64)
    want = resize_conv(x, w)
    import torch.nn.functional as F
    from psp_conv_before_resize_ref import resize2x
    z = tap_maps(x, w)
    wrong = torch.zeros_like(want)
    for t in range(9):
        ky, kx = divmod(t, 3)
        u = F.pad(resize2x(z[:, t]), (1, 1, 1, 1), mode="replicate")
        wrong = wrong + u[:, :, ky:ky + 8, kx:kx + 8]
    r = regions(8, 8)
    assert float((wrong - want)[:, :, r["interior"]].abs().max()) <= 1e-12 * float(want.abs().max())
    assert float((wrong - want)[:, :, r["corners"]].abs().max()) > 1e-3
