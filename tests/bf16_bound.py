"""TEST INFRASTRUCTURE: float64 references and the per-element error bound of the bf16 engines (csrc/gemm_bf16.hip).

The kernels take bf16 operands, form products of two bf16 (exact in fp32), accumulate in fp32 in whatever order their
tiling gives, add an fp32 bias, apply the ReLU and round ONCE to the output type.  For the reference ``ref`` of the
same contraction in float64 on the same bf16-rounded operands and ``S = sum |a_i| |w_i| (+ |bias|)`` (the contraction
on absolute values), a sum of K terms accumulated in fp32 (unit roundoff 2^-24) in ANY order obeys
``|fl(sum) - sum| <= (K - 1) 2^-24 S`` to first order; twice that leaves room for the second-order terms and for
an accumulator that truncates instead of rounding:

    fp32 output   |got - ref| <= 2 K 2^-24 S
    bf16 output   |got - ref| <= 2^-8 |ref| + 2 K 2^-24 S        (round to nearest, 8 significant bits)

The ReLU is 1-Lipschitz and applied before the rounding, so both hold behind it.  K is the reduction length: taps x
input channels (+ 1 for a bias), the rows of a weight gradient (+ the number of slabs of a split reduction).  Nothing
here is fitted to what a kernel returns; a case over the bound is a finding about the kernel.
"""
import torch
import torch.nn.functional as F

U32 = 2.0 ** -24
U16 = 2.0 ** -8

RATIOS = {}   # what -> worst |got - ref| / bound of the checks made in this process (reporting only)


def worst(got, ref, S, K, out_bf16=None):
    """-> (ratio, index, err, bound, max-norm error) of the element with the largest |got - ref| / bound."""
    if out_bf16 is None:
        out_bf16 = got.dtype == torch.bfloat16
    g = got.detach().double().cpu()
    ref, S = ref.detach().double().cpu(), S.detach().double().cpu()
    assert g.shape == ref.shape == S.shape, (g.shape, ref.shape, S.shape)
    assert bool(torch.isfinite(g).all()), "non-finite output"
    bnd = 2.0 * K * U32 * S + (U16 * ref.abs() if out_bf16 else 0.0)
    err = (g - ref).abs()
    # an element whose bound is 0 (every product zero) must be exact
    ratio = torch.where(bnd > 0, err / bnd.clamp(min=1e-300), torch.where(err > 0, torch.full_like(err, float("inf")),
                                                                          torch.zeros_like(err)))
    i = int(ratio.argmax())
    idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(i), ratio.shape))
    maxnorm = float(err.max() / ref.abs().max().clamp(min=1e-300))
    return float(ratio.flatten()[i]), idx, float(err.flatten()[i]), float(bnd.flatten()[i]), maxnorm


def assert_within(got, ref, S, K, what, out_bf16=None):
    """Every element of ``got`` within the bound of ``ref``; prints the worst one before it asserts."""
    ratio, idx, err, bnd, maxnorm = worst(got, ref, S, K, out_bf16)
    RATIOS[what] = max(RATIOS.get(what, 0.0), ratio)
    print(f"BF16BOUND {what}: worst |got-ref|/bound = {ratio:.3f} at {idx} (err {err:.3e}, bound {bnd:.3e}, "
          f"K = {K}), max-norm error {maxnorm:.2e}")
    assert ratio <= 1.0, (what, ratio, idx, err, bnd)
    return ratio


def linear_ref(A, W, bias=None):
    """A [M, K], W [N, K] (bf16 values), bias [N] -> (ref, S) float64 [M, N]."""
    A, W = A.detach().double().cpu(), W.detach().double().cpu()
    ref, S = A @ W.t(), A.abs() @ W.abs().t()
    if bias is not None:
        b = bias.detach().double().cpu()
        ref, S = ref + b, S + b.abs()
    return ref, S


def wgrad_ref(dY, A):
    """dW[n][k] = sum_m dY[m][n] A[m][k] -> (ref, S) float64 [N, K]."""
    dY, A = dY.detach().double().cpu(), A.detach().double().cpu()
    return dY.t() @ A, dY.abs().t() @ A.abs()


def _cf(t_cl, B, D, C):
    return t_cl.detach().double().cpu().reshape(B, D, D, D, C).permute(0, 4, 1, 2, 3).contiguous()


def _cl(t_cf):
    B, C = t_cf.shape[:2]
    return t_cf.permute(0, 2, 3, 4, 1).reshape(B, -1, C)


def conv_out_size(D, ks, stride, pad, dil):
    return (D + 2 * pad - dil * (ks - 1) - 1) // stride + 1


def conv_ref(x_cl, W, bias, D, geom, dz_cl=None, want_dx=True):
    """Convolution3D on a channels-last grid in float64, with its gradients.  x_cl [B, D^3, Cin] and W
    [Cout, Cin, ks, ks, ks] hold bf16 VALUES (any dtype), bias fp32 or None, geom = (ks, stride, pad, dil), dz_cl
    [B, Do^3, Cout] the gradient of the pre-activation (already masked).  -> dict of channels-last float64 tensors:
    y, Sy (pre-activation and its absolute-value contraction) and, with dz_cl, dw, Sdw [Cout, Cin, ks, ks, ks] and dx,
    Sdx [B, D^3, Cin].  The S of a gradient is the same autograd pass on absolute values (the gradients are linear
    in each operand, so that pass IS the contraction of the absolute values)."""
    ks, stride, pad, dil = geom
    B, _, Cin = x_cl.shape
    Cout = W.shape[0]
    Do = conv_out_size(D, ks, stride, pad, dil)
    res = {}
    for tag, f in (("", lambda t: t), ("S", torch.abs)):
        x = f(_cf(x_cl, B, D, Cin)).requires_grad_(True)
        w = f(W.detach().double().cpu()).requires_grad_(True)
        y = F.conv3d(x, w, None, stride=stride, padding=pad, dilation=dil)
        if dz_cl is not None:
            gz = f(_cf(dz_cl, B, Do, Cout))
            gx, gw = torch.autograd.grad(y, (x, w), gz) if want_dx else (None,) + torch.autograd.grad(y, (w,), gz)
            res[tag + "dw"] = gw
            if want_dx:
                res[tag + "dx"] = _cl(gx)
        y = y.detach()
        if bias is not None:
            y = y + f(bias.detach().double().cpu()).reshape(1, -1, 1, 1, 1)
        res[tag + "y"] = _cl(y)
    return res


def relu_mask_agrees(got, y_pre, Sy, K, what):
    """The operator's ReLU mask (``got > 0``, got bf16) may differ from the reference's (``y_pre > 0``) only where the
    reference pre-activation is within its own bound of zero."""
    g = got.detach().double().cpu()
    bnd = 2.0 * K * U32 * Sy + U16 * y_pre.abs()
    diff = (g > 0) != (y_pre > 0)
    bad = diff & (y_pre.abs() > bnd)
    print(f"BF16BOUND {what}: ReLU mask differs on {int(diff.sum())} of {diff.numel()} elements, "
          f"{int(bad.sum())} of them beyond the bound")
    assert not bool(bad.any()), what
    return g > 0
