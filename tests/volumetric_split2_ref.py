"""Checks shared by the tests of conv3's occupancy channels on the split-bf16 path: the second
occupancy convolution's split store and mf_conv3d_k4s2_split_fwd at Cin = 16 -- a per-tap K of 48, so one 64-wide
K-tile of the NT engine spans more than one tap.  Run on the GPU (test_gpu_volumetric_split2.py) and on the CPU
emulator (test_emul_volumetric_split2.py): ``L`` is the library, ``dev`` where the operators' tensors live, ``stream``
what the entry points get as their stream; references are CPU float64."""
import torch
import torch.nn.functional as F

CIN, COUT, D, W_CIN, C_OFF = 16, 256, 8, 160, 144   # conv3's slice: input channels 144 .. 159 of 160
MODE_CONV3_SPLIT = 4                                # kConvFwdS of mf_gemm_bf16_nt_plan

# tile forms of the NT engine: the MF_* knobs that force them at these small shapes, and the tile that must have run
FORMS = {
    "tile64": ({"MF_NT_BIG": "0"}, 64),
    "tile128": ({"MF_NT_BIG": "0", "MF_NT_HALF_MAX": "0"}, 128),
    "tile256": ({"MF_NT_BIG": "2"}, 256),
    "tile256_splitk2": ({"MF_NT_BIG": "2", "MF_NT_SPLITK": "2"}, 256),
}


def P(t):
    return None if t is None else t.data_ptr()


def split(x):
    """fp32 [..., C] -> bf16 [..., 2C] (hi | lo), torch restatement of the split"""
    hi = x.to(torch.bfloat16)
    return torch.cat([hi, (x - hi.float()).to(torch.bfloat16)], dim=-1).contiguous()


def bits(t):
    return t.contiguous().cpu().view(torch.int16)


def lib_split(L, x, stream):
    """mf_split_bf16 of fp32 rows [..., C] -> [..., 2C] bf16 (hi | lo)"""
    C = x.shape[-1]
    rows = x.reshape(-1, C).contiguous()
    out = torch.empty((rows.shape[0], 2 * C), dtype=torch.bfloat16, device=x.device)
    assert L.mf_split_bf16(P(rows), 0, 1, 0, C, 1, C, 1, rows.shape[0], P(out), 2 * C, C, stream) == 0
    return out.reshape(*x.shape[:-1], 2 * C)


# ---- the producer: conv2_occ's split store -------------------------------------------------------------------------
def occupancy_problem(B, Dg, seed=3):
    g = torch.Generator().manual_seed(seed)
    grid = (torch.rand(B, Dg, Dg, Dg, generator=g) < 0.4).float()
    W1 = torch.rand(8, 1, 3, 3, 3, generator=g) - 0.5
    W2 = (torch.rand(16, 8, 3, 3, 3, generator=g) - 0.5) * 0.6
    b1, b2 = (torch.rand(8, generator=g) - 0.5) * 0.2, (torch.rand(16, generator=g) - 0.5) * 0.2
    w1 = W1.permute(2, 3, 4, 1, 0).contiguous().reshape(27, 1, 8)
    w2 = W2.permute(2, 3, 4, 1, 0).contiguous().reshape(27, 8, 16)
    return grid, w1, b1, w2, b2


def check_occupancy_split_store(L, dev, stream, B=2, Dg=6):
    """h2s is mf_split_bf16 of the fp32 h2 of mf_occupancy_convs_fwd, bit for bit; the fp32 store beside it is that
    h2; without the fp32 store the split form is the same."""
    grid, w1, b1, w2, b2 = (t.to(dev) for t in occupancy_problem(B, Dg))
    n = B * Dg ** 3
    h1 = torch.empty(n, 8, device=dev)
    h2 = torch.full((n, 16), 7.0, device=dev)
    assert L.mf_occupancy_convs_fwd(P(grid), P(w1), P(b1), P(w2), P(b2), P(h1), P(h2), B, Dg, stream) == 0
    want = lib_split(L, h2, stream)
    assert torch.equal(bits(want), bits(split(h2)))
    for with32 in (True, False):
        g2 = torch.full((n, 16), 7.0, device=dev)
        h2s = torch.full((n, 32), 3.0, dtype=torch.bfloat16, device=dev)
        assert L.mf_occupancy_convs_split_fwd(P(grid), P(w1), P(b1), P(w2), P(b2), P(h1), P(g2) if with32 else None,
                                              P(h2s), B, Dg, stream) == 0
        assert torch.equal(bits(h2s), bits(want))
        assert torch.equal(g2.cpu(), h2.cpu() if with32 else torch.full((n, 16), 7.0))
    assert float((h2 > 0).float().mean()) > 0.2 and float((want[:, 16:].float() != 0).float().mean()) > 0.2
    assert L.mf_occupancy_convs_split_fwd(P(grid), P(w1), P(b1), P(w2), P(b2), P(h1), P(h2), None, B, Dg, stream) != 0


# ---- the GEMM: |y - y_fp64| <= 2^-15 conv(|x|, |w|)_fp64 per element -----------------------------------------------
def conv3_occ_problem(B, seed=11):
    """x >= 0 (the occupancy branch ends in a ReLU), half of it zero, with every corner voxel and every edge of the
    grid set well away from zero: the padding taps' masks and the K-tiles that span two taps meet real data there."""
    g = torch.Generator().manual_seed(seed + B)
    x = torch.relu(torch.randn(B, CIN, D, D, D, generator=g))
    e = torch.zeros(D, dtype=torch.bool)
    e[0] = e[-1] = True
    on_edge = (e[:, None, None] & e[None, :, None]) | (e[:, None, None] & e[None, None, :]) | (e[None, :, None] & e[None, None, :])
    x[:, :, on_edge] += 2.0 + torch.rand(B, CIN, int(on_edge.sum()), generator=g)
    W = torch.randn(COUT, W_CIN, 4, 4, 4, generator=g) / (CIN * 64) ** 0.5
    return x, W


def pack(L, W, dev, stream):
    wp = torch.empty((COUT, 64, 3 * CIN), dtype=torch.bfloat16, device=dev)
    Wd = W.to(dev).contiguous()
    assert L.mf_conv3d_k4s2_split_pack(P(Wd), COUT, CIN, W_CIN, C_OFF, P(wp), stream) == 0
    return wp


def run_conv3_occ(L, dev, stream, x, wp, expect_tile, expect_ws):
    """x [B][CIN][D]^3 fp32 (CPU) -> dense fp32 [B][(D/2)^3][COUT] (CPU): no bias, no activation, as the layer runs"""
    B = x.shape[0]
    xs = split(x.permute(0, 2, 3, 4, 1).reshape(B, D ** 3, CIN)).to(dev)
    nws = L.mf_conv3d_k4s2_split_workspace_bytes(B, CIN, COUT, D)
    assert (nws > 0) == expect_ws, nws
    ws = torch.empty(max(nws, 16), dtype=torch.uint8, device=dev)
    out = torch.full((B, (D // 2) ** 3, COUT), 9.0, device=dev)
    assert L.mf_conv3d_k4s2_split_fwd(P(xs), P(wp), None, 0, P(out), COUT, None, 0, 0, P(ws), nws, B, CIN, COUT, D,
                                      stream) == 0
    out = out.cpu()
    assert L.mf_gemm_bf16_last_tile() == expect_tile, (L.mf_gemm_bf16_last_tile(), expect_tile)
    return out


def check_conv3_occ_bound(L, dev, stream, form, B):
    """the per-element contract against float64 on the same fp32 inputs; a second run gives the same bits"""
    tile = FORMS[form][1]
    x, W = conv3_occ_problem(B)
    wp = pack(L, W, dev, stream)
    y = run_conv3_occ(L, dev, stream, x, wp, tile, form.endswith("splitk2"))
    w64 = W[:, C_OFF:C_OFF + CIN].double()
    to_rows = lambda t: t.permute(0, 2, 3, 4, 1).reshape(B, (D // 2) ** 3, COUT)  # noqa: E731
    ref = to_rows(F.conv3d(x.double(), w64, None, 2, 1))
    lim = 2.0 ** -15 * to_rows(F.conv3d(x.double().abs(), w64.abs(), None, 2, 1)) + 1e-30
    ratio = float(((y.double() - ref).abs() / lim).max())
    print(f"conv3_occ {form} B {B}: max err / bound = {ratio:.3f}")
    assert ratio <= 1.0, (form, B, ratio)
    assert torch.equal(y, run_conv3_occ(L, dev, stream, x, wp, tile, form.endswith("splitk2")))


def check_single_voxel_single_tap(L, dev, stream, form):
    """One non-zero voxel, one non-zero weight tap.  Input voxel (3, 0, 6) of object 1, channel 5, value 1.5; weight
    0.75 at output channel 200, input channel C_OFF + 5, tap (kx, ky, kz) = (2, 1, 1).  With k4 s2 p1 the input
    coordinate of output o and tap k is 2 o - 1 + k per axis, so the only output that sees the voxel through that tap
    is o = ((3 + 1 - 2) / 2, (0 + 1 - 1) / 2, (6 + 1 - 1) / 2) = (1, 0, 3): row (1 * 4 + 0) * 4 + 3 = 19 of object 1.
    1.5 and 0.75 are bf16 numbers: the product 1.125 is exact and everything else is exactly zero."""
    B = 2
    x = torch.zeros(B, CIN, D, D, D)
    x[1, 5, 3, 0, 6] = 1.5
    W = torch.zeros(COUT, W_CIN, 4, 4, 4)
    W[200, C_OFF + 5, 2, 1, 1] = 0.75
    W[200, 5, 2, 1, 1] = 4.0   # (outside the packed slice: must not be seen)
    y = run_conv3_occ(L, dev, stream, x, pack(L, W, dev, stream), FORMS[form][1], form.endswith("splitk2"))
    want = torch.zeros(B, (D // 2) ** 3, COUT)
    want[1, 19, 200] = 1.125
    assert torch.equal(y, want), (y - want).abs().nonzero()[:8]
