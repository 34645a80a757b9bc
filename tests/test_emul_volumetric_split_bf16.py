"""The split-bf16 forms of the volumetric part's fp32 layers on the CPU (fiber emulator, lane-exact
v_mfma_f32_32x32x16_bf16): csrc/gemm_bf16.hip's 3-D convolution and rows modes on split operands
(mf_conv3d_k4s2_split_*, mf_linear_split_*), and the producers that write split form (sparse conv3's reduce, the
trilinear sampler).

The GEMMs are checked against float64 results on the SAME hi / lo-rounded operands (hi hi + lo hi + hi lo): every bf16
product is exact in fp32, so only the summation order differs (1e-4 of the largest output, as
test_emul_conv2d_split_bf16.py).  Weight packs and the producers' split outputs are bit-exact against a NumPy
restatement."""

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from host_emul import emul

pytestmark = pytest.mark.skipif(not emul.available(), reason="g++ not available")


@pytest.fixture(scope="module")
def L():
    return emul.build(["gemm_bf16.hip", "backbone2d.hip"])


@pytest.fixture(params=["tile128", "tile256"])
def tile(request, monkeypatch):
    """The 128 x 128 tile of the NT engine, and with MF_NT_BIG=2 the 256 x 256 ping-pong form wherever it fits."""
    monkeypatch.setenv("MF_NT_BIG", "2" if request.param == "tile256" else "0")
    return request.param


def p(t):
    return None if t is None else t.data_ptr()


def rne(x):
    """float32 array -> bf16 bit patterns (uint16), round to nearest even (NumPy restatement of mf::bf16_bits)."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def bf_float(bits):
    return (bits.astype(np.uint32) << 16).view(np.float32)


def split_np(x):
    """(hi, lo) bit patterns of float32 x: hi = bf16(x), lo = bf16(x - hi)."""
    x = np.asarray(x, np.float32)
    hi = rne(x)
    return hi, rne((x - bf_float(hi)).astype(np.float32))


def to_bf16_tensor(bits):
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).view(torch.bfloat16)


def bits_of(t):
    return t.contiguous().view(torch.int16).numpy().view(np.uint16)


def hi_lo(t):
    hi, lo = split_np(t.numpy())
    return torch.from_numpy(bf_float(hi).astype(np.float64)), torch.from_numpy(bf_float(lo).astype(np.float64))


def close(got, want, tol=1e-4):
    scale = float(want.abs().max()) or 1.0
    err = float((got.double() - want.double()).abs().max())
    assert err <= tol * scale, (err, scale)


def split_rows(x, ld=None, off=0):
    """fp32 rows [M][K] -> split rows [M][ld] bf16: hi at off + k, lo at off + K + k (other columns 3.0)"""
    M, K = x.shape
    hi, lo = split_np(x.numpy())
    ld = ld or 2 * K
    out = np.full((M, ld), rne(np.float32(3.0)), np.uint16)
    out[:, off:off + K] = hi
    out[:, off + K:off + 2 * K] = lo
    return to_bf16_tensor(out)


def assert_split_of(spl_bits, v32, hi_off, lo_off):
    """The split output equals the split of the fp32 output, bit for bit."""
    N = v32.shape[-1]
    hi, lo = split_np(v32.numpy())
    assert np.array_equal(spl_bits[..., hi_off:hi_off + N], hi) and np.array_equal(spl_bits[..., lo_off:lo_off + N], lo)


# ---- weight packs ---------------------------------------------------------------------------------------------------
def test_conv3d_pack_bit_exact(L):
    rng = np.random.default_rng(0)
    Cout, w_cin, Cin, c_off = 24, 40, 16, 8
    W = (rng.standard_normal((Cout, w_cin, 4, 4, 4)) * 0.1).astype(np.float32)
    wp = torch.empty(Cout, 64, 3 * Cin, dtype=torch.bfloat16)
    assert L.mf_conv3d_k4s2_split_pack(p(torch.from_numpy(W)), Cout, Cin, w_cin, c_off, p(wp), None) == 0
    Wt = np.ascontiguousarray(W[:, c_off:c_off + Cin].reshape(Cout, Cin, 64).transpose(0, 2, 1))  # [Cout][tap][Cin]
    hi, lo = split_np(Wt)
    assert np.array_equal(bits_of(wp), np.concatenate([hi, hi, lo], axis=2))
    assert L.mf_conv3d_k4s2_split_pack(p(torch.from_numpy(W)), Cout, Cin, w_cin, 32, p(wp), None) != 0  # past w_cin


def test_rows_pack_bit_exact(L):
    rng = np.random.default_rng(1)
    G, N, K, Np, Kp, ldw = 2, 20, 984, 128, 992, 1000
    W = (rng.standard_normal((G, N, ldw)) * 0.1).astype(np.float32)
    wp = torch.full((G, Np, 3 * Kp), 5.0, dtype=torch.bfloat16)
    assert L.mf_linear_split_pack(p(torch.from_numpy(W)), N * ldw, ldw, N, K, Np, Kp, G, p(wp), None) == 0
    Wz = np.zeros((G, Np, Kp), np.float32)
    Wz[:, :N, :K] = W[:, :, :K]
    hi, lo = split_np(Wz)
    assert np.array_equal(bits_of(wp), np.concatenate([hi, hi, lo], axis=2))
    assert L.mf_linear_split_pack(p(torch.from_numpy(W)), N * ldw, ldw, N, K, Np, 990, G, p(wp), None) != 0


# ---- 3-D convolution (k4 s2 p1) on split operands ----------------------------------------------------------------------
def conv3_ref(x_cf, W):
    xh, xl = hi_lo(x_cf)
    wh, wl = hi_lo(W)
    c = lambda a, b: F.conv3d(a, b, stride=2, padding=1)  # noqa: E731
    return (c(xh, wh) + c(xl, wh) + c(xh, wl)).permute(0, 2, 3, 4, 1)   # [B][Do][Do][Do][Cout]


def split_grid(x_cf):
    """[B][C][D][D][D] float32 -> the split operand [B][D^3][2C]"""
    hi, lo = split_np(x_cf.permute(0, 2, 3, 4, 1).contiguous().numpy())
    B, C = x_cf.shape[0], x_cf.shape[1]
    return to_bf16_tensor(np.concatenate([hi, lo], axis=4).reshape(B, -1, 2 * C))


def conv3_problem(geom, seed):
    B, Cin, Cout, D = geom
    torch.manual_seed(seed)
    x = torch.randn(B, Cin, D, D, D)
    W = torch.randn(Cout, Cin, 4, 4, 4) / (Cin * 64) ** 0.5
    bias = torch.randn(Cout) * 0.3
    return x, W, bias


def conv3_pack(L, W):
    Cout, Cin = W.shape[0], W.shape[1]
    wp = torch.empty(Cout, 64, 3 * Cin, dtype=torch.bfloat16)
    assert L.mf_conv3d_k4s2_split_pack(p(W), Cout, Cin, Cin, 0, p(wp), None) == 0
    return wp


CONV3 = [(1, 16, 24, 8), (2, 24, 16, 4), (1, 8, 136, 8)]   # 3 Cin = 72: K-tiles straddle hi / lo / hi and the taps


@pytest.mark.parametrize("geom", CONV3)
def test_conv3d_split_forward(L, tile, geom):
    """relu(conv + bias): an fp32 output and a split output at a column offset / pitch, alone and together."""
    B, Cin, Cout, D = geom
    x, W, bias = conv3_problem(geom, 3)
    want = F.relu(conv3_ref(x, W) + bias.double()).reshape(B, -1, Cout)
    xs, wp = split_grid(x), conv3_pack(L, W)
    M = B * (D // 2) ** 3
    for o32, osp in ((1, 0), (1, 1), (0, 1)):
        out = torch.full((M, Cout + 8), 9.0)
        ldos, los, soff = 2 * Cout + 32, Cout + 8, 8
        spl = torch.full((M, ldos), 3.0, dtype=torch.bfloat16)
        assert L.mf_conv3d_k4s2_split_fwd(p(xs), p(wp), p(bias), 1, p(out[:, 8:]) if o32 else None, Cout + 8,
                                          p(spl[:, soff:]) if osp else None, ldos, los, None, 0, B, Cin, Cout, D,
                                          None) == 0
        if o32:
            close(out[:, 8:], want.reshape(M, Cout))
            assert float((out[:, :8] - 9).abs().max()) == 0
        if osp:
            hi, lo = spl[:, soff:soff + Cout].double(), spl[:, soff + los:soff + los + Cout].double()
            close(hi + lo, want.reshape(M, Cout))
            keep = torch.ones(ldos, dtype=torch.bool)
            keep[soff:soff + Cout] = False
            keep[soff + los:soff + los + Cout] = False
            assert float((spl[:, keep].float() - 3).abs().max()) == 0
        if o32 and osp:
            assert_split_of(bits_of(spl), out[:, 8:].contiguous(), soff, soff + los)
    # no bias, no ReLU
    out = torch.empty(M, Cout)
    assert L.mf_conv3d_k4s2_split_fwd(p(xs), p(wp), None, 0, p(out), Cout, None, 0, 0, None, 0, B, Cin, Cout, D, None) == 0
    close(out, conv3_ref(x, W).reshape(M, Cout))


def test_conv3d_split_splitk(L, monkeypatch):
    """The reduction over fp32 slabs (forced: MF_NT_SPLITK=3 on the 256 x 256 form): the finish pass adds the slabs in
    order and runs the same epilogue once -- bias + ReLU, both outputs; two runs give the same bits."""
    monkeypatch.setenv("MF_NT_BIG", "2")
    monkeypatch.setenv("MF_NT_SPLITK", "3")
    geom = (1, 8, 192, 8)
    B, Cin, Cout, D = geom
    x, W, bias = conv3_problem(geom, 5)
    want = F.relu(conv3_ref(x, W) + bias.double()).reshape(-1, Cout)
    M = B * (D // 2) ** 3
    nws = L.mf_conv3d_k4s2_split_workspace_bytes(B, Cin, Cout, D)
    assert nws == 3 * M * Cout * 4
    xs, wp = split_grid(x), conv3_pack(L, W)
    runs = []
    for _ in range(2):
        ws = torch.empty(nws, dtype=torch.uint8)
        out = torch.empty(M, Cout)
        spl = torch.empty(M, 2 * Cout, dtype=torch.bfloat16)
        assert L.mf_conv3d_k4s2_split_fwd(p(xs), p(wp), p(bias), 1, p(out), Cout, p(spl), 2 * Cout, Cout, p(ws), nws,
                                          B, Cin, Cout, D, None) == 0
        close(out, want)
        assert float(out.min()) == 0.0   # ReLU acted
        assert_split_of(bits_of(spl), out, 0, Cout)
        runs.append(out)
    assert torch.equal(runs[0], runs[1])


def test_conv3d_split_rejects(L):
    B, Cin, Cout, D = 1, 16, 16, 8
    xs = torch.zeros(B, D ** 3, 2 * Cin, dtype=torch.bfloat16)
    wp = torch.zeros(Cout, 64, 3 * Cin, dtype=torch.bfloat16)
    out = torch.zeros(B * 64, Cout)
    ok = dict(xs=p(xs), wp=p(wp), bias=None, relu=0, out32=p(out), ldo32=Cout, outs=None, ldos=0, los=0, ws=None, nws=0,
              B=B, Cin=Cin, Cout=Cout, D=D, st=None)
    assert L.mf_conv3d_k4s2_split_fwd(*ok.values()) == 0
    for k, v in (("out32", None), ("ldo32", 12), ("Cin", 12), ("D", 12), ("Cout", 12)):
        args = dict(ok)
        args[k] = v
        assert L.mf_conv3d_k4s2_split_fwd(*args.values()) != 0, k


# ---- rows (per-point 1x1 convolutions) on split operands ---------------------------------------------------------------
def rows_ref(x, W):
    xh, xl = hi_lo(x)
    wh, wl = hi_lo(W)
    return xh @ wh.T + xl @ wh.T + xh @ wl.T


def rows_pack(L, W, Kp):
    N, K = W.shape
    Np = -(-N // 128) * 128
    wp = torch.empty(Np, 3 * Kp, dtype=torch.bfloat16)
    assert L.mf_linear_split_pack(p(W), 0, K, N, K, Np, Kp, 1, p(wp), None) == 0
    return wp


ROWS = [  # M (ragged last row tile), N, K, Kp
    (200, 40, 984, 992),   # the heads' K padding 984 -> 992
    (130, 136, 40, 48),    # 3 Kp = 144: K-tiles straddle the segments; a second, ragged column tile
    (300, 24, 64, 64),
]


@pytest.mark.parametrize("M,N,K,Kp", ROWS)
def test_linear_split_forward(L, tile, M, N, K, Kp):
    torch.manual_seed(7)
    x = torch.randn(M, K)
    W = torch.randn(N, K) / K ** 0.5
    bias = torch.randn(N) * 0.3
    xp = torch.zeros(M, Kp)
    xp[:, :K] = x
    lda = 2 * Kp + 16
    As = split_rows(xp, lda, 8)[:, 8:]   # a column block of wider rows
    wp = rows_pack(L, W, Kp)
    want = F.relu(rows_ref(x, W) + bias.double())
    out = torch.full((M, N + 8), 9.0)
    ldos, los = 2 * N + 16, N + 8
    spl = torch.full((M, ldos), 3.0, dtype=torch.bfloat16)
    assert L.mf_linear_split_fwd(p(As), lda, p(wp), p(bias), 1, p(out), N + 8, p(spl), ldos, los, None, 0, M, N, Kp,
                                 None) == 0
    close(out[:, :N], want)
    assert float((out[:, N:] - 9).abs().max()) == 0 and float(out[:, :N].min()) == 0.0
    assert_split_of(bits_of(spl), out[:, :N].contiguous(), 0, los)
    assert float((spl[:, N:los].float() - 3).abs().max()) == 0 and float((spl[:, los + N:].float() - 3).abs().max()) == 0
    # no bias, no ReLU, the split output alone
    spl2 = torch.empty(M, 2 * N, dtype=torch.bfloat16)
    assert L.mf_linear_split_fwd(p(As), lda, p(wp), None, 0, None, 0, p(spl2), 2 * N, N, None, 0, M, N, Kp, None) == 0
    close(spl2[:, :N].double() + spl2[:, N:].double(), rows_ref(x, W))


def test_linear_split_splitk(L, monkeypatch):
    monkeypatch.setenv("MF_NT_BIG", "2")
    monkeypatch.setenv("MF_NT_SPLITK", "3")
    M, N, K, Kp = 300, 192, 120, 128
    torch.manual_seed(9)
    x = torch.randn(M, K)
    W = torch.randn(N, K) / K ** 0.5
    bias = torch.randn(N) * 0.3
    xp = torch.zeros(M, Kp)
    xp[:, :K] = x
    As, wp = split_rows(xp), rows_pack(L, W, Kp)
    nws = L.mf_linear_split_workspace_bytes(M, N, Kp)
    assert nws == 3 * M * N * 4
    want = F.relu(rows_ref(x, W) + bias.double())
    runs = []
    for _ in range(2):
        ws = torch.empty(nws, dtype=torch.uint8)
        out = torch.empty(M, N)
        spl = torch.empty(M, 2 * N, dtype=torch.bfloat16)
        assert L.mf_linear_split_fwd(p(As), 2 * Kp, p(wp), p(bias), 1, p(out), N, p(spl), 2 * N, N, p(ws), nws, M, N, Kp,
                                     None) == 0
        close(out, want)
        assert float(out.min()) == 0.0
        assert_split_of(bits_of(spl), out, 0, N)
        runs.append(out)
    assert torch.equal(runs[0], runs[1])


def test_linear_split_rejects(L):
    M, N, Kp = 8, 16, 16
    As = torch.zeros(M, 2 * Kp, dtype=torch.bfloat16)
    wp = torch.zeros(128, 3 * Kp, dtype=torch.bfloat16)
    out = torch.zeros(M, N)
    ok = dict(As=p(As), lda=2 * Kp, wp=p(wp), bias=None, relu=0, out32=p(out), ldo32=N, outs=None, ldos=0, los=0, ws=None,
              nws=0, M=M, N=N, Kp=Kp, st=None)
    assert L.mf_linear_split_fwd(*ok.values()) == 0
    for k, v in (("out32", None), ("lda", Kp), ("N", 12), ("Kp", 12), ("ldo32", 8)):
        args = dict(ok)
        args[k] = v
        assert L.mf_linear_split_fwd(*args.values()) != 0, k


# ---- producers that write split form -------------------------------------------------------------------------------
def test_reduce_and_sampler_split_outputs_bit_exact():
    """Sparse conv3's channels-last reduce writes the split of its own fp32 output; the sampler's split form is the
    split of what its fp32 form writes (columns at an offset of wider rows, neighbours untouched)."""
    lib = emul.build(["sparseconv.hip", "interp.hip"])
    rs = np.random.RandomState(11)
    B, Cs, Cout, D, n, ld = 2, 8, 256, 8, 90, 20
    points = rs.uniform(-0.6, D - 0.4, (n, 3)).astype(np.float32)
    wide = rs.uniform(-1, 1, (n, ld)).astype(np.float32)
    bi = np.sort(rs.randint(0, B, n)).astype(np.int32)
    W = (rs.uniform(-1, 1, (Cout, Cs, 4, 4, 4)) * 0.2).astype(np.float32)
    bias = rs.uniform(-0.1, 0.1, Cout).astype(np.float32)
    Do = D // 2
    dense = rs.uniform(-0.1, 0.1, (B, Do ** 3, Cout)).astype(np.float32)
    Wp = np.zeros(8 * Cs * 8 * Cout, np.float32)
    assert lib.mf_sparse_conv3d_pack_weights(W.ctypes.data, Cout, Cs, Cs, 0, Wp.ctypes.data, None) == 0
    ws = np.zeros(int(lib.mf_sparse_conv3d_workspace_bytes(B, Cs, Cout, D, n, n)) // 4 + 64, np.float32)
    args = (wide[:, 4:].ctypes.data, ld, points.ctypes.data, bi.ctypes.data, n, 0.0, 0.0, 0.0, 1.0, Wp.ctypes.data,
            dense.ctypes.data, bias.ctypes.data)
    ref = np.full(dense.shape, 7.0, np.float32)
    assert lib.mf_sparse_conv3d_k4s2_points_cl_fwd(*args, ref.ctypes.data, ws.ctypes.data, B, Cs, Cout, D, n, 1, None) == 0
    ws[:] = 0
    out = np.full(dense.shape, 7.0, np.float32)
    outs = np.zeros((B, Do ** 3, 2 * Cout), np.uint16)
    assert lib.mf_sparse_conv3d_k4s2_points_cl_split_fwd(*args, out.ctypes.data, outs.ctypes.data, ws.ctypes.data, B, Cs,
                                                         Cout, D, n, 1, None) == 0
    np.testing.assert_array_equal(out, ref)
    hi, lo = split_np(out)
    assert np.array_equal(outs[..., :Cout], hi) and np.array_equal(outs[..., Cout:], lo)
    assert (out > 0).mean() > 0.2 and (lo != 0).mean() > 0.2
    assert lib.mf_sparse_conv3d_k4s2_points_cl_split_fwd(*args, out.ctypes.data, None, ws.ctypes.data, B, Cs, Cout, D, n,
                                                         1, None) != 0

    pts = (points / 2.0).astype(np.float32)
    pts[3] = (-0.5, 1.0, 1.0)
    pts[4] = (Do - 0.5, Do - 0.2, 0.3)
    bi2 = bi.copy()
    bi2[5] = 9
    samp = np.zeros((n, Cout), np.float32)
    assert lib.mf_interpolate_voxel_grid_cl_fwd(out.ctypes.data, pts.ctypes.data, bi2.ctypes.data, n, B, Cout, Do, Do,
                                                Do, samp.ctypes.data, Cout, None) == 0
    ldos, los, off = 2 * Cout + 48, Cout + 24, 8
    fill = rne(np.float32(5.0))
    got = np.full((n, ldos), fill, np.uint16)
    assert lib.mf_interpolate_voxel_grid_cl_split_fwd(out.ctypes.data, pts.ctypes.data, bi2.ctypes.data, n, B, Cout, Do,
                                                      Do, Do, got[:, off:].ctypes.data, ldos, los, None) == 0
    hi, lo = split_np(samp)
    assert np.array_equal(got[:, off:off + Cout], hi) and np.array_equal(got[:, off + los:off + los + Cout], lo)
    keep = np.ones(ldos, bool)
    keep[off:off + Cout] = False
    keep[off + los:off + los + Cout] = False
    assert (got[:, keep] == fill).all()
    assert (samp[5] == 0).all() and np.abs(samp).sum() > 0 and (lo != 0).mean() > 0.2
    assert lib.mf_interpolate_voxel_grid_cl_split_fwd(out.ctypes.data, pts.ctypes.data, bi2.ctypes.data, n, B, Cout, Do,
                                                      Do, Do, got[:, off:].ctypes.data, ldos, Cout - 4, None) != 0
