"""TEST INFRASTRUCTURE: the cases of the fp32 3-D inference kernels, shared by tests/test_emul_volumetric_fp32.py (kernel
text on the host emulator) and tests/test_gpu_volumetric_fp32.py (the MI355X), with the code that runs them through the
C ABI -- every output pre-filled with a sentinel and, where the layout has room, embedded in a wider buffer, so that
an unwritten element or a write outside the block shows -- and checks them per element against
tests/volumetric_fp32_ref.py.  Seeded; each case is the smallest shape at which its branch is live.

mf_linear_fwd (``LINEAR``; name = M, K, N of the case)
  m1_k4_n1        M = 1 (< one tile), K = 4 (T = 1, chunks 1..7 of the only K-tile lie past K), N = 1 / Npad = 128; relu 0
  m63_k32_n63     T = 1 exact; N = 63: the scalar tail at n = 60 of an ALIGNED block; bias null; relu 0
  m64_k36_n128    T = 2 with one live chunk in the last tile; 3 groups, A a column block of a wider matrix (lda > K,
                  a_group_stride != 0), w / b / o group strides with gaps
  m65_k64_n130    even T; Npad = 256: a second N tile with two live columns; output shifted by one float (scalar stores)
  m127_k72_n63    odd T (the loop leaves through the ``break``); ldo % 4 != 0 (scalar stores); 3 groups
  m128_k100_n128  K = 100; M = one full-height tile exactly; bias null
  m129_k36_n130   a second M tile of one row; 3 groups; shifted output; relu 0
  m65_k984_n63    the heads' own K (T = 31) at lda = 992
  mi1_grid8 / mi1_grid6    k_linear_mfma<1> at a grid of 8 (M = 256, Npad = 256: the XCD remap) and 6 (M = 192: no remap);
                  every other case above also runs k_linear_mfma<1>, unmapped (grids 1 .. 9 except 8)
  mi2_grid264     k_linear_mfma<2>: M = 257, Npad = 1408, 8 groups, K = 36: 264 full tiles, grid % 8 == 0 (remap)
  mi2_grid273     k_linear_mfma<2>: M = 257, Npad = 1664, 7 groups: 273 tiles, no remap
  refusals        K % 4, lda % 4, lda < K, ldo < N, Npad % 128, Npad < N, a misaligned A: -hipErrorInvalidValue, sentinel kept
mf_conv3d_k4s2_pack_weights / _fwd / k_conv_finish (``CONV``; b, cin, cout, d, split)
  Cin 4 (eight taps per K-tile), 16, 32 (one tap per tile), 64 (half a tap); D 2 (Do = 1: every tap but the central eight
  is padding), 4, 6 (odd Do), 8; M = 1, 8, 24, 64 (< 128), 128 (b2_c32_d8, b16_c32_d4), 135 (B = 5, D = 6: a second M tile
  of seven rows); Cout 128 and 256; split 1, 2, ``default`` (mf_conv3d_k4s2_default_split), ``max`` = 2 Cin (ONE K-tile
  per split, 2 Cin / split = 1: odd) and ``half`` = Cin (two K-tiles per split: even); grids 1, 2, 3, 4 (no remap) and 8,
  256 (remap); ``add`` with c_off = 8 of w_cin = 24 at split 1 and 2; relu 0; bias null.  The pack is compared bit for
  bit; ``max`` cases are launched twice (equal bits).  The issue's D / Cin / split grid is covered pairwise, not as a
  full product.
mf_occupancy_convs_fwd (``OCC``): (B, D) = (1, 2) (every dilated tap but the centre outside), (3, 5), (1, 6), (3, 6), with a
  random, an all-zero and an all-one grid; B D^3 = 8, 375, 216, 648: no multiple of 256, the last three beyond one block.
mf_to_channels_last (``TCL``): (1, 1, 1), (2, 19, 45), (1, 256, 27): equal bits.
Sparse conv3 (``SPARSE``)
  d2_all8         D = 2 (Vo = 1): eight voxels, one per parity class; Cs 4, Cout 64
  d6_b3_mixed     B = 3 with item 1 empty, points outside the grid, batch indices outside [0, B); Cs 12, Cout 128; relu 0;
                  dense null
  d10_64_65       D = 10 (Vo = 125: a second reduce block with a tail): class 0 holds exactly 64 rows and class 7 exactly
                  65; one voxel holds 70 points (the chain fallback); max_rows == occupied voxels exactly; Cs 4, Cout 512;
                  values a column block (ldv > Cs); the pack with c_off = 3
  d6_oneclass     every point in parity class 0 (seven empty classes in the tile table); Cs 144, Cout 256; bias null
  d32_few         D = 32 with 20 points; Cs 12, Cout 256
  d6_none         n = 0: the output is act(dense + bias); Cout 512
  d6_one          one point; Cout 64; dense null, bias null
  Every entry the Cout allows (dense-grid, points, channels-last, split's fp32 output) must give equal bits, and so must
  a second launch.
mf_interpolate_voxel_grid_cl_fwd (``INTERP``): (C, X, B) = (4, 2, 1) (4: the smallest C the launcher accepts), (512, 5, 2),
  (256, 16, 1), (4, 16, 3); rows 0..7: integral coordinates, the far border, negative, outside, batch index -1 and B;
  output a column block (ldo = C + 8, offset 4).
mf_point_prep / mf_pose_epilogue (``PREP``): (B, P, Cv) = (3, 70, 8) (the case of test_emul_conv3d.py), (1, 1, 4), (2, 150, 32)
  (B P = 300 straddles a block of 256); class ids [1, 21, 7] and [0, 22, 7].

``EMUL_SKIP`` lists what the emulator run leaves out (emulated MFMA count), the only way a case may be left out there.
"""
import functools

import numpy as np

import losschain_ref as LR
import volumetric_fp32_ref as R

SENT = np.float32(-12345.0)   # pre-fill of every output buffer: an unwritten element shows
INVALID = -1                  # -hipErrorInvalidValue, the refusal code of include/mfhip.h
f32 = np.float32


class Host:
    """NumPy arrays as device memory (the emulator).  The GPU test has a torch twin."""
    @staticmethod
    def dev(a):
        return np.ascontiguousarray(a).copy()

    @staticmethod
    def host(a):
        return np.asarray(a)

    @staticmethod
    def ptr(a, off=0):
        """Address of element ``off`` (in elements) of the flat buffer; None stays None."""
        return None if a is None else a.ctypes.data + off * a.itemsize

    stream = None

    @staticmethod
    def sync():
        pass


def _sent(X, *shape):
    return X.dev(np.full(shape, SENT, f32))


def bits_equal(a, b, what):
    R.assert_bits(np.asarray(a), np.asarray(b), what)


# ---- mf_linear_fwd -------------------------------------------------------------------------------------------------------
def _lin(M, K, N, Npad, groups=1, a_off=0, a_gs=0, lda=None, o_off=0, o_gs=0, ldo=None, w_gap=0, b_gap=0, bias=True, relu=1):
    lda = lda or a_off + (groups - 1) * a_gs + K
    ldo = ldo or -(-(o_off + (groups - 1) * o_gs + N + 4) // 4) * 4
    return dict(M=M, K=K, N=N, Npad=Npad, groups=groups, a_off=a_off, a_gs=a_gs, lda=lda, o_off=o_off, o_gs=o_gs, ldo=ldo,
                w_gs=Npad * K + w_gap, b_gs=N + b_gap, bias=bias, relu=relu)


LINEAR = {
    "m1_k4_n1": _lin(1, 4, 1, 128, relu=0),
    "m63_k32_n63": _lin(63, 32, 63, 128, bias=False, relu=0, o_off=4),
    "m64_k36_n128": _lin(64, 36, 128, 128, groups=3, a_off=8, a_gs=40, lda=132, o_off=4, o_gs=132, w_gap=8, b_gap=3),
    "m65_k64_n130": _lin(65, 64, 130, 256, o_off=5),
    "m127_k72_n63": _lin(127, 72, 63, 128, groups=3, a_gs=72, o_off=4, o_gs=64, ldo=201),
    "m128_k100_n128": _lin(128, 100, 128, 128, bias=False),
    "m129_k36_n130": _lin(129, 36, 130, 256, groups=3, a_off=4, a_gs=36, lda=120, o_off=1, o_gs=131, relu=0, w_gap=4),
    "m65_k984_n63": _lin(65, 984, 63, 128, lda=992),
    "mi1_grid8": _lin(256, 32, 256, 256),
    "mi1_grid6": _lin(192, 32, 256, 256, relu=0),
    "mi2_grid264": _lin(257, 36, 1400, 1408, groups=8, a_gs=36, o_gs=1400, ldo=8 * 1400),
    "mi2_grid273": _lin(257, 36, 1601, 1664, groups=7, a_gs=36, o_gs=1601, ldo=7 * 1601 + 1),
}


def linear_grid(c):
    """(tile height MI, grid) the launcher of csrc/linear.hip picks."""
    full = -(-c["M"] // 128) * (c["Npad"] // 128) * c["groups"]
    return (2, full) if full >= 256 else (1, -(-c["M"] // 64) * (c["Npad"] // 128) * c["groups"])


@functools.lru_cache(maxsize=None)
def linear_data(name):
    c = LINEAR[name]
    rs = np.random.RandomState(sum(map(ord, name)))
    G = c["groups"]
    A = rs.uniform(-1, 1, (c["M"], c["lda"])).astype(f32)
    W = rs.uniform(-1, 1, (G, c["w_gs"])).astype(f32)            # rows N .. Npad - 1 are NOT zero: computed, never stored
    b = rs.uniform(-0.5, 0.5, (G, c["b_gs"])).astype(f32)
    A[1:][rs.uniform(size=A[1:].shape) < 0.2] = 0.0               # post-ReLU-like input (row 0 stays dense)
    return A, W, b


def run_linear(lib, X, name):
    c = LINEAR[name]
    A, W, b = linear_data(name)
    M, K, N, G = c["M"], c["K"], c["N"], c["groups"]
    dA, dW, db = X.dev(A), X.dev(W), X.dev(b)
    out = _sent(X, M + 2, c["ldo"])                                # the block starts at row 1, column o_off
    rc = lib.mf_linear_fwd(X.ptr(dA, c["a_off"]), c["a_gs"], c["lda"], X.ptr(dW), c["w_gs"], K,
                           X.ptr(db) if c["bias"] else None, c["b_gs"], X.ptr(out, c["ldo"] + c["o_off"]), c["o_gs"],
                           c["ldo"], M, N, c["Npad"], K, G, c["relu"], X.stream)
    assert rc == 0, rc
    X.sync()
    return X.host(out)


def check_linear(name, out, tag):
    c = LINEAR[name]
    A, W, b = linear_data(name)
    M, K, N, G = c["M"], c["K"], c["N"], c["groups"]
    rest = np.array(out, copy=True)
    for g in range(G):
        a0, o0 = c["a_off"] + g * c["a_gs"], c["o_off"] + g * c["o_gs"]
        Wg = W[g, :c["Npad"] * K].reshape(c["Npad"], K)[:N]
        ref, S, Kb = R.linear(A[:, a0:a0 + K], Wg, b[g, :N] if c["bias"] else None, c["relu"])
        blk = out[1:M + 1, o0:o0 + N]
        assert not (blk == SENT).any(), (tag, name, g, "unwritten element", np.argwhere(blk == SENT)[:4].tolist())
        R.assert_within(blk, ref, S, Kb, f"{tag} linear {name} group {g}", op=f"{tag} mf_linear_fwd")
        rest[1:M + 1, o0:o0 + N] = SENT
    bad = np.argwhere(rest != SENT)
    assert len(bad) == 0, (tag, name, "a write outside the output block at (row, column)", bad[:4].tolist())


def check_linear_refusals(lib, X):
    z = X.dev(np.ones(64 * 16, f32))
    W = X.dev(np.ones(256 * 16, f32))
    # (offset of A, lda, ldo, N, Npad, K)
    for what, (ao, lda, ldo, N, Npad, K) in {"K % 4": (0, 8, 8, 8, 128, 6), "lda % 4": (0, 10, 8, 8, 128, 8),
                                            "lda < K": (0, 4, 8, 8, 128, 8), "ldo < N": (0, 8, 4, 8, 128, 8),
                                            "Npad % 128": (0, 8, 8, 8, 100, 8), "Npad < N": (0, 8, 200, 130, 128, 8),
                                            "misaligned A": (1, 8, 8, 8, 128, 8)}.items():
        out = _sent(X, 8, 256)
        rc = lib.mf_linear_fwd(X.ptr(z, ao), 0, lda, X.ptr(W), 0, 16, None, 0, X.ptr(out), 0, ldo, 4, N, Npad, K, 1, 1,
                               X.stream)
        X.sync()
        assert rc == INVALID, (what, rc)
        assert (X.host(out) == SENT).all(), what


# ---- mf_conv3d_k4s2 ----------------------------------------------------------------------------------------------------
def _conv(B, Cin, Cout, D, split, relu=1, bias=True, add=False, c_off=0, w_cin=None):
    return dict(B=B, Cin=Cin, Cout=Cout, D=D, split=split, relu=relu, bias=bias, add=add, c_off=c_off, w_cin=w_cin or Cin)


CONV = {
    "b1_c4_d2_s1": _conv(1, 4, 128, 2, 1),
    "b1_c4_d2_smax": _conv(1, 4, 128, 2, "max"),                     # grid 8: the remap
    "b8_c4_d2_shalf": _conv(8, 4, 256, 2, "half", relu=0),           # M = 8; two K-tiles per split; grid 8
    "b3_c16_d4_s2": _conv(3, 16, 256, 4, 2, bias=False),             # M = 24, grid 4
    "b2_c32_d8_sdef": _conv(2, 32, 128, 8, "default"),               # M = 128 exactly
    "b16_c32_d4_s1": _conv(16, 32, 128, 4, 1, relu=0),               # M = 128 from 16 items of 8 voxels
    "b5_c16_d6_s1": _conv(5, 16, 128, 6, 1, relu=0, bias=False),     # M = 135, grid 2
    "b5_c16_d6_s2": _conv(5, 16, 128, 6, 2),                         # M = 135, grid 4, finish over a ragged M
    "b5_c64_d6_smax": _conv(5, 64, 128, 6, "max"),                   # M = 135, 128 slabs of one K-tile, grid 256
    "b1_c64_d6_shalf": _conv(1, 64, 128, 6, "half"),                 # M = 27, two K-tiles per split
    "b1_c16_d8_add_s1": _conv(1, 16, 128, 8, 1, add=True, c_off=8, w_cin=24),
    "b1_c16_d8_add_s2": _conv(1, 16, 128, 8, 2, add=True, c_off=8, w_cin=24),
    "b3_c32_d6_s1": _conv(3, 32, 384, 6, 1),                         # grid 3, three N tiles
}
CONV_REFUSED = ((1, 24, 128, 8, 1), (1, 32, 96, 8, 1), (1, 32, 128, 7, 1), (1, 32, 128, 8, 3))


def conv_split(lib, c):
    s = c["split"]
    if s == "max":
        return 2 * c["Cin"]
    if s == "half":
        return c["Cin"]
    if s == "default":
        return int(lib.mf_conv3d_k4s2_default_split(c["B"], c["Cin"], c["Cout"], c["D"]))
    return s


@functools.lru_cache(maxsize=None)
def conv_data(name):
    c = CONV[name]
    rs = np.random.RandomState(sum(map(ord, name)))
    B, D, Do = c["B"], c["D"], c["D"] // 2
    x = rs.uniform(-1, 1, (B, c["w_cin"], D, D, D)).astype(f32)
    x[rs.uniform(size=x.shape) < 0.3] = 0.0
    W = (rs.uniform(-1, 1, (c["Cout"], c["w_cin"], 4, 4, 4)) / 8).astype(f32)
    bias = rs.uniform(-0.2, 0.2, c["Cout"]).astype(f32)
    add = rs.uniform(-1, 1, (B, c["Cout"], Do, Do, Do)).astype(f32)
    return x, W, bias, add


def cl(x_cf):
    """[B, C, D, D, D] -> channels-last [B, D^3, C]."""
    B, C = x_cf.shape[:2]
    return np.ascontiguousarray(x_cf.reshape(B, C, -1).transpose(0, 2, 1))


def cf(x_cl, D):
    B, _, C = x_cl.shape
    return x_cl.reshape(B, D, D, D, C).transpose(0, 4, 1, 2, 3)


PAD = 64   # floats of sentinel on either side of an output that has no row pitch of its own


def run_conv(lib, X, name):
    c = CONV[name]
    x, W, bias, add = conv_data(name)
    B, Cin, Cout, D, co = c["B"], c["Cin"], c["Cout"], c["D"], c["c_off"]
    split = conv_split(lib, c)
    M = B * (D // 2) ** 3
    dx, dW = X.dev(cl(x[:, co:co + Cin])), X.dev(W)
    wt = _sent(X, Cout * 64 * Cin + 2 * PAD)
    assert lib.mf_conv3d_k4s2_pack_weights(X.ptr(dW), Cout, Cin, c["w_cin"], co, X.ptr(wt, PAD), X.stream) == 0
    db = X.dev(bias) if c["bias"] else None
    da = X.dev(cl(add)) if c["add"] else None
    nbytes = int(lib.mf_conv3d_k4s2_workspace_bytes(B, Cout, D, split))
    assert nbytes == (split * M * Cout * 4 if split > 1 else 0)
    ws = _sent(X, max(nbytes // 4, 4) + 2 * PAD)
    out = _sent(X, M * Cout + 2 * PAD)
    rc = lib.mf_conv3d_k4s2_fwd(X.ptr(dx), X.ptr(wt, PAD), X.ptr(db), X.ptr(da), X.ptr(out, PAD), X.ptr(ws, PAD), B, Cin,
                                Cout, D, split, c["relu"], X.stream)
    assert rc == 0, rc
    X.sync()
    return dict(wt=X.host(wt), out=X.host(out), ws=X.host(ws), split=split)


def _guards(flat, n, what):
    flat = np.asarray(flat).reshape(-1)
    assert (flat[:PAD] == SENT).all() and (flat[PAD + n:] == SENT).all(), (what, "a write outside the buffer")
    body = flat[PAD:PAD + n]
    assert not (body == SENT).any(), (what, "unwritten element", np.argwhere(body == SENT)[:4].ravel().tolist())
    return body


def check_conv(name, got, tag):
    c = CONV[name]
    x, W, bias, add = conv_data(name)
    B, Cin, Cout, D, co, split = c["B"], c["Cin"], c["Cout"], c["D"], c["c_off"], got["split"]
    M = B * (D // 2) ** 3
    what = f"{tag} conv {name} split {split}"
    bits_equal(_guards(got["wt"], Cout * 64 * Cin, what + " pack").reshape(Cout, 64, Cin), R.pack_k4s2(W, co, Cin), what + " pack")
    ws = np.asarray(got["ws"]).reshape(-1)
    used = split * M * Cout if split > 1 else 0
    assert (ws[:PAD] == SENT).all() and (ws[PAD + used:] == SENT).all(), (what, "a write outside the workspace")
    out = cf(_guards(got["out"], M * Cout, what).reshape(B, -1, Cout), D // 2)
    ref, S = R.conv3d(x[:, co:co + Cin], W[:, co:co + Cin], bias if c["bias"] else None, add if c["add"] else None,
                      c["relu"], stride=2, pad=1)
    K = R.conv_k4s2_K(Cin, split, bias if c["bias"] else None, add if c["add"] else None)
    R.assert_within(out, ref, S, K, what, op=f"{tag} mf_conv3d_k4s2_fwd" + (" + k_conv_finish" if split > 1 else ""))


def check_conv_refusals(lib, X):
    z = X.dev(np.zeros(4, f32))
    for B, Cin, Cout, D, split in CONV_REFUSED:
        out = _sent(X, 16)
        rc = lib.mf_conv3d_k4s2_fwd(X.ptr(z), X.ptr(z), None, None, X.ptr(out), X.ptr(z), B, Cin, Cout, D, split, 1, X.stream)
        X.sync()
        assert rc == INVALID, ((B, Cin, Cout, D, split), rc)
        assert (X.host(out) == SENT).all()


# ---- mf_occupancy_convs_fwd ------------------------------------------------------------------------------------------------
OCC = {"b1_d2_rand": (1, 2, "rand"), "b3_d5_rand": (3, 5, "rand"), "b1_d6_ones": (1, 6, "ones"), "b3_d6_zeros": (3, 6, "zeros"),
       "b1_d5_ones": (1, 5, "ones"), "b3_d6_rand": (3, 6, "rand")}


@functools.lru_cache(maxsize=None)
def occ_data(name):
    B, D, kind = OCC[name]
    rs = np.random.RandomState(sum(map(ord, name)))
    grid = {"rand": (rs.uniform(size=(B, D, D, D)) < 0.4), "ones": np.ones((B, D, D, D)), "zeros": np.zeros((B, D, D, D))}[kind]
    return (grid.astype(f32), rs.uniform(-0.5, 0.5, (8, 1, 3, 3, 3)).astype(f32), rs.uniform(-0.1, 0.1, 8).astype(f32),
            rs.uniform(-0.3, 0.3, (16, 8, 3, 3, 3)).astype(f32), rs.uniform(-0.1, 0.1, 16).astype(f32))


def run_occ(lib, X, name):
    B, D, _ = OCC[name]
    grid, W1, b1, W2, b2 = occ_data(name)
    w1 = np.ascontiguousarray(W1.transpose(2, 3, 4, 1, 0)).reshape(27, 1, 8)
    w2 = np.ascontiguousarray(W2.transpose(2, 3, 4, 1, 0)).reshape(27, 8, 16)
    V = B * D ** 3
    h1, h2 = _sent(X, V * 8 + 2 * PAD), _sent(X, V * 16 + 2 * PAD)
    d = [X.dev(a) for a in (grid, w1, b1, w2, b2)]
    assert lib.mf_occupancy_convs_fwd(*(X.ptr(a) for a in d), X.ptr(h1, PAD), X.ptr(h2, PAD), B, D, X.stream) == 0
    X.sync()
    return dict(h1=X.host(h1), h2=X.host(h2))


def check_occ_values(grid, W1, b1, W2, b2, h1_cl, h2_cl, what, op):
    """h1 against the grid (K = 27 + 1), h2 against the h1 it was handed (K = 27 * 8 + 1)."""
    D = grid.shape[1]
    ref, S = R.conv3d(grid[:, None], W1, b1, None, True, pad=1)
    R.assert_within(cf(h1_cl, D), ref, S, 28, what + " h1", op=op + " h1")
    ref, S = R.conv3d(cf(h1_cl, D), W2, b2, None, True, pad=2, dil=2)
    R.assert_within(cf(h2_cl, D), ref, S, 217, what + " h2", op=op + " h2")


def check_occ(name, got, tag):
    B, D, kind = OCC[name]
    data = occ_data(name)
    V = B * D ** 3
    what = f"{tag} occupancy {name}"
    h1 = _guards(got["h1"], V * 8, what + " h1").reshape(B, D ** 3, 8)
    h2 = _guards(got["h2"], V * 16, what + " h2").reshape(B, D ** 3, 16)
    check_occ_values(*data, h1, h2, what, f"{tag} mf_occupancy_convs_fwd")
    if kind == "zeros":   # relu(bias), every voxel: S = |bias| and K = 28 would allow an error; a zero input allows none
        bits_equal(h1, np.broadcast_to(np.maximum(data[2], 0), h1.shape), what + " h1 of a zero grid")


# ---- mf_to_channels_last -----------------------------------------------------------------------------------------------------
TCL = ((1, 1, 1), (2, 19, 45), (1, 256, 27))


def run_check_tcl(lib, X, shape, tag):
    B, C, V = shape
    x = np.random.RandomState(B * 1000 + C).uniform(-1, 1, shape).astype(f32)
    y, dx = _sent(X, B * V * C + 2 * PAD), X.dev(x)
    assert lib.mf_to_channels_last(X.ptr(dx), X.ptr(y, PAD), B, C, V, X.stream) == 0
    X.sync()
    bits_equal(_guards(X.host(y), B * V * C, f"{tag} to_channels_last {shape}").reshape(B, V, C), x.transpose(0, 2, 1),
               f"{tag} to_channels_last {shape}")


# ---- sparse conv3 -------------------------------------------------------------------------------------------------------------
def _sp(kind, D, B, Cs, Cout, dense=True, bias=True, relu=1, ld_gap=0, c_off=0, exact_rows=False):
    return dict(kind=kind, D=D, B=B, Cs=Cs, Cout=Cout, dense=dense, bias=bias, relu=relu, ld_gap=ld_gap, c_off=c_off,
                exact_rows=exact_rows)


SPARSE = {
    "d2_all8": _sp("all8", 2, 1, 4, 64),
    "d6_b3_mixed": _sp("mixed", 6, 3, 12, 128, dense=False, relu=0),
    "d10_64_65": _sp("64_65", 10, 1, 4, 512, ld_gap=8, c_off=3, exact_rows=True),
    "d6_oneclass": _sp("oneclass", 6, 1, 144, 256, bias=False),
    "d32_few": _sp("few", 32, 1, 12, 256, ld_gap=4),
    "d6_none": _sp("none", 6, 2, 4, 512),
    "d6_one": _sp("one", 6, 1, 4, 64, dense=False, bias=False),
}


def _centres(vox, rs, jitter=0.4):
    return (np.asarray(vox, np.float64) + rs.uniform(-jitter, jitter, (len(vox), 3))).astype(f32)


@functools.lru_cache(maxsize=None)
def sparse_data(name):
    c = SPARSE[name]
    rs = np.random.RandomState(sum(map(ord, name)))
    D, B, Cs, Cout, Do = c["D"], c["B"], c["Cs"], c["Cout"], c["D"] // 2
    kind = c["kind"]
    if kind == "all8":
        pts = _centres([(i, j, k) for i in range(2) for j in range(2) for k in range(2)], rs)
        bi = np.zeros(8, np.int32)
    elif kind == "mixed":
        pts = rs.uniform(-1.5, D + 0.9, (90, 3)).astype(f32)          # some outside the grid on every face
        pts[:10] = pts[10:20]                                         # shared voxels: means over several points
        bi = np.sort(rs.choice([0, 2], 90)).astype(np.int32)          # item 1 is empty
        bi[[3, 40, 77]] = [-1, 3, 7]                                  # outside [0, B)
    elif kind == "64_65":
        odd = [(i, j, k) for i in (1, 3, 5, 7, 9) for j in (1, 3, 5, 7, 9) for k in (1, 3, 5, 7, 9)]    # class 0
        even = [(i, j, k) for i in (0, 2, 4, 6, 8) for j in (0, 2, 4, 6, 8) for k in (0, 2, 4, 6, 8)]   # class 7
        vox = [odd[i] for i in rs.permutation(125)[:64]] + [even[i] for i in rs.permutation(125)[:65]]
        vox += [(0, 1, 1), (2, 2, 1), (9, 8, 8)]                      # a few rows in other classes
        vox += [vox[5]] * 69                                          # voxel 5 of class 0 holds 70 points: the chain fallback
        pts = _centres([vox[i] for i in rs.permutation(len(vox))], rs)
        bi = np.zeros(len(pts), np.int32)
    elif kind == "oneclass":
        odd = [(i, j, k) for i in (1, 3, 5) for j in (1, 3, 5) for k in (1, 3, 5)]
        pts = _centres([odd[i] for i in rs.randint(0, 27, 40)], rs)
        bi = np.zeros(40, np.int32)
    elif kind == "few":
        pts = rs.uniform(0, D - 1, (20, 3)).astype(f32)
        pts[0], pts[1] = (0.2, -0.3, 0.1), (31.3, 30.8, 31.4)        # the two far corners
        bi = np.zeros(20, np.int32)
    elif kind == "none":
        pts, bi = np.zeros((0, 3), f32), np.zeros(0, np.int32)
    elif kind == "one":
        pts, bi = np.array([[2.2, 3.9, 1.4]], f32), np.zeros(1, np.int32)
    n = len(pts)
    ldv = Cs + c["ld_gap"]
    wide = rs.uniform(-1, 1, (max(n, 1), ldv)).astype(f32)           # values = columns 0 .. Cs - 1 of it
    w_cin = Cs + c["c_off"] + 2
    W = (rs.uniform(-1, 1, (Cout, w_cin, 4, 4, 4)) * 0.2).astype(f32)
    bias = rs.uniform(-0.1, 0.1, Cout).astype(f32)
    dense = rs.uniform(-0.3, 0.3, (B, Cout, Do, Do, Do)).astype(f32)
    values = np.ascontiguousarray(wide[:n, :Cs])
    grid, counts = R.voxelize(values, pts, bi, B, D)
    occupied = int((counts > 0).sum())
    if kind == "64_65":   # the case is what its name says
        ix = np.argwhere(counts[0] > 0)
        cls = ((ix[:, 0] + 1) & 1) | (((ix[:, 1] + 1) & 1) << 1) | (((ix[:, 2] + 1) & 1) << 2)
        per = np.bincount(cls, minlength=8)
        assert per[0] == 64 and per[7] == 65 and counts.max() == 70, (per, counts.max())
    if kind == "oneclass":
        assert occupied > 1 and all(((ix + 1) & 1 == 0).all() for ix in np.argwhere(counts[0] > 0))
    max_rows = occupied if c["exact_rows"] else max(n, 1)
    return dict(pts=pts, bi=bi, wide=wide, values=values, W=W, bias=bias, dense=dense, grid=grid, counts=counts, n=n, ldv=ldv,
                w_cin=w_cin, max_rows=max_rows, occupied=occupied)


SPARSE_ENTRIES = ("dense", "points", "cl", "split")


def run_sparse(lib, X, name, entry):
    """One entry point on one case -> the output as channels-first [B, Cout, Do, Do, Do], guards checked."""
    c, d = SPARSE[name], sparse_data(name)
    D, B, Cs, Cout, Do = c["D"], c["B"], c["Cs"], c["Cout"], c["D"] // 2
    n, Vo = d["n"], Do ** 3
    what = f"sparse conv3 {name} {entry}"
    Wp, dW = _sent(X, 8 * Cs * 8 * Cout + 2 * PAD), X.dev(d["W"])
    assert lib.mf_sparse_conv3d_pack_weights(X.ptr(dW), Cout, Cs, d["w_cin"], c["c_off"], X.ptr(Wp, PAD), X.stream) == 0
    nb = int(lib.mf_sparse_conv3d_workspace_bytes(B, Cs, Cout, D, d["max_rows"], 0 if entry == "dense" else n))
    ws = X.dev(np.full(nb // 4 + 64, np.nan, f32))                   # NaN: a row the kernels read without writing it shows
    out = _sent(X, B * Cout * Vo + 2 * PAD)
    db = X.dev(d["bias"]) if c["bias"] else None
    pts, bi = X.dev(d["pts"] if n else np.zeros((1, 3), f32)), X.dev(d["bi"] if n else np.zeros(1, np.int32))
    tail = (X.ptr(ws), B, Cs, Cout, D, d["max_rows"], c["relu"], X.stream)
    if entry == "dense":
        dd = X.dev(d["dense"]) if c["dense"] else None
        grid, counts = X.dev(d["grid"]), X.dev(d["counts"])
        rc = lib.mf_sparse_conv3d_k4s2_fwd(X.ptr(grid), X.ptr(counts), X.ptr(Wp, PAD), X.ptr(dd),
                                           X.ptr(db), X.ptr(out, PAD), *tail)
    elif entry == "points":
        dd = X.dev(d["dense"]) if c["dense"] else None
        vals = X.dev(d["values"] if n else np.zeros((1, Cs), f32))
        rc = lib.mf_sparse_conv3d_k4s2_points_fwd(X.ptr(vals), X.ptr(pts), X.ptr(bi), n, 0.0, 0.0, 0.0, 1.0, X.ptr(Wp, PAD),
                                                  X.ptr(dd), X.ptr(db), X.ptr(out, PAD), *tail)
    else:
        dd = X.dev(cl(d["dense"])) if c["dense"] else None
        wide = X.dev(d["wide"])
        head = (X.ptr(wide), d["ldv"], X.ptr(pts), X.ptr(bi), n, 0.0, 0.0, 0.0, 1.0, X.ptr(Wp, PAD), X.ptr(dd),
                X.ptr(db), X.ptr(out, PAD))
        if entry == "cl":
            rc = lib.mf_sparse_conv3d_k4s2_points_cl_fwd(*head, *tail)
        else:
            outs = X.dev(np.zeros(B * Vo * 2 * Cout, np.int16))
            rc = lib.mf_sparse_conv3d_k4s2_points_cl_split_fwd(*head, X.ptr(outs), *tail)
    assert rc == 0, (what, rc)
    X.sync()
    bits_equal(_guards(X.host(Wp), 8 * Cs * 8 * Cout, what + " pack"), R.pack_sparse(d["W"], c["c_off"], Cs), what + " pack")
    body = _guards(X.host(out), B * Cout * Vo, what)
    if entry in ("dense", "points"):
        return body.reshape(B, Cout, Do, Do, Do)
    return np.ascontiguousarray(cf(body.reshape(B, Vo, Cout), Do))


def sparse_entries(name):
    return SPARSE_ENTRIES if SPARSE[name]["Cout"] % 256 == 0 else SPARSE_ENTRIES[:2]


def check_sparse(lib, X, name, tag):
    c, d = SPARSE[name], sparse_data(name)
    co = c["c_off"]
    ref, S, K = R.sparse_conv3(d["grid"], d["W"][:, co:co + c["Cs"]], d["dense"] if c["dense"] else None,
                               d["bias"] if c["bias"] else None, c["relu"])
    first = None
    for entry in sparse_entries(name):
        got = run_sparse(lib, X, name, entry)
        if first is None:
            first = got
            R.assert_within(got, ref, S, K, f"{tag} sparse conv3 {name} ({entry} entry)", op=f"{tag} sparse conv3 fp32")
            if c["kind"] == "none":
                assert d["occupied"] == 0
        else:
            bits_equal(got, first, f"{tag} sparse conv3 {name}: the {entry} entry against the {sparse_entries(name)[0]} entry")
    again = run_sparse(lib, X, name, sparse_entries(name)[-1])
    bits_equal(again, first, f"{tag} sparse conv3 {name}: a second launch")


# ---- mf_interpolate_voxel_grid_cl_fwd ------------------------------------------------------------------------------------------
INTERP = ((4, 2, 1), (512, 5, 2), (256, 16, 1), (4, 16, 3))


@functools.lru_cache(maxsize=None)
def interp_data(C, X_, B):
    rs = np.random.RandomState(C + 10 * X_ + B)
    n = 41
    vox = rs.uniform(-1, 1, (B, X_ ** 3, C)).astype(f32)
    pts = (rs.uniform(-0.15, 1.1, (n, 3)) * X_).astype(f32)
    bi = rs.randint(0, B, n).astype(np.int32)
    pts[0] = (0, 0, 0)                                # exactly integral
    pts[1] = (X_ - 1, 1, X_ - 1)                      # integral, on the far border
    pts[2] = (X_ - 1 + 0.25, X_ - 1, 0.5)             # between the far border and outside
    pts[3] = (-0.5, 0.75, 0.25)                       # negative
    pts[4] = (X_ + 3.2, -5.7, 0.5)                    # outside
    pts[5] = (1.0, X_ - 0.5, X_ - 1.0)
    bi[6], bi[7] = -1, B                              # rows with a batch index outside [0, B): zeros
    return vox, pts, bi


def run_check_interp(lib, X, shape, tag):
    C, X_, B = shape
    vox, pts, bi = interp_data(*shape)
    n, ldo = len(pts), C + 8
    out, dv, dp, db = _sent(X, n + 2, ldo), X.dev(vox), X.dev(pts), X.dev(bi)
    rc = lib.mf_interpolate_voxel_grid_cl_fwd(X.ptr(dv), X.ptr(dp), X.ptr(db), n, B, C, X_, X_, X_,
                                              X.ptr(out, ldo + 4), ldo, X.stream)
    assert rc == 0, rc
    X.sync()
    out = X.host(out)
    want = R.interpolate_cl(vox, X_, pts, bi)
    what = f"{tag} interpolate_cl {shape}"
    bits_equal(out[1:n + 1, 4:4 + C], want, what)
    assert (want[6] == 0).all() and (want[7] == 0).all() and np.abs(want[:6]).sum() > 0
    rest = out.copy()
    rest[1:n + 1, 4:4 + C] = SENT
    assert (rest == SENT).all(), (what, "a write outside the column block")


# ---- mf_point_prep / mf_pose_epilogue ---------------------------------------------------------------------------------------------
PREP = ((3, 70, 8), (1, 1, 4), (2, 150, 32))
NF, NP4 = 21, 128


@functools.lru_cache(maxsize=None)
def prep_data(B, P, Cv):
    rs = np.random.RandomState(9 + B + P)
    return dict(pc=rs.uniform(-0.3, 0.9, (B, 3, P)).astype(f32), vals=rs.uniform(-1, 1, (B, Cv, P)).astype(f32),
                origin=rs.uniform(-0.4, 0.2, (B, 3)).astype(f32), pitch=rs.uniform(0.004, 0.01, B).astype(f32),
                o=rs.uniform(-2, 2, (B * P, 3 * NP4)).astype(f32),
                cid=np.array([1, 21, 7][:B] if B > 1 else [21], np.int64), bad_cid=np.array([0, 22, 7][:B], np.int64))


def run_check_prep(lib, X, shape, tag):
    B, P, Cv = shape
    d = prep_data(*shape)
    n = B * P
    what = f"{tag} point_prep / pose_epilogue {shape}"
    pts, tc4, xr = _sent(X, n * 3 + 2 * PAD), _sent(X, n * 4 + 2 * PAD), _sent(X, n * Cv + 2 * PAD)
    bi = X.dev(np.full(n + 2 * PAD, -7, np.int32))
    dev = {k: X.dev(d[k]) for k in ("pc", "vals", "origin", "pitch", "o", "cid", "bad_cid")}
    assert lib.mf_point_prep(X.ptr(dev["pc"]), X.ptr(dev["vals"]), X.ptr(dev["origin"]), X.ptr(dev["pitch"]), B, P, Cv, 15.5,
                             X.ptr(pts, PAD), X.ptr(tc4, PAD), X.ptr(xr, PAD), X.ptr(bi, PAD), X.stream) == 0
    X.sync()
    want = R.point_prep(d["pc"], d["vals"], d["origin"], d["pitch"], 15.5)
    for got, w, k in zip((pts, tc4, xr), want, ("pts", "tc4", "rows")):
        bits_equal(_guards(X.host(got), w.size, what + " " + k).reshape(w.shape), w, what + " " + k)
    hb = X.host(bi)
    assert (hb[:PAD] == -7).all() and (hb[PAD + n:] == -7).all() and np.array_equal(hb[PAD:PAD + n], want[3]), what
    # the epilogue on the kernel's own points
    p_dev = X.dev(want[0])
    for cid in ("cid", "bad_cid"):
        rot, trans, conf = _sent(X, n * 4 + 2 * PAD), _sent(X, n * 3 + 2 * PAD), _sent(X, n + 2 * PAD)
        assert lib.mf_pose_epilogue(X.ptr(dev["o"]), 3 * NP4, NP4, X.ptr(dev[cid]), X.ptr(p_dev), X.ptr(dev["origin"]),
                                    X.ptr(dev["pitch"]), B, P, NF, X.ptr(rot, PAD), X.ptr(trans, PAD), X.ptr(conf, PAD),
                                    X.stream) == 0
        X.sync()
        o = d["o"]
        ref, bnd = R.pose_epilogue(o[:, :4 * NF], o[:, NP4:NP4 + 3 * NF], o[:, 2 * NP4:2 * NP4 + NF], d[cid], want[0],
                                   d["origin"], d["pitch"], NF)
        for got, r, b, k, w in zip((rot, trans, conf), ref, bnd, ("rot", "trans", "conf"), (4, 3, 1)):
            g = _guards(X.host(got), n * w, f"{what} {k}").reshape(r.shape)
            ok, worst, i = LR.compare(g, r, b)
            R.RATIOS[f"{tag} mf_pose_epilogue"] = max(R.RATIOS.get(f"{tag} mf_pose_epilogue", 0.0), worst)
            print(f"VOLFP32 {what} {cid} {k}: worst |got-ref|/bound = {worst:.3f} at {i}")
            assert ok, (what, cid, k, worst, i)
        if cid == "bad_cid":   # ids 0 and n_fg + 1: NaN rows (the reference says so; compare() demands NaN there)
            assert np.isnan(ref[0][:min(B, 2)]).all()


def report():
    for k in sorted(R.RATIOS):
        print(f"VOLFP32 worst error / bound, {k}: {R.RATIOS[k]:.3f}")


# ---- what the emulator run leaves out -----------------------------------------------------------------------------------------------
# name -> reason.  Only the emulated MFMA count may be a reason; at most a quarter of the cases; never every case of a
# branch.
EMUL_SKIP = {}   # every case runs in a few seconds there: nothing is left out
N_CASES = len(LINEAR) + len(CONV) + len(OCC) + len(TCL) + len(SPARSE) + len(INTERP) + len(PREP)
assert 4 * len(EMUL_SKIP) <= N_CASES
