"""TEST INFRASTRUCTURE: float64 references, bit-exact mirrors and the per-element error bound of the fp32 3-D inference
kernels (csrc/linear.hip, conv3d.hip, sparseconv.hip, interp.hip, pointops.hip).  NumPy / torch float64 on the CPU and
oracle/oracle_np.py only: nothing here calls the library or is fitted to what a kernel returns.

THE BOUND is the rule tests/bf16_bound.py states for an fp32 output,

    |got - ref| <= 2 K 2^-24 S        per element,

with ``ref`` the float64 contraction on the same fp32 operands, ``S`` the same contraction on absolute values plus
|bias|, |add| and |dense|, and ``K`` the reduction length (taps x channels) plus one for each further addend and each
split-K slab.  There the operands are bf16 and their products are exact in fp32; here the operands are fp32, so every
product rounds as well.  A product that rounds once is (a w)(1 + d), |d| <= 2^-24: it adds ONE more factor (1 + d) to
its own term, so a sum of K such products accumulated in fp32 in ANY order obeys |fl(sum) - sum| <= K 2^-24 S to first
order ((K - 1) additions on the deepest path + 1 for the product; an fma, which does not round the product, is below
that).  The factor 2 is the same margin as there: second-order terms and an accumulator that truncates.  An element
with S == 0 must be exact.  The ReLU is 1-Lipschitz and is applied to both sides before the comparison.  The bound is
derived, not measured: a case over it is a finding about the kernel.

Where the project already has a bit-exact mirror -- oracle_np.interpolate_voxel_grid(mode="gpu"),
oracle_np.average_voxelization_3d(mode="gpu"), the NumPy float32 restatement of mf_point_prep -- the check is equal
bits (``assert_bits``), not a bound.  mf_pose_epilogue has a sqrtf, an expf and divides: it is checked against
losschain_ref.pose_epilogue (float64, with that module's rounding counts: the inference kernel evaluates the same
expressions as the training forward).
"""
import numpy as np
import torch
import torch.nn.functional as F

from losschain_ref import pose_epilogue  # noqa: F401  (float64 reference + bound of the epilogue's expressions)
from oracle import oracle_np as O

U32 = 2.0 ** -24
f32 = np.float32

RATIOS = {}   # kernel -> worst |got - ref| / bound of the checks made in this process (reporting only)


def ratios(got, ref, S, K):
    """-> |got - ref| / (2 K 2^-24 S) per element; where the bound is 0: 0 if equal, else inf; inf where not finite."""
    got, ref, S = (np.asarray(a, np.float64) for a in (got, ref, S))
    assert got.shape == ref.shape == S.shape, (got.shape, ref.shape, S.shape)
    bnd = 2.0 * K * U32 * S
    err = np.abs(got - ref)
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.where(bnd > 0, err / np.where(bnd > 0, bnd, 1.0), np.where(err > 0, np.inf, 0.0))
    return np.where(np.isfinite(got), r, np.inf), err, bnd


def assert_within(got, ref, S, K, what, op):
    """Every element of ``got`` within the bound of ``ref``; prints the worst one before it asserts."""
    r, err, bnd = ratios(got, ref, S, K)
    if r.size == 0:
        return 0.0
    i = np.unravel_index(int(np.argmax(r)), r.shape)
    worst = float(r[i])
    RATIOS[op] = max(RATIOS.get(op, 0.0), worst)
    print(f"VOLFP32 {what}: worst |got-ref|/bound = {worst:.3f} at {tuple(int(v) for v in i)} (err {err[i]:.3e}, "
          f"bound {bnd[i]:.3e}, K = {K})")
    assert worst <= 1.0, (what, worst, tuple(int(v) for v in i), float(err[i]), float(bnd[i]))
    return worst


def assert_bits(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    v = {4: np.int32, 8: np.int64, 2: np.int16}[got.dtype.itemsize]
    bad = np.argwhere(got.view(v) != want.view(v))
    assert len(bad) == 0, (what, "bits differ at", bad[:5].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])


def _act(ref, relu):
    return np.maximum(ref, 0.0) if relu else ref


# ---- mf_linear_fwd ----------------------------------------------------------------------------------------------
def linear(A, W, bias, relu):
    """A [M, K], W [N, K], bias [N] or None -> (ref, S, Kb) float64 [M, N]; Kb = K (+ 1 with a bias)."""
    A, W = np.asarray(A, np.float64), np.asarray(W, np.float64)
    ref, S = A @ W.T, np.abs(A) @ np.abs(W).T
    if bias is not None:
        b = np.asarray(bias, np.float64)
        ref, S = ref + b, S + np.abs(b)
    return _act(ref, relu), S, A.shape[1] + (bias is not None)


# ---- dense convolutions (channels-first in, channels-first out) --------------------------------------------------
def conv3d(x_cf, W, bias=None, add_cf=None, relu=False, stride=1, pad=0, dil=1):
    """-> (ref, S) float64 [B, Cout, Do, Do, Do] of act(conv3d(x, W) + bias + add)."""
    x, w = torch.from_numpy(np.asarray(x_cf, np.float64)), torch.from_numpy(np.asarray(W, np.float64))
    ref = F.conv3d(x, w, None, stride=stride, padding=pad, dilation=dil).numpy()
    S = F.conv3d(x.abs(), w.abs(), None, stride=stride, padding=pad, dilation=dil).numpy()
    if bias is not None:
        b = np.asarray(bias, np.float64).reshape(1, -1, 1, 1, 1)
        ref, S = ref + b, S + np.abs(b)
    if add_cf is not None:
        a = np.asarray(add_cf, np.float64)
        ref, S = ref + a, S + np.abs(a)
    return _act(ref, relu), S


def conv_k4s2_K(Cin, split, bias, add):
    return 64 * Cin + (bias is not None) + (add is not None) + (split if split > 1 else 0)


def pack_k4s2(W, c_off, cin):
    """wt[co][tap][ci] = W[co][c_off + ci][tap]."""
    W = np.asarray(W)
    return np.ascontiguousarray(W[:, c_off:c_off + cin].reshape(W.shape[0], cin, 64).transpose(0, 2, 1))


def pack_sparse(W, c_off, Cs):
    """Wp[class][c][slot][co] = W[co][c_off + c][k], k = parity + 2 slot bit per axis (x: bit 0, y: bit 1, z: bit 2)."""
    W = np.asarray(W)
    Cout = W.shape[0]
    Wp = np.zeros((8, Cs, 8, Cout), f32)
    for cls in range(8):
        for slot in range(8):
            kx, ky, kz = (cls & 1) + 2 * (slot & 1), ((cls >> 1) & 1) + 2 * ((slot >> 1) & 1), ((cls >> 2) & 1) + 2 * ((slot >> 2) & 1)
            Wp[cls, :, slot, :] = W[:, c_off:c_off + Cs, kx, ky, kz].T
    return Wp.reshape(-1)


# ---- sparse conv3 ---------------------------------------------------------------------------------------------------
def voxelize(values, points, bi, B, D):
    """The grid sparse conv3 convolves: oracle_np.average_voxelization_3d(mode="gpu") of the rows whose batch index
    is inside [0, B) (origin 0, pitch 1) -> (grid [B, Cs, D, D, D] float32, counts [B, D, D, D] int32)."""
    keep = (bi >= 0) & (bi < B)
    return O.average_voxelization_3d(np.ascontiguousarray(values[keep]), np.ascontiguousarray(points[keep]), bi[keep],
                                     batch_size=B, origin=(0, 0, 0), pitch=1.0, dimensions=(D, D, D), mode="gpu")


def sparse_conv3(grid, W, dense_cf, bias, relu):
    """-> (ref, S, K) channels-first; K = 64 Cs + 2 (the issue's count: taps x channels + dense + bias)."""
    ref, S = conv3d(grid, W, bias, dense_cf, relu, stride=2, pad=1)
    return ref, S, 64 * grid.shape[1] + 2


# ---- mirrors ----------------------------------------------------------------------------------------------------------
def interpolate_cl(vox_cl, X, points, bi):
    """vox_cl [B, X^3, C] -> the bits of oracle_np.interpolate_voxel_grid(mode="gpu"); zero rows where the batch index
    is outside [0, B)."""
    B, _, C = vox_cl.shape
    vox_cf = np.ascontiguousarray(vox_cl.reshape(B, X, X, X, C).transpose(0, 4, 1, 2, 3))
    keep = (bi >= 0) & (bi < B)
    out = np.zeros((len(points), C), f32)
    out[keep] = O.interpolate_voxel_grid(vox_cf, np.ascontiguousarray(points[keep]), bi[keep], mode="gpu")
    return out


def point_prep(pc, vals, origin, pitch, center):
    """contrib/singleview_3d/models/model.py:236,101 in NumPy float32: -> pts [n,3], tc4 [n,4], rows [n,Cv], bi [n]."""
    B, _, P = pc.shape
    n = B * P
    pv = ((pc - origin[:, :, None]) / pitch[:, None, None]).astype(f32)
    pts = np.ascontiguousarray(pv.transpose(0, 2, 1).reshape(n, 3))
    tc4 = np.zeros((n, 4), f32)
    tc4[:, :3] = (f32(center) - pts).astype(f32)
    return pts, tc4, np.ascontiguousarray(vals.transpose(0, 2, 1).reshape(n, -1)), np.repeat(np.arange(B, dtype=np.int32), P)
