"""TEST INFRASTRUCTURE: NumPy mirror of csrc/pcdnet.hip (and of mf_pose_epilogue as the point-cloud baseline uses it),
in the kernels' own fp32 operation order, plus float64 evaluations of the same quantities.

fp32 order of a convolution: s = 0; s = fl(s + fl(x[k] * w[k])) for increasing k; v = max(fl(s + bias), 0).
Split form: hi = bf16(v) (round to nearest even), lo = bf16(v - hi).
Pool: row lane j of 8 adds rows j, j + 8, ... in increasing order; ((0 + 1) + (2 + 3)) + ((4 + 5) + (6 + 7)); / P."""
import numpy as np

F32 = np.float32


def bf16_rne(v):
    """float32 -> the nearest bf16 value (ties to even), as float32.  Finite inputs."""
    u = np.ascontiguousarray(v, F32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    return r.astype(np.uint32).view(F32).reshape(np.shape(v))


def bf16_bits(v_bf16_valued):
    """float32 array holding bf16 values -> their 16-bit patterns (int16, what a torch.bfloat16 tensor stores)."""
    return (np.ascontiguousarray(v_bf16_valued, F32).view(np.uint32) >> 16).astype(np.uint16).view(np.int16)


def split(v):
    v = np.asarray(v, F32)
    hi = bf16_rne(v)
    return hi, bf16_rne(v - hi)


def _conv_relu(x, w, b):
    """x [M,K], w [N,K], b [N] fp32 -> relu(x w^T + b) [M,N] in the kernel's order."""
    s = np.zeros((x.shape[0], w.shape[0]), F32)
    for k in range(x.shape[1]):
        s = s + x[:, k:k + 1] * w[None, :, k]
    return np.maximum(s + b[None, :], F32(0))


def stem(x, pcd, pix, center, w_rgb, b_rgb, w_pcd, b_pcd, P):
    """-> (pts [M,3], feat1 [M,128] fp32 = rgb 64 | pcd 64)."""
    M = x.shape[0]
    b = np.arange(M) // P
    pts = pcd.reshape(pcd.shape[0], -1, 3)[b, pix].astype(F32)
    if center is not None:
        pts = pts - center[b]
    return pts, np.concatenate([_conv_relu(x, w_rgb, b_rgb), _conv_relu(pts, w_pcd, b_pcd)], axis=1)


def stem_f64(x, pts, w_rgb, b_rgb, w_pcd, b_pcd):
    """float64 value and the contraction on absolute values (+ |bias|) of the two convolutions, from the fp32 inputs
    the convolutions received (``pts`` as the kernel wrote it)."""
    d = np.float64
    val = np.concatenate([x.astype(d) @ w_rgb.astype(d).T + b_rgb, pts.astype(d) @ w_pcd.astype(d).T + b_pcd], axis=1)
    S = np.concatenate([np.abs(x).astype(d) @ np.abs(w_rgb).astype(d).T + np.abs(b_rgb),
                        np.abs(pts).astype(d) @ np.abs(w_pcd).astype(d).T + np.abs(b_pcd)], axis=1)
    return np.maximum(val, 0), S


def pool(h, B, P):
    h = np.asarray(h, F32).reshape(B, P, -1)
    part = []
    for j in range(8):
        acc = np.zeros((B, h.shape[2]), F32)
        for p in range(j, P, 8):
            acc = acc + h[:, p]
        part.append(acc)
    s = ((part[0] + part[1]) + (part[2] + part[3])) + ((part[4] + part[5]) + (part[6] + part[7]))
    return s / F32(P)


def bias_relu(y, gbias, P):
    b = np.arange(y.shape[0]) // P
    return np.maximum(np.asarray(y, F32) + np.asarray(gbias, F32)[b], F32(0))


def head_layout(v, G):
    """fp32 [M, N] -> the bf16 bit patterns [M, 2 N] of the split rows: head g as hi G | lo G at column 2 G g."""
    hi, lo = split(v)
    M, N = v.shape
    out = np.empty((M, 2 * N), np.int16)
    for g in range(N // G):
        out[:, 2 * G * g:2 * G * g + G] = bf16_bits(hi[:, G * g:G * (g + 1)])
        out[:, 2 * G * g + G:2 * G * (g + 1)] = bf16_bits(lo[:, G * g:G * (g + 1)])
    return out


def epilogue(o, np4, class_id, pts, center, P, n_fg):
    """-> rot [M,4], trans [M,3] in the kernel's fp32 order, conf [M] in float64 (the kernel's expf is not pinned)."""
    M = o.shape[0]
    b = np.arange(M) // P
    fg = np.asarray(class_id)[b] - 1
    r = np.arange(M)
    q = np.stack([o[r, 4 * fg + a] for a in range(4)], axis=1).astype(F32)
    nrm = np.sqrt(((q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2]) + q[:, 3] * q[:, 3]) + F32(1e-5)
    rot = q / nrm[:, None]
    t = np.stack([o[r, np4 + 3 * fg + a] for a in range(3)], axis=1).astype(F32)
    c = np.zeros((M, 3), F32) if center is None else np.asarray(center, F32)[b]
    trans = (pts * F32(1) + c) + t * F32(1)
    conf = 1.0 / (1.0 + np.exp(-o[r, 2 * np4 + fg].astype(np.float64)))
    return rot.astype(F32), trans.astype(F32), conf
