"""augment_rgbd -- RGBDPoseEstimationDatasetReIndexedBase._augment_rgbd on the device, a minibatch per call.

morefusion/datasets/rgbd_pose_estimation/reindexed.py:38-153 augments one example at a time on the host (imgaug,
cv2).  Here the three stages run as HIP kernels over all ``n`` examples (csrc/augment.hip, DESIGN.md
"Augmentation"):

``augment_mask``  valid mask -> one-sided cut -> 8-connected components -> the largest and a random choice of the
                  others -> crop to the kept mask and ``imgviz.centerize`` back to S x S
``augment_rgb``   linear contrast, HSV multipliers, Gaussian blur, bicubic resize down and back
``augment_pcd``   5 % pixel drop-out and N(0, 3 mm) noise

Randomness has two sources.  The per-example scalars are drawn on the host by ``draw_params`` from one
``numpy.random.RandomState`` into a float64 table ``[n, 12]``; the per-pixel and per-component words come from
Philox4x32-10 on the device, keyed by (seed, the example's key in the table) and indexed by (pixel, stream), so an
example's result depends on its own row and the seed only -- not on its position or its neighbours in the batch.
"""
import numpy as np
import torch

from .. import _lib

N_PARAMS = 12
(P_CUT_CASE, P_CUT_U, P_BLOB_U, P_CONTRAST, P_MUL_H, P_MUL_S, P_MUL_V, P_SIGMA, P_SCALE, P_KEY) = range(10)
N_STATS = 12


def draw_params(n, random_state):
    """The per-example table, float64 [n, 12].  Drawing order (each a vector of n, from ``random_state``):
    cut case ``randint(4)``; cut uniform and blob-count uniform ``random_sample``; contrast alpha ``uniform(0.8,
    1.2)``; H multiplier ``uniform(0.95, 1.05)``; S and V multipliers ``uniform(0.8, 1.2)``; blur sigma
    ``uniform(0, 1)``; resize scale ``uniform(0.25, 1)``; example key ``randint(2**32)``.  Columns 10, 11: zero."""
    rs = random_state
    p = np.zeros((n, N_PARAMS), np.float64)
    p[:, P_CUT_CASE] = rs.randint(0, 4, n)
    p[:, P_CUT_U] = rs.random_sample(n)
    p[:, P_BLOB_U] = rs.random_sample(n)
    p[:, P_CONTRAST] = rs.uniform(0.8, 1.2, n)
    p[:, P_MUL_H] = rs.uniform(0.95, 1.05, n)
    p[:, P_MUL_S] = rs.uniform(0.8, 1.2, n)
    p[:, P_MUL_V] = rs.uniform(0.8, 1.2, n)
    p[:, P_SIGMA] = rs.uniform(0.0, 1.0, n)
    p[:, P_SCALE] = rs.uniform(0.25, 1.0, n)
    p[:, P_KEY] = rs.randint(0, 2 ** 32, n, dtype=np.int64)
    return p


def neutral_params(n):
    """A table that cuts nothing (case 0 at u = 0), draws no extra blob and leaves the colours alone."""
    p = np.zeros((n, N_PARAMS), np.float64)
    p[:, [P_CONTRAST, P_MUL_H, P_MUL_S, P_MUL_V, P_SCALE]] = 1.0
    p[:, P_KEY] = np.arange(n)
    return p


def _check(rgb, pcd):
    if rgb is not None:
        if rgb.dtype != torch.uint8 or rgb.ndim != 4 or rgb.shape[3] != 3 or rgb.shape[1] != rgb.shape[2]:
            raise TypeError("rgb must be uint8 [n, S, S, 3]")
    if pcd is not None:
        if pcd.dtype not in (torch.float32, torch.float64) or pcd.ndim != 4 or pcd.shape[3] != 3 \
                or pcd.shape[1] != pcd.shape[2]:
            raise TypeError("pcd must be float32 or float64 [n, S, S, 3]")
    if rgb is not None and pcd is not None and rgb.shape != pcd.shape:
        raise TypeError("rgb and pcd must have the same shape")
    t = rgb if rgb is not None else pcd
    n, S = int(t.shape[0]), int(t.shape[1])
    if S % 8 or not 8 <= S <= 256:
        raise ValueError("the image size must be a multiple of 8 in 8..256")
    _lib.require_gpu(*[x for x in (rgb, pcd) if x is not None])
    return n, S


def _table(params, n, device):
    p = np.ascontiguousarray(np.asarray(params, np.float64))
    if p.shape != (n, N_PARAMS):
        raise ValueError(f"params must be [{n}, {N_PARAMS}]")
    return torch.from_numpy(p).to(device)


def _workspace(n, S, device):
    nbytes = _lib.lib().mf_augment_workspace_bytes(n, S)
    if nbytes < 0:
        raise ValueError("mf_augment_workspace_bytes refused the size")
    return torch.empty((max(int(nbytes), 16),), dtype=torch.uint8, device=device)


def augment_mask(rgb, pcd, params, seed, return_components=False, workspace=None):
    """-> dict(rgb, pcd, keep [n] bool, kept_mask [n, S, S] bool (before re-centring), stats int32 [n, 12]: final
    box y1 x1 y2 x2, components, drawn K, largest id, kept pixels, cut box; with ``return_components`` also
    ``labels`` and ``sizes`` int32 [n, S, S])."""
    n, S = _check(rgb, pcd)
    dev = rgb.device
    rgb_c, pcd_c = rgb.contiguous(), pcd.contiguous()
    prm = params if isinstance(params, torch.Tensor) else _table(params, n, dev)
    out = dict(rgb=torch.empty_like(rgb_c), pcd=torch.empty_like(pcd_c))
    kept = torch.empty((n, S, S), dtype=torch.uint8, device=dev)
    stats = torch.empty((n, N_STATS), dtype=torch.int32, device=dev)
    keep = torch.empty((n,), dtype=torch.uint8, device=dev)
    labels = torch.empty((n, S, S), dtype=torch.int32, device=dev) if return_components else None
    sizes = torch.empty((n, S, S), dtype=torch.int32, device=dev) if return_components else None
    if n:
        ws = _workspace(n, S, dev) if workspace is None else workspace
        _lib.check(_lib.lib().mf_augment_mask(
            rgb_c.data_ptr(), pcd_c.data_ptr(), int(pcd_c.dtype == torch.float64), prm.data_ptr(), n, S,
            int(seed) & 0xffffffff, out["rgb"].data_ptr(), out["pcd"].data_ptr(), kept.data_ptr(), stats.data_ptr(),
            keep.data_ptr(), _lib.ptr(labels), _lib.ptr(sizes), ws.data_ptr(), _lib.stream_ptr()), "mf_augment_mask")
    out.update(keep=keep.bool(), kept_mask=kept.bool(), stats=stats)
    if return_components:
        out.update(labels=labels, sizes=sizes)
    return out


def augment_rgb(rgb, params, workspace=None):
    n, S = _check(rgb, None)
    rgb_c = rgb.contiguous()
    prm = params if isinstance(params, torch.Tensor) else _table(params, n, rgb.device)
    out = torch.empty_like(rgb_c)
    if n:
        ws = _workspace(n, S, rgb.device) if workspace is None else workspace
        _lib.check(_lib.lib().mf_augment_rgb(rgb_c.data_ptr(), prm.data_ptr(), n, S, out.data_ptr(), ws.data_ptr(),
                                             _lib.stream_ptr()), "mf_augment_rgb")
    return out


def augment_pcd(pcd, params, seed):
    n, S = _check(None, pcd)
    pcd_c = pcd.contiguous()
    prm = params if isinstance(params, torch.Tensor) else _table(params, n, pcd.device)
    out = torch.empty_like(pcd_c)
    if n:
        _lib.check(_lib.lib().mf_augment_pcd(pcd_c.data_ptr(), int(pcd_c.dtype == torch.float64), prm.data_ptr(), n, S,
                                             int(seed) & 0xffffffff, out.data_ptr(), _lib.stream_ptr()),
                   "mf_augment_pcd")
    return out


def _random_state(random_state):
    if random_state is None:
        return np.random.mtrand._rand  # numpy's global generator: np.random.seed controls it
    if isinstance(random_state, np.random.RandomState):
        return random_state
    return np.random.RandomState(int(random_state))


def augment_rgbd(rgb, pcd, random_state=None):
    """rgb uint8 [n, S, S, 3], pcd float32 / float64 [n, S, S, 3] (NaN invalid), device tensors ->
    (rgb, pcd, keep): the three stages in the reference's order; the inputs are not modified.  ``random_state``: an
    int seed or a ``numpy.random.RandomState``; it yields ``draw_params(n, .)`` and then the generator seed
    ``randint(2**32)``.  ``keep[i]`` false: the example's mask was empty at some step, its outputs are padding."""
    n, S = _check(rgb, pcd)
    rs = _random_state(random_state)
    params = draw_params(n, rs)
    seed = int(rs.randint(0, 2 ** 32, dtype=np.int64))
    prm = _table(params, n, rgb.device)
    ws = _workspace(n, S, rgb.device) if n else None
    m = augment_mask(rgb, pcd, prm, seed, workspace=ws)
    return augment_rgb(m["rgb"], prm, workspace=ws), augment_pcd(m["pcd"], prm, seed), m["keep"]
