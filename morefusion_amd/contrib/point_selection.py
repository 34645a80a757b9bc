"""Point selection shared by the pose networks (contrib/singleview_3d and contrib/singleview_pcd): the reference's
per-object ``where(mask)`` + NumPy-RNG subsample / pad to ``_n_point`` points
(contrib/singleview_3d/models/model.py:191-230; examples/ycb_video/singleview_pcd/contrib/models/model.py:87-105).
A mix-in: the model supplies ``_n_point`` and ``training``."""
import numpy as np
import torch

from .. import _lib


class PointSelection:

    _eval_keep_cache = {}

    def _keep_indices(self, n_point):
        """The reference's subsample / pad of the n valid pixels (model.py:208-219).  In eval
        mode it seeds a fresh ``RandomState(1234)`` per object, i.e. it is a pure function of
        n: memoised, so the GPU does not idle behind a host-side MT19937 permutation."""
        if n_point == 0:
            raise ValueError("an example has no valid point")
        cache = PointSelection._eval_keep_cache
        if not self.training:
            hit = cache.get((n_point, self._n_point))
            if hit is not None:
                return hit
        random_state = np.random.mtrand._rand if self.training else np.random.RandomState(1234)
        if n_point >= self._n_point:
            keep = random_state.permutation(n_point)[: self._n_point]
        else:
            keep = np.r_[np.arange(n_point),
                         random_state.randint(0, n_point, self._n_point - n_point)]
        keep = keep.astype(np.int64)
        if not self.training and len(cache) < 4096:
            cache[(n_point, self._n_point)] = keep
        return keep

    def _select_points(self, pcd):
        """pcd [B,H,W,3] -> flat pixel indices [B,P]: the row-major list of the pixels without a
        NaN coordinate (``where(mask)``, model.py:195) from one launch of ``mf_valid_pixel_order``,
        then the reference's NumPy-RNG subsample / pad of it."""
        B, HW = pcd.shape[0], pcd.shape[1] * pcd.shape[2]
        _lib.require_gpu(pcd)
        pcd = _lib.f32c(pcd)
        order = torch.empty((B, HW), dtype=torch.int32, device=pcd.device)
        counts = torch.empty((B,), dtype=torch.int32, device=pcd.device)
        _lib.check(_lib.lib().mf_valid_pixel_order(pcd.data_ptr(), B, HW, order.data_ptr(), counts.data_ptr(),
                                                   _lib.stream_ptr()), "mf_valid_pixel_order")
        return self._subsample(order, counts.cpu().numpy())  # the one host sync (the RNG needs n_point)

    def _subsample(self, order, counts):
        """order [B,HW] (valid pixels first, row-major), counts [B] on the host -> [B,P] int64:
        ``iy[keep], ix[keep]`` of model.py:207-220 as flat indices."""
        keep = torch.from_numpy(np.stack([self._keep_indices(int(c)) for c in counts])).to(order.device)
        return torch.gather(order, 1, keep).long()
