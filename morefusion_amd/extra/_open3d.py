"""morefusion/extra/_open3d.py on the device: open3d's voxel_down_sample restated (csrc/icpreg.hip)."""
import numpy as np
import torch


def voxel_down_sample(points, voxel_size):
    """[n, 3] points (rows with a NaN dropped) -> voxel means, float64, in (i, j, k) voxel order.
    NumPy in, NumPy out; a tensor gives a float64 tensor on its device."""
    from ..contrib.icp_registration import voxel_down_sample_batch
    out, off, cnt = voxel_down_sample_batch([points], voxel_size)
    res = out[:int(cnt[0])]
    return res if isinstance(points, torch.Tensor) else res.cpu().numpy().astype(np.float64)
