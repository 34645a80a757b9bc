"""The instance-tracking entry points of the C ABI without a GPU: the workspace and stats sizes are host-only
arithmetic, bad sizes are refused before any launch, and the ops refuse CPU tensors instead of falling back."""
import numpy as np
import pytest
import torch

import morefusion_amd as mf
from morefusion_amd.contrib import InstanceTracker, MultiInstanceOctreeMapping, render_instance_maps, track_instance_ids
from morefusion_amd.contrib.instance_tracking import transform_points


def test_workspace_and_stats_sizes_are_host_only_arithmetic():
    L = mf._lib.lib()
    ws = L.mf_occtrack_workspace_bytes
    n = ws(480, 640, 8)
    # a 64-bit depth key per stride-2 pixel, two int32 images (parents + counts / row minima + maxima), 2 x n_ref flags
    assert n >= 8 * 240 * 320 + 2 * 4 * 480 * 640 + 8 * 8 and n < 8 * 240 * 320 + 2 * 4 * 480 * 640 + 4096
    assert n % 16 == 0
    assert ws(121, 163, 5) >= 8 * 61 * 82 + 2 * 4 * 121 * 163 + 40  # odd sizes: the stride-2 grid rounds up
    assert ws(480, 640, 40) > n and ws(481, 640, 8) > n
    assert ws(0, 640, 8) < 0 and ws(480, -1, 8) < 0 and ws(480, 640, -1) < 0 and ws(480, 640, 1025) < 0
    assert ws(1 << 16, 1 << 15, 1) < 0  # more than 2^30 pixels
    st = L.mf_occtrack_stats_elems
    assert st(3, 3) == 9 + 9 + 9 + 12 and st(40, 40) == 1600 + 120 + 120 + 160
    assert st(0, 0) == 1 and st(-1, 3) < 0 and st(3, 1025) < 0


def test_bad_sizes_are_refused_before_any_launch():
    L = mf._lib.lib()
    assert L.mf_occtrack_render(None, None, None, 0.0, 0.0, 0.0, None, None, 1, 0, 640, None, None, None, None) < 0
    assert b"mf_occtrack_render" in L.mf_last_error_string()
    assert L.mf_occtrack_overlap(None, None, 480, 640, None, 2000, None, 1, None, None) < 0
    assert L.mf_occtrack_assign(None, None, 1, 1, 480, 640, 40000, 80, 60, 0.4, 0.9, None, None, None, None, None) < 0
    assert L.mf_occtrack_clean(None, 480, 640, 400, -1, None, None, None) < 0
    assert L.mf_occtrack_transform(None, None, -1, None, None) < 0
    assert L.mf_occtrack_transform(None, None, 0, None, None) == 0  # nothing to do: no launch


def test_tracking_ops_refuse_cpu_tensors_loudly():
    pts = torch.zeros(12, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        transform_points(pts, np.eye(4), device="cpu")
    label = torch.zeros((3, 4), dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        track_instance_ids(label, label, [1], [0], torch.zeros(1, dtype=torch.int32))
    m = MultiInstanceOctreeMapping(device="cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        render_instance_maps(m, pts, np.eye(3), np.eye(4), 3, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        InstanceTracker(m).track(np.zeros((3, 4, 3), np.float32), np.zeros((3, 4), np.int32), {0: 1}, np.eye(3), np.eye(4))
