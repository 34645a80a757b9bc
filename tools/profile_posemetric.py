#!/usr/bin/env python
"""Timings of the float64 pose metric (csrc/posemetric.hip) at an evaluation pass's size: 8 objects x 4 methods = 32
items of P = 2620 points (a dense YCB model cloud), 8 distinct clouds.  Prints CSV rows case,stage,median_us,min_us
for profiles/posemetric_table.csv:

* ``kernels``: the two launches of ``mf_average_distance_f64`` between device events, inputs packed ahead;
* ``metric_call``: ``metrics.average_distance_device`` with its packing and the copy of the [32] results back;
* ``evaluate_on_device`` / ``evaluate_host``: ``Model.evaluate`` for the 8 objects (one method), device path and the
  host path (a k-d tree per object), host clock around a device synchronise.

The FP64 rate counts the 9 VALU operations of a pair (3 subtractions, 3 products, 2 additions, 1 minimum), nothing
fused, against 256 CUs x 4 SIMDs x 16 lanes per clock at 2.4 GHz = 39.3 T unfused FP64 operations/s."""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import morefusion_amd as mf  # noqa: E402
from morefusion_amd import _lib  # noqa: E402
from morefusion_amd.contrib.singleview_3d.models import Model, PitchTableModels  # noqa: E402
from morefusion_amd.metrics import PackedClouds  # noqa: E402
from tools.profile_render import time_stage  # noqa: E402

P, OBJECTS, METHODS = 2620, 8, 4
PEAK_OPS = 256 * 4 * 16 * 2.4e9


def host_clock(fn, n=20, warm=3):
    ts = []
    for k in range(warm + n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if k >= warm:
            ts.append((time.perf_counter() - t0) * 1e6)
    return float(np.median(ts)), float(np.min(ts))


def main():
    rs = np.random.RandomState(0)
    class_ids = sorted(mf.synthetic.CLASS_PITCH)[:OBJECTS]
    pcds = {c: rs.uniform(-0.1, 0.1, (P, 3)) for c in class_ids}
    q = rs.normal(size=(OBJECTS, 4)).astype(np.float32)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    t = rs.uniform(-0.3, 0.3, (OBJECTS, 3)).astype(np.float32) + np.float32([0, 0, 0.8])
    q_pred = q + rs.normal(0, 0.02, q.shape).astype(np.float32)
    t_pred = t + rs.normal(0, 0.005, t.shape).astype(np.float32)
    dev = lambda x: torch.as_tensor(x).cuda()  # noqa: E731
    T_true = mf.functions.transformation_matrix(dev(q), dev(t)).double().repeat(METHODS, 1, 1).contiguous()
    T_pred = mf.functions.transformation_matrix(dev(q_pred), dev(t_pred)).double().repeat(METHODS, 1, 1).contiguous()
    index = list(range(OBJECTS)) * METHODS
    items = len(index)
    packed = PackedClouds([pcds[c] for c in class_ids], "cuda")
    item_cloud = torch.as_tensor(np.asarray(index, np.int32)).cuda()
    L = _lib.lib()
    ws = torch.empty(L.mf_average_distance_f64_workspace_bytes(items, P) // 8, dtype=torch.float64, device="cuda")
    add, add_s = torch.empty(items, dtype=torch.float64, device="cuda"), torch.empty(items, dtype=torch.float64, device="cuda")

    def kernels():
        _lib.check(L.mf_average_distance_f64(packed.points.data_ptr(), packed.offsets.data_ptr(), item_cloud.data_ptr(),
                                             T_true.data_ptr(), T_pred.data_ptr(), OBJECTS, items, P, 1,
                                             add.data_ptr(), add_s.data_ptr(), ws.data_ptr(), _lib.stream_ptr()), "metric")

    print("case,stage,median_us,min_us")
    med, lo = time_stage(kernels, n=50, warm=10)
    print(f"eval8x4,kernels,{med:.1f},{lo:.1f}")
    ops = 9.0 * items * P * P
    print(f"# kernels: {ops / 1e9:.2f} G FP64 VALU operations, {ops / (med * 1e-6) / 1e12:.2f} T/s at the median = "
          f"{100 * ops / (med * 1e-6) / PEAK_OPS:.1f} % of {PEAK_OPS / 1e12:.1f} T/s")
    med, lo = host_clock(lambda: [x.cpu() for x in mf.metrics.average_distance_device(
        packed, T_true, T_pred, cloud_index=index)])
    print(f"eval8x4,metric_call,{med:.1f},{lo:.1f}")
    model = Model(n_fg_class=21, models=PitchTableModels(pcds))
    kw = dict(class_id=torch.as_tensor(class_ids), quaternion_true=dev(q), translation_true=dev(t),
              quaternion_pred=dev(q_pred), translation_pred=dev(t_pred))
    a, b = model.evaluate(**kw), model.evaluate(on_device=True, **kw)
    print("# evaluate host", a, "device", b, "max difference", max(abs(a[k] - b[k]) for k in a))
    med, lo = host_clock(lambda: model.evaluate(on_device=True, **kw))
    print(f"eval8,evaluate_on_device,{med:.1f},{lo:.1f}")
    med, lo = host_clock(lambda: model.evaluate(**kw), n=10, warm=2)
    print(f"eval8,evaluate_host,{med:.1f},{lo:.1f}", flush=True)


if __name__ == "__main__":
    main()
