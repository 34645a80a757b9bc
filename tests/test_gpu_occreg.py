"""csrc/occreg.hip on the MI355X: bitwise against the NumPy mirror (tests/occreg_ref.py), against the executed
reference, teacher-forced against the host-loop OccupancyRegistration with float64 as the yardstick, and end to end
through register_fused and evaluate_batch's "occupancy" method.

Teacher-forced figures measured on the MI355X (16^3 grid, 300 points, 5 steps; error against the float64 evaluation,
relative to the largest float64 gradient component) are recorded in DESIGN.md "Occupancy registration"."""
import numpy as np
import pytest
import torch

import morefusion_amd as mf
import occreg_cases as C
import occreg_ref as R

pytestmark = pytest.mark.gpu
f32 = np.float32


class GpuBackend:
    def __init__(self):
        self.lib = mf._lib.lib()

    @staticmethod
    def to_dev(a):
        return torch.from_numpy(np.ascontiguousarray(a)).cuda()

    @staticmethod
    def to_np(t):
        torch.cuda.synchronize()
        return t.cpu().numpy()

    @staticmethod
    def ptr(t):
        return None if t is None else t.data_ptr()


@pytest.fixture(scope="module")
def be():
    torch.cuda.synchronize()  # the checks launch on the null stream
    return GpuBackend()


def test_loss_grad_bitwise_vs_mirror(be):
    C.check_loss_grad_bitwise(be)


@pytest.mark.parametrize("n_iter", [1, 2, 7])
def test_refine_bitwise_vs_mirror(be, n_iter):
    C.check_refine_bitwise(be, n_iter)


def test_refine_across_launches_bitwise_vs_mirror(be):
    C.check_refine_across_launches(be)


def test_micro_cases(be):
    C.check_micro_cases(be)


def test_loss_grad_vs_executed_reference(be):
    C.check_against_executed_reference(be)


def test_teacher_forced_vs_host_loop_with_float64_yardstick(be):
    """OccupancyRegistration.register_iterative for 5 steps on the 16^3 / P = 300 object; at every pose it visits,
    mf_occreg_loss_grad and the link's autograd loss / gradients are both compared with the float64 evaluation of the
    same formula: the new path's error may be at most twice the host-loop path's own."""
    o = C.batch_objects()[2]
    occ, unocc = C.occ_unocc(o)
    reg = mf.contrib.OccupancyRegistration(o["points"], o["grid"], pitch=float(o["pitch"]),
                                           origin=tuple(float(x) for x in o["origin"]), threshold=float(o["thr"]),
                                           transform_init=C.pose_matrix(o["q"], o["t"]).astype(np.float64))
    link = reg._optimizer.target
    bt = C.Batch(be, [o])
    it = reg.register_iterative(iteration=5)
    next(it)
    worst = dict(new=0.0, host=0.0)
    for step in range(6):
        q = link.quaternion.detach().cpu().numpy().astype(f32)
        t = link.translation.detach().cpu().numpy().astype(f32)
        loss_h = link(points_source=reg._points_source, grid_target=reg._grid_target, pitch=reg._pitch,
                      origin=reg._origin, threshold=reg._threshold)
        loss_h.backward()
        host = (float(loss_h.detach()), link.quaternion.grad.cpu().numpy().astype(np.float64),
                link.translation.grad.cpu().numpy().astype(np.float64))
        link.cleargrads()
        loss_n, gq_n, gt_n = bt.loss_grad(q[None], t[None])
        new = (float(loss_n[0]), gq_n[0].astype(np.float64), gt_n[0].astype(np.float64))
        ref = R.loss_grad_f64(o["points"], occ, unocc, q, t, pitch=o["pitch"], origin=o["origin"], threshold=o["thr"])
        scale = (abs(ref[0]), float(np.abs(ref[1]).max()), float(np.abs(ref[2]).max()))
        err = {name: [float(np.abs(np.asarray(got[k]) - ref[k]).max()) / scale[k] for k in range(3)]
               for name, got in (("new", new), ("host", host))}
        print(f"step {step}: relative error to float64 (loss, gq, gt): new {err['new']}, host loop {err['host']}")
        for k, what in enumerate(("loss", "gq", "gt")):
            assert err["new"][k] <= 2.0 * err["host"][k], (step, what, err)
        worst = {n: max(worst[n], max(err[n])) for n in worst}
        if step < 5:
            next(it)
    print("worst relative error: new", worst["new"], "host loop", worst["host"])


def _frame_tensors():
    return C.synthetic_frame()


def test_register_fused_refines_the_synthetic_frame():
    for o in _frame_tensors():
        reg = mf.contrib.OccupancyRegistration(o["points"], o["grid"], pitch=float(o["pitch"]),
                                               origin=tuple(float(x) for x in o["origin"]),
                                               threshold=C.FRAME_THRESHOLD, transform_init=o["T_init"].astype(np.float64),
                                               alpha=C.FRAME_ALPHA)
        T0 = reg._transform
        T = reg.register_fused(iteration=C.FRAME_ITERATIONS)
        assert isinstance(T, np.ndarray) and T.shape == (4, 4) and np.array_equal(T, reg._transform)
        before, after = C.add_metric(o["points"], o["T_gt"], T0), C.add_metric(o["points"], o["T_gt"], T)
        print(f"ADD {before * 1000:.2f} mm -> {after * 1000:.2f} mm")
        assert after <= before and not np.array_equal(T, T0)


class _Poses(torch.nn.Module):
    """Stands in for the network: ``predict`` returns the given poses (two candidates per object, the given one the
    more confident)."""

    def __init__(self, q, t):
        super().__init__()
        self.anchor = torch.nn.Parameter(torch.zeros(1))
        self.q, self.t = q, t

    def predict(self, **kw):
        B = self.q.shape[0]
        q = torch.stack([torch.tensor([1.0, 0, 0, 0], device=self.q.device).repeat(B, 1), self.q], 1)
        t = torch.stack([torch.zeros_like(self.t), self.t], 1)
        conf = torch.tensor([[0.1, 0.9]], device=self.q.device).repeat(B, 1)
        return q, t, conf


class _Clouds:
    def __init__(self, clouds):
        self.clouds = clouds

    def get_pcd(self, class_id):
        return self.clouds[class_id]


def test_evaluate_batch_occupancy_method_refines_the_synthetic_frame():
    from morefusion_amd.contrib.singleview_3d import METHODS, evaluate_batch
    from morefusion_amd.geometry.quaternion_from_matrix import quaternion_from_matrix, translation_from_matrix
    assert "occupancy" not in METHODS
    objs = C.synthetic_frame()
    B = len(objs)
    ids = [100 + b for b in range(B)]  # a cloud per object, whatever its class
    # the evaluation down-samples the cloud at the object's pitch: the lattice's surface points are one per voxel already
    models = _Clouds({i: o["points"].astype(np.float64) for i, o in zip(ids, objs)})
    qs = np.stack([quaternion_from_matrix(o["T_init"].astype(np.float64)) for o in objs]).astype(f32)
    ts = np.stack([translation_from_matrix(o["T_init"].astype(np.float64)) for o in objs]).astype(f32)
    model = _Poses(torch.from_numpy(qs).cuda(), torch.from_numpy(ts).cuda()).cuda()
    batch = dict(class_id=np.asarray(ids, np.int32), rgb=np.zeros((B, 3, 8, 8), f32), pcd=np.zeros((B, 3, 8, 8), f32),
                 pitch=np.asarray([o["pitch"] for o in objs], f32), origin=np.stack([o["origin"] for o in objs]),
                 grid_target=np.stack([o["grid"][0] for o in objs]),
                 grid_nontarget_empty=np.stack([o["grid"][1] for o in objs]),
                 quaternion_true=np.stack([quaternion_from_matrix(o["T_gt"].astype(np.float64)) for o in objs]).astype(f32),
                 translation_true=np.stack([translation_from_matrix(o["T_gt"].astype(np.float64)) for o in objs]).astype(f32))
    rows, T = evaluate_batch(model, batch, models, methods=("morefusion", "occupancy"), n_occ=C.FRAME_ITERATIONS)
    assert [r["method"] for r in rows] == ["morefusion"] * B + ["occupancy"] * B and T["occupancy"].shape == (B, 4, 4)
    for b in range(B):
        before, after = rows[b]["add_or_add_s"], rows[B + b]["add_or_add_s"]
        print(f"object {b}: ADD {before * 1000:.2f} mm -> {after * 1000:.2f} mm")
        assert np.isfinite(after) and after <= before
        assert not torch.equal(T["occupancy"][b], T["morefusion"][b])
    with pytest.raises(ValueError):
        evaluate_batch(model, batch, models, methods=("occupancy", "nonsense"))
