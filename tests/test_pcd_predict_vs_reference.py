"""The point-cloud baseline's ``Model.predict`` against golden outputs produced by EXECUTING THE REFERENCE'S OWN NETWORK
CODE (tools/gen_pcd_predict_golden.py: examples/ycb_video/singleview_pcd/contrib/models/model.py, resnet.py, pspnet.py
on the torch-CPU stand-in for Chainer; weights = this package's model under ``torch.manual_seed(0)``).  Two inputs: the
batch of two objects with more than 1000 valid points each (the subsample branch) and its first object cut down to 700
valid points (the pad branch).  CPU: the stock-torch formulation.  GPU: the shipped kernel path.

Translation is compared as the offset translation - point: this network's translation head is in metres."""
import numpy as np
import pytest
import torch

from conftest import golden


def few_valid_points(pcd, n_keep):
    """As the generator: keep the crop's first ``n_keep`` valid pixels (row-major), NaN elsewhere."""
    pcd = np.array(pcd, dtype=np.float32)
    flat = pcd.reshape(-1, 3)
    valid = np.flatnonzero(~np.isnan(flat).any(axis=1))
    flat[valid[n_keep:]] = np.nan
    return pcd


def _cases():
    import morefusion_amd as mf
    g = golden("ref_pcd_predict.npz")
    b = mf.synthetic.make_singleview_batch(int(g["batch_size"]), seed=int(g["seed"]))
    few = few_valid_points(b["pcd"][0], int(g["few_valid"]))[None]
    cases = {"full": (b["class_id"], b["rgb"], b["pcd"]), "few": (b["class_id"][:1], b["rgb"][:1], few)}
    counts = [int((~np.isnan(p.reshape(-1, 3)).any(1)).sum()) for c in cases.values() for p in c[2]]
    assert min(counts) < 1000 < max(counts)  # both selection branches
    return g, {k: dict(class_id=torch.as_tensor(c), rgb=torch.as_tensor(r), pcd=torch.as_tensor(p))
               for k, (c, r, p) in cases.items()}


def _model(g):
    from morefusion_amd.contrib.singleview_pcd.models import Model
    torch.manual_seed(int(g["weight_seed"]))
    return Model(n_fg_class=21).eval()


def _check(outs, g, tag, tol):
    q, t, c = (x.detach().cpu().numpy() for x in outs)
    off = t - g[f"{tag}__points"]
    for name, got, ref in (("quaternion", q, g[f"{tag}__quaternion"]), ("confidence", c, g[f"{tag}__confidence"]),
                           ("offset", off, g[f"{tag}__offset"])):
        print(f"PCD predict vs reference [{tag}] {name}: max |diff| = {np.abs(got - ref).max():.3e} (gate {tol:g})")
    np.testing.assert_allclose(q, g[f"{tag}__quaternion"], rtol=0, atol=tol)
    np.testing.assert_allclose(c, g[f"{tag}__confidence"], rtol=0, atol=tol)
    np.testing.assert_allclose(off, g[f"{tag}__offset"], rtol=0, atol=tol)


def _centers(model, pcd):
    from morefusion_amd.geometry.instance_crops import valid_points_median
    return valid_points_median(pcd.float()).cpu().numpy()


def test_predict_torch_formulation_vs_reference_network_code(monkeypatch):
    from oracle import oracle_np as O
    from morefusion_amd.contrib.singleview_pcd.models import Model

    def select_cpu(self, pcd):
        order, counts = O.valid_pixel_order(pcd.numpy())
        return self._subsample(torch.from_numpy(order), counts)

    monkeypatch.setattr(Model, "_select_points", select_cpu)
    g, cases = _cases()
    model = _model(g)
    model.sparse_pspnet_tail = False  # dense decoder + gather, as the reference
    with torch.no_grad():
        for tag, inp in cases.items():
            _check(model.predict(**inp), g, tag, 2e-4)
            c = _centers(model, inp["pcd"])
            assert np.array_equal(c.view(np.int32), g[f"{tag}__center"].view(np.int32))  # to the last bit


@pytest.mark.gpu
def test_predict_kernel_path_vs_reference_network_code():
    g, cases = _cases()
    model = _model(g).cuda()
    assert model.pcd_kernels
    with torch.no_grad():
        for tag, inp in cases.items():
            inp = {k: v.cuda() for k, v in inp.items()}
            model.predict(**inp)  # MIOpen solver choice settles on the first call of a shape
            _check(model.predict(**inp), g, tag, 1e-3)
            assert model._pcd_kernels_op is not None  # the kernel path ran
            c = _centers(model, inp["pcd"])
            assert np.array_equal(c.view(np.int32), g[f"{tag}__center"].view(np.int32))
