"""One batch of the reference's evaluation loop, on the device from the network to the metric.

Body of examples/ycb_video/singleview_3d/evaluate.py:81-291 for the objects of one frame: ``model.predict``, the
arg-max-confidence pose per object, ``transformation_matrix``, refinement by ``IccScenes.refine`` (the reference's
``IterativeCollisionCheckLink`` under Adam, alpha 0.01 for the quaternion and 0.001 for the translation) and / or
``icp_registration_batch`` (its ``ICPRegistration.register``), and ADD / ADD-S of every (object, method) against the
ground truth in ONE ``metrics.average_distance_device`` launch.  Poses stay on the device throughout; the two [I]
metric vectors are the only copies to the host.

Where this differs from the reference: ICC starts from the network's quaternion and translation themselves (the
reference goes through the 4 x 4 matrix and back, ``quaternion_from_matrix``), and all objects are refined in one
batched launch per stage.  ICP results are cast to float32, as the reference's ``np.array(..., dtype=np.float32)``.

The opt-in method ``"occupancy"`` (not in ``METHODS``) refines the arg-max poses with ``occupancy_registration_batch``
-- the reference's examples/ycb_video/dense_fusion/eval_densefusion_occupancy.py:94-114 with this network's poses
as the start: the CAD cloud voxel-down-sampled at the object's pitch against ``grid_target`` (occupied) and
``grid_nontarget_empty`` (unoccupied), threshold 2, alpha 0.01; a registration that ends in NaN keeps the start.
"""
import numpy as np
import torch

from ... import metrics
from ...functions.geometry.transformation_matrix import transformation_matrix_batch
from ...synthetic import CLASS_IDS_SYMMETRIC
from ..icc_batch import IccScenes
from ..icp_registration import icp_registration_batch
from ..occupancy_registration import occupancy_registration_batch

METHODS = ("morefusion", "morefusion+icp", "morefusion+icc", "morefusion+icc+icp")
OPTIONAL_METHODS = ("occupancy",)  # accepted by evaluate_batch, not run by default
OCCUPANCY_THRESHOLD, OCCUPANCY_ALPHA = 2, 0.01  # eval_densefusion_occupancy.py:103-108
ICC_ALPHA_QUATERNION, ICC_ALPHA_TRANSLATION = 0.01, 0.001  # evaluate.py:261-263


def argmax_pose(quaternion, translation, confidence):
    """[B,P,4], [B,P,3], [B,P] -> the most confident pose of each object, [B,4] and [B,3] (evaluate.py:94-96)."""
    indices = confidence.argmax(dim=1)
    ar = torch.arange(confidence.shape[0], device=confidence.device)
    return quaternion[ar, indices].contiguous(), translation[ar, indices].contiguous()


def icc_scene(batch, models, class_ids):
    """The arguments of ``IccScenes`` for the objects of one frame: the CAD points with a signed distance
    (``models.get_sdf``, NaN entries dropped: evaluate.py:268-270) and the batch's grids."""
    points, sdfs = [], []
    for cid in class_ids:
        pcd, sdf = models.get_sdf(cid)
        keep = ~np.isnan(np.asarray(sdf))
        points.append(np.asarray(pcd, np.float32)[keep])
        sdfs.append(np.asarray(sdf, np.float32)[keep])
    return dict(points=points, sdf=sdfs, pitch=batch["pitch"], origin=batch["origin"],
                grid_target=batch["grid_target"], grid_nontarget_empty=batch["grid_nontarget_empty"])


def evaluate_batch(model, batch, models, methods=METHODS, frame_index=0, n_icc=30, n_icp=100, n_icc_icp=30,
                   n_occ=100, icc_until_converged=False):
    """``batch``: the network's inputs for the B objects of one frame, arrays or tensors ``[B, ...]`` -- class_id,
    rgb, pcd, pitch, origin, grid_target, grid_nontarget_empty, quaternion_true, translation_true (the keys of
    ``synthetic.transform_example``, concatenated).  ``models``: ``get_pcd(class_id)`` and ``get_sdf(class_id)``.

    Returns ``(rows, transforms)``: the reference's rows -- dicts with frame_index, batch_index, class_id,
    add_or_add_s, add_s, method, the objects of one method after the other -- and ``transforms``: {method: [B,4,4]
    float32 device tensor, cad -> camera}, plus ``"true"``.

    ``icc_until_converged`` (default off: nothing changes): the ICC methods run the loop of the reference's ROS node
    -- at most ``n_icc`` iterations, left once the loss has converged (``IccScenes.refine_until_converged``, the
    node's constants) -- and the result carries the steps taken: ``transforms["icc_n_steps"]`` ([1] int32 device
    tensor; no host synchronisation is added)."""
    methods = tuple(methods)
    if not methods or any(m not in METHODS + OPTIONAL_METHODS for m in methods):
        raise ValueError(f"methods {methods}: one or more of {METHODS + OPTIONAL_METHODS}")
    dev = next(model.parameters()).device
    if dev.type != "cuda":
        raise RuntimeError("evaluate_batch runs on the MI355X: move the model to 'cuda' (there is no CPU fallback)")
    b = {k: torch.as_tensor(v).to(dev) for k, v in batch.items()}
    class_ids = [int(c) for c in torch.as_tensor(batch["class_id"]).tolist()]
    B = len(class_ids)
    with torch.no_grad():
        quaternion, translation, confidence = model.predict(
            class_id=b["class_id"], rgb=b["rgb"], pcd=b["pcd"], pitch=b["pitch"], origin=b["origin"],
            grid_nontarget_empty=b["grid_nontarget_empty"])
        quaternion, translation = argmax_pose(quaternion.float(), translation.float(), confidence)
        transforms = {"true": transformation_matrix_batch(b["quaternion_true"].float().contiguous(),
                                                          b["translation_true"].float().contiguous()),
                      "morefusion": transformation_matrix_batch(quaternion, translation)}
        cads = None
        if any("icp" in m for m in methods):
            cads = [torch.as_tensor(np.asarray(models.get_pcd(c))).to(dev) for c in class_ids]

        def icp(init, iteration):  # source: the depth points without NaN (dropped by the kernel), target: the CAD
            return icp_registration_batch(b["pcd"], cads, init, iteration=iteration)[0].float()

        if "morefusion+icp" in methods:
            transforms["morefusion+icp"] = icp(transforms["morefusion"], n_icp)
        if "morefusion+icc" in methods or "morefusion+icc+icp" in methods:
            scenes = IccScenes([icc_scene(b, models, class_ids)], device=dev)
            q, t = quaternion.clone(), translation.clone()
            adam_m = torch.zeros((B, 7), dtype=torch.float32, device=dev)
            adam_v = torch.zeros((B, 7), dtype=torch.float32, device=dev)
            if icc_until_converged:
                icc_n_steps = scenes.refine_until_converged(q, t, adam_m, adam_v, max_iter=n_icc,
                                                            alpha_q=ICC_ALPHA_QUATERNION, alpha_t=ICC_ALPHA_TRANSLATION)
            else:
                scenes.refine(q, t, adam_m, adam_v, n_icc, alpha_q=ICC_ALPHA_QUATERNION, alpha_t=ICC_ALPHA_TRANSLATION)
            icc = transformation_matrix_batch(q, t)
            if "morefusion+icc" in methods:
                transforms["morefusion+icc"] = icc
            if "morefusion+icc+icp" in methods:
                transforms["morefusion+icc+icp"] = icp(icc, n_icc_icp)
        if "occupancy" in methods:
            from ...extra import open3d as extra_open3d
            pitches = [float(p) for p in torch.as_tensor(batch["pitch"]).reshape(-1).tolist()]
            sources = [extra_open3d.voxel_down_sample(
                torch.as_tensor(np.asarray(models.get_pcd(c), np.float64)).to(dev), p).float()
                for c, p in zip(class_ids, pitches)]
            grids = torch.stack([b["grid_target"].float(), b["grid_nontarget_empty"].float()], dim=1)
            transforms["occupancy"] = occupancy_registration_batch(
                sources, grids, pitch=b["pitch"].float().reshape(-1), origin=b["origin"].float().reshape(B, 3),
                threshold=OCCUPANCY_THRESHOLD, transforms_init=transforms["morefusion"], iteration=n_occ,
                alpha=OCCUPANCY_ALPHA, device=dev, pose_init=(quaternion, translation))[0]
        # every (method, object) item in one launch: the distinct classes' clouds, ground truth as transform1
        classes = sorted(set(class_ids))
        clouds = [models.get_pcd(c) for c in classes]
        index = [classes.index(c) for c in class_ids] * len(methods)
        adds, add_ss = metrics.average_distance_device(
            clouds, transforms["true"].repeat(len(methods), 1, 1), torch.cat([transforms[m] for m in methods]),
            cloud_index=index, device=dev)
    adds, add_ss = adds.cpu().numpy(), add_ss.cpu().numpy()  # the only copies to the host
    rows = []
    for k, method in enumerate(methods):
        for i, cid in enumerate(class_ids):
            add, add_s = float(adds[k * B + i]), float(add_ss[k * B + i])
            rows.append(dict(frame_index=frame_index, batch_index=i, class_id=cid,
                             add_or_add_s=add_s if cid in CLASS_IDS_SYMMETRIC else add, add_s=add_s, method=method))
    out = {m: transforms[m] for m in ("true",) + methods}
    if icc_until_converged and any("icc" in m for m in methods):
        out["icc_n_steps"] = icc_n_steps
    return rows, out
