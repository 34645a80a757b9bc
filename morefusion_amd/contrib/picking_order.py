"""Which object to pick first to reach a target: occlusion graph and grasp poses (csrc/pickorder.hip).

What the reference's ``select_picking_order`` node does (ros/src/morefusion_ros/nodes/select_picking_order.py) with
N + 1 pybullet renders per camera frame, NumPy over whole images, skimage and networkx.  Here one launch of the mesh
renderer (geometry/render.py) draws the posed CAD models together (target 0) and each one alone (target 1 + n), and
three kernels measure them (include/mfhip.h ``mf_pick_*``, DESIGN.md "Picking order"):

* ``occluded_by[i, j]``: the pixels that are i's when it stands alone and j's in the composite; ``ratio = occluded_by
  / whole`` off the diagonal is the reference's ``count / mask_whole.sum()``, and an edge i -> j ("i is occluded by
  j") exists where it reaches ``min_ratio``;
* a grasp pose per object: the mean point and the mean surface normal of a central patch, in the camera frame.

Unpinned against the reference: pybullet / OpenGL pixels (as for ``render_meshes``), and the patch.  The reference
takes the patch from ``skimage.segmentation.slic(rgb, n_segments=30, slic_zero=True)`` on a colour render; no colour
is rendered here and SLIC is not run.  The patch is a cell of the grid SLIC seeds its segments on -- S x S pixels, S =
max(1, isqrt(h w // 30)) over the h x w box of the object -- which is what SLIC stays near on an untextured image.

``get_picking_order`` is plain Python on the host.
"""
import numpy as np
import torch

from .. import _lib
from ..geometry.render import RenderPlan

MAX_OBJECTS = 64  # MF_PICK_MAX_OBJECTS (include/mfhip.h)


def quaternion_from_two_vectors(v1, v2):
    """The (w, x, y, z) unit quaternion of the shortest rotation taking the direction of ``v1`` to that of ``v2``:
    (|v1| |v2| + v1 . v2, v1 x v2) normalised; for opposite directions the half turn about an axis perpendicular to
    ``v1``.  float64 on the host; the vectors need not be unit (``SelectPickingOrder`` passes the mean normal
    un-normalised, as the reference does).

    The reference's function of this name puts sqrt(|v1|^2 + |v2|^2) where |v1| |v2| = sqrt(|v1|^2 |v2|^2) belongs,
    so its quaternion turns about the right axis but by too small an angle (tan(phi / 2) = sin / (sqrt(2) + cos) for
    unit vectors) and the gripper's axis it yields is not the surface normal.  This one is the rotation."""
    v1, v2 = np.asarray(v1, np.float64), np.asarray(v2, np.float64)
    x, y, z = np.cross(v1, v2)
    w = np.linalg.norm(v1) * np.linalg.norm(v2) + np.dot(v1, v2)
    q = np.array([w, x, y, z], np.float64)
    norm = np.linalg.norm(q)
    if norm == 0.0 and np.linalg.norm(v1) > 0.0 and np.linalg.norm(v2) > 0.0:  # opposite: any perpendicular axis
        axis = np.cross(v1, np.eye(3)[np.argmin(np.abs(v1))])
        return np.concatenate([[0.0], axis / np.linalg.norm(axis)])
    with np.errstate(invalid="ignore", divide="ignore"):
        return q / norm


class OcclusionPlan:
    """The buffers of one ``occlusion_analysis``; ``render`` / ``occlusion`` / ``grasp`` are its launches
    (``occlusion_analysis`` runs them in order, the profile script times them one by one)."""

    def __init__(self, meshes, Ts_cad2cam, K, height, width, instance_ids=None, mesh_index=None, device=None):
        mesh_index = list(range(len(meshes))) if mesh_index is None else [int(m) for m in mesh_index]
        n = len(mesh_index)
        if n > MAX_OBJECTS:
            raise ValueError(f"{n} objects: at most MF_PICK_MAX_OBJECTS = {MAX_OBJECTS} per call")
        ids = list(range(n)) if instance_ids is None else [int(i) for i in np.asarray(instance_ids).reshape(-1)]
        if len(ids) != n:
            raise ValueError("instance_ids differ in length from the items")
        if len(set(ids)) != n or (ids and min(ids) < 0):
            raise ValueError("instance ids must be distinct and >= 0 (-1 is the background)")
        T = np.asarray(Ts_cad2cam.detach().cpu() if isinstance(Ts_cad2cam, torch.Tensor) else Ts_cad2cam,
                       np.float64).reshape(-1, 4, 4)
        if T.shape[0] != n:
            raise ValueError(f"{n} items but {T.shape[0]} transforms")
        self.n, self.ids = n, np.asarray(ids, np.int32)
        self.height, self.width = int(height), int(width)
        self.K = (float(K[0][0]), float(K[1][1]), float(K[0][2]), float(K[1][2]))
        # item n into the composite (target 0), item N + n alone (target 1 + n): the same mesh, pose and id
        self.plan = RenderPlan(meshes, np.concatenate([T, T]), K, height, width,
                               targets=[0] * n + list(range(1, n + 1)), instance_ids=ids + ids,
                               mesh_index=mesh_index + mesh_index, device=device)
        dev = self.device = self.plan.device
        self.item_id = torch.as_tensor(self.ids).to(dev)
        self.out = dict(whole=torch.zeros(n, dtype=torch.int32, device=dev),
                        occluded_by=torch.zeros((n, n), dtype=torch.int32, device=dev),
                        bbox=torch.zeros((n, 4), dtype=torch.int32, device=dev),
                        cell=torch.full((n,), -1, dtype=torch.int32, device=dev),
                        translation=torch.full((n, 3), float("nan"), dtype=torch.float64, device=dev),
                        normal=torch.full((n, 3), float("nan"), dtype=torch.float64, device=dev))
        if dev.type == "cuda":
            _lib.require_gpu(self.item_id, *self.out.values())

    def render(self):
        return self.plan.run()

    def occlusion(self):
        o, r = self.out, self.plan.out
        _lib.check(_lib.lib().mf_pick_occlusion(_lib.ptr(r["instance"]), _lib.ptr(self.item_id), self.n, self.height,
                                                self.width, _lib.ptr(o["whole"]), _lib.ptr(o["occluded_by"]),
                                                _lib.ptr(o["bbox"]), _lib.stream_ptr()), "mf_pick_occlusion")

    def grasp(self):
        o, r = self.out, self.plan.out
        fx, fy, cx, cy = self.K
        _lib.check(_lib.lib().mf_pick_grasp(_lib.ptr(r["depth"]), _lib.ptr(r["instance"]), _lib.ptr(self.item_id),
                                            _lib.ptr(o["bbox"]), self.n, self.height, self.width, fx, fy, cx, cy,
                                            _lib.ptr(o["cell"]), _lib.ptr(o["translation"]), _lib.ptr(o["normal"]),
                                            _lib.stream_ptr()), "mf_pick_grasp")

    def run(self):
        self.render()
        if self.n:
            self.occlusion()
            self.grasp()
        return self.out


def occlusion_analysis(meshes, Ts_cad2cam, K, height, width, instance_ids=None, mesh_index=None, device=None):
    """Item n = ``meshes[n]`` (``meshes[mesh_index[n]]`` with ``mesh_index``) at ``Ts_cad2cam[n]`` (float64 4 x 4)
    with the id ``instance_ids[n]`` (default n; distinct, >= 0) through the pinhole ``K``.  Returns a dict:
    ``instance`` int32 [H, W] device tensor, the composite (-1: background), and NumPy arrays -- ``instance_ids``
    [N]; ``whole`` int32 [N], the pixels of item n standing alone; ``occluded_by`` int32 [N, N], entry [i, j] the
    pixels that are i's alone and j's in the composite (the diagonal: i's visible pixels); ``bbox`` int32 [N, 4] =
    (min_row, min_col, max_row + 1, max_col + 1) of item n alone, zeros without pixels; ``ratio`` float64 [N, N] =
    ``occluded_by / whole`` with the diagonal (and the rows of items without pixels) zero; the grasp pose in the
    CAMERA frame: ``translation`` [N, 3], ``normal`` [N, 3] (a mean of unit normals: not unit), ``quaternion``
    [N, 4] (wxyz, ``quaternion_from_two_vectors((0, 0, 1), normal)``: the gripper's z axis onto the normal),
    ``cell`` int32 [N] (-1 without pixels).  More than ``MAX_OBJECTS`` items raise ``ValueError``."""
    plan = OcclusionPlan(meshes, Ts_cad2cam, K, height, width, instance_ids, mesh_index, device)
    out = {k: v.cpu().numpy() for k, v in plan.run().items()}
    n = plan.n
    whole = out["whole"].astype(np.float64)
    ratio = np.zeros((n, n), np.float64)
    np.divide(out["occluded_by"], whole[:, None], out=ratio, where=whole[:, None] > 0)
    ratio[np.arange(n), np.arange(n)] = 0.0
    quaternion = np.full((n, 4), np.nan)
    for k in range(n):
        if not np.isnan(out["normal"][k]).any():
            quaternion[k] = quaternion_from_two_vectors([0.0, 0.0, 1.0], out["normal"][k])
    return dict(instance=plan.plan.out["instance"][0], instance_ids=plan.ids, ratio=ratio, quaternion=quaternion,
                **out)


def _weighted(edges):
    """{(i, j): pixels}, or an iterable of (i, j) pairs (one pixel each) -> {i: {j: pixels}} without self-edges."""
    adj = {}
    for i, j in edges:
        adj.setdefault(i, {})
        adj.setdefault(j, {})
        if i != j:
            adj[i][j] = edges[(i, j)] if isinstance(edges, dict) else 1
    return adj


def get_picking_order(edges, target, nodes=None):
    """The order in which to remove objects so that ``target`` becomes free, ``target`` last.  ``edges``: ``{(i, j):
    pixels}`` (or an iterable of ``(i, j)`` pairs), an edge i -> j meaning "i is occluded by j";
    ``nodes``: further nodes without edges.

    As the reference's ``get_picking_order``: repeatedly collect the leaves (nodes that nothing occludes) reachable
    from ``target`` along the edges, append them -- in ascending id here; the reference iterates a set -- and remove
    them from the graph, until ``target`` itself is a leaf and is appended last.  Nodes not reachable from ``target``
    never enter the order.

    Cycles (A occludes B and B occludes A): the reference recurses for ever.  Here, when ``target`` is not a leaf
    and no node reachable from it is one, the reachable node other than ``target`` with the smallest summed pixel
    count on its outgoing edges (the least occluded one) is treated as a leaf, the lowest id on a tie."""
    adj = _weighted(edges)
    for node in (() if nodes is None else nodes):
        adj.setdefault(node, {})
    adj.setdefault(target, {})
    order = []
    while True:
        reach, stack = {target}, [target]
        while stack:
            for j in adj[stack.pop()]:
                if j not in reach:
                    reach.add(j)
                    stack.append(j)
        leaves = sorted(n for n in reach if not adj[n])
        if target in leaves:
            order.append(target)
            return order
        if not leaves:
            leaves = [min((n for n in reach if n != target), key=lambda n: (sum(adj[n].values()), n))]
        for leaf in leaves:
            order.append(leaf)
            del adj[leaf]
            for out in adj.values():
                out.pop(leaf, None)


class SelectPickingOrder:
    """``models``: ``{class_id: (vertices, faces)}`` or anything with ``get_cad(class_id)`` (``YCBVideoModels``).
    A call takes the posed objects of one frame and returns dict(``order``: instance ids to pick, the target last,
    [] if no visible object has ``target_class_id``; ``edges``: {(i, j): pixels of i hidden by j} for the pairs
    with ``ratio >= min_ratio``; ``quaternion`` / ``translation``: {instance id: grasp pose in the camera frame}
    per node; ``analysis``: the dict of ``occlusion_analysis``).  Nodes are the instances with at least one visible
    pixel in the composite, as the reference iterates ``np.unique`` of its render; with several nodes of the target
    class the highest instance id is the target, the one the reference's loop keeps."""

    def __init__(self, models, target_class_id, min_ratio=0.1, device=None):
        self._models, self._target, self._min_ratio, self._device = models, int(target_class_id), min_ratio, device

    def _cad(self, class_id):
        cad = self._models[class_id] if isinstance(self._models, dict) else self._models.get_cad(class_id)
        return cad[0], cad[1]

    def __call__(self, class_ids, instance_ids, Ts_cad2cam, K, height, width):
        class_ids = [int(c) for c in np.asarray(class_ids).reshape(-1)]
        ids = [int(i) for i in np.asarray(instance_ids).reshape(-1)]
        classes = sorted(set(class_ids))
        res = occlusion_analysis([self._cad(c) for c in classes], Ts_cad2cam, K, height, width, instance_ids=ids,
                                 mesh_index=[classes.index(c) for c in class_ids], device=self._device)
        visible = np.diagonal(res["occluded_by"]) > 0
        nodes = sorted(ids[k] for k in range(len(ids)) if visible[k])
        edges = {(ids[i], ids[j]): int(res["occluded_by"][i, j])
                 for i in range(len(ids)) for j in range(len(ids))
                 if i != j and visible[i] and visible[j] and res["ratio"][i, j] >= self._min_ratio}
        targets = [ids[k] for k in range(len(ids)) if visible[k] and class_ids[k] == self._target]
        order = get_picking_order(edges, max(targets), nodes) if targets else []
        return dict(order=order, edges=edges, analysis=res,
                    quaternion={ids[k]: res["quaternion"][k] for k in range(len(ids)) if visible[k]},
                    translation={ids[k]: res["translation"][k] for k in range(len(ids)) if visible[k]})
