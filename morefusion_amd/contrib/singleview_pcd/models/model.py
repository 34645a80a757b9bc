"""singleview_pcd pose network, the paper's point-cloud baseline: RGB crop + masked point cloud -> per-point
(quaternion, translation, confidence) through a DenseFusion-style per-point MLP.

Restates examples/ycb_video/singleview_pcd/contrib/models/model.py:12-330 on torch.  The same crops, the same
ResNet18 + PSPNet features and the same 1000 sampled points as contrib/singleview_3d; ``PoseNetExtractor`` and three
4-layer heads replace voxelize -> 3-D CNN -> trilinear sampling.  Differences that are deliberate:
  * the per-object host loop of ``predict`` (:87-110) is one batched selection with a single host synchronisation
    (contrib/point_selection.py, shared with the 3-D model; NumPy RNG kept bit for bit);
  * inference on the GPU (``torch.no_grad()``, eval mode, fp32, no autocast) runs the hand-written path of
    models/pcdnet.py: ``feat3`` -- the pooled vector repeated over the points -- is never built, its share of the
    heads' first layer is a per-object bias.  ``pcd_kernels = False`` switches that path off; training and every
    other case run the stock-torch formulation below;
  * CAD models come from an injectable ``models`` provider (``get_pcd``), like the 3-D model.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from ....geometry.instance_crops import valid_points_median
from ....models import PSPNetExtractor, ResNet18, ResNet18Extractor
from ...point_selection import PointSelection
from ...singleview_3d.models.model import Model as _Model3D, PitchTableModels
from .pcdnet import HEADS, PcdNetKernels


class PoseNetExtractor(nn.Module):
    """model.py:299-330: per-point features [B, 1408, P] = feat1 (64 | 64) | feat2 (128 | 128) | pooled 1024."""

    def __init__(self):
        super().__init__()
        self.conv1_rgb = nn.Conv1d(32, 64, 1)
        self.conv1_pcd = nn.Conv1d(3, 64, 1)
        self.conv2_rgb = nn.Conv1d(64, 128, 1)
        self.conv2_pcd = nn.Conv1d(64, 128, 1)
        self.conv3 = nn.Conv1d(256, 512, 1)
        self.conv4 = nn.Conv1d(512, 1024, 1)

    def forward(self, h_rgb, pcd):
        n_point = h_rgb.shape[2]
        h_rgb = F.relu(self.conv1_rgb(h_rgb))
        h_pcd = F.relu(self.conv1_pcd(pcd))
        feat1 = torch.cat((h_rgb, h_pcd), dim=1)
        h_rgb = F.relu(self.conv2_rgb(h_rgb))
        h_pcd = F.relu(self.conv2_pcd(h_pcd))
        feat2 = torch.cat((h_rgb, h_pcd), dim=1)
        h = F.relu(self.conv3(feat2))
        h = F.relu(self.conv4(h))
        h = h.mean(dim=2, keepdim=True)  # average_pooling_1d over all points
        feat3 = h.expand(-1, -1, n_point)
        return torch.cat((feat1, feat2, feat3), dim=1)


class Model(PointSelection, nn.Module):

    _lambda_confidence = 0.015
    _n_point = 1000

    def __init__(self, *, n_fg_class, centerize_pcd=True, pretrained_resnet18=False, loss=None, models=None):
        super().__init__()
        self._n_fg_class = n_fg_class
        self._centerize_pcd = centerize_pcd
        if loss is None:
            loss = "add/add_s"
        if loss not in ("add", "add/add_s"):  # model.py:33-36
            raise ValueError(f"unknown loss {loss!r}: the point-cloud baseline has 'add' and 'add/add_s'")
        self._loss = loss
        self._models = models or PitchTableModels()
        # evaluate the last PSPNet level only where the network samples it
        self.sparse_pspnet_tail = True
        # inference: the point MLP and the heads on csrc/pcdnet.hip + the split-bf16 GEMM engine (models/pcdnet.py);
        # False = the stock-torch formulation
        self.pcd_kernels = True

        self.resnet_extractor = ResNet18Extractor() if pretrained_resnet18 else ResNet18()
        self.pspnet_extractor = PSPNetExtractor()
        self.posenet_extractor = PoseNetExtractor()
        for name, c_out in zip(HEADS, (4, 3, 1)):
            setattr(self, f"conv1_{name}", nn.Conv1d(1408, 640, 1))
            setattr(self, f"conv2_{name}", nn.Conv1d(640, 256, 1))
            setattr(self, f"conv3_{name}", nn.Conv1d(256, 128, 1))
            setattr(self, f"conv4_{name}", nn.Conv1d(128, n_fg_class * c_out, 1))

    def __getstate__(self):
        state = dict(self.__dict__)
        state.pop("_pcd_kernels_op", None)  # packs and workspaces: run-time state, rebuilt on demand
        return state

    xp = _Model3D.xp

    # ---- inference (model.py:69-155) ---------------------------------------------------------------
    def predict(self, *, class_id, rgb, pcd):
        dev = rgb.device
        pcd = pcd.float()
        pix = self._select_points(pcd)  # [B,P]; the one host synchronisation (raises for an example without a point)
        # model.py:101-102: the median of ALL valid points of the crop, not of the kept ones
        center = valid_points_median(pcd) if self._centerize_pcd else None
        return self._predict_device(torch.as_tensor(class_id, device=dev), rgb, pcd, pix, center)

    def _kernel_path(self, rgb):
        return (self.pcd_kernels and rgb.is_cuda and not self.training and not torch.is_grad_enabled()
                and not torch.is_autocast_enabled() and self.conv1_rot.weight.dtype == torch.float32)

    def _predict_device(self, class_id, rgb, pcd, pix, center):
        """Everything after point selection: pure device work, no host synchronisation."""
        B, P = pix.shape
        image = rgb.permute(0, 3, 1, 2)  # (uint8 or float: the extractor normalises the image as it arrives)
        if self._kernel_path(rgb):
            rows = self.pspnet_extractor.forward_sampled_rows(self.resnet_extractor(image), pix)  # [B*P, 32]
            if getattr(self, "_pcd_kernels_op", None) is None:
                self.__dict__["_pcd_kernels_op"] = PcdNetKernels(self)
            return self._pcd_kernels_op.pose(class_id, rows, pcd, pix, center)
        if self.sparse_pspnet_tail:
            values = self.pspnet_extractor.forward_sampled(self.resnet_extractor(image), pix)
        else:
            h_rgb = self.pspnet_extractor(self.resnet_extractor(image))
            values = torch.gather(h_rgb.reshape(B, h_rgb.shape[1], -1), 2, pix[:, None, :].expand(B, h_rgb.shape[1], -1))
        points = torch.gather(pcd.permute(0, 3, 1, 2).reshape(B, 3, -1), 2, pix[:, None, :].expand(B, 3, -1))
        return self._pose_from_features(class_id, values, points, center)

    def _pose_from_features(self, class_id, values, points, center):
        """values [B,32,P], points [B,3,P] camera frame, center [B,3] or None: the stock-torch formulation
        (model.py:115-155), differentiable."""
        B, _, P = points.shape
        if center is not None:
            points = points - center[:, :, None]
        h = self.posenet_extractor(values, points.to(values.dtype))
        outs = {}
        for name in HEADS:
            x = F.relu(getattr(self, f"conv1_{name}")(h))
            x = F.relu(getattr(self, f"conv2_{name}")(x))
            x = F.relu(getattr(self, f"conv3_{name}")(x))
            outs[name] = getattr(self, f"conv4_{name}")(x).float()
        cls_rot = outs["rot"].reshape(B, self._n_fg_class, 4, P)
        cls_trans = outs["trans"].reshape(B, self._n_fg_class, 3, P)
        cls_conf = torch.sigmoid(outs["conf"]).reshape(B, self._n_fg_class, P)
        if center is not None:
            points = points + center[:, :, None]  # (p - c) + c in fp32, as the reference: not always p
        cls_trans = points[:, None, :, :] + cls_trans

        fg_class_id = (class_id - 1).long()
        ar = torch.arange(B, device=points.device)
        rot = cls_rot[ar, fg_class_id]
        # F.normalize of chainer (l2_normalization.py): x / (|x| + eps), eps = 1e-5 -- not torch's x / max(|x|, eps)
        rot = (rot / (rot.norm(dim=1, keepdim=True) + 1e-5)).transpose(1, 2)  # B4P -> BP4
        trans = cls_trans[ar, fg_class_id].transpose(1, 2)  # B3P -> BP3
        conf = cls_conf[ar, fg_class_id]
        return rot, trans, conf

    # ---- training (model.py:157-295) ---------------------------------------------------------------
    def forward(self, *, class_id, rgb, pcd, quaternion_true, translation_true):
        quaternion_pred, translation_pred, confidence_pred = self.predict(class_id=class_id, rgb=rgb, pcd=pcd)
        return self.loss(class_id=class_id, quaternion_true=quaternion_true, translation_true=translation_true,
                         quaternion_pred=quaternion_pred, translation_pred=translation_pred,
                         confidence_pred=confidence_pred)

    # model.py:186-236 / :238-295 are the 3-D model's evaluate / loss (the same ADD / ADD-S of 500 CAD points, the same
    # confidence terms): one implementation
    evaluate = _Model3D.evaluate
    loss_prepare = _Model3D.loss_prepare
    loss_device = _Model3D.loss_device
    loss = _Model3D.loss
