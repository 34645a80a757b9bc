# flake8: noqa
# the CAD-model side of morefusion/datasets: models whose meshes are on disk (nothing is downloaded)
from .ycb_video import YCBVideoModels
from .models_adapter import MeshModels, as_models
from .rgbd_pose_estimation import RGBDPoseEstimationDatasetBase
from .augmentation import augment_rgbd
from .reindexed import RGBDPoseEstimationDatasetReIndexedBase, reindex
