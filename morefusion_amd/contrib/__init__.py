# flake8: noqa
# the hot-path subset of morefusion/contrib/__init__.py:3-11
from .icc_batch import IccScenes
from .iterative_closest_point_link import IterativeClosestPointLink, icp_refine
from .iterative_collision_check_link import IterativeCollisionCheckLink
from .loss_observer import LossObserver
from .occupancy_registration import OccupancyRegistration, OccupancyRegistrationLink, occupancy_registration_batch
from . import singleview_3d
from . import singleview_pcd
from .multi_instance_octree_mapping import MultiInstanceOctreeMapping
from .icp_registration import ICPRegistration, icp_registration_batch
from .instance_tracking import InstanceTracker, render_instance_maps, render_voxel_grids, track_instance_ids
from .object_mapping import ObjectMapping
from .picking_order import SelectPickingOrder, get_picking_order, occlusion_analysis, quaternion_from_two_vectors
from .octomap_server import OctomapServer
from .camera_tracking import CameraTracker, align_depth
from .tsdf_volume import ModelTracker, TsdfVolume
from .instance_tsdf_volume import InstanceTsdfVolume
