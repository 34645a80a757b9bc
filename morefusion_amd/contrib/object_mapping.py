"""ObjectMapping -- promote a tracked instance to a known object once its poses agree (host side).

The voting of ros/src/morefusion_ros/nodes/object_mapping.py:23-84 without ROS: every instance keeps its last six
poses; once it has ``n_votes`` of them and at least ``n_votes - 1`` of the earlier ones lie within ADD < 0.02 m
(ADD-S < 0.01 m for a symmetric class) of the latest, the object is spawned and its pose is frozen.
"""
import collections

import numpy as np

from ..metrics import average_distance


class _Object:
    def __init__(self, class_id, pcd, is_symmetric, n_votes):
        self.class_id = class_id
        self.pcd = np.asarray(pcd, np.float64)
        self.is_symmetric = bool(is_symmetric)
        self.n_votes = n_votes
        self.poses = collections.deque([], 6)
        self.is_spawned = False

    def validate(self, add_threshold, adds_threshold):
        if self.is_spawned:
            return True
        if len(self.poses) < self.n_votes:
            return False  # too early to decide
        poses = list(self.poses)
        latest, earlier = poses[-1], poses[:-1]
        add, add_s = average_distance([self.pcd] * len(earlier), [latest] * len(earlier), earlier)
        dist, threshold = (add_s, adds_threshold) if self.is_symmetric else (add, add_threshold)
        if (np.asarray(dist) < threshold).sum() >= self.n_votes - 1:
            self.is_spawned = True
            self.poses = tuple(poses)  # frozen
        return self.is_spawned


class ObjectMapping:
    """``points_of(class_id)`` -> [n,3] model points, ``is_symmetric(class_id)`` -> bool (callables or dicts)."""

    add_threshold = 0.02
    adds_threshold = 0.01

    def __init__(self, points_of, is_symmetric=None, n_votes=3):
        self._points_of = points_of.__getitem__ if isinstance(points_of, dict) else points_of
        sym = is_symmetric if is_symmetric is not None else (lambda class_id: False)
        self._is_symmetric = sym.__getitem__ if isinstance(sym, dict) else sym
        if n_votes < 2:
            raise ValueError("n_votes must be at least 2")
        self.n_votes = int(n_votes)
        self._objects = {}

    def append_pose(self, instance_id, class_id, T_cad2base):
        """One more pose estimate of an instance (ignored once it is spawned: its pose is frozen)."""
        T = np.asarray(T_cad2base, np.float64)
        if T.shape != (4, 4):
            raise ValueError("T_cad2base must be 4x4")
        obj = self._objects.get(instance_id)
        if obj is None:
            obj = self._objects[instance_id] = _Object(class_id, self._points_of(class_id), self._is_symmetric(class_id),
                                                       self.n_votes)
        if not obj.is_spawned:
            obj.poses.append(T.copy())

    def validate(self, instance_id=None):
        """Vote on one instance (-> bool) or on all of them (-> the spawned ids)."""
        if instance_id is not None:
            obj = self._objects.get(instance_id)
            return obj is not None and obj.validate(self.add_threshold, self.adds_threshold)
        for obj in self._objects.values():
            obj.validate(self.add_threshold, self.adds_threshold)
        return self.spawned_ids()

    def spawned_ids(self):
        return [i for i, o in self._objects.items() if o.is_spawned]

    def pose(self, instance_id):
        """The frozen pose of a spawned object, else None."""
        obj = self._objects.get(instance_id)
        return obj.poses[-1].copy() if obj is not None and obj.is_spawned else None

    def class_id(self, instance_id):
        return self._objects[instance_id].class_id

    def remove(self, instance_id):
        """Forget an instance (poses, spawned state); False if it is not known."""
        return self._objects.pop(instance_id, None) is not None
