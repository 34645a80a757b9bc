"""contrib.ObjectMapping (host side): the pose voter of the reference's object_mapping node -- three agreeing poses
spawn an object, two do not; a symmetric class votes with ADD-S; a spawned pose is frozen; remove forgets."""
import numpy as np

from morefusion_amd.contrib import ObjectMapping

RS = np.random.RandomState(0)
# a solid of revolution about z (symmetric under a half turn about z) and the same with a bump (not symmetric)
ANGLES = np.linspace(0, 2 * np.pi, 40, endpoint=False)
RING = np.concatenate([np.stack([r * np.cos(ANGLES), r * np.sin(ANGLES), np.full(40, z)], 1)
                       for r, z in ((0.03, -0.02), (0.04, 0.0), (0.03, 0.02))])
BUMPY = np.concatenate([RING, [[0.08, 0.0, 0.0], [0.09, 0.01, 0.0]]])
POINTS = {1: BUMPY, 13: RING}


def pose(shift=(0, 0, 0), yaw=0.0):
    T = np.eye(4)
    T[:2, :2] = [[np.cos(yaw), -np.sin(yaw)], [np.sin(yaw), np.cos(yaw)]]
    T[:3, 3] = np.asarray(shift) + [0.1, 0.2, 0.9]
    return T


def voter():
    return ObjectMapping(POINTS, {1: False, 13: True})


def test_spawns_after_three_agreeing_poses_not_after_two():
    v = voter()
    v.append_pose(5, 1, pose())
    v.append_pose(5, 1, pose((0.001, 0, 0)))
    assert not v.validate(5) and v.spawned_ids() == []
    v.append_pose(5, 1, pose((0, 0.002, 0)))
    assert v.validate(5) and v.validate() == [5] and v.class_id(5) == 1
    far = voter()
    for s in ((0, 0, 0), (0.05, 0, 0), (0, 0.05, 0), (0, 0, 0.05)):  # ADD 0.05 >= 0.02: never two votes
        far.append_pose(5, 1, pose(s))
    assert not far.validate(5)
    assert not far.validate(6)  # unknown instance


def test_symmetric_class_votes_with_add_s():
    flips = [pose(yaw=0.0), pose(yaw=np.pi), pose((0.001, 0, 0), yaw=np.pi)]
    sym, plain = voter(), voter()
    for T in flips:
        sym.append_pose(2, 13, T)
        plain.append_pose(2, 1, T)
    assert sym.validate(2)        # a half turn about the symmetry axis: ADD-S ~ 0
    assert not plain.validate(2)  # the same poses of a class that is not symmetric: ADD is centimetres
    tight = voter()
    for s in ((0, 0, 0), (0.015, 0, 0), (0, 0.015, 0)):  # within ADD 0.02 but not within ADD-S 0.01
        tight.append_pose(3, 13, pose(s))
    assert not tight.validate(3)


def test_pose_is_frozen_once_spawned_and_remove_forgets():
    v = voter()
    for s in ((0, 0, 0), (0.001, 0, 0), (0, 0.001, 0)):
        v.append_pose(7, 1, pose(s))
    assert v.pose(7) is None
    assert v.validate(7)
    frozen = v.pose(7)
    assert np.array_equal(frozen, pose((0, 0.001, 0)))
    v.append_pose(7, 1, pose((0.5, 0.5, 0.5)))
    assert v.validate(7) and np.array_equal(v.pose(7), frozen)
    assert v.remove(7) and not v.remove(7)
    assert v.spawned_ids() == [] and not v.validate(7)
    v.append_pose(7, 1, pose((0.5, 0.5, 0.5)))
    assert not v.validate(7)  # starts over


def test_history_holds_six_poses():
    v = voter()
    for k in range(8):
        v.append_pose(1, 1, pose((0.1 * k, 0, 0)))
    assert len(v._objects[1].poses) == 6
    assert not v.validate(1)
