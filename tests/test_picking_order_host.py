"""contrib.get_picking_order, quaternion_from_two_vectors and SelectPickingOrder end to end (the kernels through the
host emulator), on the CPU."""
import numpy as np
import pytest

import meshsdf_ref as R
import picking_cases as PC
import picking_ref as PR
import render_cases as C
import morefusion_amd as mf
from host_emul import emul
from morefusion_amd.contrib import get_picking_order, quaternion_from_two_vectors
from morefusion_amd.synthetic import _euler_pose

# edges i -> j: "i is occluded by j", with the hidden pixels
CHAIN = {(1, 2): 50, (2, 3): 40}
DIAMOND = {(1, 2): 10, (1, 3): 20, (2, 4): 30, (3, 4): 5}
GRAPHS = [  # (edges, target, further nodes, expected order)
    (CHAIN, 1, (), [3, 2, 1]),
    (CHAIN, 2, (), [3, 2]),
    (DIAMOND, 1, (), [4, 2, 3, 1]),
    ({(1, 2): 10, (5, 6): 10}, 1, (9,), [2, 1]),       # a disconnected edge and a node without edges stay out
    ({(5, 6): 10}, 1, (1,), [1]),                      # an isolated target
    ({}, 4, (), [4]),
    ({(1, 5): 3, (1, 2): 3, (2, 5): 3, (1, 9): 1, (9, 7): 2}, 1, (), [5, 7, 2, 9, 1]),  # leaves in ascending id
]


@pytest.mark.parametrize("edges,target,nodes,expect", GRAPHS)
def test_get_picking_order(edges, target, nodes, expect):
    assert get_picking_order(edges, target, nodes) == expect
    assert get_picking_order(list(edges), target, nodes) == expect  # plain pairs
    order, rounds = PR.get_picking_order(edges, target, nodes)
    assert order == expect and sum(len(r) for r in rounds) == len(expect)


def _reference_rounds(edges, target, nodes):
    """The reference's procedure (get_leaves / get_picking_order of its select_picking_order node) restated with
    networkx.DiGraph: the set of leaves removed in each round."""
    networkx = pytest.importorskip("networkx")
    graph = networkx.DiGraph()
    graph.add_nodes_from(list(nodes) + [target])
    graph.add_edges_from(edges)

    def leaves(node):
        out = list(graph.edges(node))
        if not out:
            yield node
        for _, v in out:
            yield from leaves(v)
    rounds = []
    while True:
        found = set(leaves(target))
        if target in found:
            return rounds + [{target}]
        rounds.append(found)
        graph.remove_nodes_from(found)


@pytest.mark.parametrize("edges,target,nodes,expect", GRAPHS)
def test_rounds_against_networkx(edges, target, nodes, expect):
    rounds = _reference_rounds(edges, target, nodes)
    assert PR.get_picking_order(edges, target, nodes)[1] == rounds
    order, k = get_picking_order(edges, target, nodes), 0
    for r in rounds:  # the product's order, cut into the reference's rounds: the same sets, ascending inside
        assert set(order[k:k + len(r)]) == r and order[k:k + len(r)] == sorted(r)
        k += len(r)
    assert k == len(order)


def test_cycles_terminate_with_the_documented_tie_break():
    # 2-cycle: the target 1 and 2 occlude each other; 2 is the only other node: it goes first
    assert get_picking_order({(1, 2): 30, (2, 1): 80}, 1) == [2, 1]
    # 3-cycle 1 -> 2 -> 3 -> 1: 3 has the smallest hidden pixel count of the nodes other than the target
    assert get_picking_order({(1, 2): 30, (2, 3): 20, (3, 1): 10}, 1) == [3, 2, 1]
    assert get_picking_order({(1, 2): 30, (2, 3): 5, (3, 1): 10}, 1) == [2, 1]  # 2 leaves: 3 is no longer reachable
    # a tie: the lowest id
    assert get_picking_order({(1, 2): 30, (2, 3): 10, (3, 1): 10}, 1) == [2, 1]
    assert get_picking_order({(1, 3): 30, (3, 2): 10, (2, 1): 10}, 1) == [2, 3, 1]
    # a cycle behind a leaf: the leaf first, then the cycle is broken
    assert get_picking_order({(1, 2): 9, (2, 3): 9, (3, 2): 4, (1, 4): 9}, 1) == [4, 3, 2, 1]
    for edges in ({(1, 2): 30, (2, 1): 80}, {(1, 2): 30, (2, 3): 20, (3, 1): 10}, {(1, 2): 9, (2, 3): 9, (3, 2): 4, (1, 4): 9}):
        assert PR.get_picking_order(edges, 1)[0] == get_picking_order(edges, 1)
    assert get_picking_order({(1, 1): 5}, 1) == [1]  # a self-edge is no edge


def test_quaternion_from_two_vectors_rotates_z_onto_a_unit_normal():
    rs = np.random.RandomState(2)
    normals = rs.normal(size=(50, 3))
    normals /= np.linalg.norm(normals, axis=1, keepdims=True)
    for n in list(normals) + [np.array(v) for v in ((0.0, 0.0, 1.0), (1.0, 0.0, 0.0), (0.0, 0.0, -1.0))]:
        q = quaternion_from_two_vectors([0, 0, 1], n)
        assert q.shape == (4,) and q.dtype == np.float64 and abs(np.linalg.norm(q) - 1.0) <= 1e-15
        assert np.abs(PC.rotate(q, (0, 0, 1)) - n).max() <= 1e-14
    # un-normalised vectors: the same rotation; other pairs than z; a NaN normal
    q = quaternion_from_two_vectors([0, 0, 2.0], 0.3 * normals[0])
    assert np.abs(q - quaternion_from_two_vectors([0, 0, 1], normals[0])).max() <= 1e-15
    assert np.abs(PC.rotate(quaternion_from_two_vectors(normals[1], normals[2]), normals[1]) - normals[2]).max() <= 1e-14
    assert np.isnan(quaternion_from_two_vectors([0, 0, 1], [np.nan] * 3)).all()


@pytest.mark.skipif(not emul.available(), reason="g++ not available")
def test_select_picking_order_end_to_end(monkeypatch):
    emul.patch_lib(emul.build(["render.hip", "meshsdf.hip", "pickorder.hip"]), monkeypatch)
    H, W = 96, 128
    K = C.intrinsics(H, W)
    models = {2: C.ycb(2), 3: C.ycb(3), 7: R.box_mesh((-0.04, -0.04, -0.04), (0.04, 0.04, 0.04))}
    # the sugar box (class 3) stands behind the cracker box (class 2); the cube (class 7) stands apart
    class_ids, ids = [3, 2, 7], [21, 20, 22]
    Ts = np.stack([_euler_pose(np.array(a), np.array(t)) for a, t in (
        ((0.2, 1.1, 0.7), (0.0, 0.0, 0.8)), ((1.0, 0.4, 2.0), (0.09, 0.0, 0.5)), ((0.1, 0.2, 0.3), (-0.2, -0.12, 0.6)))])
    res = mf.contrib.SelectPickingOrder(models, target_class_id=3, device="cpu")(class_ids, ids, Ts, K, H, W)
    an = res["analysis"]
    assert an["ratio"][0, 1] >= 0.1 and an["ratio"][1, 0] == 0.0 and (an["ratio"][2] == 0).all()
    assert res["order"] == [20, 21] and set(res["edges"]) == {(21, 20)}
    assert res["edges"][(21, 20)] == an["occluded_by"][0, 1] > 0
    assert set(res["quaternion"]) == set(res["translation"]) == {20, 21, 22}
    for k, i in enumerate(ids):
        assert np.array_equal(res["translation"][i], an["translation"][k])
        assert abs(np.linalg.norm(res["quaternion"][i]) - 1.0) <= 1e-12
        # the grasp point lies on the object: inside its box in the image, at about its depth
        r, c = K[1, 1] * an["translation"][k][1] / an["translation"][k][2] + K[1, 2], \
            K[0, 0] * an["translation"][k][0] / an["translation"][k][2] + K[0, 2]
        y1, x1, y2, x2 = an["bbox"][k]
        assert y1 <= r <= y2 and x1 <= c <= x2 and abs(an["translation"][k][2] - Ts[k][2, 3]) < 0.15
    # a target class that is absent; a stricter threshold removes the edge
    assert mf.contrib.SelectPickingOrder(models, target_class_id=9, device="cpu")(class_ids, ids, Ts, K, H, W)["order"] == []
    strict = mf.contrib.SelectPickingOrder(models, 3, min_ratio=1.01, device="cpu")(class_ids, ids, Ts, K, H, W)
    assert strict["order"] == [21] and strict["edges"] == {}
