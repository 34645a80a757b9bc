"""TEST HELPER: an independent NumPy restatement of the reference map server's insert and grid publication --
OctomapServer::insertScan (ros/src/morefusion_ros/src/OctomapServer.cpp:283-455) and ::publishGrids (:510-618) -- on
top of tests/occmap_ref.py's OcTree (a dict from octree key to float32 log-odds): Python sets of keys as the C++ keeps
them, one updateNode per key of each set, the grids voxel by voxel.  Written from the C++, not from the kernels;
morefusion_amd's csrc/occserver.hip is checked against this bit for bit.

Where the C++ is schedule-dependent under OpenMP or leans on third-party arithmetic, the rules of DESIGN.md "Map
server" apply and are restated here:
  * the first point of an instance only creates its cloud (:345-349): the point of the smallest pixel index is dropped;
  * centroid = float32(float64 sum / count); the sum runs in one fixed order over the stride-2 pixels q (row-major):
    partial[t] takes q = t, t + 1024, ... in ascending order, then partial[t] += partial[t + off] for off = 512 .. 1;
  * min / max over float32 values order -0 below +0;
  * T_map_to_sensor = [R^T | -R^T t] in float64, rounded to float32; both transforms are ((T0 x + T1 y) + T2 z) + T3
    in float32 (tests/occtrack_ref.transform);
  * an instance gets its centre from the first frame that leaves it a point, and is published only with a centre.
The background map is id 0 (the reference's -1), tracked ids are >= 1.
"""
import math

import numpy as np

import occmap_ref as R
import occtrack_ref as T

BACKGROUND_ID = 0
LANES = 1024
DIM = 32


def logodds(p):
    return np.float32(math.log(p / (1 - p)))


def _min_max(p):
    """Per-axis min / max of float32 rows with -0 < +0."""
    lo, hi = p.min(axis=0), p.max(axis=0)
    for a in range(3):
        zeros = p[p[:, a] == 0, a]
        if lo[a] == 0:
            lo[a] = np.float32(-0.0) if np.signbit(zeros).any() else np.float32(0.0)
        if hi[a] == 0:
            hi[a] = np.float32(0.0) if (~np.signbit(zeros)).any() else np.float32(-0.0)
    return lo, hi


def _centroid(q, p, n_q):
    """float32(float64 sum / count) of the rows p (float32) at the stride-2 ordinals q, in the fixed order above."""
    rounds = (n_q + LANES - 1) // LANES
    dense = np.zeros((rounds * LANES, 3), np.float64)
    dense[q] = p.astype(np.float64)
    dense = dense.reshape(rounds, LANES, 3)
    partial = np.zeros((LANES, 3), np.float64)
    for r in range(rounds):
        partial = partial + dense[r]
    off = LANES // 2
    while off:
        partial[:off] = partial[:off] + partial[off:2 * off]
        off //= 2
    return (partial[0] / np.float64(len(q))).astype(np.float32)


class OctomapServer:
    def __init__(self, resolution=0.01, hit=0.7, miss=0.4, prob_min=0.12, prob_max=0.97, ground_as_noentry=True,
                 free_as_noentry=True):
        self.resolution, self.prob_max = resolution, prob_max
        self.lo_hit, self.lo_miss, self.lo_min, self.lo_max = logodds(hit), logodds(miss), logodds(prob_min), logodds(prob_max)
        self.ground_as_noentry, self.free_as_noentry = ground_as_noentry, free_as_noentry
        self.octrees, self.class_ids, self.centers, self.bbx = {}, {}, {}, {}

    def _update_nodes(self, tree, codes, update):
        """updateNode(key, occupied) for every key of a set: l = clamp(float32(l + update)), a new node starts at 0
        (each key is its own node, so the order within the set plays no part)."""
        codes = sorted(codes)
        zero = np.float32(0)
        l = np.array([tree.values.get(c, zero) for c in codes], np.float32) + np.float32(update)
        assert l.dtype == np.float32
        l = np.where(l < self.lo_min, self.lo_min, np.where(l > self.lo_max, self.lo_max, l))
        tree.values.update(zip(codes, l))

    def insert_scan(self, pts_map, label, instance_id_to_class_id, pitch_of, origin):
        H, W = label.shape
        pts_map = np.asarray(pts_map, np.float32).reshape(H, W, 3)
        origin = np.asarray(origin, np.float32)
        occupied = {}
        for u in sorted(set(np.unique(label).tolist()) | {-1}):  # the background map always exists
            if u == -2:
                continue
            iid = BACKGROUND_ID if u == -1 else u
            if iid not in self.octrees:
                pitch = self.resolution if u == -1 else pitch_of(instance_id_to_class_id[u])
                self.octrees[iid] = R.OcTree(pitch)
                self.class_ids[iid] = 0 if u == -1 else instance_id_to_class_id[u]
            occupied[iid] = set()
        bg = self.octrees[BACKGROUND_ID]
        # the stride-2 pixels without NaN, in index order
        Ws = (W + 1) // 2
        jj, ii = np.mgrid[0:H:2, 0:W:2]
        jj, ii = jj.reshape(-1), ii.reshape(-1)
        q = np.arange(len(jj))
        ok = ~np.isnan(pts_map[jj, ii]).any(axis=1)
        q, p, l = q[ok], pts_map[jj[ok], ii[ok]], label[jj[ok], ii[ok]]
        assert (q == (jj[ok] // 2) * Ws + ii[ok] // 2).all()
        free_bg = set(np.unique(bg.compute_ray_keys(origin, p)).tolist())
        for u in np.unique(l):
            mine = l == u
            if u != -2:
                tree = self.octrees[BACKGROUND_ID if u == -1 else int(u)]
                k, valid = tree.keys(p[mine])
                occupied[BACKGROUND_ID if u == -1 else int(u)] |= set(R.pack(k[valid]).tolist())
            if u != -1:
                k, valid = bg.keys(p[mine])
                free_bg |= set(R.pack(k[valid]).tolist())
        self._update_nodes(bg, free_bg - occupied[BACKGROUND_ID], self.lo_miss)
        for iid in sorted(occupied):
            self._update_nodes(self.octrees[iid], occupied[iid], self.lo_hit)
        # instance_id_to_points: the first point creates the cloud, the others are appended
        for u in np.unique(l):
            if u == -2:
                continue
            iid = BACKGROUND_ID if u == -1 else int(u)
            sel = np.nonzero(l == u)[0][1:]
            if len(sel) == 0:
                continue
            lo, hi = _min_max(p[sel])
            if iid in self.bbx:
                lo, hi = np.minimum(self.bbx[iid][0], lo), np.maximum(self.bbx[iid][1], hi)
            self.bbx[iid] = (lo, hi)
            if iid not in self.centers:  # centers_.insert does not overwrite
                self.centers[iid] = _centroid(q[sel], p[sel], len(jj))

    def publish_grids(self, T_sensor_to_map):
        """-> (dict of the grids, dict of branch counts over all grids)."""
        T64 = np.asarray(T_sensor_to_map, np.float64)
        inv = np.eye(4)
        inv[:3, :3] = T64[:3, :3].T
        inv[:3, 3] = -T64[:3, :3].T @ T64[:3, 3]
        T32, inv32 = T64.astype(np.float32), inv.astype(np.float32)
        ids = [i for i in sorted(self.octrees) if i != BACKGROUND_ID and i in self.centers]
        tables = {i: T._Table(t) for i, t in self.octrees.items()}
        B = len(ids)
        out = dict(instance_ids=ids, class_ids=[self.class_ids[i] for i in ids], pitch=np.zeros(B, np.float32),
                   origin=np.zeros((B, 3), np.float64), grid_target=np.zeros((B, DIM, DIM, DIM), np.float32),
                   grid_noentry=np.zeros((B, DIM, DIM, DIM), np.float32))
        counts = dict(ground=0, free_background=0, other_at_clamp=0, own_occupied=0, overwritten=0)
        index = np.argwhere(np.ones((DIM, DIM, DIM), bool))  # i, j, k in C order
        for b, iid in enumerate(ids):
            p32 = np.float32(self.octrees[iid].resolution)
            center_sensor = T.transform(self.centers[iid][None], inv32)[0]
            origin = center_sensor.astype(np.float64) - (DIM / 2.0 - 0.5) * np.float64(p32)
            sensor = (origin + (p32 * index.astype(np.float32)).astype(np.float64)).astype(np.float32)
            world = T.transform(sensor, T32)
            target = np.zeros(len(index), np.float32)
            noentry = np.zeros(len(index), np.float32)
            written = np.zeros(len(index), np.int64)
            ground = (world[:, 2] < 0) if self.ground_as_noentry else np.zeros(len(index), bool)
            noentry[ground] = np.float32(self.prob_max)
            counts["ground"] += int(ground.sum())
            occ = self._occupancy(tables[iid], self.octrees[iid], world)
            own = ~ground & (occ > 0.5)  # an unknown cell is NaN here: never > 0.5
            target[own] = occ[own].astype(np.float32)
            counts["own_occupied"] += int(own.sum())
            rest = ~ground & ~own
            for other in sorted(self.octrees):
                if other == iid:
                    continue
                occ = self._occupancy(tables[other], self.octrees[other], world)
                with np.errstate(invalid="ignore"):
                    known = rest & ~np.isnan(occ)
                    free = known & (occ < 0.5) if (other == BACKGROUND_ID and self.free_as_noentry) else np.zeros(len(index), bool)
                    clamp = known & ~free & (occ >= self.prob_max)
                noentry[free] = (1 - occ[free]).astype(np.float32)
                noentry[clamp] = occ[clamp].astype(np.float32)
                counts["free_background"] += int(free.sum())
                counts["other_at_clamp"] += int(clamp.sum())
                counts["overwritten"] += int((written[free | clamp] > 0).sum())
                written[free | clamp] += 1
            out["pitch"][b], out["origin"][b] = p32, origin
            out["grid_target"][b] = target.reshape(DIM, DIM, DIM)
            out["grid_noentry"][b] = noentry.reshape(DIM, DIM, DIM)
        out["grid_nontarget_empty"] = out["grid_noentry"] != 0
        return out, counts

    @staticmethod
    def _occupancy(table, tree, pts):
        """node->getOccupancy() at the float32 points, NaN where search() returns NULL."""
        keys, ok = tree.keys(pts)
        l = table(keys)
        l[~ok] = np.nan
        out = np.full(len(l), np.nan)
        known = ~np.isnan(l)
        prob = {float(v): R.probability(v) for v in np.unique(l[known])}
        out[known] = [prob[float(v)] for v in l[known]]
        return out


def known_cells(mapping, iid):
    """{key code: float32 log-odds} of the product's dense box."""
    lo, lg = mapping.dense_logodds(iid)
    known = ~np.isnan(lg)
    return dict(zip(R.pack(np.argwhere(known) + lo).tolist(), lg[known].tolist()))


def maps_equal(server, ref):
    """Every tree's known keys and log-odds bitwise equal to the mirror's (a map the mirror lacks must be empty)."""
    assert set(ref.octrees) <= set(server.mapping.instance_ids)
    for iid in server.mapping.instance_ids:
        got = known_cells(server.mapping, iid)
        exp = ref.octrees[iid].values if iid in ref.octrees else {}
        assert set(got) == set(exp), (iid, len(set(got) ^ set(exp)))
        assert all(np.float32(got[k]).tobytes() == np.float32(exp[k]).tobytes() for k in exp), iid


def stats_equal(server, ref):
    assert set(server.centers) == set(ref.centers) and set(server.bbx) == set(ref.bbx)
    for i in ref.centers:
        assert server.centers[i].dtype == np.float32 and server.centers[i].tobytes() == ref.centers[i].tobytes(), i
    for i in ref.bbx:
        for g, e in zip(server.bbx[i], ref.bbx[i]):
            assert g.dtype == np.float32 and g.tobytes() == e.tobytes(), i
