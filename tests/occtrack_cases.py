"""TEST HELPER: the two-frame tracking scenario of tests/test_emul_occtrack.py and tests/test_gpu_occtrack.py, and the
two drivers that run it -- the product (contrib.InstanceTracker over csrc/occtrack.hip) and the NumPy mirror
(tests/occtrack_ref.py over tests/occmap_ref.py).

Frame 0 of ``synthetic.make_tracking_sequence`` goes through the tracker into an empty mapping (every detection is
new).  Three maps are then made by hand: EDGE (a scan of a wall patch at the left image border: it renders in the
edge band, a suspicious reference id), FRONT and TWIN (``update`` with the same points at the same pitch: a slab in
front of the largest object as frame 1 sees it, so FRONT and TWIN tie exactly and the earlier slot wins, and both
are nearer than the object behind them).  Frame 1, from another sensor pose and with permuted detection ids, gets
two depth holes over the largest object (NaN pixels whose rays hit FRONT, TWIN and the object) and four hand-made
detections: one on the empty wall (a new id), one in the right edge band (edge rule), a 2 x 2 blob (size rule) and a
detached 2 x 2 blob of the largest object's detection id (a component below min_area)."""
import numpy as np

import occmap_ref as R
import occtrack_ref as T

EDGE, FRONT, TWIN = 50, 60, 61
SLAB_PITCH = 0.02


def make_pitch_of(width):
    """The class pitches are set for 640 columns (pixels 1.5 mm apart at 0.9 m); a coarser image needs coarser cells, or
    a map made of one frame is a cloud of separate cells that the next frame's rays pass through."""
    from morefusion_amd import synthetic
    scale = max(1.0, 384.0 / width)
    return lambda c: synthetic.CLASS_PITCH[int(c)] * scale


def scaled_thresholds(height):
    """The reference's thresholds (set for 480 rows) scaled to the image: lengths by s = height / 480, the area by s^2."""
    s = height / 480.0
    return dict(min_mask=max(int(40 * s), 1), min_bbox=max(int(80 * s), 1), min_side=max(int(60 * s), 1),
                min_area=max(int(400 * s * s), 1), band=max(int(round(5 * s)), 1), iou=0.4, coverage=0.9)


def make_scenario(seed, height, width, n_objects, thresholds=None):
    from morefusion_amd import geometry, synthetic
    H, W = height, width
    frames = synthetic.make_tracking_sequence(seed, 2, H, W, n_objects=n_objects)
    K = frames[0]["K"]
    for f in frames:
        f["label_detected"] = f["label_detected"].copy()
        f["class_ids_by_detection"] = dict(f["class_ids_by_detection"])
    f0, f1 = frames
    # frame 1: the largest object, two depth holes at stride-2 pixels well inside it
    label = f1["label_detected"]
    ids, counts = np.unique(label[label >= 0], return_counts=True)
    big = int(ids[np.argmax(counts)])
    m = label == big
    inner = m.copy()
    for dj in (-1, 0, 1):
        for di in (-1, 0, 1):
            inner &= np.roll(np.roll(m, dj, 0), di, 1)
    jj, ii = np.nonzero(inner[::2, ::2])
    assert len(jj) >= 2, "the largest object has no interior at stride 2"
    holes = [(2 * int(jj[k]), 2 * int(ii[k])) for k in (len(jj) // 2 - 1, len(jj) // 2)]
    pcd1_full = geometry.pointcloud_from_depth(f1["depth"], K[0, 0], K[1, 1], K[0, 2], K[1, 2])
    front = pcd1_full[m]
    front = front[~np.isnan(front).any(axis=1)] * np.float32(0.85)  # in frame 1's sensor frame, towards the sensor
    f1["depth"] = f1["depth"].copy()
    for j, i in holes:
        f1["depth"][j, i] = np.nan
    # frame 1: the hand-made detections
    nxt = int(label.max()) + 1
    r = lambda a, b: slice(int(round(a * H)), int(round(b * H)))  # noqa: E731
    c = lambda a, b: slice(int(round(a * W)), int(round(b * W)))  # noqa: E731
    bg = label == -1
    wall = np.zeros_like(bg)
    wall[r(0.125, 0.34), c(0.40, 0.60)] = True
    edge = np.zeros_like(bg)
    edge[r(0.42, 0.64), c(0.91, 1.0)] = True
    assert bg[wall].all() and bg[edge].all(), "a hand-made detection overlaps an object"
    label[wall], label[edge] = nxt, nxt + 1
    j0, i0 = int(round(0.17 * H)), int(round(0.69 * W))
    assert bg[j0:j0 + 2, i0:i0 + 2].all() and bg[j0:j0 + 2, i0 + 6:i0 + 8].all()
    label[j0:j0 + 2, i0:i0 + 2] = nxt + 2
    label[j0:j0 + 2, i0 + 6:i0 + 8] = big
    cls = sorted(synthetic.CLASS_PITCH)
    f1["class_ids_by_detection"].update({nxt: cls[0], nxt + 1: cls[1], nxt + 2: cls[2]})
    # frame 0: the wall patch at the left border that becomes the EDGE map
    edge_mask = np.zeros((H, W), bool)
    edge_mask[r(0.2, 0.7), :max(int(0.06 * W), 2)] = True
    assert (f0["label_detected"][edge_mask] == -1).all()
    for f in frames:
        f["pcd"] = geometry.pointcloud_from_depth(f["depth"], K[0, 0], K[1, 1], K[0, 2], K[1, 2])
    return dict(H=H, W=W, K=K, frames=frames, thresholds=dict(thresholds or scaled_thresholds(H)), big=big, holes=holes, front=front,
                edge_mask=edge_mask, pitch_of=make_pitch_of(W), det_new=nxt, det_edge=nxt + 1, det_small=nxt + 2)


def run_product(sc, device):
    """-> dict of NumPy results of the product's pipeline (and the mapping, the tracker)."""
    from morefusion_amd.contrib import InstanceTracker, MultiInstanceOctreeMapping
    from morefusion_amd.contrib.instance_tracking import render_instance_maps, transform_points
    H, W, K = sc["H"], sc["W"], sc["K"]
    f0, f1 = sc["frames"]
    pitch_of = sc["pitch_of"]
    m = MultiInstanceOctreeMapping(device=device)
    trk = InstanceTracker(m, thresholds=sc["thresholds"])
    out = {}
    tracked0, merged0, classes0, rendered0 = trk.track(f0["pcd"], f0["label_detected"], f0["class_ids_by_detection"], K,
                                                       f0["T_sensor_to_map"])
    out["frame0"] = dict(label_tracked=tracked0, label_merged=merged0, classes=classes0, label_rendered=rendered0,
                         remap=trk.last["remap_host"].copy(), pts_map=trk.pts_map.cpu().numpy())
    m.integrate_tracked_frame(trk.pts_map, tracked0, classes0, pitch_of, origin=f0["T_sensor_to_map"][:3, 3])
    m.initialize(EDGE, pitch=0.01)
    m.integrate(EDGE, sc["edge_mask"], trk.pts_map.reshape(H, W, 3), origin=f0["T_sensor_to_map"][:3, 3])
    slab = transform_points(sc["front"], f1["T_sensor_to_map"], device)
    for iid in (FRONT, TWIN):
        m.initialize(iid, pitch=SLAB_PITCH)
        m.update(iid, slab)
    out["slab"] = slab.cpu().numpy()
    out["boxes"] = {i: (m.dense_logodds(i)[0], m.dense_logodds(i)[1].shape) for i in m.instance_ids}
    tracked1, merged1, classes1, rendered1 = trk.track(f1["pcd"], f1["label_detected"], f1["class_ids_by_detection"], K,
                                                       f1["T_sensor_to_map"])
    ref_ids = sorted(i for i in m.instance_ids if i != 0)
    _, depth1 = render_instance_maps(m, trk.pts_map, K, f1["T_sensor_to_map"], H, W, ref_ids)
    last = trk.last
    out["frame1"] = dict(label_tracked=tracked1, label_merged=merged1, classes=classes1, label_rendered=rendered1,
                         depth_rendered=depth1.cpu().numpy(), remap=last["remap_host"].copy(),
                         det_ids=last["det_ids"], ref_ids=last["ref_ids"],
                         suspicious_ref=last["suspicious_ref"].cpu().numpy(),
                         suspicious_det=last["suspicious_det"].cpu().numpy(),
                         label_reference=last["label_reference"].cpu().numpy(), pts_map=trk.pts_map.cpu().numpy(),
                         counter=int(trk.counter.cpu()[0]))
    m.integrate_tracked_frame(trk.pts_map, tracked1, classes1, pitch_of, origin=f1["T_sensor_to_map"][:3, 3])
    return out, m, trk


def run_mirror(sc, boxes):
    """The same steps through the mirror; ``boxes`` {instance id: (lo, dim)}: the product's boxes before frame 1."""
    H, W, K = sc["H"], sc["W"], sc["K"]
    f0, f1 = sc["frames"]
    th, pitch_of = sc["thresholds"], sc["pitch_of"]
    m = R.MultiInstanceOctreeMapping()
    out = {}
    pts0 = T.transform(f0["pcd"], f0["T_sensor_to_map"])
    rendered0 = np.full((H, W), -2, np.int32)
    t0 = T.track(rendered0, f0["label_detected"], 1, th)
    classes = {t0["remap"][d]: c for d, c in f0["class_ids_by_detection"].items() if t0["remap"][d] != -2}
    out["frame0"] = dict(t0, classes=dict(classes), pts_map=pts0, label_rendered=rendered0)
    o0 = np.asarray(f0["T_sensor_to_map"][:3, 3], np.float32)
    T.integrate_tracked_frame(m, pts0, t0["label_tracked"], classes, pitch_of, o0)
    m.initialize(EDGE, pitch=0.01)
    m.integrate(EDGE, sc["edge_mask"], pts0.reshape(H, W, 3), origin=o0)
    slab = T.transform(sc["front"], f1["T_sensor_to_map"])
    for iid in (FRONT, TWIN):
        m.initialize(iid, pitch=SLAB_PITCH)
        m.update(iid, slab)
    out["slab"] = slab
    pts1 = T.transform(f1["pcd"], f1["T_sensor_to_map"])
    ref_ids = sorted(i for i in m.octrees if i != 0)
    maps = [(i, m.octrees[i], boxes[i]) for i in ref_ids]
    rendered1, depth1, winner, hits, dists = T.render(maps, pts1, K, f1["T_sensor_to_map"], H, W)
    t1 = T.track(rendered1, f1["label_detected"], t0["counter"], th)
    for d, c in f1["class_ids_by_detection"].items():
        if t1["remap"][d] != -2:
            classes[t1["remap"][d]] = c
    out["frame1"] = dict(t1, classes=dict(classes), pts_map=pts1, label_rendered=rendered1, depth_rendered=depth1,
                         winner=winner, hits=hits, dists=dists, ref_ids=ref_ids)
    T.integrate_tracked_frame(m, pts1, t1["label_tracked"], classes, pitch_of,
                              np.asarray(f1["T_sensor_to_map"][:3, 3], np.float32))
    return out, m


def logodds_equal(m, ref):
    assert m.instance_ids == list(ref.octrees)
    for iid in m.instance_ids:
        lo, lg = m.dense_logodds(iid)
        known = ~np.isnan(lg)
        got = dict(zip(R.pack(np.argwhere(known) + lo).tolist(), lg[known].tolist()))
        exp = ref.octrees[iid].values
        assert set(got) == set(exp), (iid, len(set(got) ^ set(exp)))
        assert all(np.float32(got[k]) == exp[k] for k in exp), iid


def check_frame1(got, exp):
    """Every output of frame 1 bitwise against the mirror."""
    g, e = got["frame1"], exp["frame1"]
    assert np.array_equal(g["pts_map"], e["pts_map"], equal_nan=True)
    assert np.array_equal(g["label_rendered"], e["label_rendered"])
    assert g["depth_rendered"].dtype == np.float32
    assert np.array_equal(g["depth_rendered"].view(np.uint32)[~np.isnan(e["depth_rendered"])],
                          e["depth_rendered"].view(np.uint32)[~np.isnan(e["depth_rendered"])])
    assert np.array_equal(np.isnan(g["depth_rendered"]), np.isnan(e["depth_rendered"]))
    assert dict(zip(g["det_ids"], g["remap"][:-1].tolist())) == e["remap"]
    assert int(g["remap"][-1]) == e["counter"] == g["counter"]
    assert {i for i, s in zip(g["ref_ids"], g["suspicious_ref"]) if s} == e["suspicious_ref"]
    assert {i: int(s) for i, s in zip(g["det_ids"], g["suspicious_det"]) if s} == e["suspicious_det"]
    for k in ("label_tracked", "label_reference", "label_merged"):
        assert g[k].dtype == np.int32 and np.array_equal(g[k], e[k]), k
    assert g["classes"] == e["classes"]


def check_cases(sc, exp):
    """The scenario holds every case the kernels branch on (asserted on the mirror alone)."""
    e = exp["frame1"]
    remap, best = e["remap"], e["best"]
    matched = [d for d, t in remap.items() if t >= 0 and t == best[d][0]]
    assert sc["big"] in matched and len(matched) >= 2                       # matched detections
    assert remap[sc["det_new"]] in e["new_ids"]                              # a detection that spawns a new id
    assert e["suspicious_det"].get(sc["det_edge"]) == 1                      # the edge rule alone
    assert e["suspicious_det"].get(sc["det_small"], 0) & 2                   # the size rule
    assert EDGE in e["suspicious_ref"]                                       # a suspicious reference id
    assert (e["tracked_small_removed"] != e["tracked_relabelled"]).any()     # a component below min_area
    j0, i0 = int(round(0.17 * sc["H"])), int(round(0.69 * sc["W"]))
    assert (e["tracked_small_removed"][j0:j0 + 2, i0 + 6:i0 + 8] == -2).all()
    assert (e["tracked_relabelled"][j0:j0 + 2, i0 + 6:i0 + 8] == remap[sc["big"]]).all()
    ids = e["ref_ids"]
    s_front, s_twin, s_big = ids.index(FRONT), ids.index(TWIN), ids.index(remap[sc["big"]])
    hits, dists, winner = e["hits"], e["dists"], e["winner"]
    assert s_front < s_twin
    seen_nearer = seen_tie = False
    for j, i in sc["holes"]:                                                 # NaN pixels that hit maps
        q = (j // 2, i // 2)
        assert np.isnan(sc["frames"][1]["pcd"][j, i]).all()
        assert hits[s_front][q] and hits[s_twin][q]
        assert dists[s_front][q] == dists[s_twin][q] and winner[q] == s_front  # an exact tie: the earlier slot
        seen_tie = True
        if hits[s_big][q]:
            assert dists[s_big][q] > dists[s_front][q]                       # two trees hit, the nearer one wins
            seen_nearer = True
    assert seen_tie and seen_nearer
    assert (e["label_rendered"] == FRONT).any() and not (e["label_rendered"] == TWIN).any()


def run_sequence_product(frames, thresholds, pitch_of, device, as_tensor=False):
    """Every frame through track -> integrate_tracked_frame.  -> (per frame dict(remap {detection id: tracked id},
    counter_before, counter, label_tracked, label_merged, label_rendered, boxes), the mapping)."""
    import torch
    from morefusion_amd.contrib import InstanceTracker, MultiInstanceOctreeMapping
    m = MultiInstanceOctreeMapping(device=device)
    trk = InstanceTracker(m, thresholds=thresholds)
    records = []
    for f in frames:
        boxes = {i: (m.dense_logodds(i)[0], m.dense_logodds(i)[1].shape) for i in m.instance_ids}
        before = int(trk.counter.cpu()[0])
        pcd, label = f["pcd"], f["label_detected"]
        if as_tensor:
            pcd, label = torch.as_tensor(pcd).to(device), torch.as_tensor(label).to(device)
        tracked, merged, classes, rendered = trk.track(pcd, label, f["class_ids_by_detection"], f["K"], f["T_sensor_to_map"])
        m.integrate_tracked_frame(trk.pts_map, tracked, classes, pitch_of, origin=f["T_sensor_to_map"][:3, 3])
        records.append(dict(remap=dict(zip(trk.last["det_ids"], trk.last["remap_host"][:-1].tolist())),
                            counter_before=before, counter=int(trk.last["remap_host"][-1]), label_tracked=tracked,
                            label_merged=merged, label_rendered=rendered, classes=classes, boxes=boxes))
    return records, m


def run_sequence_mirror(frames, thresholds, pitch_of, boxes_per_frame):
    m = R.MultiInstanceOctreeMapping()
    counter, classes, records = 1, {}, []
    for f, boxes in zip(frames, boxes_per_frame):
        H, W = f["label_detected"].shape
        pts = T.transform(f["pcd"], f["T_sensor_to_map"])
        maps = [(i, m.octrees[i], boxes[i]) for i in sorted(m.octrees) if i != 0]
        rendered = T.render(maps, pts, f["K"], f["T_sensor_to_map"], H, W)[0]
        t = T.track(rendered, f["label_detected"], counter, thresholds)
        for d, c in f["class_ids_by_detection"].items():
            if t["remap"][d] != -2:
                classes[t["remap"][d]] = c
        T.integrate_tracked_frame(m, pts, t["label_tracked"], classes, pitch_of,
                                  np.asarray(f["T_sensor_to_map"][:3, 3], np.float32))
        records.append(dict(t, counter_before=counter, label_rendered=rendered, classes=dict(classes), pts_map=pts))
        counter = t["counter"]
    return records, m
