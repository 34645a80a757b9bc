#!/usr/bin/env python
"""Headline benchmark: objects/sec through voxelize -> 3D-CNN -> ICC refine on 32^3 grids.

One "step" = one pass of the whole path over one batch of synthetic input, per GPU:
  ``--scenes-per-gpu`` scenes x 8 objects:
    Model.predict   (ResNet18 + PSPNet, HIP average_voxelization_3d, occupancy branch +
                     conv3/conv4 3D-CNN, HIP interpolate_voxel_grid, 3 pose heads; B = objects)
    arg-max confidence -> per-object pose
    ICC joint refinement of every scene, 100 x {forward, backward, chainer-Adam} on device
    (N > 1) RCCL all-gather of the refined [n,7] poses
Pipelining (the default, ``value``): step k issues network(k) on the main stream, records an
event, and issues ICC(k) + the pose all-gather on a second stream that WAITS on that event --
ICC(k) is ordered after the network pass that produces its poses and overlaps network(k+1),
the way a deployment refines frame k while the network runs on frame k+1.  Every step executes
both stages completely.  ``--no-overlap`` runs them back to back on one stream.
A plain run sets up, warms up, times ``--steps`` steps and prints the headline line (``value``,
``ms_per_step``, ...).  ``--full`` adds everything else the bench measures, after the timed steps:
the serial stage times (``stage_ms``, ``value_serial``), the rate of the hand-written volumetric
path alone (``value_handwritten_path``: voxelize + 3-D CNN + heads + ICC, stock 2-D backbone
excluded), the rooflines, the accuracy of the refined poses, the CPU baseline, the 8-scene and
training extras and the batch-1 latency of BASELINE configs[1] (``latency_batch1_ms``).
``--dump-outputs DIR`` writes the arrays the last timed step computed as ``DIR/<name>.npy``.
Inputs are resident in HBM before the timed region.  Weights are random (no pretrained file is
reachable offline), so the network's poses carry no information: the ICC stage consumes the
network's pose tensor only as its ordering dependency and starts from the scene's synthetic
perturbed-ground-truth poses -- same work, real grids.

Contract: python bench.py --gpus N --steps K --warmup W [--full] [--dump-outputs DIR]
          -> ONE JSON line on rank 0.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import morefusion_amd as mf  # noqa: E402
from morefusion_amd import miopen_cache, parallel  # noqa: E402
from morefusion_amd.contrib.singleview_3d.models import Model  # noqa: E402

HBM_PEAK_GBS = 8000.0  # /opt/skills/guides/MI355X_MICROARCH.md: HBM3E 8 TB/s spec


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps, also measure everything beside the headline: stage breakdown, "
                         "hand-written path, rooflines, accuracy, CPU baseline, 8-scene / training extras, "
                         "batch-1 latency (the --no-* options below trim this set)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the arrays the last timed step computed as DIR/<name>.npy (float32, <= 64 MB "
                         "in all; inputs are seeded, so two builds can be compared output for output)")
    ap.add_argument("--scenes-per-gpu", type=int, default=1)
    ap.add_argument("--objects", type=int, default=8)
    ap.add_argument("--icc-iters", type=int, default=100)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--dtype", choices=["f32", "bf16"], default="f32",
                    help="f32 (default, the reference's precision) or bf16 autocast for the stock "
                         "convolutions / GEMMs of the network (HIP voxel ops, sparse conv3 and ICC stay f32)")
    ap.add_argument("--no-overlap", action="store_true",
                    help="run the network pass and the ICC refinement back to back on one stream")
    ap.add_argument("--channels-last", action="store_true",
                    help="keep the 2-D backbone (ResNet18 + PSPNet) in NHWC memory format")
    ap.add_argument("--priority", choices=["none", "net-high", "icc-high", "icc-low"], default="none",
                    help="HIP stream priorities for the two-stream step (tuning knob)")
    ap.add_argument("--icc-cus", type=int, default=0,
                    help="run the ICC stream on this many of the 256 CUs only (CU-masked HIP stream; 0 = no mask)")
    ap.add_argument("--icc-cu-pattern", choices=["low", "spread"], default="spread")
    ap.add_argument("--split-chip", action="store_true",
                    help="with --icc-cus N: the network runs on a stream masked to the OTHER 256 - N CUs (tuning knob)")
    ap.add_argument("--stage-breakdown", action="store_true", default=True)
    ap.add_argument("--no-latency-probe", action="store_true", help="skip the batch-1 latency child process")
    ap.add_argument("--no-extras", action="store_true",
                    help="skip the un-timed extras value_scenes8 (8 scenes x 8 objects on this GPU) and "
                         "train_objects_per_s (the training step of BASELINE config 5's per-GPU share, child process)")
    ap.add_argument("--probe-latency-b1", action="store_true", help="(internal) batch-1 latency probe, own process")
    ap.add_argument("--dry-run-cpu", action="store_true",
                    help="launcher / collective plumbing check without a GPU: N gloo ranks on the CPU, a stub "
                         "step (synthetic [n_local,7] poses -> the same pose all-gather); no kernel runs and "
                         "the JSON says so -- never a performance number")
    return ap.parse_args()


def load_fixtures():
    fx = []
    for i in range(3):
        p = os.path.join(ROOT, "tests", "golden", f"fixture_pose_refinement_0000000{i}.npz")
        if os.path.exists(p):
            fx.append(dict(np.load(p)))
    return fx


def _low_priority_stream(device):
    """A HIP stream of the device's least priority (torch only exposes normal/high)."""
    import ctypes
    hip = ctypes.CDLL("libamdhip64.so")
    least, greatest = ctypes.c_int(), ctypes.c_int()
    assert hip.hipDeviceGetStreamPriorityRange(ctypes.byref(least), ctypes.byref(greatest)) == 0
    handle = ctypes.c_void_p()
    assert hip.hipStreamCreateWithPriority(ctypes.byref(handle), 1, least.value) == 0  # 1 = non-blocking
    return torch.cuda.ExternalStream(handle.value, device=device)


def _cu_masked_stream(device, n_cus, pattern="low", complement=False):
    """A HIP stream whose kernels may only run on ``n_cus`` of the 256 CUs (hipExtStreamCreateWithCUMask):
    confines the refinement's many short launches to a part of the chip while the network keeps the rest.
    ``complement``: the stream gets the OTHER 256 - n_cus CUs instead (the network's side of a split chip)."""
    import ctypes
    hip = ctypes.CDLL("libamdhip64.so")
    words = (ctypes.c_uint32 * 8)()
    total = 256
    picked = range(n_cus) if pattern == "low" else range(0, total, max(1, total // n_cus))
    for cu in list(picked)[:n_cus]:
        words[cu // 32] |= 1 << (cu % 32)
    if complement:
        for w in range(8):
            words[w] = ~words[w] & 0xffffffff
    handle = ctypes.c_void_p()
    rc = hip.hipExtStreamCreateWithCUMask(ctypes.byref(handle), 8, words)
    assert rc == 0, f"hipExtStreamCreateWithCUMask failed ({rc})"
    return torch.cuda.ExternalStream(handle.value, device=device)


class Workload:
    """Device-resident synthetic inputs + the step function for this rank."""

    def __init__(self, args, rank, device):
        self.args = args
        self.device = device
        S, Nobj = args.scenes_per_gpu, args.objects
        self.B = S * Nobj
        torch.manual_seed(0)
        self.model = Model(n_fg_class=21, with_occupancy=True).to(device).eval()
        if args.channels_last:
            self.model.resnet_extractor.to(memory_format=torch.channels_last)
            self.model.pspnet_extractor.to(memory_format=torch.channels_last)
        batch = mf.synthetic.make_singleview_batch(self.B, seed=1000 * rank)
        to = lambda x: torch.as_tensor(x).to(device)  # noqa: E731
        self.inputs = dict(class_id=to(batch["class_id"]), rgb=to(batch["rgb"]), pcd=to(batch["pcd"]),
                           pitch=to(batch["pitch"]), origin=to(batch["origin"]),
                           grid_nontarget_empty=to(batch["grid_nontarget_empty"]))
        fixtures = load_fixtures()
        self.scenes_np = [mf.synthetic.make_icc_scene(Nobj, seed=1000 * rank + s, fixtures=fixtures)
                          for s in range(S)]
        dicts = [dict(points=s["points"], sdf=s["sdf"], pitch=s["pitch"], origin=s["origin"],
                      grid_target=s["grid_target"], grid_nontarget_empty=s["grid_nontarget_empty"])
                 for s in self.scenes_np]
        self.icc = mf.contrib.IccScenes(dicts, sdf_offset=0.02, device=device)
        from morefusion_amd.geometry import quaternion_from_matrix
        q0 = np.concatenate([np.stack([quaternion_from_matrix(T) for T in s["transform_init"]])
                             for s in self.scenes_np]).astype(np.float32)
        t0 = np.concatenate([s["transform_init"][:, :3, 3] for s in self.scenes_np]).astype(np.float32)
        self.q0, self.t0 = to(q0), to(t0)
        self.q, self.t = self.q0.clone(), self.t0.clone()
        self.m = torch.zeros((self.B, 7), device=device)
        self.v = torch.zeros((self.B, 7), device=device)
        self.world = dist.get_world_size() if dist.is_initialized() else 1
        self.gathered = torch.empty((self.world * self.B, 7), device=device)
        self.events = []
        self.icc_stream = torch.cuda.Stream(device=device, priority=-1 if args.priority == "icc-high" else 0)
        self.net_stream = torch.cuda.Stream(device=device, priority=-1) if args.priority == "net-high" else None
        if args.priority == "icc-low":
            self.icc_stream = _low_priority_stream(device)
        if args.icc_cus:
            self.icc_stream = _cu_masked_stream(device, args.icc_cus, args.icc_cu_pattern)
            if args.split_chip:
                self.net_stream = _cu_masked_stream(device, args.icc_cus, args.icc_cu_pattern, complement=True)

    def _mark(self, name):
        if self._timing:
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            self.events.append((name, e))

    def _refine(self, network_poses=None):
        # network_poses [B,7]: the stream-ordered dependency of this refinement (see module doc)
        self.q.copy_(self.q0)
        self.t.copy_(self.t0)
        self.m.zero_()
        self.v.zero_()
        self.icc.refine(self.q, self.t, self.m, self.v, self.args.icc_iters, step0=0,
                        alpha_q=0.01, alpha_t=0.001)

    def _network(self):
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=self.args.dtype == "bf16"):
            rot, trans, conf = self.model.predict(**self.inputs)
        rot, trans, conf = rot.float(), trans.float(), conf.float()
        self.last_predict = dict(network_rot=rot, network_trans=trans, network_conf=conf)  # for --dump-outputs
        idx = conf.argmax(dim=1)
        ar = torch.arange(self.B, device=self.device)
        return torch.cat([rot[ar, idx], trans[ar, idx]], dim=1)  # [B,7] network poses

    @torch.no_grad()
    def step(self, timing=False):
        """One pass of the path over this rank's batch.  Default: network(k) on the main stream,
        then ICC(k) + pose all-gather on a second stream behind an event recorded after
        network(k); the next call's network(k+1) does not wait for ICC(k).  ``timing=True``
        (stage breakdown, un-timed) and ``--no-overlap`` run the stages back to back."""
        self._timing = timing
        overlap = not (timing or self.args.no_overlap)
        self._mark("start")
        if overlap:
            main = torch.cuda.current_stream()
            net = self.net_stream if self.net_stream is not None else main
            if net is not main:
                net.wait_stream(main)
            with torch.cuda.stream(net):
                pred = self._network()
                done = torch.cuda.Event()
                done.record(net)
            pred.record_stream(self.icc_stream)
            with torch.cuda.stream(self.icc_stream):
                self.icc_stream.wait_event(done)  # ICC(k) after network(k) ...
                self._refine(pred)                # ... beside network(k+1) of the next call
                poses = torch.cat([self.q, self.t], dim=1)
                out = parallel.all_gather_poses_equal(poses, out=self.gathered if self.world > 1 else None)
            return out, pred
        pred = self._network()
        self._mark("predict")
        self._refine(pred)
        self._mark("icc")
        poses = torch.cat([self.q, self.t], dim=1)
        out = parallel.all_gather_poses_equal(poses, out=self.gathered if self.world > 1 else None)
        self._mark("gather")
        return out, pred


class StubWorkload:
    """``--dry-run-cpu``: the step's communication skeleton only -- this rank's [n_local,7] "poses" are a
    deterministic function of (rank, object) and go through the same ``all_gather_poses_equal`` the real
    step ends with, over gloo.  Proves the launcher (N ranks, one JSON line from rank 0) and that the
    gathered tensor has world x n_local rows in rank order."""

    def __init__(self, args, rank, device):
        self.B = args.scenes_per_gpu * args.objects
        self.world = dist.get_world_size() if dist.is_initialized() else 1
        ids = torch.arange(rank * self.B, (rank + 1) * self.B, dtype=torch.float32, device=device)
        self.poses = torch.stack([ids * 10.0 + k for k in range(7)], dim=1)
        self.gathered = torch.empty((self.world * self.B, 7), device=device)

    def step(self):
        out = parallel.all_gather_poses_equal(self.poses, out=self.gathered if self.world > 1 else None)
        return out, self.poses


def gather_evidence(wl, device):
    """What the last step's collective saw: rows of the gathered pose tensor and the rank census."""
    out, _ = wl.step()
    return dict(gathered_rows=int(out.shape[0]), rows_per_rank=int(wl.B),
                ranks_seen=parallel.rank_census(device))


DUMP_LIMIT_BYTES = 64 * 2 ** 20


def dump_outputs(dirname, arrays):
    """``--dump-outputs``: each array as ``dirname/<name>.npy`` in float32 (float64 stays float64).  An array larger
    than its share of the 64 MB limit is replaced by a fixed, seeded sample of its elements (flattened, in index order),
    the same sample for the same shape in every run."""
    os.makedirs(dirname, exist_ok=True)
    share = DUMP_LIMIT_BYTES // max(1, len(arrays))
    for name, t in arrays.items():
        a = t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
        a = a.astype(np.float64 if a.dtype == np.float64 else np.float32)
        if a.nbytes > share:
            flat = a.reshape(-1)
            keep = np.sort(np.random.RandomState(0).choice(flat.size, share // a.itemsize, replace=False))
            a = flat[keep]
        np.save(os.path.join(dirname, f"{name}.npy"), a)


def time_kernel_live(fn, reps):
    """Average duration (ms) of ``fn``'s launches measured with HIP events on the stream
    they are issued to (torch's current stream)."""
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    torch.cuda.synchronize()
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps


def roofline_voxelize(wl):
    """The dense HBM-bound op of the volumetric API: mf_average_voxelization_3d_fwd (memset fill +
    link + scatter launches), timed on the arguments the pose network has for it (B objects,
    P = 1000 clustered surface points each, C = 144 features, 32^3 grid).  The training path
    calls it; inference feeds the same chains straight into conv3's GEMM rows
    (mf_sparse_conv3d_k4s2_points_fwd) and never builds the dense tensor.
    Algorithmic bytes / object: read P*(12+4C+4) + write C*D^3*4 + D^3*4."""
    m, inp = wl.model, wl.inputs
    with torch.no_grad():
        pix = m._select_points(inp["pcd"])
        _, points = m._backbone_features(inp["rgb"], inp["pcd"], pix)
        points = (points - inp["origin"].float()[:, :, None]) / inp["pitch"].float()[:, None, None]
    B, D = points.shape[0], m._voxel_dim
    P, C = points.shape[2], 144
    pts = points.transpose(1, 2).reshape(B * P, 3).contiguous()
    values = torch.randn(B * P, C, device=wl.device)
    bi = torch.arange(B, dtype=torch.int32, device=wl.device).repeat_interleave(P)
    kw = dict(batch_size=B, origin=(0, 0, 0), pitch=1.0, dimensions=(D, D, D), check_nan=False)
    ms = time_kernel_live(lambda: mf.functions.average_voxelization_3d(values, pts, bi, **kw), 50)
    alg = B * (P * (12 + 4 * C + 4) + C * D ** 3 * 4 + D ** 3 * 4)
    achieved = alg / (ms * 1e-3) / 1e9
    # HBM bytes per call from the PMC passes committed under profiles/ (separate rocprofv3
    # --pmc FETCH_SIZE / WRITE_SIZE runs of tools/prof_voxelize.py at this exact shape)
    traffic = None
    pmc = os.path.join(ROOT, "profiles", "r04_voxelize_pmc.json")  # this round's kernels (fill kernel + link + scatter)
    if os.path.exists(pmc):
        rec = json.load(open(pmc))
        if rec["shape"] == dict(B=B, P=P, C=C, D=D):
            traffic = rec["traffic_bytes"]
    return dict(kernel="mf_average_voxelization_3d_fwd (k_fill_words + k_avgvox_link + k_avgvox_scatter)",
                bound="hbm", achieved=round(achieved, 1), peak=HBM_PEAK_GBS, unit="GB/s",
                frac=round(achieved / HBM_PEAK_GBS, 4), traffic=traffic,
                algorithmic_bytes_per_launch=alg, avg_launch_ms=round(ms, 5),
                shape=dict(B=B, P=P, C=C, D=D))


def _icc_algorithmic_bytes(icc):
    """SURVEY.md 8d, ICC: per iteration and scene of N objects, forward reads
    sum_i (P_i + sum_{j != i} P_j) * 16 B (points + sdf, own + others) + N * 2 * D^3 * 4 B
    (target and no-entry grids), no grid bytes written (winners are an implementation buffer);
    the backward re-reads the same.  Returns (point bytes, grid bytes) of one forward."""
    so = icc.scene_off_host
    off = icc.obj_off.cpu().tolist()
    pairs = 0
    for s in range(icc.n_scenes):
        pairs += (so[s + 1] - so[s]) * (off[so[s + 1]] - off[so[s]])
    return pairs * 16, icc.n_objects * 2 * icc.dim ** 3 * 4


def icc_many_scenes(wl, n_scenes=8):
    """The same two kernels with 8 scenes x 8 objects in one batch (BASELINE config 4's per-GPU share when a
    node runs 64 objects on ONE GPU): the launches are shared, so the per-scene latency terms amortise."""
    args = wl.args
    fixtures = load_fixtures()
    scenes = [mf.synthetic.make_icc_scene(args.objects, seed=50 + s, fixtures=fixtures) for s in range(n_scenes)]
    dicts = [dict(points=s["points"], sdf=s["sdf"], pitch=s["pitch"], origin=s["origin"],
                  grid_target=s["grid_target"], grid_nontarget_empty=s["grid_nontarget_empty"]) for s in scenes]
    icc = mf.contrib.IccScenes(dicts, sdf_offset=0.02, device=wl.device)
    from morefusion_amd.geometry import quaternion_from_matrix
    q0 = torch.as_tensor(np.concatenate([np.stack([quaternion_from_matrix(T) for T in s["transform_init"]])
                                         for s in scenes]).astype(np.float32)).to(wl.device)
    t0 = torch.as_tensor(np.concatenate([s["transform_init"][:, :3, 3] for s in scenes]).astype(np.float32)).to(wl.device)
    q, t = q0.clone(), t0.clone()
    m, v = torch.zeros((q.shape[0], 7), device=wl.device), torch.zeros((q.shape[0], 7), device=wl.device)

    def run():
        q.copy_(q0); t.copy_(t0); m.zero_(); v.zero_()
        icc.refine(q, t, m, v, args.icc_iters, step0=0, alpha_q=0.01, alpha_t=0.001)

    ms = time_kernel_live(run, 3)
    pts_bytes, grid_bytes = _icc_algorithmic_bytes(icc)
    it_bytes = 2 * (pts_bytes + grid_bytes)
    us = ms * 1e3 / args.icc_iters
    gbs = it_bytes / (us * 1e-6) / 1e9
    out = dict(scenes=n_scenes, objects=int(q.shape[0]), algorithmic_bytes=it_bytes, us=round(us, 3),
               us_per_scene=round(us / n_scenes, 3), achieved=round(gbs, 1), frac=round(gbs / HBM_PEAK_GBS, 4),
               workspace_mb=round(icc.ws.numel() / 1e6, 1))
    # the throughput regime's counters (rocprofv3 --pmc passes of these launches at 8 scenes, round 6): where a wave's
    # time goes and how much of the launch is VALU issue alone
    pmc = os.path.join(ROOT, "profiles", "r06_icc_issue_pmc_scenes8.json")
    if n_scenes == 8 and args.objects == 8 and os.path.exists(pmc):
        ks = json.load(open(pmc))["kernels"]
        out["counters"] = dict(source="profiles/r06_icc_issue_pmc_scenes8.json", **{
            k: dict(us=v["avg_duration_us_kernel_trace"], insts_per_wave={n: v["per_wave"][n] for n in ("valu", "salu", "lds", "smem", "vmem_rd")},
                    valu_issue_floor_us=v["valu_floor_us_at_2.4GHz"], valu_issue_frac_of_launch=v["valu_floor_frac_of_duration"],
                    wave_life_frac=v["fractions_of_wave_lifetime"], resident_waves_per_simd=v["mean_resident_waves_per_simd"])
            for k, v in ks.items()})
    return out


def icc_issue_model(kname, icc, us_live):
    """A ceiling that is not HBM: what the kernel would take if only INSTRUCTION ISSUE and the LDS pipe limited it,
    from rocprofv3 --pmc passes of the same launches (profiles/r04_icc_issue_pmc.json: SQ_INSTS_* / SQ_WAVES /
    SQ_LDS_* / SQ_WAVE_CYCLES per launch, 1 scene x 8 objects).
      valu_floor_us      wave-level VALU instructions / 1024 SIMDs x 4 cycles (a wave64 VALU op occupies its SIMD
                         for 4 cycles) at 2.4 GHz -- perfect balance over every SIMD of the chip
      lds_floor_us       SQ_LDS_IDX_ACTIVE + SQ_LDS_BANK_CONFLICT cycles / 256 CUs
      latency_chain_us   the dependent global round trips on a workgroup's critical path (bin counts -> records ->
                         winner gathers: 3 x ~0.8 us, MI355X_MICROARCH.md) + one kernel boundary (1.45 us)
      floor_us           max(valu, lds) + latency chain: nothing overlaps the chain, issue overlaps perfectly
    ``frac_of_floor`` = floor / measured: how far the kernel is from that (unreachable) bound."""
    path = os.path.join(ROOT, "profiles", "r04_icc_issue_pmc.json")
    if not os.path.exists(path):
        return None
    rec = next((v for k, v in json.load(open(path)).items() if k.startswith(kname + " ")), None)
    if rec is None or icc.n_objects != 8:
        return None
    ghz = 2.4
    valu = rec["SQ_INSTS_VALU"] / 1024 * 4 / (ghz * 1e3)
    lds = (rec["SQ_LDS_IDX_ACTIVE"] + rec["SQ_LDS_BANK_CONFLICT"]) / 256 / (ghz * 1e3)
    chain = 3 * 0.8 + 1.45
    floor = max(valu, lds) + chain
    waves = rec["SQ_WAVES"]
    return dict(source="profiles/r04_icc_issue_pmc.json", waves=int(waves),
                insts_per_wave=dict(valu=round(rec["SQ_INSTS_VALU"] / waves, 1), salu=round(rec["SQ_INSTS_SALU"] / waves, 1),
                                    lds=round(rec["SQ_INSTS_LDS"] / waves, 1), vmem_rd=round(rec["SQ_INSTS_VMEM_RD"] / waves, 1)),
                wave_lifetime_us=round(rec["SQ_WAVE_CYCLES"] * 4 / waves / (ghz * 1e3), 2),
                wait_frac_of_wave_cycles=round(rec["SQ_WAIT_INST_ANY"] / rec["SQ_WAVE_CYCLES"], 3),
                valu_floor_us=round(valu, 2), lds_floor_us=round(lds, 2), latency_chain_us=round(chain, 2),
                floor_us=round(floor, 2), measured_us=round(us_live, 2), frac_of_floor=round(floor / us_live, 3),
                us_under_pmc=rec.get("avg_duration_us_under_pmc"))


def roofline_icc(wl, us_per_iter):
    """k_icc_fused (k_icc_tile on the two-kernel path of non-{0,1} no-entry grids) -- the hand-written
    kernel with the largest share of the step (100 launches per refinement), timed live with HIP
    events through mf_icc_launch_stage on torch's current stream.  Its algorithmic HBM bytes per
    launch (8d): every grid reads its source points once, 16 B each, plus (single-pass kernel) its
    two input grids.  ``iteration`` is the same accounting for one whole ICC iteration (k_icc_bin
    incl. the folded optimiser step + k_icc_fused): forward + backward re-read, 8d's 11.3 MB per
    8-object scene.  The working set is L2/MALL resident and the kernels are bound by
    dependent-load latency and instruction issue, not by HBM bandwidth -- the fractions below are
    what the contract asks for, not a claim that HBM is the limiter."""
    import ctypes
    icc = wl.icc
    lib = mf._lib.lib()
    stream = mf._lib.stream_ptr()
    mf._lib.check(lib.mf_icc_launch_stage(ctypes.byref(icc.desc), wl.q0.data_ptr(), wl.t0.data_ptr(),
                                          icc.ws.data_ptr(), 0, stream), "mf_icc_launch_stage")
    single_pass = bool(icc.desc.grid_ne_binary) and not os.environ.get("MF_ICC_GENERAL")
    stage = 2 if single_pass else 1
    mf._lib.check(lib.mf_icc_launch_stage(ctypes.byref(icc.desc), None, None, icc.ws.data_ptr(), stage, stream),
                  "mf_icc_launch_stage")
    ms = time_kernel_live(lambda: lib.mf_icc_launch_stage(ctypes.byref(icc.desc), None, None,
                                                          icc.ws.data_ptr(), stage, stream), 200)
    pts_bytes, grid_bytes = _icc_algorithmic_bytes(icc)
    # k_icc_fused reads the points of every (grid, source) pair once and the two input grids;
    # k_icc_tile (two-kernel path) only the points
    alg = pts_bytes + grid_bytes if single_pass else pts_bytes
    kname = "k_icc_fused" if single_pass else "k_icc_tile"
    achieved = alg / (ms * 1e-3) / 1e9
    traffic = None  # PMC passes of THIS round committed under profiles/ (tools/gpu_call.sh pmc=...), same scene; else null
    for name in ("r05_icc_pmc.json", "r04_icc_pmc.json", "r03_icc_pmc.json"):  # newest PMC passes of these kernels, same scene
        pmc = os.path.join(ROOT, "profiles", name)
        if os.path.exists(pmc):
            rec = json.load(open(pmc)).get(kname)
            if rec and rec["n_objects"] == icc.n_objects and rec["n_points"] == icc.n_points:
                traffic = rec["traffic_bytes"]
                break
    issue = icc_issue_model(kname, icc, ms * 1e3)
    it_bytes = 2 * (pts_bytes + grid_bytes)
    it_achieved = it_bytes / (us_per_iter * 1e-6) / 1e9
    many = icc_many_scenes(wl)
    return dict(kernel=(f"{kname} (launch 2 of 2 per ICC iteration; mf_icc_refine)" if single_pass else
                        f"{kname} (launch 2 of 3 per ICC iteration; mf_icc_refine)"), bound="hbm",
                achieved=round(achieved, 1), peak=HBM_PEAK_GBS, unit="GB/s",
                frac=round(achieved / HBM_PEAK_GBS, 4), traffic=traffic,
                algorithmic_bytes_per_launch=alg, avg_launch_ms=round(ms, 5),
                clock="avg_launch_ms / us: live HIP events at un-profiled clocks; traffic and issue_model counters: "
                      "rocprofv3 --pmc passes (the same launches run ~10-15 % longer under the profiler)",
                issue_model=issue,
                iteration=dict(kernels="k_icc_bin (+ folded optimiser step) + " +
                                       ("k_icc_fused" if single_pass else "k_icc_tile + k_icc_accum"),
                               algorithmic_bytes=it_bytes, us=round(us_per_iter, 3),
                               achieved=round(it_achieved, 1), frac=round(it_achieved / HBM_PEAK_GBS, 4)),
                iteration_8_scenes=many,
                note="L2-resident working set; latency / instruction-issue bound (DESIGN.md 4)")


def handwritten_path(wl, reps=10):
    """Stage times (ms) of the hand-written volumetric path alone: Model._pose_from_features
    (voxelize, occupancy convs, sparse conv3, conv4, trilinear sampling, heads) on the features
    one predict() hands it, and the ICC refinement; the stock 2-D backbone is excluded."""
    m = wl.model
    inp = wl.inputs
    with torch.no_grad():
        pix = m._select_points(inp["pcd"])
        values, points = m._backbone_features(inp["rgb"], inp["pcd"], pix)
        args = (torch.as_tensor(inp["class_id"], device=wl.device), values, points, inp["pitch"].float(),
                inp["origin"].float(), inp["grid_nontarget_empty"])
        t_vol = time_kernel_live(lambda: m._pose_from_features(*args), reps)
        t_icc = time_kernel_live(wl._refine, reps)
    return t_vol, t_icc


def latency_batch1_measure(model, one, reps=12):
    """Per-frame latency (ms, host clock around call + device sync, i.e. input ready -> poses ready) of
      predict            eager launches, incl. the host synchronisation of the point selection;
      predict_graphed    the same work with everything after the selection replayed from one hipGraph.
    (Round 3 also measured the graph with the NEXT frame's selection prefetched on a side stream,
    Model.select_points_async: 2.1-2.3 ms vs 1.8 ms -- slower, and that phase faulted the GPU in 3 of 9
    probe processes; it is not part of the probe any more)"""
    m = model

    def per_frame(fn):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
            torch.cuda.synchronize()
        return (time.perf_counter() - t0) / reps * 1e3

    out = {}
    with torch.no_grad():
        out["predict"] = round(per_frame(lambda: m.predict(**one)), 4)
        print(json.dumps(out), flush=True)  # (the probe's parent keeps the last complete line)
        out["predict_graphed"] = round(per_frame(lambda: m.predict_graphed(**one, clone=False)), 4)
        print(json.dumps(out), flush=True)
    return out


def latency_probe_main():
    """`python bench.py --probe-latency-b1`: BASELINE configs[1] (batch 1) in a process of its own."""
    torch.cuda.set_device(0)
    # MIOpen find mode on, like the bench's own model (round 3 ran this probe with immediate-mode solvers because the
    # graph phases faulted with find mode on; the cause -- memset nodes in the captured graph, DESIGN.md 6 -- is gone
    # since round 4: 6 of 6 processes clean with find mode, 20 of 20 without).  MF_PROBE_BENCHMARK=0: immediate mode.
    torch.backends.cudnn.benchmark = os.environ.get("MF_PROBE_BENCHMARK", "1") == "1"
    torch.manual_seed(0)
    model = Model(n_fg_class=21, with_occupancy=True).cuda().eval()
    batch = mf.synthetic.make_singleview_batch(1, seed=0)
    one = {k: torch.as_tensor(batch[k]).cuda() for k in
           ("class_id", "rgb", "pcd", "pitch", "origin", "grid_nontarget_empty")}
    latency_batch1_measure(model, one)


def latency_batch1(wl):
    """BASELINE configs[1]: singleview_3d inference at batch = 1.  ``predict`` (eager launches, incl. the host
    synchronisation of the point selection) is measured here, in this process, with the bench's own model
    (MIOpen find mode on).  The hipGraph replay is measured in a CHILD process (``probe``), a leftover of round 3's
    intermittent replay faults (memset nodes, replaced by fill kernels in round 4) that costs nothing
    and keeps a failure of the probe from costing the headline line.  A failed probe is reported as such."""
    import subprocess
    one = {k: v[:1].contiguous() for k, v in wl.inputs.items()}
    out = {}
    with torch.no_grad():
        for _ in range(3):
            wl.model.predict(**one)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(30):
            wl.model.predict(**one)
            torch.cuda.synchronize()
        out["predict"] = round((time.perf_counter() - t0) / 30 * 1e3, 4)
    env = {k: v for k, v in os.environ.items()
           if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    probe = {"note": "own process, MIOpen find mode on, host clock incl. device sync"}
    try:
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--probe-latency-b1"], env=env,
                           capture_output=True, text=True, timeout=150)
        lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
        probe.update(json.loads(lines[-1]) if lines else {})
        if p.returncode != 0:
            probe["probe_error"] = f"exit code {p.returncode}: " + (p.stderr.strip().splitlines() or ["?"])[-1][:200]
    except Exception as e:  # noqa: BLE001
        probe["probe_error"] = f"{type(e).__name__}: {e}"[:300]
    out["probe"] = probe
    return out


MFMA_F32_PEAK_TFLOPS = 157.3  # MI355X_MICROARCH.md: v_mfma_f32_32x32x2_f32, 64 FLOP/clk/SIMD x 1024 SIMDs x 2.4 GHz


def roofline_conv4(wl, B):
    """k_conv3d_k4s2_mfma on conv4's shape (256 -> 512 channels, 16^3 -> 8^3, B objects): the largest GEMM of the
    hand-written volumetric part, timed live with HIP events (split-K slabs + k_conv_finish included)."""
    m = wl.model
    if getattr(m, "_volumetric_cl", None) is None:
        return None
    vol = m._volumetric_cl
    h3 = torch.relu(torch.randn(B, 16 ** 3, 256, device=wl.device))
    with torch.no_grad():
        ms = time_kernel_live(lambda: vol.conv_k4s2("conv4", m.conv4, h3, B, 16, cin=256), 30)
    flop = 2.0 * B * 512 * 512 * 64 * 256
    tf = flop / (ms * 1e-3) / 1e12
    traffic, mfma_busy = None, None  # PMC passes of THIS round (profiles/r03_mfma_kernels_pmc.json), B = 8 only
    pmc = os.path.join(ROOT, "profiles", "r03_mfma_kernels_pmc.json")
    if B == 8 and os.path.exists(pmc):
        ps = json.load(open(pmc))["passes"]
        k, f = "k_conv3d_k4s2_mfma grid=131072", "k_conv_finish grid=524288"
        try:
            traffic = int(ps["fetch_conv4"][k]["fetch_bytes_x2_gfx950"] + ps["write_conv4"][k]["write_bytes"]
                          + ps["fetch_conv4"][f]["fetch_bytes_x2_gfx950"] + ps["write_conv4"][f]["write_bytes"])
            mfma_busy = ps["mfma_conv4"][k]["mfma_pipe_util"]
        except KeyError:
            pass
    return dict(kernel="k_conv3d_k4s2_mfma (+ k_conv_finish) on conv4, mf_conv3d_k4s2_fwd", bound="mfma",
                achieved=round(tf, 1), peak=MFMA_F32_PEAK_TFLOPS, unit="TFLOP/s",
                frac=round(tf / MFMA_F32_PEAK_TFLOPS, 4), traffic=traffic, mfma_pipe_busy_pmc=mfma_busy,
                flop_per_launch=flop,
                avg_launch_ms=round(ms, 5), shape=dict(B=B, Cin=256, Cout=512, D=16),
                split_k=mf._lib.lib().mf_conv3d_k4s2_default_split(B, 256, 512, 16))


MFMA_BF16_PEAK_TFLOPS = 2500.0  # MI355X_MICROARCH.md: dense bf16 MFMA (v_mfma_f32_32x32x16_bf16)


def roofline_bf16_kernels(wl, B=16):
    """The bf16 MFMA kernels of csrc/gemm_bf16.hip at BASELINE config 5's per-GPU training batch (16 objects, 1000
    points each), timed live with HIP events; TFLOP/s against the dense bf16 MFMA peak.
    * conv4 256 -> 512 on 16^3: forward (split-K over fp32 slabs), data gradient, weight gradient -- what the step runs;
    * sparse_conv3_*: the three GEMMs of conv3 on the compact parity-class rows of the OCCUPIED voxels (what the step
      runs since round 5; effective FLOP = 2 x rows x 144 x 2048, the rows incl. the class padding);
    * heads1_*: the largest 1 x 1 convolution (all heads' first layer: [n, 984] x [984, 1920]);
    * conv3_dense_*: conv3 160 -> 256 on the dense 32^3 grid -- NOT in the training step any more (sparse conv3), kept
      as the engine's large-shape reference (the shapes the round-4/5 fractions were quoted on)."""
    L, st, p = mf._lib.lib(), mf._lib.stream_ptr, (lambda t: t.data_ptr())
    dev, bf = wl.device, torch.bfloat16
    out = {}

    def rec(key, kernel, fn, flop, shape, **extra):
        ms = time_kernel_live(fn, 10)
        tf = flop / (ms * 1e-3) / 1e12
        out[key] = dict(kernel=kernel, bound="mfma", achieved=round(tf, 1), peak=MFMA_BF16_PEAK_TFLOPS, unit="TFLOP/s",
                        frac=round(tf / MFMA_BF16_PEAK_TFLOPS, 4), flop_per_launch=flop, avg_launch_ms=round(ms, 5),
                        shape=shape, **extra)

    for name, key, Cin, Cout, D in (("conv3", "conv3_dense", 160, 256, 32), ("conv4", "conv4", 256, 512, 16)):
        Do = D // 2
        flop = 2.0 * B * Do ** 3 * Cout * 64 * Cin
        x = torch.randn(B, D ** 3, Cin, device=dev).to(bf)
        dy = torch.randn(B, Do ** 3, Cout, device=dev).to(bf)
        W = torch.randn(Cout, Cin, 4, 4, 4, device=dev) / (64 * Cin) ** 0.5
        wt = torch.empty(Cout, 64, Cin, dtype=bf, device=dev)
        wd = torch.empty(8, Cin, 8, Cout, dtype=bf, device=dev)
        L.mf_conv3d_k4s2_pack_bf16(p(W), Cout, Cin, Cin, 0, p(wt), p(wd), st())
        y = torch.empty(B, Do ** 3, Cout, dtype=bf, device=dev)
        dx = torch.empty(B, D ** 3, Cin, dtype=bf, device=dev)
        dW = torch.empty_like(W)
        split = L.mf_conv3d_k4s2_bf16_wgrad_default_split(B, Cin, Cout, D)
        ws = torch.empty(L.mf_conv3d_k4s2_bf16_wgrad_workspace_bytes(Cin, Cout, split), dtype=torch.uint8, device=dev)
        nws = L.mf_conv3d_bf16_fwd_workspace_bytes(B, Cin, Cout, D, 4, 2, 1, 1)
        fws = torch.empty(max(nws, 16), dtype=torch.uint8, device=dev)
        shape = dict(B=B, Cin=Cin, Cout=Cout, D=D)
        rec(f"{key}_fwd", "k_gemm_nt_bf16_pp<conv forward>" + (" split-K + k_splitk_finish" if nws else ""),
            lambda: L.mf_conv3d_bf16_fwd_ws(p(x), p(wt), None, p(y), p(fws), nws, B, Cin, Cout, D, 4, 2, 1, 1, 1, 0, Cout, st()),
            flop, shape, splitk_workspace_mb=round(nws / 2 ** 20, 1))
        rec(f"{key}_dgrad", "k_gemm_nt_bf16_pp<conv dgrad>" + ("" if Cin >= 192 else " (N = 160: one 256-column tile, 96 columns idle)"),
            lambda: L.mf_conv3d_k4s2_bf16_dgrad(p(dy), p(wd), p(dx), B, Cin, Cout, D, 0, 0, st()), flop, shape)
        rec(f"{key}_wgrad", "k_gemm_tn_bf16 (+ k_wgrad_finish)",
            lambda: L.mf_conv3d_k4s2_bf16_wgrad(p(dy), p(x), p(dW), p(ws), B, Cin, Cout, D, Cin, 0, split, st()), flop, shape)
        del x, dy, y, dx, ws, fws
    # the heads' first layer
    n, K, N = B * 1000, 984, 1920
    A = torch.randn(n, K, device=dev).to(bf)
    Wl = (torch.randn(N, K, device=dev) / K ** 0.5).to(bf)
    Wlt = Wl.t().contiguous()
    yl = torch.empty(n, N, dtype=bf, device=dev)
    dA = torch.empty(n, K, dtype=bf, device=dev)
    dWl = torch.empty(N, K, device=dev)
    wsl = torch.empty(4 * N * K, device=dev)
    flop = 2.0 * n * K * N
    shape = dict(M=n, K=K, N=N)
    rec("heads1_fwd", "k_gemm_nt_bf16_pp<rows>", lambda: L.mf_linear_bf16(p(A), 0, K, p(Wl), 0, K, None, 0, p(yl), 0, N, n, N, K, 1, 1, 0, 0, st()), flop, shape)
    rec("heads1_dgrad", "k_gemm_nt_bf16_pp<rows>", lambda: L.mf_linear_bf16(p(yl), 0, N, p(Wlt), 0, N, None, 0, p(dA), 0, K, n, K, N, 1, 0, 0, 0, st()), flop, shape)
    rec("heads1_wgrad", "k_gemm_tn_bf16 (+ k_wgrad_finish), split 4", lambda: L.mf_linear_wgrad_bf16(p(yl), 0, N, p(A), 0, K, p(dWl), 0, K, p(wsl), n, N, K, 1, 4, st()), flop, shape)
    del A, yl, dA, wsl
    # conv3 on the compact rows of the occupied voxels (clustered surface points as the model sees them)
    import ctypes
    P, Cs, Cout, D = 1000, 144, 256, 32
    n = B * P
    torch.manual_seed(5)
    u = torch.rand(n, 2, device=dev) * 2 - 1
    pts = torch.stack([16 + 9 * u[:, 0], 16 + 9 * u[:, 1], 16 - 8 * torch.sqrt((1 - (u ** 2).sum(1) / 2).clamp(min=0))], 1).contiguous()
    bi = torch.arange(B, dtype=torch.int32, device=dev).repeat_interleave(P)
    wsb = torch.empty(L.mf_sparse_conv3_bf16_workspace_bytes(n, B, D), dtype=torch.uint8, device=dev)
    mf._lib.check(L.mf_sparse_conv3_bf16_index(p(pts), p(bi), n, B, D, p(wsb), st()), "index")
    tabs = (ctypes.c_int64 * 7)()
    L.mf_sparse_conv3_bf16_tables(p(wsb), n, B, D, tabs)
    t_group, t_range = int(tabs[0]), int(tabs[1])
    Mp, N8 = int(L.mf_sparse_conv3_bf16_max_rows(n)), 8 * Cout
    off = t_range - p(wsb)  # the 9 class offsets live inside the workspace tensor
    rows = int(wsb[off:off + 36].view(torch.int32)[8])  # rows incl. the padding of each class to a multiple of 128
    A = torch.randn(Mp, Cs, device=dev).to(bf)
    Wp = (torch.randn(8, N8, Cs, device=dev) / Cs ** 0.5).to(bf)
    Wq = Wp.transpose(1, 2).contiguous()
    C = torch.empty(Mp, N8, dtype=bf, device=dev)
    dAr = torch.empty(Mp, Cs, dtype=bf, device=dev)
    dWp = torch.empty(8, N8, Cs, device=dev)
    flop = 2.0 * rows * Cs * N8
    shape = dict(B=B, P=P, rows=rows, K=Cs, N=N8)
    rec("sparse_conv3_fwd", "k_gemm_nt_bf16<rows + tile_group>", lambda: L.mf_linear_bf16_tiles(p(A), Cs, p(Wp), N8 * Cs, Cs, t_group, p(C), N8, Mp, N8, Cs, 0, st()), flop, shape,
        note="K = 144: 2.25 K-tiles per output tile -- bound by writing C [rows, 2048] bf16, not by the MFMA pipe")
    rec("sparse_conv3_dgrad", "k_gemm_nt_bf16<rows + tile_group>", lambda: L.mf_linear_bf16_tiles(p(C), N8, p(Wq), Cs * N8, N8, t_group, p(dAr), Cs, Mp, Cs, N8, 0, st()), flop, shape)
    rec("sparse_conv3_wgrad", "k_gemm_tn_bf16<m_range>", lambda: L.mf_linear_wgrad_bf16_ranges(p(C), N8, p(A), Cs, p(dWp), N8 * Cs, Cs, t_range, 8, N8, Cs, st()), flop, shape)
    return out


def accuracy(wl):
    """The accuracy half of BASELINE's metric, as far as it is measurable offline: ADD of the
    ICC-refined poses to the known ground truth of the synthetic objects of this rank's first
    scene (the three recorded fixtures carry no ground truth), before and after refinement,
    with the YCB-Video AUC (<= 0.1 m).  Un-timed; uses the poses the timed steps produced."""
    from morefusion_amd.metrics import average_distance, ycb_video_add_auc
    sc = wl.scenes_np[0]
    idx = [i for i, T in enumerate(sc["transform_gt"]) if T is not None]
    if not idx:
        return None
    T_ref = mf.functions.transformation_matrix(wl.q, wl.t).cpu().numpy().astype(np.float64)
    pts = [sc["points"][i].astype(np.float64) for i in idx]
    gt = [np.asarray(sc["transform_gt"][i], np.float64) for i in idx]
    add0, _ = average_distance(pts, gt, [sc["transform_init"][i].astype(np.float64) for i in idx])
    add1, _ = average_distance(pts, gt, [T_ref[i] for i in idx])
    return dict(objects_with_ground_truth=len(idx),
                add_init_mm=round(float(add0.mean()) * 1e3, 3), add_refined_mm=round(float(add1.mean()) * 1e3, 3),
                add_auc_init=round(float(ycb_video_add_auc(add0, max_value=0.1)), 4),
                add_auc_refined=round(float(ycb_video_add_auc(add1, max_value=0.1)), 4),
                note="ICC refinement of synthetic perturbed-GT poses; network weights are random, so "
                     "network-pose accuracy is not measurable offline")


def cpu_baseline(wl, args):
    """The same workload on the host cores: torch-CPU convolutions/GEMMs + the C port of
    the voxel ops and of the ICC loop (oracle/mf_oracle.c, OpenMP over grids).  Bounded
    sample: one scene's objects through predict and all ICC iterations of one scene on all
    cores; then 1 object + 10 ICC iterations on ONE thread (scaled) for ``value_1thread``."""
    from oracle import oracle_c as OC

    cores = min(os.cpu_count() or 1, 64)  # more threads only add oversubscription noise
    torch.backends.cudnn.benchmark = False
    model = Model(n_fg_class=21, with_occupancy=True).eval()
    model.load_state_dict({k: v.cpu() for k, v in wl.model.state_dict().items()})
    nb = min(wl.B, args.objects)  # one whole scene's objects
    inp = {k: v[:nb].cpu() for k, v in wl.inputs.items()}

    # route the two HIP ops of predict through the C port for this leg only

    def avg_cpu(values, points, batch_indices, *, batch_size, origin, pitch, dimensions,
                return_counts=False, **kw):
        m, c = OC.average_voxelization_3d(values.numpy(), points.numpy(), batch_indices.numpy(),
                                          batch_size=batch_size, origin=origin, pitch=pitch,
                                          dimensions=dimensions)
        if return_counts:
            return torch.from_numpy(m), torch.from_numpy(c)
        return torch.from_numpy(m)

    def interp_cpu(vox, points, batch_indices, channels_first=False, batch_start=None):
        out = torch.from_numpy(OC.interpolate_voxel_grid(vox.numpy(), points.numpy(), batch_indices.numpy()))
        return out.t().contiguous() if channels_first else out

    import morefusion_amd.contrib.singleview_3d.models.model as model_mod
    def select_cpu(self, pcd):
        from oracle import oracle_np as O
        order, counts = O.valid_pixel_order(pcd.numpy())
        return self._subsample(torch.from_numpy(order), counts)

    saved = (model_mod.functions_module.average_voxelization_3d,
             model_mod.functions_module.interpolate_voxel_grid, Model._select_points)
    model_mod.functions_module.average_voxelization_3d = avg_cpu
    model_mod.functions_module.interpolate_voxel_grid = interp_cpu
    Model._select_points = select_cpu
    sc = wl.scenes_np[0]
    q0 = wl.q0[: len(sc["points"])].cpu().numpy()
    t0_ = wl.t0[: len(sc["points"])].cpu().numpy()
    a = (sc["points"], sc["sdf"], sc["pitch"], sc["origin"], sc["grid_target"], sc["grid_nontarget_empty"])

    def timed(threads, iters, n_obj):
        torch.set_num_threads(threads)
        OC.set_threads(threads)
        sub = {k: v[:n_obj] for k, v in inp.items()}
        with torch.no_grad():
            if threads > 1:
                model.predict(**{k: v[:1] for k, v in inp.items()})  # warm-up
            t0 = time.perf_counter()
            model.predict(**sub)
            t_pred = (time.perf_counter() - t0) * (wl.B / n_obj)
        OC.set_threads(min(threads, 2 * len(sc["points"])))  # the port parallelises over the 2N grids
        OC.icc_refine(*a, q0, t0_, n_iter=1, sdf_offset=0.02)
        t0 = time.perf_counter()
        OC.icc_refine(*a, q0, t0_, n_iter=iters, sdf_offset=0.02)
        t_icc = (time.perf_counter() - t0) * (args.icc_iters / iters) * args.scenes_per_gpu
        return t_pred, t_icc

    iters = args.icc_iters
    try:
        t_pred, t_icc = timed(cores, iters, nb)
        t_pred1, t_icc1 = timed(1, min(10, iters), 1)
    finally:
        (model_mod.functions_module.average_voxelization_3d,
         model_mod.functions_module.interpolate_voxel_grid, Model._select_points) = saved
        torch.set_num_threads(cores)
        OC.set_threads(cores)
    value = wl.B / (t_pred + t_icc)
    return dict(value=round(value, 3), unit="objects/sec", cores=cores, kind="port",
                value_1thread=round(wl.B / (t_pred1 + t_icc1), 3),
                sample=f"predict on {nb} of {wl.B} object(s) (torch-CPU convs + C port of voxelize/"
                       f"interpolate) scaled x{wl.B / nb:g}; ICC C port (OpenMP) all {iters} "
                       f"iterations of 1 scene on min(cores, 2N) threads; predict {t_pred:.2f}s + icc {t_icc:.2f}s per step. "
                       f"value_1thread: 1 object + {min(10, iters)} ICC iterations on one thread, scaled "
                       f"({t_pred1:.2f}s + {t_icc1:.2f}s per step)")


def extra_scenes8(args, rank, device):
    """BASELINE configs[3]'s per-GPU share as a driver-run number: the same pipelined step with 8 scenes x 8 objects
    (64 objects: predict at B = 64 -> ICC of 8 scenes in one batch) on this one GPU.  Not the headline (`value` stays
    configs[1] + configs[2]); reported beside it."""
    import copy
    a8 = copy.copy(args)
    a8.scenes_per_gpu = 8
    wl8 = Workload(a8, rank, device)
    steps, warm = 6, 2
    el = parallel.timed_steps(wl8.step, steps, warm, device=device)
    return {"value": round(wl8.B * steps / el, 3), "unit": "objects/sec", "ms_per_step": round(el / steps * 1e3, 4),
            "objects_per_gpu": wl8.B, "steps": steps, "warmup": warm,
            "workload": "8 scenes x 8 objects on one GPU, full pipelined step (BASELINE configs[3] per-GPU share)"}


def extra_training(graph=False):
    """BASELINE configs[4]'s per-GPU share as a driver-run number: examples/singleview_3d_train.py (global batch 16,
    bf16 autocast, every 3-D / 1x1 convolution + voxel op hand-written, forward + backward + Adam) in a child
    process on this GPU; the steady mean of its per-step rates (first two steps excluded there)."""
    import subprocess
    import tempfile
    with tempfile.TemporaryDirectory() as td:
        rec = os.path.join(td, "train.json")
        cmd = [sys.executable, os.path.join(ROOT, "examples", "singleview_3d_train.py"), "--global-batch", "16",
               "--steps", "12" if graph else "10", "--json", rec] + (["--graph"] if graph else [])
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=240)
            d = json.load(open(rec))
        except Exception as e:  # the extras must never take the headline line down
            return {"error": repr(e)[:200]}
    return {"train_objects_per_s": d.get("objects_per_s_steady_mean"), "global_batch": d.get("global_batch"),
            "dtype": d.get("dtype"), "steps": d.get("steps"), "hipgraph_step": d.get("hipgraph_step"),
            "loss_first_last": [d["loss_per_step"][0], d["loss_per_step"][-1]] if d.get("loss_per_step") else None,
            "workload": "singleview_3d training step, global batch 16 on this GPU (BASELINE configs[4] per-GPU share)"}


def dry_run_cpu(args, world, rank):
    """N gloo ranks, stub step, the bench's own timing contract and JSON shape."""
    device = torch.device("cpu")
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("gloo", rank=rank, world_size=world)
    wl = StubWorkload(args, rank, device)
    last = {}

    def step():
        last["poses"], _ = wl.step()

    elapsed = parallel.timed_steps(step, args.steps, args.warmup, device=None)
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, last)
    ev = gather_evidence(wl, device)
    expect = torch.arange(world * wl.B, dtype=torch.float32) * 10.0
    ev["rank_order_ok"] = bool(torch.equal(wl.step()[0][:, 0].cpu(), expect))
    if rank == 0:
        print(json.dumps({
            "metric": "objects/sec (32^3 voxelize+3D-CNN+ICC refine)", "value": None, "unit": "objects/sec",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(elapsed / args.steps * 1e3, 4), "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": "f32",
            "data": "DRY RUN on CPU (gloo): launcher + pose all-gather only, no kernel ran, not a measurement",
            "config": {"workload": "stub step", "objects_per_gpu": wl.B,
                       "parallelism": f"scene-sharded x{world}, pose all_gather"},
            "collective": dict(ev, backend="gloo")}))
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


def full_extras(args, wl, world, rank, device, out, lap):
    """``--full``: the un-timed measurements beside the headline, added to rank 0's line ``out``: stage breakdown,
    live kernel timing, rooflines, accuracy, CPU baseline (rank 0, N=1), the 8-scene and training extras, the batch-1
    latency probe."""
    wl.events = []
    for _ in range(5):
        wl.step(timing=True)
    torch.cuda.synchronize()
    stages = {}
    ev = wl.events
    for (n0, e0), (n1, e1) in zip(ev[:-1], ev[1:]):
        if n1 != "start":
            stages[n1] = stages.get(n1, 0.0) + e0.elapsed_time(e1) / 5
    collective = gather_evidence(wl, device) if world > 1 else None  # every rank takes part
    torch.cuda.synchronize()
    if rank == 0:
        out["stage_ms"] = {k: round(v, 4) for k, v in stages.items()}
        out["serial_ms_per_step"] = round(sum(stages.values()), 4)
        # the same step with the two stages back to back on one stream (no pipelining credit)
        out["value_serial"] = round(world * wl.B / (sum(stages.values()) / 1e3), 3) if stages else None
        if collective is not None:
            out["collective"] = dict(collective, backend="nccl (RCCL)")
        t_vol, t_icc = handwritten_path(wl)
        out["value_handwritten_path"] = round(world * wl.B / ((t_vol + t_icc) / 1e3), 3)
        out["handwritten_path_ms"] = {"volumetric_network_part": round(t_vol, 4), "icc": round(t_icc, 4)}
        out["roofline_conv4"] = roofline_conv4(wl, wl.B)
        out["roofline_conv4_batch1"] = roofline_conv4(wl, 1)
        out["roofline"] = roofline_icc(wl, t_icc * 1e3 / args.icc_iters)  # all scenes share the launches
        out["roofline_voxelize"] = roofline_voxelize(wl)
        out["roofline_bf16_kernels"] = roofline_bf16_kernels(wl)
        lap("rooflines")
        out["accuracy"] = accuracy(wl)
        lap("accuracy")
        if world == 1 and not args.no_cpu_baseline:
            out["cpu_baseline"] = cpu_baseline(wl, args)
        torch.cuda.synchronize()
        lap("cpu_baseline")
        if world == 1 and not args.no_extras and args.scenes_per_gpu == 1:
            # configs[3] / configs[4] per-GPU shares inside the driver-run line (round-4 verdict item 7)
            try:  # (the extras must never take the headline line down)
                s8 = extra_scenes8(args, rank, device)
                out["value_scenes8"] = s8["value"]
                out["scenes8"] = s8
            except Exception as e:
                out["scenes8"] = {"error": repr(e)[:200]}
            lap("extra_scenes8")
            tr = extra_training()
            out["train_objects_per_s"] = tr.get("train_objects_per_s")
            out["training"] = tr
            lap("extra_training")
            if time.perf_counter() - T_START < 150.0:  # the same step replayed from hipGraphs (--graph), time permitting
                tg = extra_training(graph=True)
                out["train_objects_per_s_hipgraph"] = tg.get("train_objects_per_s")
                out["training_hipgraph"] = tg
            torch.cuda.synchronize()
        if not args.no_latency_probe:
            out["latency_batch1_ms"] = latency_batch1(wl)  # child process, last: nothing of this one depends on it
            lap("latency_probe")
        # (where the wall time goes: MIOpen's solver search runs its candidates on the GPU for every new shape --
        # ~12 s for the headline's B = 8, ~45 s for the 8-scene extra's B = 64, ~30 s for the training child)


T_START = time.perf_counter()
# the stock 2-D backbone's MIOpen solver choices for the bench's shapes, found once on an MI355X and shipped as a
# find-db (morefusion_amd/miopen_cache.py): without it the un-timed search costs ~100 s of wall per bench run
miopen_cache.enable()


def main():
    args = parse()
    if args.probe_latency_b1:
        return latency_probe_main()
    if args.gpus > 1 and not parallel.launched():
        # `python bench.py --gpus N` on its own: become N ranks of one node (the driver's
        # torch.distributed.run launch arrives here with WORLD_SIZE set and skips this)
        raise SystemExit(parallel.self_launch(args.gpus, os.path.abspath(__file__), sys.argv[1:]))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    assert world == args.gpus, f"--gpus {args.gpus} but WORLD_SIZE={world}"
    if args.dry_run_cpu:
        return dry_run_cpu(args, world, rank)
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X (torch.cuda.is_available() is False)")
    torch.cuda.set_device(local_rank)
    device = torch.device("cuda", local_rank)
    # MIOpen algorithm search for the stock convolutions (runs during warm-up)
    torch.backends.cudnn.benchmark = True
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=device)

    walls = {}
    t_sec = [time.perf_counter()]

    def lap(name):  # wall seconds of the bench's sections (reported as bench_wall_sections_s)
        now = time.perf_counter()
        walls[name] = round(now - t_sec[0], 1)
        t_sec[0] = now

    wl = Workload(args, rank, device)
    lap("setup")

    mark = os.environ.get("MF_BENCH_MARK")  # profiling aid: bracket the timed steps in the kernel trace
    if mark:  # (k_icc_scene_setup only runs in mf_icc_prepare: its 2nd / 3rd instance are the brackets)
        for _ in range(args.warmup):
            wl.step()
        torch.cuda.synchronize()
        wl.icc.prepare()
    last = {}

    def step():  # keeps what the step hands its caller, for --dump-outputs
        last["refined_poses"], last["network_poses"] = wl.step()

    elapsed = parallel.timed_steps(step, args.steps, 0 if mark else args.warmup, device=device)
    if mark:
        wl.icc.prepare()
        torch.cuda.synchronize()

    lap("warmup_and_timed_steps")
    out = None
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, dict(last, **wl.last_predict))
        lap("dump_outputs")
    if rank == 0:
        total_objects = world * wl.B * args.steps
        out = {
            "metric": "objects/sec (32^3 voxelize+3D-CNN+ICC refine)",
            "value": round(total_objects / elapsed, 3),
            "unit": "objects/sec",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(elapsed / args.steps * 1e3, 4),
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": args.dtype, "data": "synthetic",
            "config": {
                "workload": f"{args.scenes_per_gpu} scene(s) x {args.objects} objects per GPU: "
                            "singleview_3d Model.predict (ResNet18+PSPNet, 32^3 voxelize, occupancy "
                            f"3D-CNN, heads; B={wl.B}) -> ICC joint refine {args.icc_iters} iters "
                            "(BASELINE configs[1]+configs[2]); random weights, ICC starts from "
                            "synthetic perturbed-GT poses"
                            + ("" if args.no_overlap else "; ICC(k) on a second HIP stream, event-ordered "
                               "after network(k), beside network(k+1)"),
                "objects_per_gpu": wl.B, "icc_iters": args.icc_iters,
                "parallelism": f"scene-sharded x{world}, pose all_gather",
                "streams": "1 (serial)" if args.no_overlap else
                           "2 (pipelined: ICC(k) waits on network(k)'s event and overlaps network(k+1); "
                           "stage_ms are the serial stage times)",
                "stream_priority": args.priority, "icc_cu_mask": args.icc_cus or None, "backbone_memory_format":
                    "channels_last" if args.channels_last else "contiguous",
            },
        }
    if args.full:
        full_extras(args, wl, world, rank, device, out, lap)
    if rank == 0:
        out["bench_wall_sections_s"] = walls
        out["bench_wall_s"] = round(time.perf_counter() - T_START, 1)  # this process, after the imports
        print(json.dumps(out))
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
