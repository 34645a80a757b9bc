// Fused Iterative Collision Check (ICC) for gfx950: forward, backward and the
// chainer-Adam step of IterativeCollisionCheckLink, batched over independent scenes.
//
// Reference call graph (one iteration, N objects):
//   contrib/iterative_collision_check_link.py:31-99   transformation_matrix, N x
//   transform_points, 2N x pseudo_occupancy_voxelization (each: TDF kernel K7 with
//   global float atomics + ~15 elementwise launches), N x isnan().any() D2H syncs,
//   stack/maximum/sum; backward = 2N x K8 (truncated_distance_function.py:105-166)
//   + matmul/quaternion backward; optimizer.update().  ~300 launches and N host
//   syncs per iteration, x100 iterations
//   (examples/ycb_video/pose_refinement/check_iterative_collision_check_link.py:52-79).
//
// Here one iteration is TWO launches and the whole n_iter loop is one hipGraph:
//   k_icc_bin    one workgroup per (target grid, source object, chunk of 1024 points).  Inside
//                the loop it first applies the PREVIOUS iteration's optimiser step for its source
//                object (the reduced gradient is ~200 fixed-point words: every workgroup
//                recomputes the same bits, one designated workgroup per object stores them),
//                then transforms its points once and appends the survivors' voxel-frame
//                coordinates to the bin of their rounded x-plane.
//   k_icc_fused  grid (x-plane * y-half, O): the TDFs of the "own" and the "other" point set of object o
//                from bins x-h..x+h -- (min distance, arg-min id) live in LDS as two 32-bit words per
//                voxel, resolved with two passes of 32-bit LDS atomics (64-bit LDS atomics measured ~10x
//                slower) -- and, without leaving LDS, the per-voxel pseudo-occupancy weights, the sums of
//                reward / penalty and the pose-gradient moments as monomials in 1 / (per-grid maximum of
//                the inside weight), which the step applies once every tile of the grid is done
//                (icc_fused.h).  Scenes of 65 .. 128 objects: k_icc_fused_big, the same with the collision
//                rows of LDS re-used chunk by chunk.  Block sums are added as 64-bit fixed point with
//                global integer atomics: exact, order-independent.
//   k_icc_step   (once, after the last iteration; and for mf_icc_loss_grad) the same per-object
//                step as a kernel of its own: loss, chain rule to (q, t), chainer-Adam.
// The monomial form needs no-entry grids of exactly {0, 1} (what every caller of the reference passes) and one
// voxel of a half-plane per lane.  Any other batch falls back to THREE launches, k_icc_bin -> k_icc_tile (the
// winners of every grid to global memory, the per-grid maximum by integer atomicMax) -> k_icc_accum (weights,
// max() with the no-entry grid, sums and moments per coefficient {1/S_t, 1/S_in, PN/S_in^2}): icc_general.h.
// Every reduction has a fixed order or is an integer sum: bitwise reproducible run to run.
// No host synchronisation anywhere.
//
// This file: the launch plan (icc_plan: validity, path, kernel variant, grids, LDS sizes and the workspace layout
// of a batch -- pure host arithmetic over the descriptor and the MF_ICC_* knobs, answered to the outside by
// mf_icc_plan), one launch helper per kernel, the graph cache and the C entry points.  The kernels, in the order of
// the translation unit: icc_common.h (constants, arguments), icc_setup.h (once per batch / call), icc_step.h (the
// optimiser step's device functions), icc_bin.h, icc_general.h (k_icc_tile, k_icc_accum), icc_fused.h, icc_tail.h
// (k_icc_step and k_pack: behind the others, so that the library's device code keeps the order it always had).
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <mutex>
#include <type_traits>
#include <vector>

#include "mf_common.h"

#include "icc_common.h"
#include "icc_setup.h"
#include "icc_step.h"
#include "icc_bin.h"
#include "icc_general.h"
#include "icc_fused.h"
#include "icc_tail.h"

namespace {

// ---- knobs and plan: no device call, no HIP type ------------------------------------------------------------------
// The environment, read once per entry-point call (who honours what: DESIGN.md, "Knobs and plan of ICC").
// MF_ICC_GENERAL: non-zero number = the two-kernel path even for {0,1} no-entry grids (A/B measurements and tests; only
// the value 1 is in use -- bench.py's restatement takes any non-empty value for "set", so "0" or text would disagree);
// MF_ICC_BIN_CAP=<n>: every bin's capacity (tests of the overflow path).  -DMF_ICC_DEBUG_BUILD=1 builds only
// (`make ICC_DEBUG=1`): MF_ICC_DEBUG, the bit mask of the tuning aids (32: phase stamps; 128 / 256 / 512: skip a phase,
// WRONG results; 2048 / 4096: XCD-contiguous workgroup order forced on / off), and MF_ICC_LDS_PAD, bytes of unused
// dynamic LDS on top of the fused kernel's -- from ~48 KB on only ONE of its workgroups fits a CU (half the resident
// waves: the experiment of leaving wave slots to a network running beside it).
// MF_ICC_FUSED_FORM=auto|generic (default auto): generic = the kernels that carry every case (k_icc_fused /
// k_icc_fused_big) even where the batch is eligible for a specialised form -- the same bits, for A/B
// timing and the bitwise tests of the forms.
struct IccKnobs { int general, bin_cap, dbg, lds_pad, form_generic; };
IccKnobs read_icc_knobs() {
  auto num = [](const char *name) { const char *e = getenv(name); return e ? atoi(e) : 0; };
  const char *form = getenv("MF_ICC_FUSED_FORM");
  IccKnobs k = {num("MF_ICC_GENERAL") != 0, num("MF_ICC_BIN_CAP"), 0, 0, form && strcmp(form, "generic") == 0};
#if MF_ICC_DEBUG_BUILD
  k.dbg = num("MF_ICC_DEBUG");
  k.lds_pad = num("MF_ICC_LDS_PAD");
#endif
  return k;
}

inline int64_t align256(int64_t x) { return (x + 255) & ~(int64_t)255; }

struct WsLayout {  // byte offsets of the workspace arrays (IccArgs), records of `rec`, bytes in all
  int64_t W, M, Rt, bound, St, acc_own, acc_oth, state_alt, meta, tab, tab2, bin_cnt, bin_cap, bin_pts, bin_base,
      rec, rec_n, total;
};
struct IccLaunch { int gx, gy, threads, lds; };  // grid (gx, gy), workgroup size, bytes of dynamic LDS
enum { kTileAccum = 0, kFused = 1, kFusedBig = 2 };  // the kernel(s) behind k_icc_bin
// The form of the single-pass kernel a batch runs.  kFormGeneric: k_icc_fused / k_icc_fused_big as they always were.
// The others: k_icc_fused3<MAXNS> (icc_fused.h), which hard-codes kernel size 3 and therefore needs the PROOF that
// every grid's ksize_of(thr, pitch) is 3, whatever its pitch: the float32 quotient (thr * pitch) / pitch is within 2 ulp
// of thr, so ceil of it is 2 or 3 for every pitch exactly when both ends of thr * (1 -+ 1e-6) round up to 2 or 3
// (ksize_lo_host == ksize_host == 3).  thr = 1 and its neighbours (ksize_of = 1 for some or all grids) and thr just
// above 3 stay on the kernels that read the size per grid.
//   every ks == 3 proved   largest scene   form
//   no                     any             kFormGeneric
//   yes                    <= 16           kForm3Ns16     k_icc_fused3<16>
//   yes                    17 .. 64        kForm3Ns64     k_icc_fused3<64>
//   yes                    65 .. 128       kFormGeneric   (k_icc_fused_big)
// and kFormGeneric for the two-kernel path and under MF_ICC_FUSED_FORM=generic.
enum { kFormGeneric = 0, kForm3Ns16 = 1, kForm3Ns64 = 2 };

// Everything the host decides about a batch.  Integers only and no padding (asserted below): its bytes are part of
// mf_icc_refine's graph key, so whatever can change a captured launch is in the key by construction.
struct IccPlan {
  int ok;           // the descriptor is valid; nothing else is defined otherwise
  int single_pass;  // {0,1} no-entry grids on a tile that fits the workgroup, and no MF_ICC_GENERAL
  int variant;      // kTileAccum / kFused / kFusedBig
  int launches;     // per iteration: 2 or 3
  int fused_form;   // kFormGeneric / kForm3*: which single-pass kernel (table above)
  int pad_;         // (0: the plan is hashed by its bytes, in 64-bit words)
  IccLaunch bin, tile, accum, fused, step;  // (tile: also what mf_icc_launch_stage(1) times on a single-pass batch;
                                            // fused: zeros on the two-kernel path)
  int hmax, nbins, n_tab, NB, uniform_ns, xcd_order, bin_cap_force, dbg;  // IccArgs; NB = k_icc_accum's blocks per object
  WsLayout ws;
};
static_assert(std::has_unique_object_representations<IccPlan>::value, "IccPlan is hashed by its bytes");

int ksize_host(float thr) {
  // Upper bound of the per-grid kernel size ksize_of(thr, pitch): the float32 quotient
  // (thr * pitch) / pitch is within 2 ulp of thr (exactly thr for thr = 2, the link's default).
  int ks = (int)ceilf(thr * 1.000001f);
  if (ks % 2 == 0) ks += 1;
  return ks;
}

int ksize_lo_host(float thr) {
  // Lower bound of the same: ceil of the smallest value the float32 quotient can take (thr less 2 ulp), made odd.
  int ks = (int)ceilf(thr * 0.999999f);
  if (ks % 2 == 0) ks += 1;
  return ks;
}

WsLayout ws_layout(const mfIccBatch *b, int nbins, int n_tab, int force) {
  WsLayout l;
  const int O = b->n_objects, S = b->n_scenes, D = b->dim, max_ns = b->max_scene_objects;
  const int64_t V = (int64_t)D * D * D;
  int64_t off = 0;
  l.W = off; off = align256(off + 2 * O * V * 8);
  l.M = off; off = align256(off + kParities * 2 * O * 4);
  l.Rt = off; off = align256(off + 2 * O * 12 * 4);
  l.bound = off; off = align256(off + O * 4 * 4);
  l.St = off; off = align256(off + S * 4);
  l.acc_own = off; off = align256(off + (int64_t)kParities * O * kOwnSlots * 8);
  l.acc_oth = off; off = align256(off + (int64_t)kParities * O * max_ns * 12 * 8);
  l.state_alt = off; off = align256(off + (int64_t)O * kStateFloats * 4);
  l.meta = off; off = align256(off + (int64_t)O * 16);
  l.tab = off; off = align256(off + (int64_t)n_tab * 16);
  l.tab2 = off; off = align256(off + (int64_t)n_tab * 16);
  l.bin_cnt = off; off = align256(off + (int64_t)kParities * 2 * O * nbins * 4);
  l.bin_cap = off; off = align256(off + (int64_t)2 * O * 4);
  l.bin_pts = off; off = align256(off + (int64_t)2 * O * 4);
  l.bin_base = off; off = align256(off + (int64_t)2 * O * 8);
  // records: per grid (nbins - 1) bins of cap_g <= P_g / kBinShare + kBinMinCap + 1 slots + an overflow list of
  // 2 P_g; sum_g P_g = sum over scenes of Ns * P_scene <= max_ns * n_points  ->  O(N * sum P), not nbins x that
  const int64_t sumP = (int64_t)max_ns * b->n_points;
  const int64_t per_grid_extra = (force > 0 ? force : kBinMinCap) + 1;
  const int64_t binned = force > 0 ? 0 : sumP / kBinShare;
  l.rec_n = (int64_t)(nbins - 1) * (binned + 2 * O * per_grid_extra) + 2 * sumP;
  l.rec = off; off = align256(off + l.rec_n * 16);
  l.total = off;
  return l;
}

IccPlan icc_plan(const mfIccBatch *b, const IccKnobs &k) {
  IccPlan p;
  memset(&p, 0, sizeof(p));
  if (!b) return p;
  const int O = b->n_objects, D = b->dim, max_ns = b->max_scene_objects;
  // {0,1} no-entry grids on a tile that fits the workgroup (one voxel of a half-plane per lane) take the single-pass
  // kernel, unless MF_ICC_GENERAL asks for the two-kernel path
  p.single_pass = b->grid_ne_binary != 0 && ((D + 1) / 2) * D <= kTileThreads && !k.general;
  p.ok = O > 0 && b->n_scenes > 0 && D > 0 && D <= 64 && b->n_points >= 0 && max_ns > 0 &&
         max_ns <= (p.single_pass ? kMaxSceneObjects : kMaxSceneObjectsGeneral) && b->voxel_threshold > 0.0f &&
         ksize_host(b->voxel_threshold) <= 7 && (double)b->n_points * 343.0 < 4294967295.0 &&
         b->n_points < (1 << 27) && b->flags == 0;
  if (!p.ok) return p;
  p.variant = !p.single_pass ? kTileAccum : max_ns > kRows2Chunk ? kFusedBig : kFused;
  p.launches = p.single_pass ? 2 : 3;
  p.hmax = ksize_host(b->voxel_threshold) / 2;
  p.nbins = kHalves * (D + 2 * p.hmax) + 1;  // + the overflow counter
  // every (target, source) pair of a scene in chunks of kBinChunk points:
  // sum_pairs ceil(P_j / chunk) <= max_ns * n_points / chunk + O * max_ns (+ O designated entries)
  p.n_tab = (int)(((int64_t)max_ns * b->n_points + kBinChunk - 1) / kBinChunk) + O * max_ns + O;
  p.n_tab = (p.n_tab + 7) & ~7;  // (a multiple of 8: the XCD-contiguous order of k_icc_bin)
  p.NB = (int)(((int64_t)D * D * D + kVoxPerBlock - 1) / kVoxPerBlock);
  p.uniform_ns = (int64_t)b->n_scenes * max_ns == O ? max_ns : 0;
  p.dbg = k.dbg;
  p.xcd_order = ((O >= 32) || (k.dbg & 2048)) && !(k.dbg & 4096);
  p.bin_cap_force = k.bin_cap;
  if (p.single_pass && !k.form_generic && p.variant == kFused && ksize_host(b->voxel_threshold) == 3 &&
      ksize_lo_host(b->voxel_threshold) == 3)
    p.fused_form = max_ns > 16 ? kForm3Ns64 : kForm3Ns16;
  // the collision rows: 53 KB at 32, 106 KB at 64 objects; beyond that the single-pass kernel re-uses them chunk by chunk
  const int lds_rows2 = std::min(max_ns, kRows2Chunk) * (kAccThreads / 16) * 13 * (int)sizeof(float);
  p.bin = {p.n_tab, 1, kBinThreads, 0};
  p.tile = {D * kHalves, 2 * O, kTileThreads, ((D + 1) / 2) * D * 2 * (int)sizeof(uint32_t)};  // 4 KB at D = 32
  p.accum = {p.NB, O, kAccThreads, lds_rows2};
  if (p.single_pass)
    p.fused = {D * kHalves, O, kTileThreads, 4 * fused_tile_words(D) * (int)sizeof(uint32_t) + lds_rows2 + k.lds_pad};
  p.step = {O, 1, 64, 0};
  p.ws = ws_layout(b, p.nbins, p.n_tab, k.bin_cap);
  return p;
}

// plan + base pointer -> kernel arguments
IccArgs make_args(const mfIccBatch *b, const IccPlan &pl, void *ws) {
  IccArgs a;
  a.pts4 = (const float4 *)b->pts4;
  a.obj_off = b->obj_off;
  a.scene_off = b->scene_off;
  a.obj_scene = b->obj_scene;
  a.pitch = b->pitch;
  a.origin = b->origin;
  a.grid_target = b->grid_target;
  a.grid_ne = b->grid_ne;
  a.O = b->n_objects;
  a.S = b->n_scenes;
  a.D = b->dim;
  a.thr = b->voxel_threshold;
  a.sdf_offset = b->sdf_offset;
  a.max_ns = b->max_scene_objects;
  a.ne_binary = pl.single_pass;
  a.dbg = pl.dbg;
  const WsLayout &l = pl.ws;
  char *p = (char *)ws;
  a.W = (unsigned long long *)(p + l.W);
  a.Mbits = (uint32_t *)(p + l.M);
  a.Rt = (float *)(p + l.Rt);
  a.bound = (float *)(p + l.bound);
  a.St = (float *)(p + l.St);
  a.acc_own = (long long *)(p + l.acc_own);
  a.acc_oth = (long long *)(p + l.acc_oth);
  a.state_alt = (float *)(p + l.state_alt);
  a.meta = (int4 *)(p + l.meta);
  a.tab = (int4 *)(p + l.tab);
  a.tab2 = (int4 *)(p + l.tab2);
  a.n_tab = pl.n_tab;
  a.nbins = pl.nbins;
  a.hmax = pl.hmax;
  a.bin_cnt = (uint32_t *)(p + l.bin_cnt);
  a.bin_cap = (int32_t *)(p + l.bin_cap);
  a.bin_pts = (int32_t *)(p + l.bin_pts);
  a.bin_cap_force = pl.bin_cap_force;
  a.bin_base = (int64_t *)(p + l.bin_base);
  a.rec = (float4 *)(p + l.rec);
  a.uniform_ns = pl.uniform_ns;
  a.xcd_order = pl.xcd_order;
  return a;
}

// ---- one launch helper per kernel of an iteration: a stage (mf_icc_launch_stage) and an iteration make the same launch
constexpr int kBigLds = 124 * 1024;  // dynamic LDS every entry point allows the kernels with collision rows (icc_enter)
#define ICC_LAUNCH(kernel_, l_, stream_, ...) \
  hipLaunchKernelGGL(kernel_, dim3((l_).gx, (l_).gy), dim3((l_).threads), (size_t)(l_).lds, stream_, __VA_ARGS__)

// (ob: the loss observer of mf_icc_refine_converge, which rides on the steps; NULL everywhere else)
void launch_bin(const IccPlan &p, const IccArgs &a, const IccStepArgs &sp, hipStream_t stream,
                const IccObsArgs *ob = nullptr) {
  if (ob && sp.mode == 1) {
    const IccObsArgs o = *ob;  // (a copy of this launch's own)
    ICC_LAUNCH(k_icc_bin<true>, p.bin, stream, a, sp, o);
  } else {
    ICC_LAUNCH(k_icc_bin<false>, p.bin, stream, a, sp, IccNoObs{});
  }
}
void launch_tile(const IccPlan &p, const IccArgs &a, int par, hipStream_t stream) {
  ICC_LAUNCH(k_icc_tile, p.tile, stream, a, par);
}
void launch_accum(const IccPlan &p, const IccArgs &a, int par, hipStream_t stream) {
  ICC_LAUNCH(k_icc_accum, p.accum, stream, a, par);
}
void (*fused_kernel(const IccPlan &p))(IccArgs, int) {
  switch (p.fused_form) {
    case kForm3Ns16: return k_icc_fused3<16>;
    case kForm3Ns64: return k_icc_fused3<kRows2Chunk>;
    default: return p.variant == kFusedBig ? k_icc_fused_big : k_icc_fused;
  }
}
void launch_fused(const IccPlan &p, const IccArgs &a, int par, hipStream_t stream) {
  auto *kernel = fused_kernel(p);
  if (MF_ICC_DEBUG_BUILD && p.fused.lds > kBigLds) mf::allow_big_lds((const void *)kernel, p.fused.lds);  // (MF_ICC_LDS_PAD)
  ICC_LAUNCH(kernel, p.fused, stream, a, par);
}
void launch_step(const IccPlan &p, const IccArgs &a, const IccStepArgs &sp, hipStream_t stream,
                 const IccObsArgs *ob = nullptr) {
  if (ob) {
    const IccObsArgs o = *ob;
    ICC_LAUNCH(k_icc_step<true>, p.step, stream, a, sp, o);
  } else {
    ICC_LAUNCH(k_icc_step<false>, p.step, stream, a, sp, IccNoObs{});
  }
}

// One iteration k (counters / accumulators / maxima of parity k & 1): bin (+ the previous
// iteration's step when sp.mode == 1), then either the single-pass kernel or tile -> accum.
void launch_iteration(const IccPlan &p, const IccArgs &a, IccStepArgs sp, int k, hipStream_t stream,
                      const IccObsArgs *ob = nullptr) {
  const int par = k & 1;
  sp.cpar = par;
  sp.fused = p.single_pass;
  launch_bin(p, a, sp, stream, ob);
  if (p.single_pass) {
    launch_fused(p, a, par, stream);
  } else {
    launch_tile(p, a, par, stream);
    launch_accum(p, a, par, stream);
  }
}

// chainer Adam: alpha_t = alpha * sqrt(1 - b2^t) / (1 - b1^t), in double, cast once
float adam_alpha_t(float alpha, int step) {
  const double fix1 = 1.0 - pow(0.9, (double)step), fix2 = 1.0 - pow(0.999, (double)step);
  return (float)((double)alpha * sqrt(fix2) / fix1);
}

struct GraphKey {
  std::vector<uint64_t> v;
  bool operator<(const GraphKey &o) const { return v < o.v; }
};
std::map<GraphKey, hipGraphExec_t> g_graphs;
std::mutex g_graph_mu;

// the observer of one mf_icc_refine_converge call, as the caller gave it
struct IccObsCall {
  void *rec;
  int32_t *n_steps;
  double max_delta;
  int window, n_pass;
};

}  // namespace

// Start of every launching entry point: the kernels' LDS limits, then the plan of this call (the only one).
static int icc_enter(const mfIccBatch *b, IccPlan &p) {
  // collision-moment rows: max_scene_objects x 1664 B of dynamic LDS (106 KB at 64 objects)
  if (int e = mf::allow_big_lds((const void *)k_icc_fused, kBigLds)) return e;
  if (int e = mf::allow_big_lds((const void *)k_icc_fused_big, kBigLds)) return e;
  if (int e = mf::allow_big_lds((const void *)k_icc_fused3<16>, kBigLds)) return e;
  if (int e = mf::allow_big_lds((const void *)k_icc_fused3<kRows2Chunk>, kBigLds)) return e;
  if (int e = mf::allow_big_lds((const void *)k_icc_accum, kBigLds)) return e;
  p = icc_plan(b, read_icc_knobs());
  if (!p.ok) {
    mf::set_last_error(hipErrorInvalidValue, "mf_icc: invalid batch descriptor");
    return -(int)hipErrorInvalidValue;
  }
  return 0;
}

extern "C" int64_t mf_icc_workspace_bytes(const mfIccBatch *batch) {
  const IccPlan p = icc_plan(batch, read_icc_knobs());
  return p.ok ? p.ws.total : -1;
}

extern "C" int mf_icc_iteration_launches(const mfIccBatch *batch) {
  const IccPlan p = icc_plan(batch, read_icc_knobs());
  return p.ok ? p.launches : -1;
}

extern "C" int mf_icc_plan(const mfIccBatch *batch, int64_t *out, int32_t n) {
  const IccPlan p = icc_plan(batch, read_icc_knobs());
  if (!p.ok || !out || n <= 0) return -1;
  const int64_t slots[] = {p.single_pass, p.launches, p.variant, p.ws.total, p.n_tab,      p.nbins,         p.hmax,       p.fused.lds,
                           p.tile.lds,    p.accum.lds, p.NB,     p.xcd_order, p.bin_cap_force, p.uniform_ns, p.ws.rec_n};
  const int defined = (int)(sizeof(slots) / sizeof(slots[0]));
  for (int i = 0; i < std::min((int)n, defined); ++i) out[i] = slots[i];
  return defined;
}

// Tuning aid and test hook, not part of the interface of include/mfhip.h: the form of the single-pass kernel this
// batch will run (0 generic, 1 k_icc_fused3<16>, 2 k_icc_fused3<64>; negative: invalid descriptor).  Host arithmetic.
extern "C" int mf_icc_debug_form(const mfIccBatch *batch) {
  const IccPlan p = icc_plan(batch, read_icc_knobs());
  return p.ok ? p.fused_form : -1;
}

extern "C" int mf_pack_points_sdf(const float *points, const float *sdf, int64_t n, void *pts4,
                                  mfStream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (n == 0) return 0;
  hipLaunchKernelGGL(k_pack, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, points, sdf,
                     n, (float4 *)pts4);
  return mf::check_launch("mf_pack_points_sdf");
}

extern "C" int mf_icc_debug_stamps(unsigned long long *host_out, int n) {
  if (!MF_ICC_DEBUG_BUILD) {
    mf::set_last_error(hipErrorInvalidValue, "mf_icc_debug_stamps: build with `make ICC_DEBUG=1`");
    return -(int)hipErrorInvalidValue;
  }
  return -(int)hipMemcpyFromSymbol(host_out, HIP_SYMBOL(g_dbg_stamps), sizeof(unsigned long long) * n);
}

extern "C" int mf_icc_launch_stage(const mfIccBatch *batch, const float *q, const float *t, void *ws,
                                   int32_t stage, mfStream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  IccPlan p;
  if (int e = icc_enter(batch, p)) return e;
  const IccArgs a = make_args(batch, p, ws);
  if (stage == 0) {
    if (q && t) hipLaunchKernelGGL(k_icc_pose, dim3(a.O), dim3(256), 0, stream, a, q, t, (float *)nullptr);
    // inside an iteration k_icc_accum empties the bins; this hook has no accum launch
    if (int e_ = mf::fill_bytes(a.bin_cnt, 0, sizeof(uint32_t) * 2 * a.O * a.nbins, stream)) return e_;
    launch_bin(p, a, IccStepArgs{}, stream);
  } else if (stage == 1) {
    launch_tile(p, a, 0, stream);
  } else if (stage == 2) {
    if (!p.single_pass) {
      mf::set_last_error(hipErrorInvalidValue, "mf_icc_launch_stage: stage 2 needs {0,1} no-entry grids");
      return -(int)hipErrorInvalidValue;
    }
    launch_fused(p, a, 0, stream);
  } else {
    mf::set_last_error(hipErrorInvalidValue, "mf_icc_launch_stage: stage must be 0, 1 or 2");
    return -(int)hipErrorInvalidValue;
  }
  return mf::check_launch("mf_icc_launch_stage");
}

extern "C" int mf_icc_prepare(const mfIccBatch *batch, void *ws, mfStream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  IccPlan p;
  if (int e = icc_enter(batch, p)) return e;
  const IccArgs a = make_args(batch, p, ws);
  hipLaunchKernelGGL(k_icc_bound, dim3(a.O), dim3(256), 0, stream, a);
  hipLaunchKernelGGL(k_icc_scene_setup, dim3(a.S), dim3(256), 0, stream, a, 0);
  hipLaunchKernelGGL(k_icc_tables, dim3(1), dim3(256), 0, stream, a);
  return mf::check_launch("mf_icc_prepare");
}

extern "C" int mf_icc_loss_grad(const mfIccBatch *batch, const float *q, const float *t,
                                float *loss, float *gq, float *gt, void *ws,
                                mfStream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  IccPlan p;
  if (int e = icc_enter(batch, p)) return e;
  const IccArgs a = make_args(batch, p, ws);
  hipLaunchKernelGGL(k_icc_pose, dim3(a.O), dim3(256), 0, stream, a, q, t, (float *)nullptr);
  launch_iteration(p, a, IccStepArgs{}, 0, stream);
  IccStepArgs sp = {};
  sp.mode = 2;
  sp.fused = p.single_pass;
  sp.par = 0;
  sp.q_in = q;
  sp.t_in = t;
  sp.loss_out = loss;
  sp.gq_out = gq;
  sp.gt_out = gt;
  launch_step(p, a, sp, stream);
  return mf::check_launch("mf_icc_loss_grad");
}

// The loop of mf_icc_refine (oc == NULL) and of mf_icc_refine_converge: one cached hipGraph, replayed on `stream`.
static int icc_refine_graph(const mfIccBatch *batch, const IccPlan &p, float *q, float *t, float *adam_m, float *adam_v,
                            int32_t n_iter, int32_t step0, float alpha_q, float alpha_t, float *losses, float *traj,
                            const IccObsCall *oc, void *ws, hipStream_t stream) {
  const IccArgs a = make_args(batch, p, ws);

  // the key: what the kernels are handed from the caller (pointers, scalars of the descriptor and of this call, the
  // device), then the plan itself, byte for byte
  GraphKey key;
  auto push = [&](const void *ptr) { key.v.push_back((uint64_t)(uintptr_t)ptr); };
  push(batch->pts4); push(batch->obj_off); push(batch->scene_off); push(batch->obj_scene);
  push(batch->pitch); push(batch->origin); push(batch->grid_target); push(batch->grid_ne);
  push(q); push(t); push(adam_m); push(adam_v); push(losses); push(traj); push(ws);
  uint32_t fb[4];
  memcpy(&fb[0], &alpha_q, 4); memcpy(&fb[1], &alpha_t, 4);
  memcpy(&fb[2], &a.thr, 4); memcpy(&fb[3], &a.sdf_offset, 4);
  key.v.push_back(((uint64_t)fb[0] << 32) | fb[1]);
  key.v.push_back(((uint64_t)fb[2] << 32) | fb[3]);
  key.v.push_back(((uint64_t)(uint32_t)a.O << 32) | (uint32_t)a.S);
  key.v.push_back(((uint64_t)(uint32_t)a.D << 32) | (uint32_t)batch->n_points);
  key.v.push_back(((uint64_t)(uint32_t)n_iter << 32) | (uint32_t)step0);
  int dev = 0;
  MF_TRY(hipGetDevice(&dev));
  key.v.push_back(((uint64_t)(uint32_t)dev << 32) | (uint32_t)a.max_ns);
  if (oc) {  // (a key of another length than the fixed loop's: the two never meet)
    push(oc->rec); push(oc->n_steps);
    uint64_t thr_bits;
    memcpy(&thr_bits, &oc->max_delta, 8);
    key.v.push_back(thr_bits);
    key.v.push_back(((uint64_t)(uint32_t)oc->window << 32) | (uint32_t)oc->n_pass);
  }
  static_assert(sizeof(IccPlan) % sizeof(uint64_t) == 0, "IccPlan is hashed in 64-bit words");
  key.v.resize(key.v.size() + sizeof(IccPlan) / sizeof(uint64_t));
  memcpy(&key.v[key.v.size() - sizeof(IccPlan) / sizeof(uint64_t)], &p, sizeof(IccPlan));

  std::lock_guard<std::mutex> lock(g_graph_mu);
  auto itg = g_graphs.find(key);
  if (itg == g_graphs.end()) {
    hipGraph_t graph = nullptr;
    // The caller's stream may be the legacy NULL stream (torch's default), which cannot be
    // captured: record the graph on a private stream, replay it on the caller's.
    static std::map<int, hipStream_t> caps;  // one capture stream per device (under g_graph_mu)
    hipStream_t &cap = caps[dev];
    if (!cap) MF_TRY(hipStreamCreateWithFlags(&cap, hipStreamNonBlocking));
    MF_TRY(hipStreamBeginCapture(cap, hipStreamCaptureModeThreadLocal));
    // State after i steps lives in the caller's arrays for even i and in the workspace copy for
    // odd i: the step folded into k_icc_bin reads one while its designated workgroups write the
    // other.  Iteration k: [bin: step k-1 (k > 0), binning] -> fused (or tile -> accum); then one last step.
    float *alt = a.state_alt;
    float *sq[2] = {q, alt}, *st[2] = {t, alt + 4 * a.O}, *sm[2] = {adam_m, alt + 7 * a.O},
          *sv[2] = {adam_v, alt + 14 * a.O};
    IccObsArgs ob = {};
    if (oc) {  // fresh observers first: a replay starts where the first launch did
      ob.rec = (IccObsRec *)oc->rec;
      ob.n_steps = oc->n_steps;
      ob.max_delta = oc->max_delta;
      ob.window = oc->window;
      ob.n_pass = oc->n_pass;
      hipLaunchKernelGGL(k_icc_obs_reset, dim3((2 * a.S + 63) / 64), dim3(64), 0, cap, ob.rec, 2 * a.S);
    }
    hipLaunchKernelGGL(k_icc_pose, dim3(a.O), dim3(256), 0, cap, a, (const float *)q,
                       (const float *)t, traj);
    for (int k = 0; k <= n_iter; ++k) {
      IccStepArgs sp = {};
      ob.in = (k - 1) & 1;  // step k reads the records step k - 1 wrote (step 1: the fresh ones of copy 0)
      if (k > 0) {
        const int in = (k - 1) & 1, out = k == n_iter ? 0 : (k & 1);
        sp.mode = 1;
        sp.par = (k - 1) & 1;
        sp.it = k;
        sp.aq = adam_alpha_t(alpha_q, step0 + k);
        sp.at = adam_alpha_t(alpha_t, step0 + k);
        sp.q_in = sq[in]; sp.t_in = st[in]; sp.m_in = sm[in]; sp.v_in = sv[in];
        sp.q_out = sq[out]; sp.t_out = st[out]; sp.m_out = sm[out]; sp.v_out = sv[out];
        sp.loss_out = losses ? losses + (int64_t)(k - 1) * a.S : nullptr;
        sp.traj = k < n_iter ? traj : nullptr;
      }
      if (k == n_iter) {  // the step of the last iteration, as a kernel of its own
        sp.fused = p.single_pass;
        launch_step(p, a, sp, cap, oc ? &ob : nullptr);
        break;
      }
      launch_iteration(p, a, sp, k, cap, oc ? &ob : nullptr);
    }
    hipError_t ce = hipStreamEndCapture(cap, &graph);
    if (ce != hipSuccess) {
      mf::set_last_error(ce, "hipStreamEndCapture(icc)");
      return -(int)ce;
    }
    hipGraphExec_t exec = nullptr;
    hipError_t ie = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
    (void)hipGraphDestroy(graph);
    if (ie != hipSuccess) {
      mf::set_last_error(ie, "hipGraphInstantiate(icc)");
      return -(int)ie;
    }
    if (g_graphs.size() >= 64) {  // bounded cache
      for (auto &kv : g_graphs) (void)hipGraphExecDestroy(kv.second);
      g_graphs.clear();
    }
    itg = g_graphs.emplace(key, exec).first;
  }
  MF_TRY(hipGraphLaunch(itg->second, stream));
  return 0;
}

extern "C" int mf_icc_refine(const mfIccBatch *batch, float *q, float *t, float *adam_m,
                             float *adam_v, int32_t n_iter, int32_t step0, float alpha_q,
                             float alpha_t, float *losses, float *traj, void *ws,
                             mfStream_t stream_) {
  IccPlan p;
  if (int e = icc_enter(batch, p)) return e;
  if (n_iter <= 0) return 0;
  return icc_refine_graph(batch, p, q, t, adam_m, adam_v, n_iter, step0, alpha_q, alpha_t, losses, traj, nullptr, ws,
                          (hipStream_t)stream_);
}

extern "C" int64_t mf_icc_observer_bytes(int32_t n_scenes, int32_t window) {
  if (n_scenes <= 0 || window < 1 || window > kObsMaxWindow) return -1;
  return (int64_t)2 * n_scenes * (int64_t)sizeof(IccObsRec);
}

extern "C" int mf_icc_refine_converge(const mfIccBatch *batch, float *q, float *t, float *adam_m, float *adam_v,
                                      int32_t max_iter, int32_t step0, float alpha_q, float alpha_t,
                                      double max_delta_threshold, int32_t window, int32_t n_passed_threshold,
                                      float *losses, float *traj, int32_t *n_steps, void *observer, void *ws,
                                      mfStream_t stream_) {
  IccPlan p;
  if (int e = icc_enter(batch, p)) return e;
  if (max_iter < 1 || window < 1 || window > kObsMaxWindow || !observer || !n_steps || ((uintptr_t)observer & 7)) {
    mf::set_last_error(hipErrorInvalidValue,
                       "mf_icc_refine_converge: needs max_iter >= 1, 1 <= window <= 16, n_steps and an 8-byte aligned "
                       "observer buffer of mf_icc_observer_bytes()");
    return -(int)hipErrorInvalidValue;
  }
  const IccObsCall oc = {observer, n_steps, max_delta_threshold, window, n_passed_threshold};
  return icc_refine_graph(batch, p, q, t, adam_m, adam_v, max_iter, step0, alpha_q, alpha_t, losses, traj, &oc, ws,
                          (hipStream_t)stream_);
}
