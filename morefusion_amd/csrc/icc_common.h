// What every piece of the ICC code shares: the tuning-aid macro and its stamp table, constants, the kernel
// arguments (IccArgs, IccStepArgs), the per-grid kernel size and the voxel -> unit-residual helpers.
// A piece of csrc/icc.hip's single translation unit: included there, in the order of that file, nowhere else.
#pragma once
#include <math.h>

#include "mf_common.h"
#include "quat.h"

namespace {

// Tuning aids (per-phase time stamps, phase skipping: MF_ICC_DEBUG bit mask at run time) exist only in a
// build with -DMF_ICC_DEBUG_BUILD=1 (`make ICC_DEBUG=1`, tools/stamps_*.py); the production kernels carry
// none of their branches.
#ifndef MF_ICC_DEBUG_BUILD
#define MF_ICC_DEBUG_BUILD 0
#endif
#define MF_DBG(a_, bits_) (MF_ICC_DEBUG_BUILD != 0 && ((a_).dbg & (bits_)) != 0)
#if MF_ICC_DEBUG_BUILD
__device__ unsigned long long g_dbg_stamps[4096 * 8];  // (MF_ICC_DEBUG & 32)
#else
__device__ unsigned long long g_dbg_stamps[8];
#endif

constexpr int kAccThreads = 512;
constexpr int kVoxPerBlock = 1024;  // k_icc_accum: voxels per workgroup
constexpr int kNumOwn = 39;         // RN, S_in, PN + 3 x 12 gradient moments
constexpr uint32_t kNoCand = 0xffffffffu;
constexpr double kFixOth = 1099511627776.0;  // 2^40 fixed point: collision moments summed over blocks
constexpr double kFixOwn = 4294967296.0;     // 2^32: reward / penalty sums and own-gradient moments
constexpr int kNumF = 65;                    // single-pass path: 5 scene sums + 5 x 12 moments (below)
constexpr int kOwnSlots = kNumF + 1;         // accumulator words per object; the slot after the sums
                                             // counts non-finite block sums (-> NaN loss)
constexpr int kStateFloats = 21;             // q[4] t[3] m[7] v[7] of one object
// Objects per scene.  The single-pass path (k_icc_fused, {0,1} no-entry grids: what every caller of the reference
// passes) takes up to 128 (round 6): its LDS tables of a scene (R|t, offsets) are sized for that, and the collision
// moments -- 1664 bytes of LDS rows per other object and workgroup -- are reduced in chunks of kRows2Chunk objects (one
// chunk up to 64: the round-3 code path; > 64: the voxels' collision terms stay in registers and a second chunk reuses
// the rows).  The two-kernel path (k_icc_accum: any no-entry grid values) carries the objects a block meets as a
// 64-bit mask and stays at 64.  Scenes beyond 32 objects take > 64 KB of dynamic LDS (one workgroup per CU).
constexpr int kMaxSceneObjects = 128;
constexpr int kMaxSceneObjectsGeneral = 64;
constexpr int kRows2Chunk = 64;

struct IccArgs {
  const float4 *pts4;
  const int32_t *obj_off;
  const int32_t *scene_off;
  const int32_t *obj_scene;
  const float *pitch;
  const float *origin;
  const float *grid_target;
  const float *grid_ne;
  int O, S, D;
  float thr, sdf_offset;
  // workspace
  unsigned long long *W;  // [2*O][V]
  uint32_t *Mbits;        // [3 parities][2*O] per-grid max of the raw inside weight (float bits)
                          // (the two-launch path uses parities 0 and 1 of every three-parity array)
  int ne_binary;          // every grid_ne value is exactly 0 or 1 -> single-pass path (see k_icc_fused)
  float *Rt;              // [2][O][12]  R row-major, then t (the two-launch path uses copy 0)
  float *bound;           // [O][4]   model-frame bounding sphere
  float *St;              // [S]
  // reduced sums of one iteration, 64-bit fixed point, two parities (iteration k adds into
  // k & 1 while the step folded into k_icc_bin still reads (k - 1) & 1)
  long long *acc_own;     // [2][O][kOwnSlots]
  long long *acc_oth;     // [2][O][max_ns][12]  collision moments of grid o onto scene object e
  float *state_alt;       // [O][kStateFloats] second copy of (q, t, m, v): odd iterates
  int max_ns;
  int4 *meta;             // [O] {scene first object, scene end object, point begin, point end}
  // x-plane bins of the per-iteration point binning (k_icc_bin -> k_icc_tile)
  int4 *tab;              // [n_tab] {target object o, source object j, point begin, point end}; o < 0: unused
  int4 *tab2;             // [n_tab] {scene first object, objects in scene, scene, 1 = designated entry of j}
  int n_tab;
  int hmax;               // largest TDF half-kernel of the batch
  int nbins;              // COUNTER STRIDE of a grid: kHalves * (D + 2 hmax) real bins ((x-plane of the rounded x in
                          // [-hmax, D-1+hmax], y-half)) + 1: the last word counts the grid's OVERFLOW records
  uint32_t *bin_cnt;      // [2 parities][2*O][nbins] records in each bin: iteration k fills parity k & 1,
                          // the step side of k_icc_bin empties the other one for iteration k + 1
  // A (point, grid) pair lands in ONE plane (two bins when its rows straddle the halves), so a bin can
  // hold all P_g source points of its grid in the worst case -- but reserving that for every bin is
  // nbins x the records that can exist (3.3 GB for 32 objects x 3000 points).  A bin therefore gets
  // cap_g = max(kBinMinCap, P_g / kBinShare) slots; records beyond it go to the grid's overflow list
  // (2 P_g slots behind its bins), which EVERY tile of the grid scans with the bin-membership test
  // when its counter is non-zero.  Winners are exact minima with lowest-id ties and the sums are
  // fixed point: where a record is stored cannot change a bit of the result.
  int32_t *bin_cap;       // [2*O] capacity cap_g of each bin of grid g
  int32_t *bin_pts;       // [2*O] P_g = source points of grid g (overflow capacity = 2 P_g)
  int64_t *bin_base;      // [2*O] first record of grid g; bin b starts at base + b*cap_g, overflow at base + nreal*cap_g
  int bin_cap_force;      // > 0: every cap_g = this (MF_ICC_BIN_CAP: exercises the overflow path in tests)
  float4 *rec;            // records {fx, fy, fz, point id bits}: voxel-frame coordinates
  int dbg;                // tuning aid: MF_ICC_DEBUG bit mask (0 in production)
  int uniform_ns;         // > 0: every scene holds exactly this many objects (scene tables need no load)
  int xcd_order;          // k_icc_fused: XCD-contiguous logical workgroup order (see there)
};

using mf::quat_backward;
using mf::quat_to_R;

// Kernel size of one grid: truncated_distance_function.py:36-38 evaluates
// ceil(truncation / pitch) in float32 with truncation = threshold * pitch
// (:184), made odd.  For threshold 2 (the link's default) the quotient is exactly 2 -> 3;
// for other thresholds it depends on the rounding of the two float32 operations, i.e. on the
// grid's pitch -- so it is evaluated per grid, like the reference does.
__device__ __forceinline__ int ksize_of(float thr, float pitch) {
  int ks = (int)ceilf((thr * pitch) / pitch);
  if (ks % 2 == 0) ks += 1;
  return ks;
}

// ---- front end: per-iteration x-plane binning + bin-fed TDF tiles ----------------------
// Round 1 let every one of the 32 plane workgroups of a grid re-scan all source points of the
// scene (32x read amplification, a dependent global load per work item).  Now every (source
// point, target grid) pair is transformed ONCE (k_icc_bin), the survivors' voxel-frame
// coordinates are appended to the bin of their rounded x-plane, and the tile of plane x reads
// only bins x-h..x+h (k_icc_tile): records arrive as coalesced 16 B loads, both LDS passes run
// on registers + LDS only.  Coordinates are computed with the oracle's expressions and (min,
// arg-min) are exact -> the same winners (verified bit-identical against round 1 on the GPU).
constexpr int kBinThreads = 256;
constexpr int kBinPPT = 4;                          // points per thread (2: 23.0 vs 23.1 us/iteration, twice the redundant steps)
constexpr int kBinChunk = kBinThreads * kBinPPT;    // points per workgroup
constexpr int kHalves = 2;                          // y-halves of a plane: rows [0, D/2), [D/2, D)
constexpr int kMaxBins = kHalves * (64 + 8);        // D <= 64, ks <= 7, + one margin plane per side 
constexpr int kBinShare = 8;                        // a bin holds 1/8 of its grid's source points ...
constexpr int kBinMinCap = 64;                      // ... at least this many, the rest overflows

__host__ __device__ inline int bin_cap_of(int P, int force) {
  int c = force > 0 ? force : max(kBinMinCap, (P + kBinShare - 1) / kBinShare);
  return min(max(c, 1), max(P, 1));
}

struct IccStepArgs {
  int mode;        // 0: none (bin reads a.Rt), 1: Adam step + outputs, 2: gradients only (k_icc_step)
  int fused;       // the sums come from k_icc_fused (monomials in 1/M_own, 1/M_oth) instead of k_icc_accum
  int par;         // parity of the accumulators / per-grid maxima to read
  int cpar;        // parity of the bin counters this launch fills
  int it;          // iteration whose pose is produced (traj row; its loss goes to losses[it - 1])
  float aq, at;    // alpha_t of chainer's Adam for this step (evaluated in double on the host)
  const float *q_in, *t_in, *m_in, *v_in;  // state before the step
  float *q_out, *t_out, *m_out, *v_out;    // state after it (may alias the inputs)
  float *loss_out;                         // [S] or NULL
  float *gq_out, *gt_out;                  // mode 2
  float *traj;                             // [n_iter][O][7] or NULL
};

// ---- the per-scene loss observer of mf_icc_refine_converge (the LossObserver of the reference's ROS node,
// ros/.../collision_based_pose_refinement.py:18-45, next to the optimiser step) ----------------------------------
// One record per scene and parity copy, in a buffer of the caller's (mf_icc_observer_bytes).  The launch that
// computes step k reads the copy launch k - 1 wrote and writes the other one: workgroups of one launch are not
// ordered, so every one of them sees the same `frozen` flag and the same window, whoever runs first.
constexpr int kObsMaxWindow = 16;
struct IccObsRec {
  double delta[kObsMaxWindow];  // ring of the most recent |last - loss|: slots [0, fill), the oldest at `head` once full
  float last;                   // the loss of the previous step (valid when has_last)
  int32_t has_last, fill, head;
  int32_t n_passed;             // steps in a row whose whole window was finite and below the threshold
  int32_t frozen;               // converged: no object of the scene takes another step
  int32_t n_steps;              // optimiser steps applied to the scene so far
  int32_t pad_;
};
static_assert(sizeof(IccObsRec) == 8 * kObsMaxWindow + 32, "IccObsRec: mf_icc_observer_bytes counts these bytes");
struct IccObsArgs {
  IccObsRec *rec;      // [2 copies][S]
  int32_t *n_steps;    // [S]: written by the last step of the call
  double max_delta;    // a delta passes when it is finite and < this (compared in double)
  int window, n_pass;  // deltas kept (<= kObsMaxWindow); passes in a row that freeze a scene
  int in;              // the copy this launch reads; it writes copy in ^ 1
};
struct IccNoObs {};    // what the kernels without an observer are handed instead
template <bool OBS> struct IccObsOf { using type = IccNoObs; };
template <> struct IccObsOf<true> { using type = IccObsArgs; };

constexpr int kTileThreads = 512;
constexpr int kTileKeep = 4;  // records per lane kept in registers over both passes
constexpr int kTileR = 4;     // records in flight per lane beyond those
constexpr int kFusedKeepOwn = 2, kFusedKeepOth = 4;  // k_icc_fused: kept records per lane and grid
constexpr int kPad = 2;  // margin cells of its LDS tile on every side (ks = 3: candidates reach 2 cells out)
// LDS words of one (dist | id) array of the single-pass kernel's padded half-plane tile
__host__ __device__ constexpr int fused_tile_words(int D) { return ((D + 1) / 2 + 2 * kPad) * (D + 2 * kPad); }

__device__ __forceinline__ void world_frac(const float *Rt, const float4 m, float ox, float oy,
                                           float oz, float pitch, int ix, int iy, int iz,
                                           float &ux, float &uy, float &uz, bool &ok) {
  const float wx = ((Rt[0] * m.x + Rt[1] * m.y) + Rt[2] * m.z) + Rt[9];
  const float wy = ((Rt[3] * m.x + Rt[4] * m.y) + Rt[5] * m.z) + Rt[10];
  const float wz = ((Rt[6] * m.x + Rt[7] * m.y) + Rt[8] * m.z) + Rt[11];
  const float dx = (wx - ox) / pitch - (float)ix;
  const float dy = (wy - oy) / pitch - (float)iy;
  const float dz = (wz - oz) / pitch - (float)iz;
  const float n = sqrtf((dx * dx + dy * dy) + dz * dz);
  ok = n > 0.0f;  // truncated_distance_function.py:141
  ux = dx / n; uy = dy / n; uz = dz / n;
}

// the same with reciprocal multiplies (k_icc_fused's voxel phase; see there)
__device__ __forceinline__ void world_frac_r(const float *Rt, const float4 m, float ox, float oy,
                                             float oz, float inv_pitch, int ix, int iy, int iz,
                                             float &ux, float &uy, float &uz, bool &ok) {
  const float wx = ((Rt[0] * m.x + Rt[1] * m.y) + Rt[2] * m.z) + Rt[9];
  const float wy = ((Rt[3] * m.x + Rt[4] * m.y) + Rt[5] * m.z) + Rt[10];
  const float wz = ((Rt[6] * m.x + Rt[7] * m.y) + Rt[8] * m.z) + Rt[11];
  const float dx = (wx - ox) * inv_pitch - (float)ix;
  const float dy = (wy - oy) * inv_pitch - (float)iy;
  const float dz = (wz - oz) * inv_pitch - (float)iz;
  const float n2 = (dx * dx + dy * dy) + dz * dz;
  ok = n2 > 0.0f;  // truncated_distance_function.py:141
  const float rn = __frsqrt_rn(n2);
  ux = dx * rn; uy = dy * rn; uz = dz * rn;
}

}  // namespace
