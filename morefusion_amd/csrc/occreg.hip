// OccupancyRegistration for a batch of objects (contrib/occupancy_registration.py) -- gfx950.
//
// Reference: morefusion/contrib/occupancy_registration.py:10-139: per iteration transformation_matrix ->
// transform_points -> occupancy_grid_3d (three dense [X, Y, Z, P] tensors) -> penalty - reward -> backward -> Adam,
// one object at a time, the pose read back after every step.  Here one workgroup (256 lanes) owns one object and
// runs every iteration of it inside one launch; DESIGN.md "Occupancy registration" has the contract and
// tests/occreg_ref.py the NumPy mirror this file is pinned to bit for bit.
//
// Per iteration, for the object's pose (q, t):
//   reset    dmin[v] := +inf for every voxel (one sweep over the object's dmin array).
//   scatter  lane k takes points k, k + 256, ...: pf = ((R0 x + R1 y) + R2 z + t - origin) / pitch, then every voxel
//            (i, j, k) of the point's window [floor(pf - thr), ceil(pf + thr)] (clamped to the grid) gets
//            d = sqrtf((a a + b b) + c c), a = i - pf.x ..., and, where d < thr, an unsigned atomicMin of d's bits
//            (d >= 0: integer order is float order; the minimum does not depend on the order).  A voxel outside every
//            window has d >= thr for every point, i.e. m = 0 in the dense formulation too: the pruning is exact.
//   sums     m = min(max(thr - dmin, 0), 1); lane k adds voxels k, k + 256, ... in order into float64 (sum unocc m,
//            sum m, sum occ m); the 256 partials are folded by a stride-halving tree (p[k] += p[k + s], s = 128 ..
//            1).  loss = A / Sm - Bq / So in float64, rounded once (So = sum occ, summed the same way once per launch).
//   gather   lane k takes points k, k + 256, ... again: over the point's window in (i, j, k) lexicographic order, where
//            0 < thr - dmin <= 1 and this point's d == dmin (ties: every such point), g_d = -((unocc iSm - c2) - occ
//            iSo) with iSm = 1 / Sm, c2 = (A / Sm) / Sm, iSo = 1 / So (float64, each rounded once to float32), and the
//            point's gradient gains -(2 a (g_d / (2 d))) per axis in float32; the sum is divided by pitch once.  The
//            lane adds g and g x src^T of its points in order into 12 float64 partials, folded by the same tree and
//            rounded once -> gt, gR -> mf::quat_backward.
//   step     lane 0: mf::adam_pose_step with the bias-corrected alphas the host evaluated in double.
// No float atomic anywhere: every result is bitwise reproducible.
//
// dmin lives in LDS when the object's X Y Z <= MF_OCCREG_LDS_VOXELS (32^3: 128 KB beside the 12 KB point tile and
// the 12 KB reduction scratch), else in the workspace (read and written with atomics only: never through L1).  The
// first MF_OCCREG_POINT_TILE points keep pf in LDS between scatter and gather; later points are transformed again
// from global memory (the same arithmetic, the same bits).  Objects of one launch take either path independently.
#include <limits.h>
#include <math.h>

#include <algorithm>
#include <cmath>

#include "mf_common.h"
#include "quat.h"

namespace {

constexpr int kThreads = 256;
constexpr int kTileP = MF_OCCREG_POINT_TILE;
constexpr int kLdsVox = MF_OCCREG_LDS_VOXELS;
constexpr int kChunk = MF_OCCREG_STEPS_PER_LAUNCH;
constexpr int kRedDoubles = 6 * kThreads;  // reduction scratch: 6 components of 256 float64 partials (12 KB)
constexpr uint32_t kInfBits = 0x7f800000u;

struct Args {
  mfOccRegBatch P;
  float *q, *t, *adam_m, *adam_v;  // refine: updated in place; loss_grad: q, t read only, the others NULL
  float *loss, *gq, *gt;           // loss_grad outputs
  float *losses, *traj;            // refine outputs (may be NULL), whole arrays
  uint32_t *ws;
  int refine;      // 0: one loss + gradient into loss, gq, gt; 1: n_steps x {loss, gradient, Adam step}
  int n_steps;     // steps of this launch
  int step_base;   // index of this launch's first step in losses / traj (0: this launch writes traj entry 0)
  int lds_vox;     // voxels of the dynamic dmin region
  int vox_total;   // voxels of the batch (the host's sum of X Y Z): the length of grid_occ / grid_unocc
  float aq[kChunk], at[kChunk];
};

struct Obj {
  const float *pts, *occ, *unocc;
  int P, X, Y, Z, V;
  float pitch, ox, oy, oz, thr;
};

template <bool LDS>
__device__ __forceinline__ uint32_t dmin_load(uint32_t *p) {
  if (LDS) return *p;
  return atomicOr(p, 0u);
}
template <bool LDS>
__device__ __forceinline__ void dmin_store(uint32_t *p, uint32_t v) {
  if (LDS) *p = v; else atomicExch(p, v);
}

__device__ __forceinline__ void point_pf(const Obj &o, const float *R, const float *t, int p, float *pf) {
  const float x = o.pts[3 * p], y = o.pts[3 * p + 1], z = o.pts[3 * p + 2];
  // transform_points: ((R0 x + R1 y) + R2 z) + t, un-fused; then (points - origin) / pitch
  pf[0] = ((((R[0] * x + R[1] * y) + R[2] * z) + t[0]) - o.ox) / o.pitch;
  pf[1] = ((((R[3] * x + R[4] * y) + R[5] * z) + t[1]) - o.oy) / o.pitch;
  pf[2] = ((((R[6] * x + R[7] * y) + R[8] * z) + t[2]) - o.oz) / o.pitch;
}

// Voxels of one axis that can lie within thr of c: conservative (d >= |i - c| in float arithmetic, and the excluded
// indices are a whole voxel further out); clamped in float, so a far or non-finite coordinate never overflows an int.
__device__ __forceinline__ bool axis_window(float c, float thr, int n, int &lo, int &hi) {
  const float l = fmaxf(floorf(c - thr), 0.0f), h = fminf(ceilf(c + thr), (float)(n - 1));
  if (!(l <= h)) return false;
  lo = (int)l;
  hi = (int)h;
  return true;
}

// fold the 256 partials of n components (component-major in s); all lanes call it, the result is in s[c * 256]
__device__ __forceinline__ void tree_fold(double *s, int n) {
  for (int st = kThreads / 2; st > 0; st >>= 1) {
    if ((int)threadIdx.x < st)
      for (int c = 0; c < n; ++c) s[c * kThreads + threadIdx.x] += s[c * kThreads + threadIdx.x + st];
    __syncthreads();
  }
}

struct Pose {
  float q[4], t[3], m[7], v[7];
  double So;
};

// one forward + backward of the object at the pose in S; every lane returns the same loss, lane 0 holds gq, gt
template <bool LDS>
__device__ __forceinline__ float loss_grad(const Obj &o, const Pose &S, uint32_t *dmin, double *s_red, float *s_pf,
                                           float *gq, float *gt) {
  const int tid = threadIdx.x;
  float R[9];
  mf::quat_to_R(S.q, R);
  const float tt[3] = {S.t[0], S.t[1], S.t[2]};
  const int YZ = o.Y * o.Z;
  for (int v = tid; v < o.V; v += kThreads) dmin_store<LDS>(&dmin[v], kInfBits);
  __syncthreads();
  for (int p = tid; p < o.P; p += kThreads) {
    float pf[3];
    point_pf(o, R, tt, p, pf);
    if (p < kTileP) {
      s_pf[3 * p] = pf[0];
      s_pf[3 * p + 1] = pf[1];
      s_pf[3 * p + 2] = pf[2];
    }
    int lo[3], hi[3];
    if (!axis_window(pf[0], o.thr, o.X, lo[0], hi[0]) || !axis_window(pf[1], o.thr, o.Y, lo[1], hi[1]) ||
        !axis_window(pf[2], o.thr, o.Z, lo[2], hi[2]))
      continue;
    for (int i = lo[0]; i <= hi[0]; ++i) {
      const float a = (float)i - pf[0];
      const float aa = a * a;
      for (int j = lo[1]; j <= hi[1]; ++j) {
        const float b = (float)j - pf[1];
        const float ab = aa + b * b;
        uint32_t *row = dmin + (i * YZ + j * o.Z);
        for (int k = lo[2]; k <= hi[2]; ++k) {
          const float c = (float)k - pf[2];
          const float d = sqrtf(ab + c * c);
          if (d < o.thr) atomicMin(&row[k], __float_as_uint(d));
        }
      }
    }
  }
  __syncthreads();
  double sA = 0.0, sM = 0.0, sB = 0.0;  // float64 sums of the float32 terms (the products are exact in float64)
  for (int v = tid; v < o.V; v += kThreads) {
    float m = o.thr - __uint_as_float(dmin_load<LDS>(&dmin[v]));
    m = m > 0.0f ? m : 0.0f;  // relu
    m = m < 1.0f ? m : 1.0f;  // minimum(., 1)
    if (m > 0.0f) {
      sA += (double)o.unocc[v] * (double)m;
      sM += (double)m;
      sB += (double)o.occ[v] * (double)m;
    }
  }
  s_red[tid] = sA;
  s_red[kThreads + tid] = sM;
  s_red[2 * kThreads + tid] = sB;
  __syncthreads();
  tree_fold(s_red, 3);
  const double A = s_red[0], Sm = s_red[kThreads], Bq = s_red[2 * kThreads];
  __syncthreads();  // s_red is written again below
  const double pen = A / Sm;
  const float loss = (float)(pen - Bq / S.So);  // rounded once
  const float iSm = (float)(1.0 / Sm), c2 = (float)(pen / Sm), iSo = (float)(1.0 / S.So);
  double acc[12];
#pragma unroll
  for (int c = 0; c < 12; ++c) acc[c] = 0.0;
  for (int p = tid; p < o.P; p += kThreads) {
    float pf[3];
    if (p < kTileP) {
      pf[0] = s_pf[3 * p];
      pf[1] = s_pf[3 * p + 1];
      pf[2] = s_pf[3 * p + 2];
    } else {
      point_pf(o, R, tt, p, pf);
    }
    int lo[3], hi[3];
    if (!axis_window(pf[0], o.thr, o.X, lo[0], hi[0]) || !axis_window(pf[1], o.thr, o.Y, lo[1], hi[1]) ||
        !axis_window(pf[2], o.thr, o.Z, lo[2], hi[2]))
      continue;
    float g[3] = {0.0f, 0.0f, 0.0f};
    for (int i = lo[0]; i <= hi[0]; ++i) {
      const float a = (float)i - pf[0];
      const float aa = a * a;
      for (int j = lo[1]; j <= hi[1]; ++j) {
        const float b = (float)j - pf[1];
        const float ab = aa + b * b;
        const int vrow = i * YZ + j * o.Z;
        for (int k = lo[2]; k <= hi[2]; ++k) {
          const float dm = __uint_as_float(dmin_load<LDS>(&dmin[vrow + k]));
          const float r = o.thr - dm;
          if (!(r > 0.0f && r <= 1.0f)) continue;  // relu passes where > 0, minimum(a, 1) where a <= 1
          const float c = (float)k - pf[2];
          const float d = sqrtf(ab + c * c);
          if (d != dm) continue;  // F.min: every point at the minimum
          const float g_d = -((o.unocc[vrow + k] * iSm - c2) - o.occ[vrow + k] * iSo);
          if (g_d == 0.0f) continue;
          const float g_dd = g_d / (2.0f * d);  // sqrt backward gy / (2 y): NaN for a point on the voxel centre
          g[0] += -(2.0f * a * g_dd);
          g[1] += -(2.0f * b * g_dd);
          g[2] += -(2.0f * c * g_dd);
        }
      }
    }
    const float x = o.pts[3 * p], y = o.pts[3 * p + 1], z = o.pts[3 * p + 2];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const float ga = g[a] / o.pitch;
      acc[3 * a] += (double)ga * (double)x;
      acc[3 * a + 1] += (double)ga * (double)y;
      acc[3 * a + 2] += (double)ga * (double)z;
      acc[9 + a] += (double)ga;
    }
  }
  float g12[12];  // lane 0: the 12 sums, each rounded once
#pragma unroll
  for (int half = 0; half < 2; ++half) {  // the scratch holds 6 components
#pragma unroll
    for (int c = 0; c < 6; ++c) s_red[c * kThreads + tid] = acc[6 * half + c];
    __syncthreads();
    tree_fold(s_red, 6);
#pragma unroll
    for (int c = 0; c < 6; ++c) g12[6 * half + c] = (float)s_red[c * kThreads];
    __syncthreads();  // s_red is written again (here, or by the next call)
  }
  if (tid == 0) {
#pragma unroll
    for (int a = 0; a < 3; ++a) gt[a] = g12[9 + a];
    mf::quat_backward(S.q, g12, gq);
  }
  return loss;
}

template <bool LDS>
__device__ __forceinline__ void run_object(const Args &A, const Obj &o, Pose &S, uint32_t *dmin, double *s_red,
                                           float *s_pf, int b) {
  const int tid = threadIdx.x, B = A.P.n_objects;
  {  // So = sum occ, lane-strided then the tree: once per launch
    double s = 0.0;
    for (int v = tid; v < o.V; v += kThreads) s += (double)o.occ[v];
    s_red[tid] = s;
    __syncthreads();
    tree_fold(s_red, 1);
    if (tid == 0) S.So = s_red[0];
    __syncthreads();
  }
  float gq[4], gt[3];
  if (!A.refine) {
    const float loss = loss_grad<LDS>(o, S, dmin, s_red, s_pf, gq, gt);
    if (tid == 0) {
      A.loss[b] = loss;
      for (int i = 0; i < 4; ++i) A.gq[4 * b + i] = gq[i];
      for (int i = 0; i < 3; ++i) A.gt[3 * b + i] = gt[i];
    }
    return;
  }
  for (int k = 0; k < A.n_steps; ++k) {
    const float loss = loss_grad<LDS>(o, S, dmin, s_red, s_pf, gq, gt);
    if (tid == 0) {
      const int64_t step = (int64_t)A.step_base + k;
      if (A.losses) A.losses[step * B + b] = loss;
      mf::adam_pose_step(gq, gt, A.aq[k], A.at[k], S.q, S.t, S.m, S.v);
      if (A.traj) {
        float *tr = A.traj + ((step + 1) * B + b) * 7;
        for (int i = 0; i < 4; ++i) tr[i] = S.q[i];
        for (int i = 0; i < 3; ++i) tr[4 + i] = S.t[i];
      }
    }
    __syncthreads();
  }
  if (tid == 0) {
    for (int i = 0; i < 4; ++i) A.q[4 * b + i] = S.q[i];
    for (int i = 0; i < 3; ++i) A.t[3 * b + i] = S.t[i];
    for (int i = 0; i < 7; ++i) {
      A.adam_m[7 * b + i] = S.m[i];
      A.adam_v[7 * b + i] = S.v[i];
    }
  }
}

__global__ __launch_bounds__(kThreads) void k_occreg(Args A) {
  MF_DYN_LDS(double, s_dyn);
  __shared__ Pose S;
  double *s_red = s_dyn;
  float *s_pf = reinterpret_cast<float *>(s_dyn + kRedDoubles);
  uint32_t *s_dmin = reinterpret_cast<uint32_t *>(s_pf + 3 * kTileP);
  const int b = blockIdx.x, tid = threadIdx.x, B = A.P.n_objects;
  Obj o;
  const int p0 = A.P.pts_off[b];
  o.P = A.P.pts_off[b + 1] - p0;
  o.pts = A.P.points + 3 * (int64_t)p0;
  o.X = A.P.dims[3 * b];
  o.Y = A.P.dims[3 * b + 1];
  o.Z = A.P.dims[3 * b + 2];
  o.pitch = A.P.pitch[b];
  o.ox = A.P.origin[3 * b];
  o.oy = A.P.origin[3 * b + 1];
  o.oz = A.P.origin[3 * b + 2];
  o.thr = A.P.threshold[b];
  const int64_t g0 = A.P.grid_off[b];
  o.occ = A.P.grid_occ + g0;
  o.unocc = A.P.grid_unocc + g0;
  // the host checked its mirror of the descriptor; the device arrays are checked again, so that a mismatch between
  // the two cannot index outside the packed grids (vox_total voxels), the points or the workspace
  const int64_t V64 = (int64_t)o.X * o.Y * o.Z;
  const bool valid = o.X >= 1 && o.Y >= 1 && o.Z >= 1 && V64 <= A.P.max_voxels && o.P >= 0 && p0 >= 0 &&
                     (int64_t)p0 + o.P <= A.P.n_points_total && g0 >= 0 && g0 + V64 <= A.vox_total && o.thr > 0.0f &&
                     o.thr <= MF_OCCREG_MAX_THRESHOLD && o.pitch > 0.0f && isfinite(o.pitch) &&
                     (V64 <= A.lds_vox || (A.ws != nullptr && A.P.max_voxels > kLdsVox));  // a home for dmin
  o.V = valid ? (int)V64 : 0;
  if (!valid || (A.P.active && !A.P.active[b])) {  // the pose passes through (block-uniform)
    if (tid == 0) {
      const float fill = valid ? 0.0f : NAN;
      if (!A.refine) {
        A.loss[b] = fill;
        for (int i = 0; i < 4; ++i) A.gq[4 * b + i] = 0.0f;
        for (int i = 0; i < 3; ++i) A.gt[3 * b + i] = 0.0f;
      }
      const int n = A.refine ? A.n_steps : 0;
      for (int k = A.step_base == 0 ? -1 : 0; k < n; ++k) {  // k = -1: traj entry 0
        const int64_t step = (int64_t)A.step_base + k;
        if (A.losses && k >= 0) A.losses[step * B + b] = fill;
        if (A.traj && A.refine)
          for (int i = 0; i < 7; ++i) A.traj[((step + 1) * B + b) * 7 + i] = i < 4 ? A.q[4 * b + i] : A.t[3 * b + i - 4];
      }
    }
    return;
  }
  if (tid == 0) {
    for (int i = 0; i < 4; ++i) S.q[i] = A.q[4 * b + i];
    for (int i = 0; i < 3; ++i) S.t[i] = A.t[3 * b + i];
    for (int i = 0; i < 7; ++i) {
      S.m[i] = A.adam_m ? A.adam_m[7 * b + i] : 0.0f;
      S.v[i] = A.adam_v ? A.adam_v[7 * b + i] : 0.0f;
    }
    if (A.refine && A.traj && A.step_base == 0)
      for (int i = 0; i < 7; ++i) A.traj[(int64_t)b * 7 + i] = i < 4 ? S.q[i] : S.t[i - 4];
  }
  __syncthreads();
  if (o.V <= A.lds_vox)
    run_object<true>(A, o, S, s_dmin, s_red, s_pf, b);
  else
    run_object<false>(A, o, S, A.ws + (int64_t)b * A.P.max_voxels, s_red, s_pf, b);
}

int bad(const char *what) {
  mf::set_last_error(hipErrorInvalidValue, what);
  return -(int)hipErrorInvalidValue;
}

// the refusals of the header, from the host mirror of the descriptor; -> voxels of the dynamic dmin region
int validate(const mfOccRegBatch *batch, const void *workspace, int &lds_vox, int &vox_total) {
  if (!batch) return bad("mf_occreg: no batch");
  const mfOccRegBatch &P = *batch;
  if (mf_occreg_workspace_bytes(P.n_objects, P.n_points_total, P.max_voxels) < 0)
    return bad("mf_occreg: need 1..65535 objects, 0 <= points and 1 <= max_voxels within int32");
  if (!P.host_pts_off || !P.host_pitch || !P.host_dims || !P.host_threshold)
    return bad("mf_occreg: the host mirrors of pts_off, pitch, dims and threshold are required");
  int64_t total = 0;
  lds_vox = 0;
  bool need_ws = false;
  if (P.host_pts_off[0] != 0 || P.host_pts_off[P.n_objects] != P.n_points_total)
    return bad("mf_occreg: pts_off must run from 0 to n_points_total");
  for (int b = 0; b < P.n_objects; ++b) {
    if (P.host_pts_off[b + 1] < P.host_pts_off[b]) return bad("mf_occreg: pts_off must not decrease");
    const int32_t *d = P.host_dims + 3 * b;
    if (d[0] < 1 || d[1] < 1 || d[2] < 1) return bad("mf_occreg: a grid dimension < 1");
    const int64_t V = (int64_t)d[0] * d[1];
    if (V > INT_MAX || V * d[2] > P.max_voxels) return bad("mf_occreg: an object's X Y Z exceeds max_voxels");
    total += V * d[2];
    if (total > INT_MAX) return bad("mf_occreg: more than 2^31 - 1 voxels in the batch");
    if (V * d[2] <= kLdsVox) lds_vox = std::max(lds_vox, (int)(V * d[2])); else need_ws = true;
    const float thr = P.host_threshold[b], pitch = P.host_pitch[b];
    if (!(thr > 0.0f) || !(thr <= MF_OCCREG_MAX_THRESHOLD))
      return bad("mf_occreg: threshold must be finite, > 0 and <= MF_OCCREG_MAX_THRESHOLD");
    if (!(pitch > 0.0f) || !std::isfinite(pitch)) return bad("mf_occreg: pitch must be finite and > 0");
  }
  vox_total = (int)total;
  if (need_ws && !workspace) return bad("mf_occreg: a grid beyond MF_OCCREG_LDS_VOXELS needs the workspace");
  return 0;
}

int launch(Args &A, hipStream_t stream) {
  const int lds = kRedDoubles * 8 + (3 * kTileP + A.lds_vox) * 4;
  if (lds > 64 * 1024)
    if (int e = mf::allow_big_lds((const void *)k_occreg, lds)) return e;
  hipLaunchKernelGGL(k_occreg, dim3(A.P.n_objects), dim3(kThreads), lds, stream, A);
  return mf::check_launch("mf_occreg");
}

}  // namespace

extern "C" int64_t mf_occreg_workspace_bytes(int64_t n_objects, int64_t n_points_total, int64_t max_voxels) {
  if (n_objects < 1 || n_objects > MF_OCCREG_MAX_OBJECTS) return -1;
  if (n_points_total < 0 || n_points_total > INT_MAX) return -1;
  if (max_voxels < 1 || max_voxels > INT_MAX) return -1;
  // dmin of the objects whose grid does not fit LDS: one slot of max_voxels per object
  return max_voxels > kLdsVox ? 4 * n_objects * max_voxels : 0;
}

extern "C" int mf_occreg_loss_grad(const mfOccRegBatch *batch, const float *q, const float *t, float *loss, float *gq,
                                   float *gt, void *workspace, mfStream_t stream) {
  Args A = {};
  if (int e = validate(batch, workspace, A.lds_vox, A.vox_total)) return e;
  A.P = *batch;
  A.q = const_cast<float *>(q);
  A.t = const_cast<float *>(t);
  A.loss = loss;
  A.gq = gq;
  A.gt = gt;
  A.ws = static_cast<uint32_t *>(workspace);
  return launch(A, (hipStream_t)stream);
}

extern "C" int mf_occreg_refine(const mfOccRegBatch *batch, float *q, float *t, float *adam_m, float *adam_v,
                                int32_t n_iter, int32_t step0, float alpha_q, float alpha_t, float *losses, float *traj,
                                void *workspace, mfStream_t stream) {
  Args A = {};
  if (int e = validate(batch, workspace, A.lds_vox, A.vox_total)) return e;
  if (n_iter < 0 || step0 < 0) return bad("mf_occreg_refine: negative n_iter or step0");
  if (!adam_m || !adam_v) return bad("mf_occreg_refine: the Adam moments are required");
  A.P = *batch;
  A.q = q;
  A.t = t;
  A.adam_m = adam_m;
  A.adam_v = adam_v;
  A.losses = losses;
  A.traj = traj;
  A.ws = static_cast<uint32_t *>(workspace);
  A.refine = 1;
  if (n_iter == 0 && !traj) return 0;
  // entry 0 of traj and the launches of up to kChunk steps: the state lives in q, t, adam_m, adam_v between them
  for (int base = 0; base == 0 || base < n_iter; base += kChunk) {
    A.n_steps = std::min(kChunk, n_iter - base);
    A.step_base = base;
    for (int k = 0; k < A.n_steps; ++k) {
      // chainer Adam: alpha_t = alpha * sqrt(1 - b2^t) / (1 - b1^t), in double, cast once
      const int st = step0 + base + k + 1;
      const double fix1 = 1.0 - pow(0.9, (double)st), fix2 = 1.0 - pow(0.999, (double)st);
      A.aq[k] = (float)((double)alpha_q * sqrt(fix2) / fix1);
      A.at[k] = (float)((double)alpha_t * sqrt(fix2) / fix1);
    }
    if (int e = launch(A, (hipStream_t)stream)) return e;
  }
  return 0;
}
