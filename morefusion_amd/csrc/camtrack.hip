// Camera tracking: dense point-to-plane depth alignment over a pyramid (contrib/camera_tracking.py) -- gfx950, float64.
//
// The tracking step of KinectFusion (Newcombe et al., ISMAR 2011, section 3.5): the pose the rest of the online path
// takes as T_sensor_to_map, from the depth images alone.  include/mfhip.h "camera tracking" is the contract -- the
// layouts, every formula and every summation order -- and tests/camtrack_ref.py the NumPy mirror this file is pinned
// to bit for bit; DESIGN.md "Camera tracking" has the cost model.
//
//   k_ct_level0    a lane per pixel: depth_0 = the input, vertex_0; the first lanes also write the rectangles.
//   k_ct_down      a lane per pixel of level l + 1: the banded mean of its 2 x 2 block of level l, vertex_(l+1).
//   (normals)      mf_pick_normals (csrc/pickorder.hip) on each vertex map: its arithmetic is the contract.
//   k_ct_start     a lane per alignment: T_init -> (q, t), the frames the residual launch reads, status, T_cur_to_map.
//   k_ct_residual  256 lanes per 1024 pixels and alignment: 28 float64 sums and a count per workgroup.
//   k_ct_solve     a workgroup per alignment: the partials summed, the 6 x 6 Cholesky solve, the pose update.
//
// Reduction of k_ct_residual: the sums stay in registers over a lane's 4 pixels, fold over the wave with __shfl_down
// (6 steps, lane 0 holds the wave's sum), cross the 4 waves through 4 x 29 LDS words and leave as ONE partial per
// workgroup with plain vector stores; k_ct_solve -- the next launch on the stream -- adds the partials.  No float
// atomic, no "last workgroup finishes" hand-off: the launch boundary is the only ordering, so the order of every
// sum is fixed by the shape alone.  Nothing is contracted (-ffp-contract=off); only + - x / sqrt and floor are used.
#include <math.h>

#include "mf_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kPixPerLane = MF_CAMTRACK_GROUP_PIXELS / kThreads;
constexpr int kTerms = 28;                       // 21 of J^T J, 6 of J^T r, r r; term 28 of a partial = the pairs
constexpr int kPartial = MF_CAMTRACK_PARTIAL;
constexpr int kSub = 8;                          // sub-sums of k_ct_solve

__device__ __forceinline__ double qnan() { return (double)__uint_as_float(0x7fc00000u); }

// ---- the pyramid's layout (host) ---------------------------------------------------------------------------------
struct Level {
  int H, W;
  int64_t depth, vertex, normal;  // byte offsets
  double fx, fy, cx, cy;
};
struct Layout {
  Level level[MF_CAMTRACK_MAX_LEVELS];
  int64_t rect, bytes;
};

int64_t align16(int64_t n) { return (n + 15) & ~(int64_t)15; }

bool bad_shape(int32_t B, int32_t height, int32_t width, int32_t levels) {
  if (B < 1 || B > MF_CAMTRACK_MAX_BATCH || levels < 1 || levels > MF_CAMTRACK_MAX_LEVELS) return true;
  if (height < 1 || width < 1 || height > MF_RENDER_MAX_SIDE || width > MF_RENDER_MAX_SIDE) return true;
  if ((int64_t)B * height * width > MF_CAMTRACK_MAX_PIXELS) return true;
  return (height >> (levels - 1)) < 8 || (width >> (levels - 1)) < 8;
}

Layout layout_of(int32_t B, int32_t height, int32_t width, int32_t levels, double fx, double fy, double cx,
                 double cy) {
  Layout lay;
  int64_t off = 0;
  for (int l = 0; l < levels; ++l) {
    Level &v = lay.level[l];
    v.H = height >> l;
    v.W = width >> l;
    if (l == 0) {
      v.fx = fx; v.fy = fy; v.cx = cx; v.cy = cy;
    } else {
      const Level &u = lay.level[l - 1];
      v.fx = u.fx / 2.0; v.fy = u.fy / 2.0; v.cx = (u.cx - 0.5) / 2.0; v.cy = (u.cy - 0.5) / 2.0;
    }
    const int64_t n = (int64_t)B * v.H * v.W;
    v.depth = off;  off = align16(off + 4 * n);
    v.vertex = off; off = align16(off + 24 * n);
    v.normal = off; off = align16(off + 24 * n);
  }
  lay.rect = off;
  lay.bytes = align16(off + 16 * (int64_t)levels * B);
  return lay;
}

int64_t groups_of(int H, int W) {
  return ((int64_t)H * W + MF_CAMTRACK_GROUP_PIXELS - 1) / MF_CAMTRACK_GROUP_PIXELS;
}

// mf_camtrack_align's workspace: pose0 [B, 7], cur [B, 12] (R row-major, t), ref_inv [B, 12], partials
struct Workspace {
  int64_t pose0, cur, ref_inv, partial, bytes;
};
Workspace workspace_of(int32_t B, int32_t height, int32_t width) {
  Workspace w;
  w.pose0 = 0;
  w.cur = align16(w.pose0 + 8 * 7 * (int64_t)B);
  w.ref_inv = align16(w.cur + 8 * 12 * (int64_t)B);
  w.partial = align16(w.ref_inv + 8 * 12 * (int64_t)B);
  w.bytes = align16(w.partial + 8 * (int64_t)kPartial * B * groups_of(height, width));
  return w;
}

// ---- prepare -----------------------------------------------------------------------------------------------------
__device__ __forceinline__ void store_vertex(double *out, float zf, int r, int c, double fx, double fy, double cx,
                                             double cy) {
  if (zf > 0.0f) {
    const double z = (double)zf;
    out[0] = (z * ((double)c - cx)) / fx;
    out[1] = (z * ((double)r - cy)) / fy;
    out[2] = z;
  } else {
    out[0] = out[1] = out[2] = qnan();
  }
}

__global__ void __launch_bounds__(kThreads) k_ct_level0(const float *__restrict__ depth_in, int B, int H, int W,
                                                         int levels, double fx, double fy, double cx, double cy,
                                                         float *__restrict__ depth, double *__restrict__ vertex,
                                                         int32_t *__restrict__ rect) {
  const int64_t plane = (int64_t)H * W;
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i < (int64_t)levels * B) {
    const int l = (int)(i / B);
    rect[4 * i] = 0; rect[4 * i + 1] = 0; rect[4 * i + 2] = H >> l; rect[4 * i + 3] = W >> l;
  }
  if (i >= plane * B) return;
  const int64_t p = i % plane;
  const float z = depth_in[i];
  depth[i] = z;
  store_vertex(vertex + 3 * i, z, (int)(p / W), (int)(p % W), fx, fy, cx, cy);
}

__global__ void __launch_bounds__(kThreads) k_ct_down(const float *__restrict__ src, int B, int Hs, int Ws, int Hd,
                                                       int Wd, double band, double fx, double fy, double cx,
                                                       double cy, float *__restrict__ depth,
                                                       double *__restrict__ vertex) {
  const int64_t plane = (int64_t)Hd * Wd;
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= plane * B) return;
  const int64_t b = i / plane, p = i % plane;
  const int r = (int)(p / Wd), c = (int)(p % Wd);
  const float *s = src + (b * Hs + 2 * r) * (int64_t)Ws + 2 * c;  // (2 r + 1 < Hs and 2 c + 1 < Ws: Hd = Hs >> 1)
  const float d[4] = {s[0], s[1], s[Ws], s[Ws + 1]};
  float dmin = 0.0f;
  bool any = false;
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (d[k] > 0.0f && (!any || d[k] < dmin)) { dmin = d[k]; any = true; }
  double sum = 0.0;
  int n = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (d[k] > 0.0f && (double)d[k] - (double)dmin <= band) { sum += (double)d[k]; ++n; }
  const float z = any ? (float)(sum / (double)n) : __uint_as_float(0x7fc00000u);
  depth[i] = z;
  store_vertex(vertex + 3 * i, z, r, c, fx, fy, cx, cy);
}

// ---- quaternions (w, x, y, z), float64 ----------------------------------------------------------------------------
__device__ __forceinline__ void quat_normalise(double *q) {
  const double n = sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]);
  q[0] = q[0] / n; q[1] = q[1] / n; q[2] = q[2] / n; q[3] = q[3] / n;
}

__device__ __forceinline__ void quat_matrix(const double *q, double *R) {  // of a unit quaternion, row-major
  const double w = q[0], x = q[1], y = q[2], z = q[3];
  R[0] = 1.0 - 2.0 * (y * y + z * z); R[1] = 2.0 * (x * y - w * z);       R[2] = 2.0 * (x * z + w * y);
  R[3] = 2.0 * (x * y + w * z);       R[4] = 1.0 - 2.0 * (x * x + z * z); R[5] = 2.0 * (y * z - w * x);
  R[6] = 2.0 * (x * z - w * y);       R[7] = 2.0 * (y * z + w * x);       R[8] = 1.0 - 2.0 * (x * x + y * y);
}

__device__ __forceinline__ void quat_from_matrix(const double *m, double *q) {  // m [4, 4] row-major; Shepperd
  const double m00 = m[0], m01 = m[1], m02 = m[2], m10 = m[4], m11 = m[5], m12 = m[6], m20 = m[8], m21 = m[9],
               m22 = m[10];
  const double tr = (m00 + m11) + m22;
  if (tr > 0.0) {
    const double s = sqrt(tr + 1.0) * 2.0;
    q[0] = 0.25 * s; q[1] = (m21 - m12) / s; q[2] = (m02 - m20) / s; q[3] = (m10 - m01) / s;
  } else if (m00 > m11 && m00 > m22) {
    const double s = sqrt(((1.0 + m00) - m11) - m22) * 2.0;
    q[0] = (m21 - m12) / s; q[1] = 0.25 * s; q[2] = (m01 + m10) / s; q[3] = (m02 + m20) / s;
  } else if (m11 > m22) {
    const double s = sqrt(((1.0 + m11) - m00) - m22) * 2.0;
    q[0] = (m02 - m20) / s; q[1] = (m01 + m10) / s; q[2] = 0.25 * s; q[3] = (m12 + m21) / s;
  } else {
    const double s = sqrt(((1.0 + m22) - m00) - m11) * 2.0;
    q[0] = (m10 - m01) / s; q[1] = (m02 + m20) / s; q[2] = (m12 + m21) / s; q[3] = 0.25 * s;
  }
  quat_normalise(q);
}

// the frame the residual launch reads (R row-major, then t) and the 4 x 4 matrix of a pose (q, t)
__device__ __forceinline__ void publish_pose(const double *pose, double *cur, double *T) {
  double R[9];
  quat_matrix(pose, R);
  for (int k = 0; k < 9; ++k) cur[k] = R[k];
  for (int k = 0; k < 3; ++k) cur[9 + k] = pose[4 + k];
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) T[4 * i + j] = R[3 * i + j];
    T[4 * i + 3] = pose[4 + i];
  }
  T[12] = 0.0; T[13] = 0.0; T[14] = 0.0; T[15] = 1.0;
}

__global__ void __launch_bounds__(kThreads) k_ct_start(const double *__restrict__ T_ref, const double *__restrict__ T_init,
                                                        int B, double *__restrict__ pose, double *__restrict__ pose0,
                                                        double *__restrict__ cur, double *__restrict__ ref_inv,
                                                        double *__restrict__ T_out, int32_t *__restrict__ status) {
  const int b = blockIdx.x * kThreads + threadIdx.x;
  if (b >= B) return;
  const double *m = T_init + 16 * (int64_t)b;
  double p[7];
  quat_from_matrix(m, p);
  p[4] = m[3]; p[5] = m[7]; p[6] = m[11];
  for (int k = 0; k < 7; ++k) { pose[7 * (int64_t)b + k] = p[k]; pose0[7 * (int64_t)b + k] = p[k]; }
  publish_pose(p, cur + 12 * (int64_t)b, T_out + 16 * (int64_t)b);
  const double *r = T_ref + 16 * (int64_t)b;  // the rigid inverse: R^T, -(R^T t)
  double *inv = ref_inv + 12 * (int64_t)b;
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) inv[3 * i + j] = r[4 * j + i];
    inv[9 + i] = -((r[i] * r[3] + r[4 + i] * r[7]) + r[8 + i] * r[11]);
  }
  status[b] = MF_CAMTRACK_TRACKING;
}

// ---- residuals ---------------------------------------------------------------------------------------------------
__device__ __forceinline__ void rotate(const double *R, const double *v, double *out) {
  out[0] = (R[0] * v[0] + R[1] * v[1]) + R[2] * v[2];
  out[1] = (R[3] * v[0] + R[4] * v[1]) + R[5] * v[2];
  out[2] = (R[6] * v[0] + R[7] * v[1]) + R[8] * v[2];
}

__global__ void __launch_bounds__(kThreads) k_ct_residual(
    const double *__restrict__ vertex, const double *__restrict__ normal, const double *__restrict__ ref_vertex,
    const double *__restrict__ ref_normal, int H, int W, double fx, double fy, double cx, double cy,
    const double *__restrict__ T_ref, const double *__restrict__ cur_all, const double *__restrict__ ref_inv_all,
    const int32_t *__restrict__ status, double dist_thr, double cos_thr, int groups, double *__restrict__ partial) {
  __shared__ double s_part[kThreads / 64][kTerms];
  __shared__ int s_cnt[kThreads / 64];
  const int b = blockIdx.y, t = threadIdx.x, lane = t & 63, wave = t >> 6;
  if (status[b] != MF_CAMTRACK_TRACKING) return;  // (uniform over the workgroup)
  const int64_t plane = (int64_t)H * W;
  const double *cur = cur_all + 12 * (int64_t)b, *inv = ref_inv_all + 12 * (int64_t)b, *tr = T_ref + 16 * (int64_t)b;
  double R[9], tt[3], Ri[9], ti[3], Rr[9], tref[3];
  for (int k = 0; k < 9; ++k) { R[k] = cur[k]; Ri[k] = inv[k]; Rr[k] = tr[4 * (k / 3) + k % 3]; }
  for (int k = 0; k < 3; ++k) { tt[k] = cur[9 + k]; ti[k] = inv[9 + k]; tref[k] = tr[4 * k + 3]; }
  const double *vb = vertex + 3 * plane * b, *nb = normal + 3 * plane * b;
  const double *rvb = ref_vertex + 3 * plane * b, *rnb = ref_normal + 3 * plane * b;
  double acc[kTerms];
#pragma unroll
  for (int k = 0; k < kTerms; ++k) acc[k] = 0.0;
  int cnt = 0;
  for (int s = 0; s < kPixPerLane; ++s) {
    const int64_t p = ((int64_t)blockIdx.x * kPixPerLane + s) * kThreads + t;
    if (p >= plane) continue;
    const double v[3] = {vb[3 * p], vb[3 * p + 1], vb[3 * p + 2]};
    const double n[3] = {nb[3 * p], nb[3 * p + 1], nb[3 * p + 2]};
    if (v[0] != v[0] || v[1] != v[1] || v[2] != v[2] || n[0] != n[0] || n[1] != n[1] || n[2] != n[2]) continue;
    double vg[3], ng[3], pr[3];
    rotate(R, v, vg);
    vg[0] += tt[0]; vg[1] += tt[1]; vg[2] += tt[2];
    rotate(R, n, ng);
    rotate(Ri, vg, pr);
    pr[0] += ti[0]; pr[1] += ti[1]; pr[2] += ti[2];
    if (!(pr[2] > 0.0)) continue;
    const double uf = floor(((fx * pr[0]) / pr[2] + cx) + 0.5), vf = floor(((fy * pr[1]) / pr[2] + cy) + 0.5);
    if (!(uf >= 0.0 && uf < (double)W && vf >= 0.0 && vf < (double)H)) continue;
    const int64_t o = 3 * ((int64_t)vf * W + (int64_t)uf);
    const double rv[3] = {rvb[o], rvb[o + 1], rvb[o + 2]};
    const double rn[3] = {rnb[o], rnb[o + 1], rnb[o + 2]};
    if (rv[0] != rv[0] || rv[1] != rv[1] || rv[2] != rv[2] || rn[0] != rn[0] || rn[1] != rn[1] || rn[2] != rn[2])
      continue;
    double rvg[3], rng[3];
    rotate(Rr, rv, rvg);
    rvg[0] += tref[0]; rvg[1] += tref[1]; rvg[2] += tref[2];
    rotate(Rr, rn, rng);
    const double d[3] = {rvg[0] - vg[0], rvg[1] - vg[1], rvg[2] - vg[2]};
    if (sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]) > dist_thr) continue;
    if ((ng[0] * rng[0] + ng[1] * rng[1]) + ng[2] * rng[2] < cos_thr) continue;
    const double res = (rng[0] * d[0] + rng[1] * d[1]) + rng[2] * d[2];
    const double J[6] = {rng[0], rng[1], rng[2], vg[1] * rng[2] - vg[2] * rng[1], vg[2] * rng[0] - vg[0] * rng[2],
                         vg[0] * rng[1] - vg[1] * rng[0]};
    int k = 0;
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
      for (int j = i; j < 6; ++j) acc[k++] += J[i] * J[j];
#pragma unroll
    for (int i = 0; i < 6; ++i) acc[21 + i] += J[i] * res;
    acc[27] += res * res;
    ++cnt;
  }
  // every lane is here: fold the wave, lane 0 ends with its sum
#pragma unroll
  for (int h = 32; h >= 1; h >>= 1) {
#pragma unroll
    for (int k = 0; k < kTerms; ++k) acc[k] += __shfl_down(acc[k], h);
    cnt += __shfl_down(cnt, h);
  }
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < kTerms; ++k) s_part[wave][k] = acc[k];
    s_cnt[wave] = cnt;
  }
  __syncthreads();
  double *out = partial + kPartial * ((int64_t)b * groups + blockIdx.x);
  if (t < kTerms) out[t] = ((s_part[0][t] + s_part[1][t]) + s_part[2][t]) + s_part[3][t];
  if (t == kTerms) out[t] = (double)(((s_cnt[0] + s_cnt[1]) + s_cnt[2]) + s_cnt[3]);
}

// ---- solve -------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kThreads) k_ct_solve(const double *__restrict__ partial, int groups, int groups_stride,
                                                        int min_pairs, int it, int n_iters,
                                                        double *__restrict__ pose_all, const double *__restrict__ pose0_all,
                                                        double *__restrict__ cur_all, double *__restrict__ T_out,
                                                        int32_t *__restrict__ status, double *__restrict__ stats) {
  __shared__ double s_sub[kSub][kPartial];
  __shared__ double s_tot[kPartial];
  const int b = blockIdx.x, t = threadIdx.x;
  if (status[b] != MF_CAMTRACK_TRACKING) return;  // (uniform over the workgroup)
  const int k = t & (kPartial - 1), j = t / kPartial;  // 256 = kSub * kPartial
  if (k <= kTerms) {
    const double *src = partial + kPartial * (int64_t)b * groups_stride;
    double s = 0.0;
    for (int g = j; g < groups; g += kSub) s += src[kPartial * (int64_t)g + k];
    s_sub[j][k] = s;
  }
  __syncthreads();
  if (t <= kTerms) {
    double s = s_sub[0][t];
    for (int jj = 1; jj < kSub; ++jj) s += s_sub[jj][t];
    s_tot[t] = s;
  }
  __syncthreads();
  if (t != 0) return;
  double *pose = pose_all + 7 * (int64_t)b;
  double *st = stats + 3 * ((int64_t)b * n_iters + it);
  const int pairs = (int)s_tot[kTerms];
  int lost = pairs < min_pairs ? MF_CAMTRACK_LOST_PAIRS : MF_CAMTRACK_TRACKING;
  double L[6][6], x[6], y[6];
  if (!lost) {
    double A[6][6];
    int kk = 0;
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
      for (int jj = i; jj < 6; ++jj) { A[i][jj] = s_tot[kk]; A[jj][i] = s_tot[kk]; ++kk; }
#pragma unroll
    for (int c = 0; c < 6 && !lost; ++c) {
      double d = A[c][c];
#pragma unroll
      for (int m = 0; m < c; ++m) d -= L[c][m] * L[c][m];
      if (!(d > 0.0)) { lost = MF_CAMTRACK_LOST_PIVOT; break; }
      L[c][c] = sqrt(d);
#pragma unroll
      for (int i = c + 1; i < 6; ++i) {
        double s = A[i][c];
#pragma unroll
        for (int m = 0; m < c; ++m) s -= L[i][m] * L[c][m];
        L[i][c] = s / L[c][c];
      }
    }
  }
  if (lost) {
#pragma unroll
    for (int m = 0; m < 7; ++m) pose[m] = pose0_all[7 * (int64_t)b + m];
    publish_pose(pose, cur_all + 12 * (int64_t)b, T_out + 16 * (int64_t)b);
    status[b] = lost;
    st[0] = (double)pairs; st[1] = s_tot[27]; st[2] = 0.0;
    return;
  }
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    double s = s_tot[21 + i];
#pragma unroll
    for (int m = 0; m < i; ++m) s -= L[i][m] * y[m];
    y[i] = s / L[i][i];
  }
#pragma unroll
  for (int i = 5; i >= 0; --i) {
    double s = y[i];
#pragma unroll
    for (int m = i + 1; m < 6; ++m) s -= L[m][i] * x[m];
    x[i] = s / L[i][i];
  }
  double dq[4] = {1.0, x[3] / 2.0, x[4] / 2.0, x[5] / 2.0}, Rinc[9], tn[3];
  quat_normalise(dq);
  quat_matrix(dq, Rinc);
  rotate(Rinc, pose + 4, tn);
  const double a0 = dq[0], a1 = dq[1], a2 = dq[2], a3 = dq[3], b0 = pose[0], b1 = pose[1], b2 = pose[2], b3 = pose[3];
  double q[4] = {((a0 * b0 - a1 * b1) - a2 * b2) - a3 * b3, ((a0 * b1 + a1 * b0) + a2 * b3) - a3 * b2,
                 ((a0 * b2 - a1 * b3) + a2 * b0) + a3 * b1, ((a0 * b3 + a1 * b2) - a2 * b1) + a3 * b0};
  quat_normalise(q);
  for (int m = 0; m < 4; ++m) pose[m] = q[m];
  for (int m = 0; m < 3; ++m) pose[4 + m] = tn[m] + x[m];
  publish_pose(pose, cur_all + 12 * (int64_t)b, T_out + 16 * (int64_t)b);
  st[0] = (double)pairs;
  st[1] = s_tot[27];
  st[2] = sqrt(((((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2]) + x[3] * x[3]) + x[4] * x[4]) + x[5] * x[5]);
}

int bad(const char *what) {
  mf::set_last_error(hipErrorInvalidValue, what);
  return -(int)hipErrorInvalidValue;
}

}  // namespace

extern "C" int64_t mf_camtrack_workspace_bytes(int32_t B, int32_t height, int32_t width, int32_t levels,
                                               int32_t which) {
  if (bad_shape(B, height, width, levels) || (which != MF_CAMTRACK_PYRAMID && which != MF_CAMTRACK_ALIGN))
    return bad("mf_camtrack_workspace_bytes: 1..MF_CAMTRACK_MAX_BATCH images within the caps, 1..8 levels, the "
               "coarsest at least 8 x 8, which = MF_CAMTRACK_PYRAMID or _ALIGN");
  if (which == MF_CAMTRACK_PYRAMID) return layout_of(B, height, width, levels, 1.0, 1.0, 0.0, 0.0).bytes;
  return workspace_of(B, height, width).bytes;
}

extern "C" int mf_camtrack_prepare(const float *depth, int32_t B, int32_t height, int32_t width, int32_t levels,
                                   double fx, double fy, double cx, double cy, double block_band, void *pyramid,
                                   mfStream_t stream) {
  if (bad_shape(B, height, width, levels) || !(fx != 0.0) || !(fy != 0.0) || !(block_band >= 0.0))
    return bad("mf_camtrack_prepare: 1..MF_CAMTRACK_MAX_BATCH images within the caps, 1..8 levels, the coarsest at "
               "least 8 x 8, fx, fy != 0, block_band >= 0");
  if (!depth || !pyramid) return bad("mf_camtrack_prepare: null depth or pyramid");
  const Layout lay = layout_of(B, height, width, levels, fx, fy, cx, cy);
  char *base = (char *)pyramid;
  int32_t *rect = (int32_t *)(base + lay.rect);
  for (int l = 0; l < levels; ++l) {
    const Level &v = lay.level[l];
    const int64_t n = (int64_t)B * v.H * v.W;
    const unsigned blocks = (unsigned)((n + kThreads - 1) / kThreads);
    float *d = (float *)(base + v.depth);
    double *vert = (double *)(base + v.vertex);
    if (l == 0) {
      hipLaunchKernelGGL(k_ct_level0, dim3(blocks), dim3(kThreads), 0, (hipStream_t)stream, depth, (int)B, v.H, v.W,
                         (int)levels, v.fx, v.fy, v.cx, v.cy, d, vert, rect);
      if (int rc = mf::check_launch("mf_camtrack_prepare (level 0)")) return rc;
    } else {
      const Level &u = lay.level[l - 1];
      hipLaunchKernelGGL(k_ct_down, dim3(blocks), dim3(kThreads), 0, (hipStream_t)stream,
                         (const float *)(base + u.depth), (int)B, u.H, u.W, v.H, v.W, block_band, v.fx, v.fy, v.cx,
                         v.cy, d, vert);
      if (int rc = mf::check_launch("mf_camtrack_prepare (down)")) return rc;
    }
    if (int rc = mf_pick_normals(vert, rect + 4 * (int64_t)l * B, B, v.H, v.W, (double *)(base + v.normal), stream))
      return rc;
  }
  return 0;
}

extern "C" int mf_camtrack_align(const void *current, const void *reference, int32_t B, int32_t height,
                                 int32_t width, int32_t levels, double fx, double fy, double cx, double cy,
                                 const double *T_ref_to_map, const double *T_init, const int32_t *iterations,
                                 double distance_threshold, double cos_angle_threshold, int32_t min_pairs,
                                 double *pose, double *T_cur_to_map, int32_t *status, double *stats, void *workspace,
                                 mfStream_t stream) {
  if (bad_shape(B, height, width, levels) || !(fx != 0.0) || !(fy != 0.0) || !iterations ||
      !(distance_threshold >= 0.0) || !(cos_angle_threshold >= -1.0 && cos_angle_threshold <= 1.0) || min_pairs < 0)
    return bad("mf_camtrack_align: 1..MF_CAMTRACK_MAX_BATCH images within the caps, 1..8 levels, the coarsest at "
               "least 8 x 8, fx, fy != 0, iterations given, distance_threshold >= 0, |cos_angle_threshold| <= 1, "
               "min_pairs >= 0");
  int64_t n_iters = 0;
  for (int l = 0; l < levels; ++l) {
    if (iterations[l] < 0 || iterations[l] > MF_CAMTRACK_MAX_ITERATIONS)
      return bad("mf_camtrack_align: iteration counts in 0..MF_CAMTRACK_MAX_ITERATIONS");
    n_iters += iterations[l];
  }
  if (n_iters > MF_CAMTRACK_MAX_ITERATIONS) return bad("mf_camtrack_align: more than MF_CAMTRACK_MAX_ITERATIONS");
  if (!current || !reference || !T_ref_to_map || !T_init || !pose || !T_cur_to_map || !status || !workspace ||
      (n_iters && !stats))
    return bad("mf_camtrack_align: null array");
  const Layout lay = layout_of(B, height, width, levels, fx, fy, cx, cy);
  const Workspace ws = workspace_of(B, height, width);
  char *w = (char *)workspace;
  double *pose0 = (double *)(w + ws.pose0), *cur = (double *)(w + ws.cur), *ref_inv = (double *)(w + ws.ref_inv);
  double *partial = (double *)(w + ws.partial);
  if (n_iters)
    if (int rc = mf::fill_bytes(stats, 0, 8 * 3 * n_iters * B, (hipStream_t)stream)) return rc;
  hipLaunchKernelGGL(k_ct_start, dim3((unsigned)((B + kThreads - 1) / kThreads)), dim3(kThreads), 0,
                     (hipStream_t)stream, T_ref_to_map, T_init, (int)B, pose, pose0, cur, ref_inv, T_cur_to_map,
                     status);
  if (int rc = mf::check_launch("mf_camtrack_align (start)")) return rc;
  const char *pc = (const char *)current, *pr = (const char *)reference;
  int it = 0;
  for (int l = levels - 1; l >= 0; --l) {
    const Level &v = lay.level[l];
    const int groups = (int)groups_of(v.H, v.W);
    for (int k = 0; k < iterations[levels - 1 - l]; ++k, ++it) {
      hipLaunchKernelGGL(k_ct_residual, dim3((unsigned)groups, (unsigned)B), dim3(kThreads), 0, (hipStream_t)stream,
                         (const double *)(pc + v.vertex), (const double *)(pc + v.normal),
                         (const double *)(pr + v.vertex), (const double *)(pr + v.normal), v.H, v.W, v.fx, v.fy, v.cx,
                         v.cy, T_ref_to_map, (const double *)cur, (const double *)ref_inv, (const int32_t *)status,
                         distance_threshold, cos_angle_threshold, groups, partial);
      if (int rc = mf::check_launch("mf_camtrack_align (residuals)")) return rc;
      hipLaunchKernelGGL(k_ct_solve, dim3((unsigned)B), dim3(kThreads), 0, (hipStream_t)stream,
                         (const double *)partial, groups, groups, (int)min_pairs, it, (int)n_iters, pose,
                         (const double *)pose0, cur, T_cur_to_map, status, stats);
      if (int rc = mf::check_launch("mf_camtrack_align (solve)")) return rc;
    }
  }
  return 0;
}
