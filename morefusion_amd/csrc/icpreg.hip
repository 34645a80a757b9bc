// Point-to-point ICP registration (contrib/icp_registration.py) -- gfx950, float64 throughout.
//
// Reference: morefusion/contrib/icp_registration.py (open3d's voxel_down_sample + registration_icp with
// TransformationEstimationPointToPoint(False)).  open3d is restated, not linked; DESIGN.md "ICP registration"
// has the contract, tests/icpreg_ref.py the NumPy mirror this file is pinned to bit for bit.
//
// Sets are ragged packed float64 [n, 3] arrays with int64 [n_sets + 1] row offsets.
//   k_icpreg_bounds   one workgroup per set: min / max of the non-NaN points (exact, order-free) ->
//                     vmin = min - 0.5 v and the voxel extents {nx, ny, nz, n_valid}; the host reads the
//                     extents back (the batch's one readback) to size the dense voxel boxes.
//   k_icpreg_prepare  one workgroup per set: voxel counts (int atomics), exclusive scan in box order,
//                     scatter of point indices, then one lane per non-empty voxel sorts its indices and sums
//                     the points in input order (float64, sequential) / count.  Box order is (i, j, k)
//                     lexicographic, so the compaction IS the output order.  Target sets are binned in the
//                     same launch into a uniform grid (cell >= r), each cell's indices ascending.
//   k_icpreg_run      one workgroup (256 lanes) per object runs every ICP iteration in one launch.
// Reduction order (part of the contract): lane k sums source rows k, k + 256, ... in order; then the 256
// partials are folded by a stride-halving tree (stride 128, 64, ..., 1: p[k] += p[k + s]).  Lane 0 solves
// the 3 x 3 problem (one-sided Jacobi SVD), composes the transforms and tests convergence; results go to
// the other lanes through LDS.  No float atomics anywhere: every result is bitwise reproducible.
#include <float.h>
#include <limits.h>
#include <math.h>

#include <algorithm>

#include "mf_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kJacobiSweeps = 32;
constexpr double kJacobiTol = 1e-15;    // skip a rotation when |gamma| <= tol * sqrt(alpha * beta)
constexpr double kRankTol = 1e-13;      // singular value <= tol * largest: completed from the others
constexpr double kConvTol = 1e-6;       // ICPConvergenceCriteria's relative_fitness / relative_rmse

__device__ __forceinline__ bool load_valid(const double *p, int64_t i, double &x, double &y, double &z) {
  x = p[3 * i];
  y = p[3 * i + 1];
  z = p[3 * i + 2];
  return !(isnan(x) || isnan(y) || isnan(z));
}

// 256-lane inclusive scan of two ints in LDS (Hillis-Steele); every lane calls it
__device__ void block_scan2(int &a, int &b, int *s_a, int *s_b) {
  const int t = threadIdx.x;
  s_a[t] = a;
  s_b[t] = b;
  __syncthreads();
  for (int off = 1; off < kThreads; off <<= 1) {
    const int xa = t >= off ? s_a[t - off] : 0;
    const int xb = t >= off ? s_b[t - off] : 0;
    __syncthreads();
    s_a[t] += xa;
    s_b[t] += xb;
    __syncthreads();
  }
  a = s_a[t];
  b = s_b[t];
}

__device__ __forceinline__ int64_t voxel_cell(double x, double y, double z, const double *vmin, double v, const int *n) {
  int i[3];
  const double c[3] = {x, y, z};
  for (int a = 0; a < 3; ++a) {
    double f = floor((c[a] - vmin[a]) / v);
    f = f < 0.0 ? 0.0 : (f > (double)(n[a] - 1) ? (double)(n[a] - 1) : f);  // never taken: vmin / extents bound every point
    i[a] = (int)f;
  }
  return ((int64_t)i[0] * n[1] + i[1]) * n[2] + i[2];
}

__device__ __forceinline__ int grid_coord(double c, double o, double cell, int g) {
  double f = floor((c - o) / cell);
  f = f < 0.0 ? 0.0 : (f > (double)(g - 1) ? (double)(g - 1) : f);
  return (int)f;
}

// insertion sort of a few int32 in global memory (one lane)
__device__ void sort_small(int32_t *a, int n) {
  for (int i = 1; i < n; ++i) {
    const int32_t v = a[i];
    int j = i - 1;
    while (j >= 0 && a[j] > v) {
      a[j + 1] = a[j];
      --j;
    }
    a[j + 1] = v;
  }
}

// counts -> exclusive starts [cells + 1] (and the rank of every non-empty cell), chunked over the box.
// `cnt` was filled with int atomics in this launch: it is read back with atomics, never through the cache.
__device__ void scan_cells(int32_t *cnt, int64_t cells, int32_t *start, int32_t *rank, int *s_a, int *s_b, int &n_nonempty) {
  int carry = 0, carry_r = 0;
  for (int64_t base = 0; base < cells; base += kThreads) {  // uniform trip count
    const int64_t c = base + threadIdx.x;
    int v = c < cells ? atomicAdd(&cnt[c], 0) : 0;
    int ne = v > 0 ? 1 : 0;
    int iv = v, ine = ne;
    block_scan2(iv, ine, s_a, s_b);
    if (c < cells) {
      start[c] = carry + iv - v;
      if (rank) rank[c] = carry_r + ine - ne;
    }
    const int tot = s_a[kThreads - 1], tot_r = s_b[kThreads - 1];
    __syncthreads();
    carry += tot;
    carry_r += tot_r;
  }
  if (threadIdx.x == 0) start[cells] = carry;
  n_nonempty = carry_r;
}

__global__ __launch_bounds__(kThreads) void k_icpreg_bounds(const double *__restrict__ pts, const int64_t *__restrict__ off,
                                                            double v, double *vmin, int32_t *ext) {
  __shared__ double s_mn[3][kThreads], s_mx[3][kThreads];
  __shared__ int s_n[kThreads];
  const int b = blockIdx.x, t = threadIdx.x;
  double mn[3] = {DBL_MAX, DBL_MAX, DBL_MAX}, mx[3] = {-DBL_MAX, -DBL_MAX, -DBL_MAX};
  int nv = 0;
  for (int64_t i = off[b] + t; i < off[b + 1]; i += kThreads) {
    double c[3];
    if (!load_valid(pts, i, c[0], c[1], c[2])) continue;
    ++nv;
    for (int a = 0; a < 3; ++a) {
      mn[a] = c[a] < mn[a] ? c[a] : mn[a];
      mx[a] = c[a] > mx[a] ? c[a] : mx[a];
    }
  }
  for (int a = 0; a < 3; ++a) {
    s_mn[a][t] = mn[a];
    s_mx[a][t] = mx[a];
  }
  s_n[t] = nv;
  __syncthreads();
  for (int s = kThreads / 2; s > 0; s >>= 1) {
    if (t < s) {
      for (int a = 0; a < 3; ++a) {
        s_mn[a][t] = s_mn[a][t + s] < s_mn[a][t] ? s_mn[a][t + s] : s_mn[a][t];
        s_mx[a][t] = s_mx[a][t + s] > s_mx[a][t] ? s_mx[a][t + s] : s_mx[a][t];
      }
      s_n[t] += s_n[t + s];
    }
    __syncthreads();
  }
  if (t == 0) {
    int e[3] = {0, 0, 0};
    for (int a = 0; a < 3; ++a) {
      const double lo = s_n[0] > 0 ? s_mn[a][0] - v * 0.5 : 0.0;  // open3d: min_bound - voxel_size * 0.5
      vmin[3 * b + a] = lo;
      if (s_n[0] > 0) {
        const double f = floor((s_mx[a][0] - lo) / v) + 1.0;
        e[a] = f < (double)(1 << 30) ? (int)f : -1;  // -1: refused by the host
      }
    }
    for (int a = 0; a < 3; ++a) ext[4 * b + a] = e[a];
    ext[4 * b + 3] = s_n[0];
  }
}

struct PrepArgs {
  const double *pts;
  const int64_t *off;
  const double *vmin;
  const int32_t *ext;
  const int64_t *box_off;   // [n_sets + 1] voxel cells
  const int64_t *grid_off;  // [n_sets + 1] grid_start entries (G + 1 per gridded set, 0 otherwise)
  const int32_t *grid_dim;  // [n_sets, 3]
  int32_t *zeroed;          // cnt | cursor over the boxes, then gcnt | gcursor over the grids (all zero on entry)
  int32_t *start, *rank, *pidx;
  double *out;
  int32_t *out_cnt;
  double *grid_origin;
  int32_t *grid_start, *grid_idx;
  int64_t total_cells, total_grid;
  double v, cell;
};

__global__ __launch_bounds__(kThreads) void k_icpreg_prepare(PrepArgs A) {
  __shared__ int s_a[kThreads], s_b[kThreads];
  const int b = blockIdx.x;
  const int64_t p0 = A.off[b], np = A.off[b + 1] - p0;
  const int n[3] = {A.ext[4 * b], A.ext[4 * b + 1], A.ext[4 * b + 2]};
  const int64_t cells = A.box_off[b + 1] - A.box_off[b];
  const double vmin[3] = {A.vmin[3 * b], A.vmin[3 * b + 1], A.vmin[3 * b + 2]};
  int n_out = 0;
  if (cells > 0) {
    int32_t *cnt = A.zeroed + A.box_off[b];
    int32_t *cursor = A.zeroed + A.total_cells + A.box_off[b];
    int32_t *start = A.start + A.box_off[b] + b;  // cells + 1 entries per set
    int32_t *rank = A.rank + A.box_off[b];
    int32_t *pidx = A.pidx + p0;
    for (int64_t i = threadIdx.x; i < np; i += kThreads) {
      double x, y, z;
      if (load_valid(A.pts, p0 + i, x, y, z)) atomicAdd(&cnt[voxel_cell(x, y, z, vmin, A.v, n)], 1);
    }
    __syncthreads();
    scan_cells(cnt, cells, start, rank, s_a, s_b, n_out);
    __syncthreads();
    for (int64_t i = threadIdx.x; i < np; i += kThreads) {
      double x, y, z;
      if (!load_valid(A.pts, p0 + i, x, y, z)) continue;
      const int64_t c = voxel_cell(x, y, z, vmin, A.v, n);
      pidx[start[c] + atomicAdd(&cursor[c], 1)] = (int32_t)i;
    }
    __syncthreads();
    for (int64_t c = threadIdx.x; c < cells; c += kThreads) {
      const int s = start[c], m = start[c + 1] - s;
      if (m == 0) continue;
      sort_small(pidx + s, m);  // input order
      double sx = 0.0, sy = 0.0, sz = 0.0;
      for (int k = 0; k < m; ++k) {
        const int64_t i = p0 + pidx[s + k];
        sx += A.pts[3 * i];
        sy += A.pts[3 * i + 1];
        sz += A.pts[3 * i + 2];
      }
      const double dm = (double)m;
      double *o = A.out + 3 * (p0 + rank[c]);
      o[0] = sx / dm;
      o[1] = sy / dm;
      o[2] = sz / dm;
    }
  }
  if (threadIdx.x == 0) A.out_cnt[b] = n_out;
  const int64_t gcells1 = A.grid_off[b + 1] - A.grid_off[b];
  if (gcells1 <= 0) return;  // not a target set (uniform over the workgroup)
  __syncthreads();
  // the down-sampled set (written above by this workgroup) into the uniform grid: origin vmin - cell
  const int g[3] = {A.grid_dim[3 * b], A.grid_dim[3 * b + 1], A.grid_dim[3 * b + 2]};
  const double go[3] = {vmin[0] - A.cell, vmin[1] - A.cell, vmin[2] - A.cell};
  if (threadIdx.x < 3) A.grid_origin[3 * b + threadIdx.x] = go[threadIdx.x];
  const int64_t gcells = gcells1 - 1;
  int32_t *gcnt = A.zeroed + 2 * A.total_cells + A.grid_off[b];
  int32_t *gcursor = A.zeroed + 2 * A.total_cells + A.total_grid + A.grid_off[b];
  int32_t *gstart = A.grid_start + A.grid_off[b];
  int32_t *gidx = A.grid_idx + p0;
  const double *q = A.out + 3 * p0;
  auto gcell = [&](int j) -> int64_t {
    const int ix = grid_coord(q[3 * j], go[0], A.cell, g[0]), iy = grid_coord(q[3 * j + 1], go[1], A.cell, g[1]),
              iz = grid_coord(q[3 * j + 2], go[2], A.cell, g[2]);
    return ((int64_t)ix * g[1] + iy) * g[2] + iz;
  };
  for (int j = threadIdx.x; j < n_out; j += kThreads) atomicAdd(&gcnt[gcell(j)], 1);
  __syncthreads();
  int unused;
  scan_cells(gcnt, gcells, gstart, nullptr, s_a, s_b, unused);
  __syncthreads();
  for (int j = threadIdx.x; j < n_out; j += kThreads) {
    const int64_t c = gcell(j);
    gidx[gstart[c] + atomicAdd(&gcursor[c], 1)] = j;
  }
  __syncthreads();
  for (int64_t c = threadIdx.x; c < gcells; c += kThreads) sort_small(gidx + gstart[c], gstart[c + 1] - gstart[c]);
}

// ---- 4 x 4 and 3 x 3 algebra (lane 0; tests/icpreg_ref.py mirrors every operation in the same order) -------------

// general 4 x 4 inverse by 2 x 2 minors (row-major)
__device__ void inv4(const double *a, double *o) {
  const double s0 = a[0] * a[5] - a[4] * a[1];
  const double s1 = a[0] * a[6] - a[4] * a[2];
  const double s2 = a[0] * a[7] - a[4] * a[3];
  const double s3 = a[1] * a[6] - a[5] * a[2];
  const double s4 = a[1] * a[7] - a[5] * a[3];
  const double s5 = a[2] * a[7] - a[6] * a[3];
  const double c5 = a[10] * a[15] - a[14] * a[11];
  const double c4 = a[9] * a[15] - a[13] * a[11];
  const double c3 = a[9] * a[14] - a[13] * a[10];
  const double c2 = a[8] * a[15] - a[12] * a[11];
  const double c1 = a[8] * a[14] - a[12] * a[10];
  const double c0 = a[8] * a[13] - a[12] * a[9];
  const double det = s0 * c5 - s1 * c4 + s2 * c3 + s3 * c2 - s4 * c1 + s5 * c0;
  const double id = 1.0 / det;
  o[0] = (a[5] * c5 - a[6] * c4 + a[7] * c3) * id;
  o[1] = (-a[1] * c5 + a[2] * c4 - a[3] * c3) * id;
  o[2] = (a[13] * s5 - a[14] * s4 + a[15] * s3) * id;
  o[3] = (-a[9] * s5 + a[10] * s4 - a[11] * s3) * id;
  o[4] = (-a[4] * c5 + a[6] * c2 - a[7] * c1) * id;
  o[5] = (a[0] * c5 - a[2] * c2 + a[3] * c1) * id;
  o[6] = (-a[12] * s5 + a[14] * s2 - a[15] * s1) * id;
  o[7] = (a[8] * s5 - a[10] * s2 + a[11] * s1) * id;
  o[8] = (a[4] * c4 - a[5] * c2 + a[7] * c0) * id;
  o[9] = (-a[0] * c4 + a[1] * c2 - a[3] * c0) * id;
  o[10] = (a[12] * s4 - a[13] * s2 + a[15] * s0) * id;
  o[11] = (-a[8] * s4 + a[9] * s2 - a[11] * s0) * id;
  o[12] = (-a[4] * c3 + a[5] * c1 - a[6] * c0) * id;
  o[13] = (a[0] * c3 - a[1] * c1 + a[2] * c0) * id;
  o[14] = (-a[12] * s3 + a[13] * s1 - a[14] * s0) * id;
  o[15] = (a[8] * s3 - a[9] * s1 + a[10] * s0) * id;
}

// o = a * b (4 x 4, row-major); o may alias b
__device__ void mul4(const double *a, const double *b, double *o) {
  double r[16];
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j)
      r[4 * i + j] = ((a[4 * i] * b[j] + a[4 * i + 1] * b[4 + j]) + a[4 * i + 2] * b[8 + j]) + a[4 * i + 3] * b[12 + j];
  for (int k = 0; k < 16; ++k) o[k] = r[k];
}

__device__ __forceinline__ double det3(const double *m) {  // row-major 3 x 3
  return (m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6])) + m[2] * (m[3] * m[7] - m[4] * m[6]);
}

// Eigen::umeyama(src, dst, false) from the covariance sigma = (1/n) sum (t - mt)(s - ms)^T (row-major) and the
// means: one-sided Jacobi SVD of sigma, singular values descending, reflection fix on the smallest.
__device__ void umeyama(const double *sig, const double *ms, const double *mt, double *upd) {
  double a[9], v[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
  for (int k = 0; k < 9; ++k) a[k] = sig[k];
  const int P[3] = {0, 0, 1}, Q[3] = {1, 2, 2};
  for (int sweep = 0; sweep < kJacobiSweeps; ++sweep) {
    bool rotated = false;
    for (int r = 0; r < 3; ++r) {
      const int p = P[r], q = Q[r];
      const double alpha = (a[p] * a[p] + a[3 + p] * a[3 + p]) + a[6 + p] * a[6 + p];
      const double beta = (a[q] * a[q] + a[3 + q] * a[3 + q]) + a[6 + q] * a[6 + q];
      const double gamma = (a[p] * a[q] + a[3 + p] * a[3 + q]) + a[6 + p] * a[6 + q];
      if (!(fabs(gamma) > kJacobiTol * sqrt(alpha * beta))) continue;
      rotated = true;
      const double zeta = (beta - alpha) / (2.0 * gamma);
      const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
      const double c = 1.0 / sqrt(1.0 + t * t);
      const double s = c * t;
      for (int i = 0; i < 3; ++i) {
        const double x = a[3 * i + p], y = a[3 * i + q];
        a[3 * i + p] = c * x - s * y;
        a[3 * i + q] = s * x + c * y;
        const double vx = v[3 * i + p], vy = v[3 * i + q];
        v[3 * i + p] = c * vx - s * vy;
        v[3 * i + q] = s * vx + c * vy;
      }
    }
    if (!rotated) break;
  }
  double sv[3];
  for (int j = 0; j < 3; ++j) sv[j] = sqrt((a[j] * a[j] + a[3 + j] * a[3 + j]) + a[6 + j] * a[6 + j]);
  int ord[3] = {0, 1, 2};
  if (sv[ord[1]] > sv[ord[0]]) { const int x = ord[0]; ord[0] = ord[1]; ord[1] = x; }
  if (sv[ord[2]] > sv[ord[1]]) { const int x = ord[1]; ord[1] = ord[2]; ord[2] = x; }
  if (sv[ord[1]] > sv[ord[0]]) { const int x = ord[0]; ord[0] = ord[1]; ord[1] = x; }
  double U[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, V[9];
  for (int k = 0; k < 3; ++k)
    for (int i = 0; i < 3; ++i) V[3 * i + k] = v[3 * i + ord[k]];
  const double smax = sv[ord[0]];
  int rank = 0;
  if (smax > 0.0)
    for (int k = 0; k < 3; ++k)
      if (sv[ord[k]] > kRankTol * smax) rank = k + 1;
  for (int k = 0; k < rank; ++k)
    for (int i = 0; i < 3; ++i) U[3 * i + k] = a[3 * i + ord[k]] / sv[ord[k]];
  if (rank == 1) {  // u1: the axis least aligned with u0, orthogonalised
    int e = 0;
    if (fabs(U[3]) < fabs(U[3 * e])) e = 1;
    if (fabs(U[6]) < fabs(U[3 * e])) e = 2;
    double w[3];
    for (int i = 0; i < 3; ++i) w[i] = (i == e ? 1.0 : 0.0) - U[3 * e] * U[3 * i];
    const double nw = sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]);
    for (int i = 0; i < 3; ++i) U[3 * i + 1] = w[i] / nw;
  }
  if (rank >= 1 && rank <= 2) {  // u2 = u0 x u1
    U[2] = U[3] * U[7] - U[6] * U[4];
    U[5] = U[6] * U[1] - U[0] * U[7];
    U[8] = U[0] * U[4] - U[3] * U[1];
  }
  const double sgn = det3(U) * det3(V) < 0.0 ? -1.0 : 1.0;
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j)
      upd[4 * i + j] = (U[3 * i] * V[3 * j] + U[3 * i + 1] * V[3 * j + 1]) + (U[3 * i + 2] * sgn) * V[3 * j + 2];
  }
  for (int i = 0; i < 3; ++i)
    upd[4 * i + 3] = mt[i] - ((upd[4 * i] * ms[0] + upd[4 * i + 1] * ms[1]) + upd[4 * i + 2] * ms[2]);
  upd[12] = 0.0;
  upd[13] = 0.0;
  upd[14] = 0.0;
  upd[15] = 1.0;
}

__device__ __forceinline__ void xform(const double *m, double x, double y, double z, double *o) {
  // open3d's TransformPoints: (M * [p, 1]).head<3>() / w
  const double w = ((m[12] * x + m[13] * y) + m[14] * z) + m[15];
  for (int a = 0; a < 3; ++a) o[a] = (((m[4 * a] * x + m[4 * a + 1] * y) + m[4 * a + 2] * z) + m[4 * a + 3]) / w;
}

// fold the 256 partials of `n` components (component-major in s) with the stride-halving tree; all lanes call it
__device__ void tree_fold(double *s, int n) {
  for (int st = kThreads / 2; st > 0; st >>= 1) {
    if ((int)threadIdx.x < st)
      for (int c = 0; c < n; ++c) s[c * kThreads + threadIdx.x] += s[c * kThreads + threadIdx.x + st];
    __syncthreads();
  }
}

__device__ __forceinline__ void tree_fold_int(int *s) {
  for (int st = kThreads / 2; st > 0; st >>= 1) {
    if ((int)threadIdx.x < st) s[threadIdx.x] += s[threadIdx.x + st];
    __syncthreads();
  }
}

struct RunShared {
  double red[9 * kThreads];
  int cnt[kThreads];
  double M[16];    // matrix the next pass A applies
  double T[16];    // current transformation (depth -> cad)
  double X[16];    // current transform (cad -> cam), iterative mode
  double mean[6];  // ms, mt of the last pass A
  double fit, rmse;
  int n_corr, stop;
};

__global__ __launch_bounds__(kThreads) void k_icpreg_run(mfIcpRegBatch P) {
  __shared__ RunShared S;
  const int b = blockIdx.x, t = threadIdx.x;
  const double *init = P.transform_init + 16 * b;
  const int H = P.max_iter + 1;
  if (P.active && !P.active[b]) {  // skipped: the pose passes through
    if (t < 16) {
      P.transform[16 * b + t] = init[t];
      if (P.hist_transform)
        for (int k = 0; k < H; ++k) P.hist_transform[((int64_t)b * H + k) * 16 + t] = init[t];
    }
    if (t == 0) {
      inv4(init, P.transformation + 16 * b);
      P.fitness[b] = 0.0;
      P.inlier_rmse[b] = 0.0;
      P.n_iter[b] = 0;
      if (P.hist_fitness)
        for (int k = 0; k < H; ++k) {
          P.hist_fitness[(int64_t)b * H + k] = 0.0;
          P.hist_rmse[(int64_t)b * H + k] = 0.0;
        }
    }
    return;
  }
  const int64_t s0 = P.src_off[b], t0 = P.tgt_off[b];
  const int ns = P.src_cnt[b];
  const double *src = P.src + 3 * s0;
  double *cur = P.cur + 3 * s0;
  int32_t *corr = P.corr + s0;
  const double *tgt = P.tgt + 3 * t0;
  const int32_t *gidx = P.grid_idx + t0;
  const int32_t *gstart = P.grid_start + P.grid_off[b];
  const int g[3] = {P.grid_dim[3 * b], P.grid_dim[3 * b + 1], P.grid_dim[3 * b + 2]};
  const double go[3] = {P.grid_origin[3 * b], P.grid_origin[3 * b + 1], P.grid_origin[3 * b + 2]};
  const double r2 = P.max_corr_dist * P.max_corr_dist;
  const bool gridded = g[0] > 0 && g[1] > 0 && g[2] > 0 && P.tgt_cnt[b] > 0;

  // pass A: cur := S.M applied to (fresh ? src : cur); nearest target within r; partial sums -> S.mean, S.fit, S.rmse
  auto pass_a = [&](bool fresh) {
    double acc[7] = {0, 0, 0, 0, 0, 0, 0};  // d2, s xyz, t xyz
    int n = 0;
    for (int i = t; i < ns; i += kThreads) {
      const double *p = fresh ? src + 3 * i : cur + 3 * i;
      double q[3];
      xform(S.M, p[0], p[1], p[2], q);
      cur[3 * i] = q[0];
      cur[3 * i + 1] = q[1];
      cur[3 * i + 2] = q[2];
      int best = -1;
      double bd = r2;
      if (gridded) {
        int lo[3], hi[3];
        for (int a = 0; a < 3; ++a) {
          double f = floor((q[a] - go[a]) / P.cell);
          f = f < -2.0 ? -2.0 : (f > (double)g[a] + 1.0 ? (double)g[a] + 1.0 : f);
          lo[a] = std::max((int)f - 1, 0);
          hi[a] = std::min((int)f + 1, g[a] - 1);
        }
        for (int ix = lo[0]; ix <= hi[0]; ++ix)
          for (int iy = lo[1]; iy <= hi[1]; ++iy)
            for (int iz = lo[2]; iz <= hi[2]; ++iz) {
              const int64_t c = ((int64_t)ix * g[1] + iy) * g[2] + iz;
              for (int k = gstart[c]; k < gstart[c + 1]; ++k) {
                const int j = gidx[k];
                const double dx = q[0] - tgt[3 * j], dy = q[1] - tgt[3 * j + 1], dz = q[2] - tgt[3 * j + 2];
                const double d2 = (dx * dx + dy * dy) + dz * dz;
                if (d2 < bd || (d2 == bd && best >= 0 && j < best)) {
                  bd = d2;
                  best = j;
                }
              }
            }
      }
      corr[i] = best;
      if (best >= 0) {
        ++n;
        acc[0] += bd;
        for (int a = 0; a < 3; ++a) {
          acc[1 + a] += q[a];
          acc[4 + a] += tgt[3 * best + a];
        }
      }
    }
    for (int c = 0; c < 7; ++c) S.red[c * kThreads + t] = acc[c];
    S.cnt[t] = n;
    __syncthreads();
    tree_fold(S.red, 7);
    tree_fold_int(S.cnt);
    if (t == 0) {
      const int nc = S.cnt[0];
      S.n_corr = nc;
      if (nc > 0) {
        const double inv_n = 1.0 / (double)nc;
        for (int a = 0; a < 6; ++a) S.mean[a] = S.red[(1 + a) * kThreads] * inv_n;
        S.fit = (double)nc / (double)ns;
        S.rmse = sqrt(S.red[0] / (double)nc);
      } else {
        S.fit = 0.0;
        S.rmse = 0.0;
      }
    }
    __syncthreads();
  };

  // pass B + solve: covariance over the stored correspondences -> S.M = update, S.T = update * S.T
  auto update = [&]() {
    const int nc = S.n_corr;  // uniform
    if (nc > 0) {
      double acc[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
      const double ms[3] = {S.mean[0], S.mean[1], S.mean[2]}, mt[3] = {S.mean[3], S.mean[4], S.mean[5]};
      for (int i = t; i < ns; i += kThreads) {
        const int j = corr[i];
        if (j < 0) continue;
        double ds[3], dt[3];
        for (int a = 0; a < 3; ++a) {
          ds[a] = cur[3 * i + a] - ms[a];
          dt[a] = tgt[3 * j + a] - mt[a];
        }
        for (int a = 0; a < 3; ++a)
          for (int c = 0; c < 3; ++c) acc[3 * a + c] += dt[a] * ds[c];
      }
      for (int c = 0; c < 9; ++c) S.red[c * kThreads + t] = acc[c];
      __syncthreads();
      tree_fold(S.red, 9);
    }
    if (t == 0) {
      double upd[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};  // no correspondences: identity
      if (nc > 0) {
        const double inv_n = 1.0 / (double)nc;
        double sig[9];
        for (int c = 0; c < 9; ++c) sig[c] = inv_n * S.red[c * kThreads];
        umeyama(sig, S.mean, S.mean + 3, upd);
      }
      for (int k = 0; k < 16; ++k) S.M[k] = upd[k];
      mul4(upd, S.T, S.T);
    }
    __syncthreads();
  };

  auto put_hist = [&](int k, const double *X) {  // lane 0
    if (!P.hist_transform) return;
    for (int e = 0; e < 16; ++e) P.hist_transform[((int64_t)b * H + k) * 16 + e] = X[e];
    P.hist_fitness[(int64_t)b * H + k] = S.fit;
    P.hist_rmse[(int64_t)b * H + k] = S.rmse;
  };

  int it = 0;
  if (P.mode == 0) {  // registration_icp(source, target, r, inverse(init), max_iteration = max_iter)
    if (t == 0) {
      inv4(init, S.T);
      for (int k = 0; k < 16; ++k) S.M[k] = S.T[k];
    }
    __syncthreads();
    pass_a(true);
    if (t == 0) put_hist(0, init);
    while (it < P.max_iter) {
      ++it;
      const double pf = S.fit, pr = S.rmse;  // read before the lanes pass the barriers of update()
      update();
      pass_a(false);
      if (t == 0) {
        double X[16];
        inv4(S.T, X);
        put_hist(it, X);
        S.stop = fabs(pf - S.fit) < kConvTol && fabs(pr - S.rmse) < kConvTol;
      }
      __syncthreads();
      if (S.stop) break;
    }
    if (t == 0) {
      double X[16];
      inv4(S.T, X);
      for (int k = 0; k < 16; ++k) {
        P.transform[16 * b + k] = X[k];
        P.transformation[16 * b + k] = S.T[k];
      }
    }
  } else {  // register_iterative: per step a fresh registration_icp(init = inverse(X), max_iteration = 1)
    if (t == 0)
      for (int k = 0; k < 16; ++k) S.X[k] = init[k];
    __syncthreads();
    while (it < P.max_iter) {
      ++it;
      if (t == 0) {
        inv4(S.X, S.T);
        for (int k = 0; k < 16; ++k) S.M[k] = S.T[k];
      }
      __syncthreads();
      pass_a(true);
      if (t == 0 && it == 1) put_hist(0, init);  // the result at init
      update();
      pass_a(false);
      if (t == 0) {
        inv4(S.T, S.X);
        put_hist(it, S.X);
      }
      __syncthreads();
    }
    if (P.max_iter == 0) {  // no step: the result at init
      if (t == 0) {
        inv4(S.X, S.T);
        for (int k = 0; k < 16; ++k) S.M[k] = S.T[k];
      }
      __syncthreads();
      pass_a(true);
      if (t == 0) put_hist(0, init);
    }
    if (t == 0)
      for (int k = 0; k < 16; ++k) {
        P.transform[16 * b + k] = S.X[k];
        P.transformation[16 * b + k] = S.T[k];
      }
  }
  if (t == 0) {
    P.fitness[b] = S.fit;
    P.inlier_rmse[b] = S.rmse;
    P.n_iter[b] = it;
  }
  __syncthreads();
  if (P.hist_transform) {  // entries past the last iteration repeat the final one
    for (int k = it + 1 + t / 16; k < H; k += kThreads / 16) {
      P.hist_transform[((int64_t)b * H + k) * 16 + (t & 15)] = P.hist_transform[((int64_t)b * H + it) * 16 + (t & 15)];
      if ((t & 15) == 0) {
        P.hist_fitness[(int64_t)b * H + k] = S.fit;
        P.hist_rmse[(int64_t)b * H + k] = S.rmse;
      }
    }
  }
}

int bad(const char *what) {
  mf::set_last_error(hipErrorInvalidValue, what);
  return -(int)hipErrorInvalidValue;
}

}  // namespace

extern "C" int64_t mf_icpreg_workspace_bytes(int64_t total_cells, int64_t total_grid, int64_t n_points) {
  if (total_cells < 0 || total_grid < 0 || n_points < 0) return -1;
  if (total_cells > MF_ICPREG_MAX_CELLS || total_grid > MF_ICPREG_MAX_CELLS || n_points > INT_MAX) return -1;
  // zeroed: cnt | cursor (boxes), gcnt | gcursor (grids); then start (+1 per set, <= n_points sets), rank, pidx
  return 4 * (2 * total_cells + 2 * total_grid + (total_cells + n_points + 1) + total_cells + n_points);
}

extern "C" int mf_icpreg_bounds(const double *pts, const int64_t *off, int32_t n_sets, double voxel_size, double *vmin,
                                int32_t *ext, mfStream_t stream) {
  if (n_sets < 0 || n_sets > 65535) return bad("mf_icpreg_bounds: 0..65535 sets");
  if (!(voxel_size > 0.0)) return bad("mf_icpreg_bounds: voxel_size must be positive");
  if (n_sets == 0) return 0;
  hipLaunchKernelGGL(k_icpreg_bounds, dim3(n_sets), dim3(kThreads), 0, (hipStream_t)stream, pts, off, voxel_size, vmin,
                     ext);
  return mf::check_launch("mf_icpreg_bounds");
}

extern "C" int mf_icpreg_prepare(const double *pts, const int64_t *off, int32_t n_sets, double voxel_size,
                                 const double *vmin, const int32_t *ext, const int64_t *box_off, int64_t total_cells,
                                 const int64_t *grid_off, const int32_t *grid_dim, int64_t total_grid, double cell,
                                 int64_t n_points, void *workspace, double *out, int32_t *out_cnt, double *grid_origin,
                                 int32_t *grid_start, int32_t *grid_idx, mfStream_t stream) {
  if (n_sets < 0 || n_sets > 65535) return bad("mf_icpreg_prepare: 0..65535 sets");
  if (!(voxel_size > 0.0) || !(cell > 0.0)) return bad("mf_icpreg_prepare: voxel_size and cell must be positive");
  if (mf_icpreg_workspace_bytes(total_cells, total_grid, n_points) < 0)
    return bad("mf_icpreg_prepare: box cells past MF_ICPREG_MAX_CELLS");
  if (n_sets == 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  int32_t *w = (int32_t *)workspace;
  const int rc = mf::fill_bytes(w, 0, 4 * (2 * total_cells + 2 * total_grid), s);
  if (rc) return rc;
  PrepArgs A;
  A.pts = pts;
  A.off = off;
  A.vmin = vmin;
  A.ext = ext;
  A.box_off = box_off;
  A.grid_off = grid_off;
  A.grid_dim = grid_dim;
  A.zeroed = w;
  A.start = w + 2 * total_cells + 2 * total_grid;
  A.rank = A.start + total_cells + n_sets;
  A.pidx = A.rank + total_cells;
  A.out = out;
  A.out_cnt = out_cnt;
  A.grid_origin = grid_origin;
  A.grid_start = grid_start;
  A.grid_idx = grid_idx;
  A.total_cells = total_cells;
  A.total_grid = total_grid;
  A.v = voxel_size;
  A.cell = cell;
  hipLaunchKernelGGL(k_icpreg_prepare, dim3(n_sets), dim3(kThreads), 0, s, A);
  return mf::check_launch("mf_icpreg_prepare");
}

extern "C" int mf_icpreg_run(const mfIcpRegBatch *batch, mfStream_t stream) {
  if (!batch) return bad("mf_icpreg_run: no batch");
  const mfIcpRegBatch &P = *batch;
  if (P.n_objects < 0 || P.n_objects > 65535) return bad("mf_icpreg_run: 0..65535 objects");
  if (P.max_iter < 0) return bad("mf_icpreg_run: negative max_iter");
  if (P.mode != 0 && P.mode != 1) return bad("mf_icpreg_run: mode 0 (register) or 1 (register_iterative)");
  if (!(P.max_corr_dist > 0.0) || !(P.cell >= P.max_corr_dist)) return bad("mf_icpreg_run: need 0 < max_corr_dist <= cell");
  if ((P.hist_transform == nullptr) != (P.hist_fitness == nullptr) || (P.hist_fitness == nullptr) != (P.hist_rmse == nullptr))
    return bad("mf_icpreg_run: the three history arrays together");
  if (P.n_objects == 0) return 0;
  hipLaunchKernelGGL(k_icpreg_run, dim3(P.n_objects), dim3(kThreads), 0, (hipStream_t)stream, P);
  return mf::check_launch("mf_icpreg_run");
}
