// Pose metric: batched ADD and ADD-S of model clouds under two poses (metrics/average_distance_device.py) -- gfx950,
// float64.
//
// Reference: morefusion/metrics/average_distance.py:6-35 (one object at a time through a k-d tree on the host).  Here
// an item is (cloud, T1, T2); with a_j = T1 p_j and b_k = T2 p_k
//     add   = mean_j |a_j - b_j|          add_s = mean_j min_k |a_j - b_k|
// for every item of a call, clouds shared between items and of any lengths.  The search is exact brute force.
// DESIGN.md "Pose metric" has the contract and the bound, tests/posemetric_ref.py the NumPy mirror this file is pinned
// to bit for bit.
//
//   k_posemetric_dist    a workgroup per (item, 256 queries), 128 lanes with two queries each (j and j + 128): a target
//                        tile of 256 points is transformed once by the workgroup into LDS (x y z and a pad: two 16-byte
//                        reads per target, the same address in every lane), every lane keeps the running minimum of the
//                        squared distance of its queries in registers.  |a_j - b_j| and sqrt(min) go to the workspace.
//   k_posemetric_mean    a workgroup of 256 lanes per item: the two means in the fixed order below.
//
// The arithmetic (nothing is contracted: -ffp-contract=off; divide and sqrt are IEEE):
//   transform   x' = ((R00 x + R01 y) + R02 z) + tx, rows y and z likewise; without `translate` the + t is dropped
//   distance^2  (dx dx + dy dy) + dz dz; ADD-S takes the minimum of the squares, then one sqrt
//   mean        lane l of 256 adds the distances of the points j = l, l + 256, ... in increasing j; the partial sums
//               are folded by s[l] += s[l + h] for h = 128, 64, ... 1; the result is divided by P.  The order depends
//               on P alone.
// An item whose cloud index is outside 0 .. n_clouds - 1, or whose cloud is empty or longer than max_points, reads and
// writes nothing in the workspace and gets NaN (the Python layer raises for these before the launch).
#include <math.h>

#include "mf_common.h"

namespace {

constexpr int kQueries = 256;  // queries of a workgroup = targets of a tile = lanes of the mean
constexpr int kLanes = 128;    // lanes of k_posemetric_dist: two queries each

struct Pose {  // the upper 3 x 4 of a row-major 4 x 4
  double r[3][3], t[3];
};

__device__ __forceinline__ Pose load_pose(const double *T) {
  Pose p;
  for (int a = 0; a < 3; ++a) {
    for (int b = 0; b < 3; ++b) p.r[a][b] = T[4 * a + b];
    p.t[a] = T[4 * a + 3];
  }
  return p;
}

__device__ __forceinline__ void apply(const Pose &T, const double *p, bool translate, double *out) {
  for (int a = 0; a < 3; ++a) {
    const double v = (T.r[a][0] * p[0] + T.r[a][1] * p[1]) + T.r[a][2] * p[2];
    out[a] = translate ? v + T.t[a] : v;
  }
}

// the cloud of an item: its first point and its length, 0 for an item that cannot be scored
__device__ __forceinline__ int item_points(const int32_t *cloud_off, const int32_t *item_cloud, int item, int n_clouds,
                                           int max_points, int *first) {
  const int c = item_cloud[item];
  if (c < 0 || c >= n_clouds) return 0;
  const int lo = cloud_off[c], P = cloud_off[c + 1] - lo;
  *first = lo;
  return (lo < 0 || P < 1 || P > max_points) ? 0 : P;
}

__global__ void __launch_bounds__(kLanes) k_posemetric_dist(const double *__restrict__ points,
                                                            const int32_t *__restrict__ cloud_off,
                                                            const int32_t *__restrict__ item_cloud,
                                                            const double *__restrict__ T1,
                                                            const double *__restrict__ T2, int n_clouds,
                                                            int max_points, int translate,
                                                            double *__restrict__ dist) {
  __shared__ __attribute__((aligned(16))) double s_b[kQueries][4];
  const int item = blockIdx.y, t = threadIdx.x;
  int first = 0;
  const int P = item_points(cloud_off, item_cloud, item, n_clouds, max_points, &first);  // (uniform)
  const int q0 = blockIdx.x * kQueries;
  if (q0 >= P) return;
  const double *cloud = points + 3 * (int64_t)first;
  const Pose A = load_pose(T1 + 16 * (int64_t)item), B = load_pose(T2 + 16 * (int64_t)item);
  const bool tr = translate != 0;
  double a[2][3], best[2];
  bool live[2];
  for (int u = 0; u < 2; ++u) {
    const int j = q0 + t + u * kLanes;
    live[u] = j < P;
    const double *p = cloud + 3 * (int64_t)(live[u] ? j : q0);  // (a lane without a query follows the first one)
    apply(A, p, tr, a[u]);
    best[u] = INFINITY;
  }
  for (int k0 = 0; k0 < P; k0 += kQueries) {
    const int count = min(kQueries, P - k0);
    for (int u = 0; u < 2; ++u) {
      const int k = t + u * kLanes;
      if (k < count) {
        double b[3];
        apply(B, cloud + 3 * (int64_t)(k0 + k), tr, b);
        s_b[k][0] = b[0]; s_b[k][1] = b[1]; s_b[k][2] = b[2]; s_b[k][3] = 0.0;
      }
    }
    __syncthreads();
#pragma unroll 4
    for (int k = 0; k < count; ++k) {
      const double bx = s_b[k][0], by = s_b[k][1], bz = s_b[k][2];
      for (int u = 0; u < 2; ++u) {
        const double dx = a[u][0] - bx, dy = a[u][1] - by, dz = a[u][2] - bz;
        const double d2 = (dx * dx + dy * dy) + dz * dz;
        best[u] = d2 < best[u] ? d2 : best[u];
      }
    }
    __syncthreads();
  }
  double *add = dist + 2 * (int64_t)item * max_points, *add_s = add + max_points;
  for (int u = 0; u < 2; ++u) {
    const int j = q0 + t + u * kLanes;
    if (!live[u]) continue;
    double b[3];
    apply(B, cloud + 3 * (int64_t)j, tr, b);
    const double dx = a[u][0] - b[0], dy = a[u][1] - b[1], dz = a[u][2] - b[2];
    add[j] = sqrt((dx * dx + dy * dy) + dz * dz);
    add_s[j] = sqrt(best[u]);
  }
}

__global__ void __launch_bounds__(kQueries) k_posemetric_mean(const int32_t *__restrict__ cloud_off,
                                                              const int32_t *__restrict__ item_cloud, int n_clouds,
                                                              int max_points, const double *__restrict__ dist,
                                                              double *__restrict__ out_add,
                                                              double *__restrict__ out_add_s) {
  __shared__ double s_sum[2][kQueries];
  const int item = blockIdx.x, t = threadIdx.x;
  int first = 0;
  const int P = item_points(cloud_off, item_cloud, item, n_clouds, max_points, &first);  // (uniform)
  if (P == 0) {
    if (t == 0) out_add[item] = out_add_s[item] = (double)__uint_as_float(0x7fc00000u);
    return;
  }
  const double *add = dist + 2 * (int64_t)item * max_points, *add_s = add + max_points;
  double acc0 = 0.0, acc1 = 0.0;
  for (int j = t; j < P; j += kQueries) { acc0 += add[j]; acc1 += add_s[j]; }
  s_sum[0][t] = acc0;
  s_sum[1][t] = acc1;
  __syncthreads();
  for (int half = kQueries / 2; half >= 1; half /= 2) {
    if (t < half) {
      s_sum[0][t] += s_sum[0][t + half];
      s_sum[1][t] += s_sum[1][t + half];
    }
    __syncthreads();
  }
  if (t == 0) {
    out_add[item] = s_sum[0][0] / (double)P;
    out_add_s[item] = s_sum[1][0] / (double)P;
  }
}

int bad(const char *what) {
  mf::set_last_error(hipErrorInvalidValue, what);
  return -(int)hipErrorInvalidValue;
}

}  // namespace

extern "C" int64_t mf_average_distance_f64_workspace_bytes(int32_t n_items, int32_t max_points) {
  if (n_items < 0 || n_items > 65535 || max_points < 1) return -1;
  return 16 * (int64_t)n_items * max_points;
}

extern "C" int mf_average_distance_f64(const double *points, const int32_t *cloud_off, const int32_t *item_cloud,
                                       const double *T1, const double *T2, int32_t n_clouds, int32_t n_items,
                                       int32_t max_points, int32_t translate, double *add, double *add_s,
                                       void *workspace, mfStream_t stream) {
  if (n_items < 0 || n_items > 65535 || n_clouds < 1 || max_points < 1)
    return bad("mf_average_distance_f64: 0..65535 items, at least one cloud, max_points >= 1 (no empty cloud)");
  if (n_items == 0) return 0;
  const unsigned qblocks = (unsigned)(((int64_t)max_points + kQueries - 1) / kQueries);
  hipLaunchKernelGGL(k_posemetric_dist, dim3(qblocks, (unsigned)n_items), dim3(kLanes), 0, (hipStream_t)stream, points,
                     cloud_off, item_cloud, T1, T2, (int)n_clouds, (int)max_points, (int)translate,
                     (double *)workspace);
  if (int rc = mf::check_launch("mf_average_distance_f64 (distances)")) return rc;
  hipLaunchKernelGGL(k_posemetric_mean, dim3((unsigned)n_items), dim3(kQueries), 0, (hipStream_t)stream, cloud_off,
                     item_cloud, (int)n_clouds, (int)max_points, (const double *)workspace, add, add_s);
  return mf::check_launch("mf_average_distance_f64 (means)");
}
