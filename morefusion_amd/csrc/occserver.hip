// The map server's insert and grid publication (contrib/octomap_server.py) -- gfx950.
//
// Reference: ros/src/morefusion_ros/src/OctomapServer.cpp, insertScan (:283-455) and publishGrids (:510-618), over
// the dense log-odds boxes of occmap.hip (mfOccTree).  What differs from occmap.hip's insertPointCloud model:
//   * only the stride-2 pixels of the frame take part (even row and even column);
//   * ONE free set per frame, in the background tree, from the rays of every valid pixel whatever its label; the
//     end point's background key is free too unless the pixel is background itself;
//   * an instance tree only ever gets the hit of its own end keys, at its own pitch;
//   * the sensor model (hit, miss, clamps) is an argument.
//
// One frame:
//   k_srv_bounds   per tree key box: the background's over every valid point, an instance's over its own;
//   k_srv_stats    one workgroup per label: point count, float32 min / max and the centroid of its points (the
//                  point with the smallest pixel index left out, see DESIGN.md "Map server"), plus one workgroup
//                  that looks for a label >= 0 without a slot;
//   k_srv_raycast  one lane per stride-2 pixel: the shared DDA (occmap_scan.h) into the background's free word,
//                  the end key into the occupied word of the label's tree;
//   k_srv_apply    one lane per cell: occupied -> one clamped hit, else free -> one clamped miss; bits cleared.
// publishGrids: k_srv_publish, one lane per voxel of all B grids; getGridsInWorldFrame (:456-508): k_srv_map_grids.
// No float atomics; every result is independent of the order in which lanes run.
#include <limits.h>
#include <math.h>

#include <algorithm>

#include "mf_common.h"
#include "occmap_keys.h"
#include "occmap_scan.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxBoundTrees = 256;  // LDS bounds table of k_srv_bounds
constexpr int kBoundBlocks = 256;
constexpr int kStatThreads = 1024;   // the centroid's summation order is defined over this many lanes
constexpr int kStatCols = 10;        // count, centroid xyz, min xyz, max xyz

// stride-2 pixel q of an H x W image -> its row-major pixel index
__device__ __forceinline__ int64_t pixel_of(int64_t q, int Ws, int W) { return (q / Ws) * 2 * (int64_t)W + (q % Ws) * 2; }

__global__ __launch_bounds__(kThreads) void k_srv_bounds(const float *__restrict__ pts, const int32_t *__restrict__ label,
                                                         int H, int W, const int32_t *__restrict__ slots, int n_slots,
                                                         const mfOccTree *__restrict__ trees, int bg_tree, int n_trees,
                                                         int32_t *bounds) {
  __shared__ int32_t s_b[6 * kMaxBoundTrees];
  for (int j = threadIdx.x; j < 6 * n_trees; j += blockDim.x) s_b[j] = (j % 6) < 3 ? INT_MAX : INT_MIN;
  __syncthreads();
  const int Ws = (W + 1) / 2;
  const int64_t n = (int64_t)((H + 1) / 2) * Ws;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t base = (int64_t)blockIdx.x * blockDim.x; base < n; base += stride) {  // uniform trip count
    const int64_t q = base + threadIdx.x;
    int tb = -1, to = -1, kb[3] = {0, 0, 0}, ko[3] = {0, 0, 0};
    if (q < n) {
      const int64_t i = pixel_of(q, Ws, W);
      float x, y, z;
      if (load_point(pts, i, x, y, z)) {
        const double rb = trees[bg_tree].res_factor;
        if (coord_key(x, rb, kb[0]) && coord_key(y, rb, kb[1]) && coord_key(z, rb, kb[2])) tb = bg_tree;
        const int s = find_slot(slots, n_slots, label[i]);
        if (s >= 0 && slots[3 * s + 1] != bg_tree) {
          const int t = slots[3 * s + 1];
          const double rf = trees[t].res_factor;
          if (coord_key(x, rf, ko[0]) && coord_key(y, rf, ko[1]) && coord_key(z, rf, ko[2])) to = t;
        }
      }
    }
    wave_key_bounds(tb, kb, s_b);
    wave_key_bounds(to, ko, s_b);
  }
  __syncthreads();
  for (int j = threadIdx.x; j < 6 * n_trees; j += blockDim.x) {
    const int32_t v = s_b[j];
    if ((j % 6) < 3) {
      if (v != INT_MAX) atomicMin(&bounds[j], v);
    } else if (v != INT_MIN) {
      atomicMax(&bounds[j], v);
    }
  }
}

__global__ void k_srv_bounds_init(int32_t *bounds, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < 6 * n) bounds[i] = (i % 6) < 3 ? INT_MAX : INT_MIN;
}

__global__ __launch_bounds__(kThreads) void k_srv_raycast(const float *__restrict__ pts, const int32_t *__restrict__ label,
                                                          int H, int W, const int32_t *__restrict__ slots, int n_slots,
                                                          const mfOccTree *__restrict__ trees, int bg_tree, float ox,
                                                          float oy, float oz, int32_t *overflow) {
  const int Ws = (W + 1) / 2;
  const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= (int64_t)((H + 1) / 2) * Ws) return;
  const int64_t i = pixel_of(q, Ws, W);
  float p[3];
  if (!load_point(pts, i, p[0], p[1], p[2])) return;
  const int32_t l = label[i];
  const mfOccTree bg = trees[bg_tree];
  const float o[3] = {ox, oy, oz};
  // free cells: the ray in the background tree, whatever the label (-2 included)
  ray_keys(o, p, bg.resolution, bg.res_factor, [&](int kx, int ky, int kz) { mark(bg, kx, ky, kz, 0, 1u, overflow); });
  int k[3];
  if (l != -2) {  // occupied end point in the label's own tree
    const int s = find_slot(slots, n_slots, l);
    if (s >= 0) {
      const mfOccTree t = trees[slots[3 * s + 1]];
      if (coord_key(p[0], t.res_factor, k[0]) && coord_key(p[1], t.res_factor, k[1]) && coord_key(p[2], t.res_factor, k[2]))
        mark(t, k[0], k[1], k[2], 1, 1u, overflow);
    }
  }
  if (l != -1 && coord_key(p[0], bg.res_factor, k[0]) && coord_key(p[1], bg.res_factor, k[1]) &&
      coord_key(p[2], bg.res_factor, k[2]))
    mark(bg, k[0], k[1], k[2], 0, 1u, overflow);  // another label's end point: free in the background
}

__global__ __launch_bounds__(kThreads) void k_srv_apply(const mfOccTree *__restrict__ trees, float hit, float miss,
                                                        float lo_min, float lo_max) {
  const mfOccTree t = trees[blockIdx.y];
  const int64_t n = (int64_t)t.dim[0] * t.dim[1] * t.dim[2];
  for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < n; c += (int64_t)gridDim.x * blockDim.x) {
    const uint32_t f = t.bits[2 * c], o = t.bits[2 * c + 1];
    if ((f | o) == 0u) continue;
    float l = t.logodds[c];
    if (isnan(l)) l = 0.0f;          // a new node starts at log-odds 0
    l = l + (o ? hit : miss);        // occupied wins over free within the frame
    if (l < lo_min) l = lo_min;      // OccupancyOcTreeBase::updateNodeLogOdds
    if (l > lo_max) l = lo_max;
    t.logodds[c] = l;
    t.bits[2 * c] = 0u;
    t.bits[2 * c + 1] = 0u;
  }
}

// float32 <-> unsigned keys that order like the values (-0 below +0), for integer min / max
__device__ __forceinline__ uint32_t order_key(float f) {
  const uint32_t u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float order_value(uint32_t k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

__global__ __launch_bounds__(kStatThreads) void k_srv_stats(const float *__restrict__ pts, const int32_t *__restrict__ label,
                                                            int H, int W, const int32_t *__restrict__ slots, int n_slots,
                                                            double *__restrict__ table) {
  __shared__ double s_sum[3][kStatThreads];
  __shared__ uint32_t s_mn[3], s_mx[3];
  __shared__ int s_first, s_cnt;
  const int tid = threadIdx.x;
  if ((int)blockIdx.x == n_slots) {  // the smallest label >= 0 of the whole image that has no slot (-1: none)
    if (tid == 0) s_first = INT_MAX;
    __syncthreads();
    int32_t lo = INT_MAX;
    for (int64_t i = tid; i < (int64_t)H * W; i += kStatThreads) {
      const int32_t l = label[i];
      if (l >= 0 && l < lo && find_slot(slots, n_slots, l) < 0) lo = l;
    }
    if (lo != INT_MAX) atomicMin(&s_first, lo);
    __syncthreads();
    if (tid == 0) table[(int64_t)kStatCols * n_slots] = s_first == INT_MAX ? -1.0 : (double)s_first;
    return;
  }
  const int32_t mine = slots[3 * blockIdx.x];
  const int Ws = (W + 1) / 2;
  const int n = ((H + 1) / 2) * Ws;
  if (tid == 0) {
    s_first = INT_MAX;
    s_cnt = 0;
    for (int a = 0; a < 3; ++a) {
      s_mn[a] = 0xffffffffu;
      s_mx[a] = 0u;
    }
  }
  __syncthreads();
  // the first point of a label only creates its cloud (insertScan :345-349): the smallest pixel index is left out
  for (int q = tid; q < n; q += kStatThreads) {
    const int64_t i = pixel_of(q, Ws, W);
    float x, y, z;
    if (label[i] == mine && load_point(pts, i, x, y, z)) {
      atomicMin(&s_first, q);
      break;  // q only grows along a lane
    }
  }
  __syncthreads();
  const int first = s_first;
  // float64 sums of the float32 coordinates: lane t adds its pixels q = t, t + 1024, ... in ascending order, then
  // the lanes are folded pairwise (t += t + off for off = 512 .. 1): one fixed order
  double sum[3] = {0.0, 0.0, 0.0};
  uint32_t mn[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, mx[3] = {0u, 0u, 0u};
  int cnt = 0;
  for (int q = tid; q < n; q += kStatThreads) {
    if (q == first) continue;
    const int64_t i = pixel_of(q, Ws, W);
    float c[3];
    if (label[i] != mine || !load_point(pts, i, c[0], c[1], c[2])) continue;
    ++cnt;
    for (int a = 0; a < 3; ++a) {
      sum[a] = sum[a] + (double)c[a];
      const uint32_t k = order_key(c[a]);
      mn[a] = min(mn[a], k);
      mx[a] = max(mx[a], k);
    }
  }
  for (int a = 0; a < 3; ++a) s_sum[a][tid] = sum[a];
  if (cnt) {
    atomicAdd(&s_cnt, cnt);
    for (int a = 0; a < 3; ++a) {
      atomicMin(&s_mn[a], mn[a]);
      atomicMax(&s_mx[a], mx[a]);
    }
  }
  __syncthreads();
  for (int off = kStatThreads / 2; off > 0; off >>= 1) {
    if (tid < off)
      for (int a = 0; a < 3; ++a) s_sum[a][tid] = s_sum[a][tid] + s_sum[a][tid + off];
    __syncthreads();
  }
  if (tid == 0) {
    double *row = table + (int64_t)kStatCols * blockIdx.x;
    const int c = s_cnt;
    row[0] = (double)c;
    for (int a = 0; a < 3; ++a) {
      row[1 + a] = c ? (double)(float)(s_sum[a][0] / (double)c) : 0.0;
      row[4 + a] = c ? (double)order_value(s_mn[a]) : 0.0;
      row[7 + a] = c ? (double)order_value(s_mx[a]) : 0.0;
    }
  }
}

// log-odds of the cell that holds the float32 point c; NaN: unknown (OcTreeBaseImpl::search == NULL)
__device__ __forceinline__ float search(const mfOccTree &t, const float (&c)[3]) {
  int k[3];
  if (!(coord_key(c[0], t.res_factor, k[0]) && coord_key(c[1], t.res_factor, k[1]) && coord_key(c[2], t.res_factor, k[2])))
    return __int_as_float(0x7fc00000);
  const int64_t cell = cell_of(t, k[0], k[1], k[2]);
  return cell < 0 ? __int_as_float(0x7fc00000) : t.logodds[cell];
}

__device__ __forceinline__ void rigid(const float *__restrict__ T, const float (&p)[3], float (&out)[3]) {
  for (int r = 0; r < 3; ++r) out[r] = ((T[4 * r] * p[0] + T[4 * r + 1] * p[1]) + T[4 * r + 2] * p[2]) + T[4 * r + 3];
}

__global__ __launch_bounds__(kThreads) void k_srv_publish(const mfOccTree *__restrict__ trees, int n_trees,
                                                          const int32_t *__restrict__ order, int bg_tree,
                                                          const int32_t *__restrict__ target_tree,
                                                          const float *__restrict__ pitch, const float *__restrict__ center_map,
                                                          const float *__restrict__ T_map_to_sensor,
                                                          const float *__restrict__ T_sensor_to_map, double prob_max,
                                                          int flags, int B, int D, double *__restrict__ origin_out,
                                                          float *__restrict__ grid_target, float *__restrict__ grid_noentry,
                                                          uint8_t *__restrict__ grid_nte) {
  const int64_t nvox = (int64_t)D * D * D;
  const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= nvox * B) return;
  const int b = (int)(g / nvox);
  const int64_t v = g - (int64_t)b * nvox;
  const int idx[3] = {(int)(v / ((int64_t)D * D)), (int)((v / D) % D), (int)(v % D)};
  const float p32 = pitch[b];
  const float cm[3] = {center_map[3 * b], center_map[3 * b + 1], center_map[3 * b + 2]};
  float cs[3], s[3], m[3];
  rigid(T_map_to_sensor, cm, cs);
  for (int a = 0; a < 3; ++a) {
    const double origin = (double)cs[a] - ((double)D / 2.0 - 0.5) * (double)p32;
    if (v == 0) origin_out[3 * b + a] = origin;
    s[a] = (float)(origin + (double)(p32 * (float)idx[a]));  // grid.pitch * i: float; PCLPoint: float
  }
  rigid(T_sensor_to_map, s, m);
  float gt = 0.0f, ne = 0.0f;
  if ((flags & 1) && m[2] < 0.0f) {
    ne = (float)prob_max;  // below the ground plane
  } else {
    const int target = target_tree[b];
    const float lt = target >= 0 && target < n_trees ? search(trees[target], m) : __int_as_float(0x7fc00000);
    const double own = isnan(lt) ? 0.0 : 1.0 - 1.0 / (1.0 + exp((double)lt));
    if (own > 0.5) {
      gt = (float)own;
    } else {
      for (int j = 0; j < n_trees; ++j) {  // ascending id, the last writer wins
        const int ti = order[j];
        if (ti == target || ti < 0 || ti >= n_trees) continue;
        const float l = search(trees[ti], m);
        if (isnan(l)) continue;
        const double occ = 1.0 - 1.0 / (1.0 + exp((double)l));
        if (ti == bg_tree && (flags & 2) && occ < 0.5) ne = (float)(1.0 - occ);
        else if (occ >= prob_max) ne = (float)occ;
      }
    }
  }
  grid_target[g] = gt;
  grid_noentry[g] = ne;
  grid_nte[g] = ne != 0.0f;
}

// getGridsInWorldFrame: one lane per voxel of all B grids; the sample is a float64 coordinate (search(double x, ...))
__device__ __forceinline__ bool coord_key_f64(double c, double rf, int &key) {
  const double s = floor(c * rf);
  if (!(s >= -(double)kKeyMax && s < (double)kKeyMax)) return false;
  key = (int)s + kKeyMax;
  return true;
}

__global__ __launch_bounds__(kThreads) void k_srv_map_grids(const mfOccTree *__restrict__ trees, int n_trees,
                                                            const int32_t *__restrict__ target_tree,
                                                            const float *__restrict__ pitch,
                                                            const float *__restrict__ center_map, int B, int D,
                                                            double *__restrict__ origin_out, float *__restrict__ grid) {
  const int64_t nvox = (int64_t)D * D * D;
  const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= nvox * B) return;
  const int b = (int)(g / nvox);
  const int64_t v = g - (int64_t)b * nvox;
  const int idx[3] = {(int)(v / ((int64_t)D * D)), (int)((v / D) % D), (int)(v % D)};
  const float p32 = pitch[b];
  const int target = target_tree[b];
  bool ok = target >= 0 && target < n_trees;
  int k[3] = {0, 0, 0};
  for (int a = 0; a < 3; ++a) {
    const double origin = (double)center_map[3 * b + a] - ((double)D / 2.0 - 0.5) * (double)p32;
    if (v == 0) origin_out[3 * b + a] = origin;
    const double x = origin + (double)(p32 * (float)idx[a]);  // grid.pitch * i: float
    if (ok) ok = coord_key_f64(x, trees[target].res_factor, k[a]);
  }
  float out = 0.0f;
  if (ok) {
    const mfOccTree t = trees[target];
    const int64_t cell = cell_of(t, k[0], k[1], k[2]);
    const float l = cell < 0 ? __int_as_float(0x7fc00000) : t.logodds[cell];
    if (!isnan(l)) {
      const double occ = 1.0 - 1.0 / (1.0 + exp((double)l));
      if (occ > 0.5) out = (float)occ;
    }
  }
  grid[g] = out;
}

int bad(const char *what) {
  mf::set_last_error(hipErrorInvalidValue, what);
  return -(int)hipErrorInvalidValue;
}

bool bad_image(int H, int W) { return H <= 0 || W <= 0 || (int64_t)H * W > INT_MAX; }

int blocks_for(int64_t n) { return (int)((n + kThreads - 1) / kThreads); }

int64_t stride2(int H, int W) { return (int64_t)((H + 1) / 2) * ((W + 1) / 2); }

}  // namespace

extern "C" int mf_occserver_bounds(const float *pts, const int32_t *label, int32_t H, int32_t W, const int32_t *slots,
                                   int32_t n_slots, const mfOccTree *trees, int32_t bg_tree, int32_t n_trees,
                                   int32_t *bounds, mfStream_t stream) {
  if (bad_image(H, W) || n_slots < 0) return bad("mf_occserver_bounds: bad sizes");
  if (n_trees <= 0 || n_trees > kMaxBoundTrees) return bad("mf_occserver_bounds: 1 .. 256 trees");
  if (bg_tree < 0 || bg_tree >= n_trees) return bad("mf_occserver_bounds: bg_tree out of range");
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(k_srv_bounds_init, dim3((6 * n_trees + 255) / 256), dim3(256), 0, s, bounds, (int)n_trees);
  hipLaunchKernelGGL(k_srv_bounds, dim3(std::min(blocks_for(stride2(H, W)), kBoundBlocks)), dim3(kThreads), 0, s, pts,
                     label, (int)H, (int)W, slots, (int)n_slots, trees, (int)bg_tree, (int)n_trees, bounds);
  return mf::check_launch("mf_occserver_bounds");
}

extern "C" int mf_occserver_stats(const float *pts, const int32_t *label, int32_t H, int32_t W, const int32_t *slots,
                                  int32_t n_slots, double *table, mfStream_t stream) {
  if (bad_image(H, W) || n_slots < 0 || n_slots > 65535) return bad("mf_occserver_stats: bad sizes");
  hipLaunchKernelGGL(k_srv_stats, dim3(n_slots + 1), dim3(kStatThreads), 0, (hipStream_t)stream, pts, label, (int)H,
                     (int)W, slots, (int)n_slots, table);
  return mf::check_launch("mf_occserver_stats");
}

extern "C" int mf_occserver_raycast(const float *pts, const int32_t *label, int32_t H, int32_t W, const int32_t *slots,
                                    int32_t n_slots, const mfOccTree *trees, int32_t bg_tree, float origin_x,
                                    float origin_y, float origin_z, int32_t *overflow, mfStream_t stream) {
  if (bad_image(H, W) || n_slots < 0 || bg_tree < 0) return bad("mf_occserver_raycast: bad sizes");
  hipLaunchKernelGGL(k_srv_raycast, dim3(blocks_for(stride2(H, W))), dim3(kThreads), 0, (hipStream_t)stream, pts, label,
                     (int)H, (int)W, slots, (int)n_slots, trees, (int)bg_tree, origin_x, origin_y, origin_z, overflow);
  return mf::check_launch("mf_occserver_raycast");
}

extern "C" int mf_occserver_apply(const mfOccTree *trees, int32_t n_trees, int64_t max_cells, float hit, float miss,
                                  float lo_min, float lo_max, mfStream_t stream) {
  if (n_trees > 65535) return bad("mf_occserver_apply: at most 65535 trees");
  if (!(lo_min <= lo_max)) return bad("mf_occserver_apply: lo_min > lo_max");
  if (n_trees <= 0 || max_cells <= 0) return 0;
  const int bx = (int)std::min<int64_t>((max_cells + kThreads - 1) / kThreads, 4096);
  hipLaunchKernelGGL(k_srv_apply, dim3(bx, n_trees), dim3(kThreads), 0, (hipStream_t)stream, trees, hit, miss, lo_min,
                     lo_max);
  return mf::check_launch("mf_occserver_apply");
}

extern "C" int mf_occserver_publish(const mfOccTree *trees, int32_t n_trees, const int32_t *order, int32_t bg_tree,
                                    const int32_t *target_tree, const float *pitch, const float *center_map,
                                    const float *T_map_to_sensor, const float *T_sensor_to_map, double prob_max,
                                    int32_t flags, int32_t B, int32_t D, double *origin, float *grid_target,
                                    float *grid_noentry, uint8_t *grid_nontarget_empty, mfStream_t stream) {
  if (B < 0 || D <= 0 || D > 1024 || n_trees <= 0 || bg_tree < 0 || bg_tree >= n_trees)
    return bad("mf_occserver_publish: bad sizes");
  const int64_t n = (int64_t)B * D * D * D;
  if (n == 0) return 0;
  if ((n + kThreads - 1) / kThreads > INT_MAX) return bad("mf_occserver_publish: too many voxels");
  hipLaunchKernelGGL(k_srv_publish, dim3((unsigned)((n + kThreads - 1) / kThreads)), dim3(kThreads), 0,
                     (hipStream_t)stream, trees, (int)n_trees, order, (int)bg_tree, target_tree, pitch, center_map,
                     T_map_to_sensor, T_sensor_to_map, prob_max, (int)flags, (int)B, (int)D, origin, grid_target,
                     grid_noentry, grid_nontarget_empty);
  return mf::check_launch("mf_occserver_publish");
}

extern "C" int mf_occserver_map_grids(const mfOccTree *trees, int32_t n_trees, const int32_t *target_tree,
                                      const float *pitch, const float *center_map, int32_t B, int32_t D,
                                      double *origin, float *grid, mfStream_t stream) {
  if (B < 0 || D <= 0 || D > 1024 || n_trees <= 0) return bad("mf_occserver_map_grids: bad sizes");
  const int64_t n = (int64_t)B * D * D * D;
  if (n == 0) return 0;
  if ((n + kThreads - 1) / kThreads > INT_MAX) return bad("mf_occserver_map_grids: too many voxels");
  hipLaunchKernelGGL(k_srv_map_grids, dim3((unsigned)((n + kThreads - 1) / kThreads)), dim3(kThreads), 0,
                     (hipStream_t)stream, trees, (int)n_trees, target_tree, pitch, center_map, (int)B, (int)D, origin,
                     grid);
  return mf::check_launch("mf_occserver_map_grids");
}
