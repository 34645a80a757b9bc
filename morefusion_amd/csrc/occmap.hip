// Occupancy mapping (contrib/multi_instance_octree_mapping.py) -- gfx950.
//
// Reference: morefusion/contrib/multi_instance_octree_mapping.py:20-94 over OctoMap (one OcTree per
// instance, insertPointCloud / updateNodes / search) and its driver
// datasets/rgbd_pose_estimation/base.py:28-46 (build_octomap).
//
// Representation: one dense float32 log-odds volume per instance over a box of octree keys, NaN =
// never touched (OctoMap's missing node).  OctoMap prunes equal children into their parent, which
// changes nothing a leaf search returns, so the dense box is exact as long as it holds every key a
// scan touches: the caller sizes it from k_occ_bounds (end keys + origin key, one cell of margin for
// a DDA that overshoots the end key by one cell through rounding).
//
// One scan (= one insertPointCloud) in three launches, any number of trees at once:
//   k_occ_bounds   per tree key box of the scan's points (per-wave min/max, LDS int atomics per wave and
//                  tree present in the wave, one global int atomic per bound and workgroup: deterministic);
//   k_occ_raycast  one lane per point: octomap's computeRayKeys DDA (float direction / length, double
//                  tMax / tDelta, the same tie rule) from the origin to the point; every visited key
//                  ORs the scan's bit into the cell's free word, the end key into its occupied word.
//                  OR is order-free, and the word is read first: most rays near the sensor find their
//                  bit already set and issue no atomic.  Up to 32 scans per tree and launch;
//   k_occ_apply    one lane per cell: the scans in order, occupied bit -> +logodds(0.7), else free bit
//                  -> +logodds(0.4), float32 adds clamped to [logodds(0.1192), logodds(0.971)] at each
//                  step (octomap's updateNodeLogOdds), then the bits are cleared.
// update(): k_occ_count_hits (integer atomics) + k_occ_apply mode 1 (n clamped hit-adds: every
// update has the same sign, so the order of the hits does not matter).
// get_target_grids: k_occ_extract, one lane per output voxel, trees in insertion order.
// Every result is independent of the order in which lanes run: bitwise deterministic.
#include <float.h>
#include <limits.h>
#include <math.h>

#include <algorithm>

#include "mf_common.h"
#include "occmap_keys.h"
#include "occmap_scan.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxBoundTrees = 256;  // LDS bounds table of k_occ_bounds
constexpr int kBoundBlocks = 256;

// octomap's logodds(p) = (float) log(p / (1 - p)) of its default sensor model (hit 0.7, miss 0.4) and clamping
// thresholds (0.1192, 0.971), as exact float32 literals (a device log could differ from the host's in the last bit)
constexpr float kLoHit = 0x1.b1d106p-1f;    //  0.84729785
constexpr float kLoMiss = -0x1.9f323ep-2f;  // -0.4054651
constexpr float kLoMin = -0x1.0000eap+1f;   // -2.000028
constexpr float kLoMax = 0x1.c16974p+1f;    //  3.5110307

__device__ __forceinline__ float clamp_add(float l, float u) {  // OccupancyOcTreeBase::updateNodeLogOdds
  l = l + u;
  if (l < kLoMin) return kLoMin;
  if (l > kLoMax) return kLoMax;
  return l;
}

__global__ void k_occ_regrid(mfOccTree src, int has_src, mfOccTree dst) {
  const int64_t n = (int64_t)dst.dim[0] * dst.dim[1] * dst.dim[2];
  for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < n; c += (int64_t)gridDim.x * blockDim.x) {
    const int z = (int)(c % dst.dim[2]), y = (int)((c / dst.dim[2]) % dst.dim[1]), x = (int)(c / ((int64_t)dst.dim[1] * dst.dim[2]));
    float v = __int_as_float(0x7fc00000);  // NaN: unknown
    if (has_src) {
      const int64_t s = cell_of(src, x + dst.lo[0], y + dst.lo[1], z + dst.lo[2]);
      if (s >= 0) v = src.logodds[s];
    }
    dst.logodds[c] = v;
    dst.bits[2 * c] = 0u;
    dst.bits[2 * c + 1] = 0u;
  }
}

__global__ void k_occ_bounds_init(int32_t *bounds, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < 6 * n) bounds[i] = (i % 6) < 3 ? INT_MAX : INT_MIN;
}

__global__ __launch_bounds__(kThreads) void k_occ_bounds(const float *__restrict__ pts, const int32_t *__restrict__ label,
                                                         int64_t n, const int32_t *__restrict__ slots, int n_slots,
                                                         const mfOccTree *__restrict__ trees, int n_trees,
                                                         int32_t *bounds) {
  // per-wave min / max -> LDS (int atomics) -> one global atomic per bound and workgroup: every step is an exact
  // min / max, so the result does not depend on the order (per-wave global atomics on the same six words per tree
  // were measured at 330 us for one frame: same-address atomics serialise)
  __shared__ int32_t s_b[6 * kMaxBoundTrees];
  for (int j = threadIdx.x; j < 6 * n_trees; j += blockDim.x) s_b[j] = (j % 6) < 3 ? INT_MAX : INT_MIN;
  __syncthreads();
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t base = (int64_t)blockIdx.x * blockDim.x; base < n; base += stride) {  // uniform trip count
    const int64_t i = base + threadIdx.x;
    int tree = -1, k[3] = {0, 0, 0};
    if (i < n) {
      const int s = find_slot(slots, n_slots, label[i]);
      float x, y, z;
      if (s >= 0 && load_point(pts, i, x, y, z)) {
        const int t = slots[3 * s + 1];
        const double rf = trees[t].res_factor;
        if (coord_key(x, rf, k[0]) && coord_key(y, rf, k[1]) && coord_key(z, rf, k[2])) tree = t;
      }
    }
    wave_key_bounds(tree, k, s_b);  // one pass per tree present in the wave
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

__global__ __launch_bounds__(kThreads) void k_occ_raycast(const float *__restrict__ pts, const int32_t *__restrict__ label,
                                                          int64_t n, const int32_t *__restrict__ slots, int n_slots,
                                                          const mfOccTree *__restrict__ trees, float ox, float oy, float oz,
                                                          int32_t *overflow) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int s = find_slot(slots, n_slots, label[i]);
  if (s < 0) return;
  float p[3];
  if (!load_point(pts, i, p[0], p[1], p[2])) return;
  const mfOccTree t = trees[slots[3 * s + 1]];
  const uint32_t m = 1u << slots[3 * s + 2];
  const double res = t.resolution, rf = t.res_factor;
  const float o[3] = {ox, oy, oz};
  // computeUpdate: the free cells of the ray (computeRayKeys), then the end point's key
  ray_keys(o, p, res, rf, [&](int kx, int ky, int kz) { mark(t, kx, ky, kz, 0, m, overflow); });
  int ke[3];
  if (coord_key(p[0], rf, ke[0]) && coord_key(p[1], rf, ke[1]) && coord_key(p[2], rf, ke[2]))
    mark(t, ke[0], ke[1], ke[2], 1, m, overflow);
}

__global__ __launch_bounds__(kThreads) void k_occ_count_hits(const float *__restrict__ pts, int64_t n,
                                                             const mfOccTree *__restrict__ trees, int tree,
                                                             int32_t *overflow) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float x, y, z;
  if (!load_point(pts, i, x, y, z)) return;
  const mfOccTree t = trees[tree];
  int k[3];
  if (!(coord_key(x, t.res_factor, k[0]) && coord_key(y, t.res_factor, k[1]) && coord_key(z, t.res_factor, k[2])))
    return;
  const int64_t c = cell_of(t, k[0], k[1], k[2]);
  if (c < 0) {
    if (overflow) atomicAdd(overflow, 1);
    return;
  }
  atomicAdd(t.bits + 2 * c, 1u);
}

__global__ __launch_bounds__(kThreads) void k_occ_apply(const mfOccTree *__restrict__ trees, int mode) {
  const mfOccTree t = trees[blockIdx.y];
  const int64_t n = (int64_t)t.dim[0] * t.dim[1] * t.dim[2];
  for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < n; c += (int64_t)gridDim.x * blockDim.x) {
    const uint32_t f = t.bits[2 * c], o = t.bits[2 * c + 1];
    if ((f | o) == 0u) continue;
    float l = t.logodds[c];
    if (isnan(l)) l = 0.0f;  // a new node starts at log-odds 0
    if (mode == 0) {
      // scans in order; within a scan occupied wins over free (insertPointCloud's disjoint key sets)
      for (uint32_t any = f | o; any; any &= any - 1u) {
        const uint32_t b = any & (0u - any);
        l = clamp_add(l, (o & b) ? kLoHit : kLoMiss);
      }
      t.bits[2 * c + 1] = 0u;
    } else {
      for (uint32_t h = 0; h < f && l < kLoMax; ++h) l = clamp_add(l, kLoHit);
    }
    t.logodds[c] = l;
    t.bits[2 * c] = 0u;
  }
}

__global__ __launch_bounds__(kThreads) void k_occ_extract(const mfOccTree *__restrict__ trees, int n_trees,
                                                          const int32_t *__restrict__ target_tree,
                                                          const double *__restrict__ pitch,
                                                          const double *__restrict__ origin, int B, int D0, int D1, int D2,
                                                          float *grid_target, float *grid_nontarget, float *grid_empty,
                                                          uint8_t *net_target, uint8_t *net_nte) {
  const int64_t nvox = (int64_t)D0 * D1 * D2;
  const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= nvox * B) return;
  const int b = (int)(g / nvox);
  const int64_t v = g - (int64_t)b * nvox;
  const int iz = (int)(v % D2), iy = (int)((v / D2) % D1), ix = (int)(v / ((int64_t)D1 * D2));
  // trimesh matrix_to_points: index * pitch + origin in float64; octomap's search takes a float point3d
  const double pb = pitch[b];
  const float c[3] = {(float)((double)ix * pb + origin[3 * b]), (float)((double)iy * pb + origin[3 * b + 1]),
                      (float)((double)iz * pb + origin[3 * b + 2])};
  const int target = target_tree[b];
  float gt = 0.0f, gn = 0.0f, ge = 0.0f;
  for (int ti = 0; ti < n_trees; ++ti) {
    const mfOccTree t = trees[ti];
    int k[3];
    if (!(coord_key(c[0], t.res_factor, k[0]) && coord_key(c[1], t.res_factor, k[1]) &&
          coord_key(c[2], t.res_factor, k[2])))
      continue;
    const int64_t cell = cell_of(t, k[0], k[1], k[2]);
    if (cell < 0) continue;
    const float l = t.logodds[cell];
    if (isnan(l)) continue;  // unknown (-1 in the reference)
    const double occ = 1.0 - 1.0 / (1.0 + exp((double)l));
    if (occ >= 0.5) {
      if (ti == target) gt = (float)occ;
      else gn = (float)occ;
    } else if (occ >= 0.0) {
      ge = (float)(1.0 - occ);
    }
  }
  grid_target[g] = gt;
  grid_nontarget[g] = gn;
  grid_empty[g] = ge;
  if (net_target) {  // data_formats.grids_for_network(train=False)
    const bool tg = gt > 0.5f;
    net_target[g] = tg;
    net_nte[g] = ((gn > 0.5f) != tg) || ((ge > 0.5f) != tg);
  }
}

int bad(const char *what) {
  mf::set_last_error(hipErrorInvalidValue, what);
  return -(int)hipErrorInvalidValue;
}

int blocks_for(int64_t n) { return (int)std::min<int64_t>((n + kThreads - 1) / kThreads, 1 << 20); }

}  // namespace

extern "C" int mf_occmap_regrid(const mfOccTree *src, const mfOccTree *dst, mfStream_t stream) {
  if (!dst || dst->dim[0] <= 0 || dst->dim[1] <= 0 || dst->dim[2] <= 0) return bad("mf_occmap_regrid: empty box");
  const int64_t n = (int64_t)dst->dim[0] * dst->dim[1] * dst->dim[2];
  mfOccTree none = {};
  hipLaunchKernelGGL(k_occ_regrid, dim3((int)std::min<int64_t>((n + kThreads - 1) / kThreads, 8192)), dim3(kThreads), 0,
                     (hipStream_t)stream, src ? *src : none, src ? 1 : 0, *dst);
  return mf::check_launch("mf_occmap_regrid");
}

extern "C" int mf_occmap_bounds(const float *pts, const int32_t *label, int64_t n, const int32_t *slots, int32_t n_slots,
                                const mfOccTree *trees, int32_t n_trees, int32_t *bounds, mfStream_t stream) {
  if (n_trees <= 0) return 0;
  if (n < 0 || n_slots < 0) return bad("mf_occmap_bounds: negative size");
  if (n_trees > kMaxBoundTrees) return bad("mf_occmap_bounds: at most 256 trees");
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(k_occ_bounds_init, dim3((6 * n_trees + 255) / 256), dim3(256), 0, s, bounds, n_trees);
  if (n > 0 && n_slots > 0)
    hipLaunchKernelGGL(k_occ_bounds, dim3(std::min(blocks_for(n), kBoundBlocks)), dim3(kThreads), 0, s, pts, label, n,
                       slots, n_slots, trees, (int)n_trees, bounds);
  return mf::check_launch("mf_occmap_bounds");
}

extern "C" int mf_occmap_raycast(const float *pts, const int32_t *label, int64_t n, const int32_t *slots, int32_t n_slots,
                                 const mfOccTree *trees, float origin_x, float origin_y, float origin_z,
                                 int32_t *overflow, mfStream_t stream) {
  if (n < 0 || n_slots < 0) return bad("mf_occmap_raycast: negative size");
  if (n == 0 || n_slots == 0) return 0;
  hipLaunchKernelGGL(k_occ_raycast, dim3(blocks_for(n)), dim3(kThreads), 0, (hipStream_t)stream, pts, label, n, slots,
                     n_slots, trees, origin_x, origin_y, origin_z, overflow);
  return mf::check_launch("mf_occmap_raycast");
}

extern "C" int mf_occmap_count_hits(const float *pts, int64_t n, const mfOccTree *trees, int32_t tree,
                                    int32_t *overflow, mfStream_t stream) {
  if (n < 0 || tree < 0) return bad("mf_occmap_count_hits: negative size or tree");
  if (n == 0) return 0;
  hipLaunchKernelGGL(k_occ_count_hits, dim3(blocks_for(n)), dim3(kThreads), 0, (hipStream_t)stream, pts, n, trees,
                     (int)tree, overflow);
  return mf::check_launch("mf_occmap_count_hits");
}

extern "C" int mf_occmap_apply(const mfOccTree *trees, int32_t n_trees, int64_t max_cells, int32_t mode,
                               mfStream_t stream) {
  if (mode != 0 && mode != 1) return bad("mf_occmap_apply: mode 0 (scans) or 1 (hit counts)");
  if (n_trees > 65535) return bad("mf_occmap_apply: at most 65535 trees");
  if (n_trees <= 0 || max_cells <= 0) return 0;
  const int bx = (int)std::min<int64_t>((max_cells + kThreads - 1) / kThreads, 4096);
  hipLaunchKernelGGL(k_occ_apply, dim3(bx, n_trees), dim3(kThreads), 0, (hipStream_t)stream, trees, (int)mode);
  return mf::check_launch("mf_occmap_apply");
}

extern "C" int mf_occmap_extract(const mfOccTree *trees, int32_t n_trees, const int32_t *target_tree, const double *pitch,
                                 const double *origin, int32_t B, int32_t D0, int32_t D1, int32_t D2, float *grid_target,
                                 float *grid_nontarget, float *grid_empty, uint8_t *net_target, uint8_t *net_nte,
                                 mfStream_t stream) {
  if (B < 0 || D0 <= 0 || D1 <= 0 || D2 <= 0 || n_trees < 0) return bad("mf_occmap_extract: bad sizes");
  if ((net_target == nullptr) != (net_nte == nullptr)) return bad("mf_occmap_extract: net_target and net_nte together");
  const int64_t n = (int64_t)B * D0 * D1 * D2;
  if (n == 0) return 0;
  if ((n + kThreads - 1) / kThreads > INT_MAX) return bad("mf_occmap_extract: too many voxels");
  hipLaunchKernelGGL(k_occ_extract, dim3((unsigned)((n + kThreads - 1) / kThreads)), dim3(kThreads), 0,
                     (hipStream_t)stream, trees, (int)n_trees, target_tree, pitch, origin, (int)B, (int)D0, (int)D1,
                     (int)D2, grid_target, grid_nontarget, grid_empty, net_target, net_nte);
  return mf::check_launch("mf_occmap_extract");
}
