// Instance tracking across frames (contrib/instance_tracking.py) -- gfx950.
//
// Reference: ros/src/morefusion_ros/src/OctomapServer.cpp:95-281 (the per-frame loop: render the instance maps
// into the camera, then track_instance_id) and include/morefusion_ros/utils/geometry.h:20-281.  The reference
// runs OpenMP loops with critical sections and one OpenCV pass per id; here every step is one pass over pixels
// (x trees), see DESIGN.md "Instance tracking".
//
//   transform  pts_map = T * pts_sensor in float32, (T00 x + T01 y) + T02 z + T03 without contraction;
//   render     k_trk_cast: one lane per (stride-2 pixel, tree): OctoMap's castRay (ignoreUnknownCells, occupied =
//              log-odds >= 0, maxRange 1.1 |p - o|) on the dense box; depth test = one 64-bit atomic minimum per
//              pixel on (float bits of d) << 32 | slot order, so the winner does not depend on the order of the
//              lanes and an exact tie goes to the earlier slot.  k_trk_resolve: the 2 x 2 splat as a gather (the
//              splats of stride-2 pixels do not overlap);
//   overlap    one pass over both label images: intersection matrix, areas, edge / non-edge counts, detection
//              boxes; integer bins per workgroup in LDS, one atomic per non-zero bin (global atomics when the
//              bins do not fit);
//   assign     one workgroup: best IoU per detection, the vetoes, new ids from the counter in detection order;
//   relabel    the remap table applied to the detection image, suspicious ids blanked in both images;
//   clean      8-connected components by union-find in global memory (the root of a component is its smallest
//              pixel index), components below min_area -> -2, then a separable min / max filter: a pixel whose
//              (2 band + 1)^2 window holds two values or leaves the image -> -2;
//   merge      the merged label of the pose stage.
// Integer atomics and exact minima only: every output is bitwise independent of the order in which lanes run.
#include <float.h>
#include <limits.h>
#include <math.h>

#include <algorithm>

#include "mf_common.h"
#include "occmap_keys.h"

namespace {

typedef unsigned long long u64;

constexpr int kThreads = 256;
constexpr int kMaxBlocks = 2048;
constexpr int kLdsBins = 1024;    // integer bins of k_trk_overlap kept in LDS (4 KB)
constexpr int kMaxIds = 1024;     // ids per list
constexpr u64 kNoHit = ~0ull;

int bad(const char *what) {
  mf::set_last_error(hipErrorInvalidValue, what);
  return -(int)hipErrorInvalidValue;
}

int blocks_for(int64_t n) { return (int)std::max<int64_t>(1, std::min<int64_t>((n + kThreads - 1) / kThreads, kMaxBlocks)); }

int64_t align16(int64_t n) { return (n + 15) & ~(int64_t)15; }

// workspace layout: [z-buffer u64 Hs * Ws][a int32 H * W][b int32 H * W][presence int32 2 * n_ref]
struct Layout {
  int64_t z, a, b, presence, total;
};
Layout layout_of(int64_t H, int64_t W, int64_t n_ref) {
  Layout l;
  l.z = 0;
  l.a = align16(8 * ((H + 1) / 2) * ((W + 1) / 2));
  l.b = l.a + align16(4 * H * W);
  l.presence = l.b + align16(4 * H * W);
  l.total = l.presence + align16(8 * std::max<int64_t>(n_ref, 1));
  return l;
}

bool bad_image(int32_t H, int32_t W) { return H <= 0 || W <= 0 || (int64_t)H * W > (int64_t)1 << 30; }

// ---- transform ---------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void k_trk_transform(const float *__restrict__ pts, const float *__restrict__ T,
                                                            int64_t n, float *__restrict__ out) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const float x = pts[3 * i], y = pts[3 * i + 1], z = pts[3 * i + 2];
    for (int r = 0; r < 3; ++r) out[3 * i + r] = ((T[4 * r] * x + T[4 * r + 1] * y) + T[4 * r + 2] * z) + T[4 * r + 3];
  }
}

// ---- render ------------------------------------------------------------------------------------
__global__ void k_trk_fill_u64(u64 *p, int64_t n, u64 v) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) p[i] = v;
}

// OccupancyOcTreeBase::castRay(origin, direction, end, ignoreUnknownCells = true, maxRange) on the dense box: the
// centre of the first occupied cell in `end`.  Outside the box every cell is unknown, and the box is convex: a ray
// that has been inside and leaves it cannot hit any more.
__device__ bool cast_ray(const mfOccTree &t, const float o[3], const float p[3], float end[3]) {
  const double res = t.resolution, rf = t.res_factor;
  int cur[3];
  if (!(coord_key(o[0], rf, cur[0]) && coord_key(o[1], rf, cur[1]) && coord_key(o[2], rf, cur[2]))) return false;
  int64_t c = cell_of(t, cur[0], cur[1], cur[2]);
  bool inside = c >= 0;
  if (inside && t.logodds[c] >= 0.0f) {  // (NaN: unknown, compares false)
    for (int a = 0; a < 3; ++a) end[a] = (float)(((double)(cur[a] - kKeyMax) + 0.5) * res);
    return true;
  }
  // point3d arithmetic in float, as k_occ_raycast: direction = p - o, norm() = sqrt(double(float nsq))
  float d[3] = {p[0] - o[0], p[1] - o[1], p[2] - o[2]};
  const float nsq = d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
  const double norm = sqrt((double)nsq);
  const double max_range = norm * 1.1, max_range_sq = max_range * max_range;
  const float length = (float)norm;
  if (!(length > 0.0f)) return false;
  for (int a = 0; a < 3; ++a) d[a] = d[a] / length;
  int step[3];
  double tmax[3], tdelta[3];
  for (int a = 0; a < 3; ++a) {
    step[a] = d[a] > 0.0f ? 1 : (d[a] < 0.0f ? -1 : 0);
    if (step[a] != 0) {
      double border = ((double)(cur[a] - kKeyMax) + 0.5) * res;  // keyToCoord
      border += (double)(float)((double)step[a] * res * 0.5);
      tmax[a] = (border - (double)o[a]) / (double)d[a];
      tdelta[a] = res / (double)fabsf(d[a]);
    } else {
      tmax[a] = DBL_MAX;
      tdelta[a] = DBL_MAX;
    }
  }
  if (step[0] == 0 && step[1] == 0 && step[2] == 0) return false;
  for (int it = 0; it < 6 * kKeyMax; ++it) {  // (the range check ends the loop long before)
    const int a = tmax[0] < tmax[1] ? (tmax[0] < tmax[2] ? 0 : 2) : (tmax[1] < tmax[2] ? 1 : 2);
    if ((step[a] < 0 && cur[a] == 0) || (step[a] > 0 && cur[a] == 2 * kKeyMax - 1)) return false;
    cur[a] += step[a];
    tmax[a] += tdelta[a];
    double dist_sq = 0.0;
    for (int b = 0; b < 3; ++b) {
      end[b] = (float)(((double)(cur[b] - kKeyMax) + 0.5) * res);
      const float e = end[b] - o[b];
      dist_sq += (double)(e * e);
    }
    if (dist_sq > max_range_sq) return false;
    c = cell_of(t, cur[0], cur[1], cur[2]);
    if (c >= 0) {
      inside = true;
      if (t.logodds[c] >= 0.0f) return true;
    } else if (inside) {
      return false;
    }
  }
  return false;
}

__global__ __launch_bounds__(kThreads) void k_trk_cast(const float *__restrict__ pts, const float *__restrict__ K,
                                                       const float *__restrict__ T, float ox, float oy, float oz,
                                                       const mfOccTree *__restrict__ trees,
                                                       const int32_t *__restrict__ slots, int n_slots, int H, int W,
                                                       u64 *z) {
  const int Hs = (H + 1) / 2, Ws = (W + 1) / 2;
  const int64_t n = (int64_t)Hs * Ws * n_slots;
  const float o[3] = {ox, oy, oz};
  for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < n; g += (int64_t)gridDim.x * blockDim.x) {
    // neighbouring lanes: neighbouring pixels of one tree (coherent rays)
    const int s = (int)(g / ((int64_t)Hs * Ws));
    const int64_t q = g - (int64_t)s * Hs * Ws;
    const int j = 2 * (int)(q / Ws), i = 2 * (int)(q % Ws);
    const mfOccTree t = trees[slots[2 * s]];
    if (t.dim[0] <= 0) continue;
    const int64_t pix = (int64_t)j * W + i;
    float p[3] = {pts[3 * pix], pts[3 * pix + 1], pts[3 * pix + 2]};
    if (isnan(p[0]) || isnan(p[1]) || isnan(p[2])) {
      // no measurement: the ray through the pixel at z = 1 (OctomapServer.cpp:225-237), no box check
      const float x = ((float)i - K[2]) / K[0], y = ((float)j - K[5]) / K[4];
      for (int r = 0; r < 3; ++r) p[r] = ((T[4 * r] * x + T[4 * r + 1] * y) + T[4 * r + 2]) + T[4 * r + 3];
    } else {
      int k[3];  // inBBX stand-in: the point lies in the tree's box
      if (!(coord_key(p[0], t.res_factor, k[0]) && coord_key(p[1], t.res_factor, k[1]) &&
            coord_key(p[2], t.res_factor, k[2])) || cell_of(t, k[0], k[1], k[2]) < 0)
        continue;
    }
    float end[3];
    if (!cast_ray(t, o, p, end)) continue;
    const float e[3] = {end[0] - o[0], end[1] - o[1], end[2] - o[2]};
    const float dist = (float)sqrt((double)(e[0] * e[0] + e[1] * e[1] + e[2] * e[2]));
    atomicMin(z + q, ((u64)__float_as_uint(dist) << 32) | (u64)(uint32_t)s);  // dist >= 0: bits order like values
  }
}

__global__ __launch_bounds__(kThreads) void k_trk_resolve(const u64 *__restrict__ z, const int32_t *__restrict__ slots,
                                                          int H, int W, int32_t *__restrict__ label,
                                                          float *__restrict__ depth) {
  const int Ws = (W + 1) / 2;
  const int64_t n = (int64_t)H * W;
  for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < n; g += (int64_t)gridDim.x * blockDim.x) {
    const int r = (int)(g / W), c = (int)(g % W);
    const int sr = r + (r & 1), sc = c + (c & 1);  // the stride-2 pixel whose splat (dj, di in {-1, 0}) covers (r, c)
    int32_t l = -2;
    float d = __int_as_float(0x7fc00000);
    if (sr < H && sc < W) {
      const u64 key = z[(int64_t)(sr >> 1) * Ws + (sc >> 1)];
      if (key != kNoHit) {
        l = slots[2 * (int)(key & 0xffffffffull) + 1];
        if (sr == r && sc == c) d = __uint_as_float((uint32_t)(key >> 32));  // the depth image is not splatted
      }
    }
    label[g] = l;
    depth[g] = d;
  }
}

// ---- overlap -----------------------------------------------------------------------------------
// stats layout (int32): inter [n_ref * n_det], then per reference id {area, edge, non-edge}, then per detection
// {area, edge, non-edge}, then per detection {min row, min col, max row, max col}
struct Stats {
  int inter, ref, det, box, total;
};
__host__ __device__ inline Stats stats_of(int n_ref, int n_det) {
  Stats s;
  s.inter = 0;
  s.ref = n_ref * n_det;
  s.det = s.ref + 3 * n_ref;
  s.box = s.det + 3 * n_det;
  s.total = s.box + 4 * n_det;
  return s;
}

__global__ void k_trk_stats_init(int32_t *stats, int n_ref, int n_det) {
  const Stats S = stats_of(n_ref, n_det);
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < S.total; i += gridDim.x * blockDim.x)
    stats[i] = i < S.box ? 0 : (((i - S.box) & 3) < 2 ? INT_MAX : INT_MIN);
}

__device__ __forceinline__ int find_id(const int32_t *ids, int n, int32_t v) {
  if (v < 0) return -1;
  for (int k = 0; k < n; ++k)
    if (ids[k] == v) return k;
  return -1;
}

struct Band {
  int x0, y0, x1, y1;  // the non-edge rectangle, corners included
};
__device__ __forceinline__ bool in_edge(const Band &b, int r, int c) { return !(c >= b.x0 && c <= b.x1 && r >= b.y0 && r <= b.y1); }

template <bool LDS>
__global__ __launch_bounds__(kThreads) void k_trk_overlap(const int32_t *__restrict__ ref, const int32_t *__restrict__ det,
                                                          int H, int W, const int32_t *__restrict__ ref_ids, int n_ref,
                                                          const int32_t *__restrict__ det_ids, int n_det, Band band,
                                                          int32_t *stats) {
  const Stats S = stats_of(n_ref, n_det);
  __shared__ int32_t s_bins[kLdsBins];
  int32_t *bins = stats;
  if (LDS) {
    for (int i = threadIdx.x; i < S.total; i += blockDim.x) s_bins[i] = i < S.box ? 0 : (((i - S.box) & 3) < 2 ? INT_MAX : INT_MIN);
    __syncthreads();
    bins = s_bins;
  }
  const int64_t n = (int64_t)H * W;
  for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < n; g += (int64_t)gridDim.x * blockDim.x) {
    const int r = (int)(g / W), c = (int)(g % W);
    const int a = find_id(ref_ids, n_ref, ref[g]), b = find_id(det_ids, n_det, det[g]);
    if (a < 0 && b < 0) continue;
    const int e = in_edge(band, r, c) ? 1 : 2;
    if (a >= 0) {
      atomicAdd(&bins[S.ref + 3 * a], 1);
      atomicAdd(&bins[S.ref + 3 * a + e], 1);
    }
    if (b >= 0) {
      atomicAdd(&bins[S.det + 3 * b], 1);
      atomicAdd(&bins[S.det + 3 * b + e], 1);
      atomicMin(&bins[S.box + 4 * b], r);
      atomicMin(&bins[S.box + 4 * b + 1], c);
      atomicMax(&bins[S.box + 4 * b + 2], r);
      atomicMax(&bins[S.box + 4 * b + 3], c);
      if (a >= 0) atomicAdd(&bins[S.inter + a * n_det + b], 1);
    }
  }
  if (LDS) {
    __syncthreads();
    for (int i = threadIdx.x; i < S.total; i += blockDim.x) {
      const int32_t v = s_bins[i];
      if (i < S.box) {
        if (v != 0) atomicAdd(&stats[i], v);
      } else if (((i - S.box) & 3) < 2) {
        if (v != INT_MAX) atomicMin(&stats[i], v);
      } else if (v != INT_MIN) {
        atomicMax(&stats[i], v);
      }
    }
  }
}

// ---- assign ------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void k_trk_assign(const int32_t *__restrict__ stats,
                                                         const int32_t *__restrict__ ref_ids, int n_ref, int n_det, int H,
                                                         int W, int min_mask, int min_bbox, int min_side, double iou_thr,
                                                         double cov_thr, int32_t *counter, int32_t *remap,
                                                         int32_t *susp_ref, int32_t *susp_det) {
  const Stats S = stats_of(n_ref, n_det);
  for (int a = threadIdx.x; a < n_ref; a += blockDim.x)
    susp_ref[a] = stats[S.ref + 3 * a + 1] > stats[S.ref + 3 * a + 2];
  for (int b = threadIdx.x; b < n_det; b += blockDim.x) {
    const int area = stats[S.det + 3 * b];
    // best IoU, strict >, from (-1, 0, 0), reference ids in ascending order (geometry.h:150-166)
    int best = -1;
    float best_iou = 0.0f, best_cov = 0.0f;
    for (int a = 0; a < n_ref; ++a) {
      const int area_ref = stats[S.ref + 3 * a];
      if (area_ref == 0) continue;  // not in the rendering: std::set would not hold it
      const int inter = stats[S.inter + a * n_det + b];
      const float iou = (float)inter / (float)(area_ref + area - inter);
      const float cov = (float)inter / (float)area_ref;
      if (iou > best_iou) {
        best = ref_ids[a];
        best_iou = iou;
        best_cov = cov;
      }
    }
    // mask_to_bbox (geometry.h:22-38): one pixel of margin, clipped to the image
    int bh = 0 - (H - 1), bw = 0 - (W - 1);
    if (area > 0) {
      const int y1 = max(stats[S.box + 4 * b] - 1, 0), x1 = max(stats[S.box + 4 * b + 1] - 1, 0);
      const int y2 = min(stats[S.box + 4 * b + 2] + 1, H - 1), x2 = min(stats[S.box + 4 * b + 3] + 1, W - 1);
      bh = y2 - y1;
      bw = x2 - x1;
    }
    const bool small = area < min_mask * min_mask || bh * bw < min_bbox * min_bbox || bh < min_side || bw < min_side;
    const bool edge = stats[S.det + 3 * b + 1] > stats[S.det + 3 * b + 2];
    susp_det[b] = (small ? 2 : 0) | (edge ? 1 : 0);
    // INT_MIN: wants a new id (numbered below, in detection order)
    remap[b] = (small || edge) ? -2 : (((double)best_iou >= iou_thr || (double)best_cov >= cov_thr) ? best : INT_MIN);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int32_t next = *counter;
    for (int b = 0; b < n_det; ++b)
      if (remap[b] == INT_MIN) remap[b] = next++;
    *counter = next;
    remap[n_det] = next;
  }
}

// ---- relabel -----------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void k_trk_relabel(const int32_t *__restrict__ ref, const int32_t *__restrict__ det,
                                                          int H, int W, const int32_t *__restrict__ ref_ids, int n_ref,
                                                          const int32_t *__restrict__ det_ids, int n_det,
                                                          const int32_t *__restrict__ remap,
                                                          const int32_t *__restrict__ susp_ref, Band band,
                                                          int32_t *__restrict__ tracked, int32_t *__restrict__ ref_out) {
  const int64_t n = (int64_t)H * W;
  for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < n; g += (int64_t)gridDim.x * blockDim.x) {
    const int32_t v = det[g];
    int32_t out;
    if (v < 0) {
      out = in_edge(band, (int)(g / W), (int)(g % W)) ? -2 : v;
    } else {
      const int b = find_id(det_ids, n_det, v);
      out = b < 0 ? -2 : remap[b];  // (an id the host did not list: uncertain)
    }
    tracked[g] = out;
    const int32_t u = ref[g];
    const int a = find_id(ref_ids, n_ref, u);
    ref_out[g] = (a >= 0 && susp_ref[a]) ? -2 : u;
  }
}

// ---- clean -------------------------------------------------------------------------------------
// Union-find over pixel indices (parents only ever decrease, committed by atomicMin): a stale read of a parent is
// still an ancestor, so find() stays inside the set and the atomic decides.
__device__ __forceinline__ int uf_find(const int32_t *parent, int x) {
  const volatile int32_t *p = parent;
  int y = p[x];
  while (y != x) {
    x = y;
    y = p[x];
  }
  return x;
}

__device__ void uf_unite(int32_t *parent, int a, int b) {
  for (;;) {
    a = uf_find(parent, a);
    b = uf_find(parent, b);
    if (a == b) return;
    if (a > b) {
      const int t = a;
      a = b;
      b = t;
    }
    const int old = atomicMin(&parent[b], a);  // a < b
    if (old == b) return;
    b = old;
  }
}

__global__ __launch_bounds__(kThreads) void k_trk_cc_init(int64_t n, int32_t *parent, int32_t *count) {
  for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < n; g += (int64_t)gridDim.x * blockDim.x) {
    parent[g] = (int32_t)g;
    count[g] = 0;
  }
}

__global__ __launch_bounds__(kThreads) void k_trk_cc_merge(const int32_t *__restrict__ img, int H, int W, int32_t *parent) {
  const int64_t n = (int64_t)H * W;
  for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < n; g += (int64_t)gridDim.x * blockDim.x) {
    const int32_t v = img[g];
    if (v < 0) continue;
    const int r = (int)(g / W), c = (int)(g % W);
    // the four already-visited neighbours of an 8-neighbourhood: W, NW, N, NE
    if (c > 0 && img[g - 1] == v) uf_unite(parent, (int)g, (int)g - 1);
    if (r > 0) {
      if (c > 0 && img[g - W - 1] == v) uf_unite(parent, (int)g, (int)g - W - 1);
      if (img[g - W] == v) uf_unite(parent, (int)g, (int)g - W);
      if (c + 1 < W && img[g - W + 1] == v) uf_unite(parent, (int)g, (int)g - W + 1);
    }
  }
}

__global__ __launch_bounds__(kThreads) void k_trk_cc_count(const int32_t *__restrict__ img, int64_t n, int32_t *parent,
                                                           int32_t *count) {
  for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < n; g += (int64_t)gridDim.x * blockDim.x) {
    if (img[g] < 0) continue;
    const int root = uf_find(parent, (int)g);
    atomicMin(&parent[g], root);  // flatten (an atomic: other lanes still walk through this entry)
    atomicAdd(&count[root], 1);
  }
}

__global__ __launch_bounds__(kThreads) void k_trk_cc_apply(const int32_t *__restrict__ img, int64_t n,
                                                           const int32_t *__restrict__ parent,
                                                           const int32_t *__restrict__ count, int min_area,
                                                           int32_t *__restrict__ out) {
  for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < n; g += (int64_t)gridDim.x * blockDim.x) {
    const int32_t v = img[g];
    out[g] = (v >= 0 && count[parent[g]] < min_area) ? -2 : v;
  }
}

__global__ __launch_bounds__(kThreads) void k_trk_band_rows(const int32_t *__restrict__ img, int H, int W, int band,
                                                            int32_t *__restrict__ lo, int32_t *__restrict__ hi) {
  const int64_t n = (int64_t)H * W;
  for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < n; g += (int64_t)gridDim.x * blockDim.x) {
    const int c = (int)(g % W);
    const int c0 = max(c - band, 0), c1 = min(c + band, W - 1);
    int32_t mn = INT_MAX, mx = INT_MIN;
    for (int k = c0; k <= c1; ++k) {
      const int32_t v = img[g - c + k];
      mn = min(mn, v);
      mx = max(mx, v);
    }
    lo[g] = mn;
    hi[g] = mx;
  }
}

__global__ __launch_bounds__(kThreads) void k_trk_band_cols(const int32_t *__restrict__ lo, const int32_t *__restrict__ hi,
                                                            int H, int W, int band, int32_t *img) {
  const int64_t n = (int64_t)H * W;
  for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < n; g += (int64_t)gridDim.x * blockDim.x) {
    const int r = (int)(g / W), c = (int)(g % W);
    bool blank = r < band || c < band || r + band > H - 1 || c + band > W - 1;  // the window leaves the image
    if (!blank) {
      int32_t mn = INT_MAX, mx = INT_MIN;
      for (int k = r - band; k <= r + band; ++k) {
        mn = min(mn, lo[(int64_t)k * W + c]);
        mx = max(mx, hi[(int64_t)k * W + c]);
      }
      blank = mn != mx;
    }
    if (blank) img[g] = -2;
  }
}

// ---- merge -------------------------------------------------------------------------------------
__global__ void k_trk_fill_i32(int32_t *p, int n, int32_t v) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) p[i] = v;
}

__global__ __launch_bounds__(kThreads) void k_trk_presence(const int32_t *__restrict__ ref, const int32_t *__restrict__ tgt,
                                                           int64_t n, const int32_t *__restrict__ ref_ids, int n_ref,
                                                           int32_t *presence) {
  for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < n; g += (int64_t)gridDim.x * blockDim.x) {
    const int a = find_id(ref_ids, n_ref, ref[g]), b = find_id(ref_ids, n_ref, tgt[g]);
    if (a >= 0 && !presence[a]) atomicOr(&presence[a], 1);
    if (b >= 0 && !presence[n_ref + b]) atomicOr(&presence[n_ref + b], 1);
  }
}

__global__ __launch_bounds__(kThreads) void k_trk_merge(const int32_t *__restrict__ ref, const int32_t *__restrict__ tgt,
                                                        int64_t n, const int32_t *__restrict__ ref_ids, int n_ref,
                                                        const int32_t *__restrict__ presence, int32_t *__restrict__ merged) {
  // geometry.h:264-280 visits the reference's ids in ascending order and the later mask overwrites: per pixel the
  // larger of {the target's id, if the reference has it too; the reference's id, if the target lacks it}
  for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < n; g += (int64_t)gridDim.x * blockDim.x) {
    int32_t out = -2;
    const int b = find_id(ref_ids, n_ref, tgt[g]);
    if (b >= 0 && presence[b]) out = tgt[g];
    const int a = find_id(ref_ids, n_ref, ref[g]);
    if (a >= 0 && !presence[n_ref + a]) out = max(out, ref[g]);
    merged[g] = out;
  }
}

Band band_of(int H, int W) {  // cv::rectangle(Point(cols * 0.1, rows * 0.1), Point(cols * 0.9, rows * 0.9)): truncated
  Band b;
  b.x0 = (int)(W * 0.1);
  b.y0 = (int)(H * 0.1);
  b.x1 = (int)(W * 0.9);
  b.y1 = (int)(H * 0.9);
  return b;
}

}  // namespace

extern "C" int64_t mf_occtrack_workspace_bytes(int32_t H, int32_t W, int32_t n_ref) {
  if (bad_image(H, W) || n_ref < 0 || n_ref > kMaxIds) return -1;
  return layout_of(H, W, n_ref).total;
}

extern "C" int64_t mf_occtrack_stats_elems(int32_t n_ref, int32_t n_det) {
  if (n_ref < 0 || n_det < 0 || n_ref > kMaxIds || n_det > kMaxIds) return -1;
  return std::max(stats_of(n_ref, n_det).total, 1);
}

extern "C" int mf_occtrack_transform(const float *pts, const float *T, int64_t n, float *out, mfStream_t stream) {
  if (n < 0) return bad("mf_occtrack_transform: negative size");
  if (n == 0) return 0;
  hipLaunchKernelGGL(k_trk_transform, dim3(blocks_for(n)), dim3(kThreads), 0, (hipStream_t)stream, pts, T, n, out);
  return mf::check_launch("mf_occtrack_transform");
}

extern "C" int mf_occtrack_render(const float *pts, const float *K, const float *T, float origin_x, float origin_y,
                                  float origin_z, const mfOccTree *trees, const int32_t *slots, int32_t n_slots,
                                  int32_t H, int32_t W, void *workspace, int32_t *label_rendered, float *depth_rendered,
                                  mfStream_t stream) {
  if (bad_image(H, W) || n_slots < 0 || n_slots > kMaxIds) return bad("mf_occtrack_render: bad sizes");
  if (((uintptr_t)workspace & 15) != 0) return bad("mf_occtrack_render: workspace must be 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  u64 *z = (u64 *)workspace;
  const int64_t nz = (int64_t)((H + 1) / 2) * ((W + 1) / 2);
  hipLaunchKernelGGL(k_trk_fill_u64, dim3(blocks_for(nz)), dim3(kThreads), 0, s, z, nz, kNoHit);
  if (n_slots > 0)
    hipLaunchKernelGGL(k_trk_cast, dim3(blocks_for(nz * n_slots)), dim3(kThreads), 0, s, pts, K, T, origin_x, origin_y,
                       origin_z, trees, slots, (int)n_slots, (int)H, (int)W, z);
  hipLaunchKernelGGL(k_trk_resolve, dim3(blocks_for((int64_t)H * W)), dim3(kThreads), 0, s, z, slots, (int)H, (int)W,
                     label_rendered, depth_rendered);
  return mf::check_launch("mf_occtrack_render");
}

extern "C" int mf_occtrack_overlap(const int32_t *label_rendered, const int32_t *label_detected, int32_t H, int32_t W,
                                   const int32_t *ref_ids, int32_t n_ref, const int32_t *det_ids, int32_t n_det,
                                   int32_t *stats, mfStream_t stream) {
  if (bad_image(H, W) || n_ref < 0 || n_det < 0 || n_ref > kMaxIds || n_det > kMaxIds)
    return bad("mf_occtrack_overlap: bad sizes");
  hipStream_t s = (hipStream_t)stream;
  const Stats S = stats_of(n_ref, n_det);
  if (S.total == 0) return 0;
  hipLaunchKernelGGL(k_trk_stats_init, dim3((S.total + 255) / 256), dim3(256), 0, s, stats, (int)n_ref, (int)n_det);
  const Band band = band_of(H, W);
  const int blocks = std::min(blocks_for((int64_t)H * W), 256);
  if (S.total <= kLdsBins)
    hipLaunchKernelGGL(k_trk_overlap<true>, dim3(blocks), dim3(kThreads), 0, s, label_rendered, label_detected, (int)H,
                       (int)W, ref_ids, (int)n_ref, det_ids, (int)n_det, band, stats);
  else
    hipLaunchKernelGGL(k_trk_overlap<false>, dim3(blocks), dim3(kThreads), 0, s, label_rendered, label_detected, (int)H,
                       (int)W, ref_ids, (int)n_ref, det_ids, (int)n_det, band, stats);
  return mf::check_launch("mf_occtrack_overlap");
}

extern "C" int mf_occtrack_assign(const int32_t *stats, const int32_t *ref_ids, int32_t n_ref, int32_t n_det, int32_t H,
                                  int32_t W, int32_t min_mask, int32_t min_bbox, int32_t min_side, double iou_threshold,
                                  double coverage_threshold, int32_t *counter, int32_t *remap, int32_t *suspicious_ref,
                                  int32_t *suspicious_det, mfStream_t stream) {
  if (bad_image(H, W) || n_ref < 0 || n_det < 0 || n_ref > kMaxIds || n_det > kMaxIds)
    return bad("mf_occtrack_assign: bad sizes");
  if (min_mask < 0 || min_bbox < 0 || min_mask > 32767 || min_bbox > 32767) return bad("mf_occtrack_assign: bad thresholds");
  hipLaunchKernelGGL(k_trk_assign, dim3(1), dim3(kThreads), 0, (hipStream_t)stream, stats, ref_ids, (int)n_ref, (int)n_det,
                     (int)H, (int)W, (int)min_mask, (int)min_bbox, (int)min_side, iou_threshold, coverage_threshold,
                     counter, remap, suspicious_ref, suspicious_det);
  return mf::check_launch("mf_occtrack_assign");
}

extern "C" int mf_occtrack_relabel(const int32_t *label_rendered, const int32_t *label_detected, int32_t H, int32_t W,
                                   const int32_t *ref_ids, int32_t n_ref, const int32_t *det_ids, int32_t n_det,
                                   const int32_t *remap, const int32_t *suspicious_ref, int32_t *label_tracked,
                                   int32_t *label_reference, mfStream_t stream) {
  if (bad_image(H, W) || n_ref < 0 || n_det < 0 || n_ref > kMaxIds || n_det > kMaxIds)
    return bad("mf_occtrack_relabel: bad sizes");
  hipLaunchKernelGGL(k_trk_relabel, dim3(blocks_for((int64_t)H * W)), dim3(kThreads), 0, (hipStream_t)stream, label_rendered,
                     label_detected, (int)H, (int)W, ref_ids, (int)n_ref, det_ids, (int)n_det, remap, suspicious_ref,
                     band_of(H, W), label_tracked, label_reference);
  return mf::check_launch("mf_occtrack_relabel");
}

extern "C" int mf_occtrack_clean(const int32_t *label, int32_t H, int32_t W, int32_t min_area, int32_t band,
                                 void *workspace, int32_t *label_out, mfStream_t stream) {
  if (bad_image(H, W) || band < 0 || min_area < 0) return bad("mf_occtrack_clean: bad sizes");
  if (label == label_out) return bad("mf_occtrack_clean: in place");
  if (((uintptr_t)workspace & 15) != 0) return bad("mf_occtrack_clean: workspace must be 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  const Layout l = layout_of(H, W, 0);
  int32_t *a = (int32_t *)((char *)workspace + l.a), *b = (int32_t *)((char *)workspace + l.b);
  const int64_t n = (int64_t)H * W;
  const dim3 g(blocks_for(n)), t(kThreads);
  hipLaunchKernelGGL(k_trk_cc_init, g, t, 0, s, n, a, b);
  hipLaunchKernelGGL(k_trk_cc_merge, g, t, 0, s, label, (int)H, (int)W, a);
  hipLaunchKernelGGL(k_trk_cc_count, g, t, 0, s, label, n, a, b);
  hipLaunchKernelGGL(k_trk_cc_apply, g, t, 0, s, label, n, a, b, (int)min_area, label_out);
  hipLaunchKernelGGL(k_trk_band_rows, g, t, 0, s, label_out, (int)H, (int)W, (int)band, a, b);
  hipLaunchKernelGGL(k_trk_band_cols, g, t, 0, s, a, b, (int)H, (int)W, (int)band, label_out);
  return mf::check_launch("mf_occtrack_clean");
}

extern "C" int mf_occtrack_merge(const int32_t *label_reference, const int32_t *label_tracked, int32_t H, int32_t W,
                                 const int32_t *ref_ids, int32_t n_ref, void *workspace, int32_t *label_merged,
                                 mfStream_t stream) {
  if (bad_image(H, W) || n_ref < 0 || n_ref > kMaxIds) return bad("mf_occtrack_merge: bad sizes");
  if (((uintptr_t)workspace & 15) != 0) return bad("mf_occtrack_merge: workspace must be 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  int32_t *presence = (int32_t *)((char *)workspace + layout_of(H, W, n_ref).presence);
  const int64_t n = (int64_t)H * W;
  if (n_ref > 0) {
    hipLaunchKernelGGL(k_trk_fill_i32, dim3((2 * n_ref + 255) / 256), dim3(256), 0, s, presence, 2 * (int)n_ref, 0);
    hipLaunchKernelGGL(k_trk_presence, dim3(blocks_for(n)), dim3(kThreads), 0, s, label_reference, label_tracked, n,
                       ref_ids, (int)n_ref, presence);
  }
  hipLaunchKernelGGL(k_trk_merge, dim3(blocks_for(n)), dim3(kThreads), 0, s, label_reference, label_tracked, n, ref_ids,
                     (int)n_ref, presence, label_merged);
  return mf::check_launch("mf_occtrack_merge");
}
