// Picking order: occlusion counts, organised-point-cloud normals and grasp poses (contrib/picking_order.py,
// geometry/estimate_pointcloud_normals.py) -- gfx950, float64.
//
// Reference: ros/src/morefusion_ros/nodes/select_picking_order.py (N + 1 pybullet renders per frame, NumPy over whole
// images, skimage, networkx) and geometry/estimate_pointcloud_normals.py:29-81.  Here the renderer of csrc/render.hip
// draws the composite (target 0) and every item alone (target 1 + n) in one launch, and the three entry points below
// measure them.  DESIGN.md "Picking order" has the contract, tests/picking_ref.py the NumPy mirror this file is
// pinned to bit for bit.
//
//   k_pick_count   a lane per pixel, the items in turn: pixel p is item i's if alone-image i holds item_id[i] there;
//                  it then counts for whole[i], for occluded_by[i][j] with j the composite's owner of p, and for i's
//                  box.  Counted per workgroup in LDS (one LDS atomic per (wave, i, j)), flushed once with integer
//                  atomics: any order gives the same integers.
//   k_pick_finish  a lane per item: the box from the maxima the count kernel kept, (0, 0, 0, 0) for no pixels.
//   k_pick_normals a lane per pixel of every image: pick_normal with the image's rectangle, NaN outside it.
//   k_pick_grasp   a workgroup per item: cells of S x S pixels over the item's box, integer sums per cell in LDS,
//                  the cell nearest the mean centroid, then the mean point and the mean normal of that cell.
//
// pick_normal (shared by both): the anchor p1 at (r, c) and its eight neighbours at offset 2, k = 0 .. 7 at (dy, dx) =
// (-2, 0) (-2, 2) (0, 2) (2, 2) (2, 0) (2, -2) (0, -2) (-2, -2); a neighbour outside the RECTANGLE is NaN.  d_k =
// sqrt((dx dx + dy dy) + dz dz) of (neighbour k - p1); pair k = (neighbour k, neighbour (k + 2) % 8) costs d_k +
// d_(k+2), NaN -> +inf, the first minimum wins; n = a x b with a = p2 - p1, b = p3 - p1 (a1 b2 - a2 b1, a2 b0 - a0 b2,
// a0 b1 - a1 b0), each component divided by sqrt((n0 n0 + n1 n1) + n2 n2).  Nothing is contracted (-ffp-contract=off).
//
// The two float sums of k_pick_grasp (points, normals) are taken in ONE fixed order: the chosen cell's pixels are
// numbered q = 0, 1, ... row-major over the cell's rectangle (clipped to the box); lane t of 256 adds the pixels
// q = t, t + 256, ... in increasing q (a pixel that does not count is skipped); the 256 partial sums are folded by
// s[t] += s[t + h] for h = 128, 64, ... 1.  The kernel is always launched with 256 lanes.
#include <float.h>
#include <limits.h>
#include <math.h>

#include "mf_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kPixPerLane = 4;      // k_pick_count: pixels a lane walks
constexpr int kMaxCells = 1024;     // k_pick_grasp: cells of one box (sides <= MF_RENDER_MAX_SIDE give < 512)
typedef unsigned long long u64;

__device__ __forceinline__ double qnan() { return (double)__uint_as_float(0x7fc00000u); }

__device__ __forceinline__ int last_lane(u64 m) {  // the highest set bit of a non-zero mask
  const uint32_t hi = (uint32_t)(m >> 32), lo = (uint32_t)m;
  return hi ? 63 - __clz((int)hi) : 31 - __clz((int)lo);
}

__global__ void __launch_bounds__(kThreads) k_pick_count(const int32_t *__restrict__ instance,
                                                          const int32_t *__restrict__ item_id, int n, int height,
                                                          int width, int32_t *__restrict__ whole,
                                                          int32_t *__restrict__ occluded_by,
                                                          int32_t *__restrict__ box) {
  __shared__ int32_t s_occ[MF_PICK_MAX_OBJECTS * MF_PICK_MAX_OBJECTS];
  __shared__ int32_t s_whole[MF_PICK_MAX_OBJECTS];
  __shared__ int32_t s_box[4 * MF_PICK_MAX_OBJECTS];
  __shared__ int32_t s_id[MF_PICK_MAX_OBJECTS];
  const int t = threadIdx.x, lane = t & 63;
  for (int k = t; k < n * n; k += kThreads) s_occ[k] = 0;
  for (int k = t; k < n; k += kThreads) { s_whole[k] = 0; s_id[k] = item_id[k]; }
  for (int k = t; k < 4 * n; k += kThreads) s_box[k] = 0;
  __syncthreads();
  const int64_t plane = (int64_t)height * width;
  for (int step = 0; step < kPixPerLane; ++step) {  // (uniform: every lane stays for the wave collectives)
    const int64_t p = ((int64_t)blockIdx.x * kPixPerLane + step) * kThreads + t;
    const bool valid = p < plane;
    const int row = valid ? (int)(p / width) : 0, col = valid ? (int)(p % width) : 0;
    int owner = -1;  // the item that owns p in the composite
    if (valid) {
      const int32_t c = instance[p];
      for (int j = 0; j < n; ++j)
        if (s_id[j] == c) { owner = j; break; }
    }
    for (int i = 0; i < n; ++i) {
      const bool hit = valid && instance[(int64_t)(1 + i) * plane + p] == s_id[i];
      const u64 hits = __ballot(hit);
      if (!hits) continue;  // (uniform over the wave)
      const int first = __ffsll(hits) - 1, last = last_lane(hits);
      const int r0 = __shfl(row, first), r1 = __shfl(row, last), c0 = __shfl(col, first), c1 = __shfl(col, last);
      if (r0 == r1) {  // one image row: rows and columns grow with the lane
        if (lane == first) {
          atomicAdd(&s_whole[i], __popcll(hits));
          atomicMax(&s_box[4 * i], height - r0);
          atomicMax(&s_box[4 * i + 1], width - c0);
          atomicMax(&s_box[4 * i + 2], r1 + 1);
          atomicMax(&s_box[4 * i + 3], c1 + 1);
        }
      } else {
        if (lane == first) {
          atomicAdd(&s_whole[i], __popcll(hits));
          atomicMax(&s_box[4 * i], height - r0);
          atomicMax(&s_box[4 * i + 2], r1 + 1);
        }
        if (hit) {
          atomicMax(&s_box[4 * i + 1], width - col);
          atomicMax(&s_box[4 * i + 3], col + 1);
        }
      }
      // one LDS atomic per (wave, owner): the lanes of the first pending owner are counted and retired
      int mine = hit ? owner : -1;
      u64 pending = __ballot(mine >= 0);
      while (pending) {
        const int j = __shfl(mine, __ffsll(pending) - 1);
        const u64 same = __ballot(mine == j);
        if (lane == __ffsll(same) - 1) atomicAdd(&s_occ[i * n + j], __popcll(same));
        if (mine == j) mine = -1;
        pending = __ballot(mine >= 0);
      }
    }
  }
  __syncthreads();
  for (int k = t; k < n * n; k += kThreads)
    if (s_occ[k]) atomicAdd(occluded_by + k, s_occ[k]);
  for (int k = t; k < n; k += kThreads)
    if (s_whole[k]) atomicAdd(whole + k, s_whole[k]);
  for (int k = t; k < 4 * n; k += kThreads)
    if (s_box[k]) atomicMax(box + k, s_box[k]);
}

// box held (height - min_row, width - min_col, max_row + 1, max_col + 1), zeros for no pixels -> the box
__global__ void __launch_bounds__(kThreads) k_pick_finish(int n, int height, int width,
                                                           const int32_t *__restrict__ whole,
                                                           int32_t *__restrict__ box) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  const bool any = whole[i] > 0;
  box[4 * i] = any ? height - box[4 * i] : 0;
  box[4 * i + 1] = any ? width - box[4 * i + 1] : 0;
  if (!any) { box[4 * i + 2] = 0; box[4 * i + 3] = 0; }
}

struct ArrayPoints {  // points [H, W, 3]
  const double *p;
  int width;
  __device__ __forceinline__ void operator()(int r, int c, double *out) const {
    const double *q = p + 3 * ((int64_t)r * width + c);
    out[0] = q[0]; out[1] = q[1]; out[2] = q[2];
  }
};

struct DepthPoints {  // pointcloud_from_depth of a float32 z-depth image: (z (col - cx)) / fx, (z (row - cy)) / fy, z
  const float *depth;
  int width;
  double fx, fy, cx, cy;
  __device__ __forceinline__ void operator()(int r, int c, double *out) const {
    const float zf = depth[(int64_t)r * width + c];
    if (zf != zf) { out[0] = out[1] = out[2] = qnan(); return; }
    const double z = (double)zf;
    out[0] = (z * ((double)c - cx)) / fx;
    out[1] = (z * ((double)r - cy)) / fy;
    out[2] = z;
  }
};

// the normal of pixel (r, c) of the rectangle rows y1 .. y2 - 1, columns x1 .. x2 - 1 (the header of this file)
template <class Points>
__device__ __forceinline__ void pick_normal(const Points &points, int y1, int x1, int y2, int x2, int r, int c,
                                            double *normal) {
  const int dy[8] = {-2, -2, 0, 2, 2, 2, 0, -2}, dx[8] = {0, 2, 2, 2, 0, -2, -2, -2};
  double p1[3], e[8][3], d[8];
  points(r, c, p1);
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int rr = r + dy[k], cc = c + dx[k];
    if (rr < y1 || rr >= y2 || cc < x1 || cc >= x2) {
      e[k][0] = e[k][1] = e[k][2] = qnan();
    } else {
      double q[3];
      points(rr, cc, q);
      e[k][0] = q[0] - p1[0]; e[k][1] = q[1] - p1[1]; e[k][2] = q[2] - p1[2];
    }
    d[k] = sqrt((e[k][0] * e[k][0] + e[k][1] * e[k][1]) + e[k][2] * e[k][2]);
  }
  int best = 0;
  double best_cost = 0.0;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    double cost = d[k] + d[(k + 2) & 7];
    if (cost != cost) cost = INFINITY;
    if (k == 0 || cost < best_cost) { best = k; best_cost = cost; }
  }
  double a[3] = {0.0, 0.0, 0.0}, b[3] = {0.0, 0.0, 0.0};
#pragma unroll
  for (int k = 0; k < 8; ++k)  // (selects, not indexed loads: the neighbours stay in registers)
    if (k == best)
      for (int x = 0; x < 3; ++x) { a[x] = e[k][x]; b[x] = e[(k + 2) & 7][x]; }
  const double n0 = a[1] * b[2] - a[2] * b[1], n1 = a[2] * b[0] - a[0] * b[2], n2 = a[0] * b[1] - a[1] * b[0];
  const double len = sqrt((n0 * n0 + n1 * n1) + n2 * n2);
  normal[0] = n0 / len; normal[1] = n1 / len; normal[2] = n2 / len;
}

__global__ void __launch_bounds__(kThreads) k_pick_normals(const double *__restrict__ points,
                                                            const int32_t *__restrict__ rect, int height, int width,
                                                            double *__restrict__ normals) {
  const int64_t plane = (int64_t)height * width;
  const int64_t p = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (p >= plane) return;
  const int img = blockIdx.y;
  const int r = (int)(p / width), c = (int)(p % width);
  const int y1 = max(rect[4 * img], 0), x1 = max(rect[4 * img + 1], 0);
  const int y2 = min(rect[4 * img + 2], height), x2 = min(rect[4 * img + 3], width);
  double n[3] = {qnan(), qnan(), qnan()};
  if (r >= y1 && r < y2 && c >= x1 && c < x2) {
    const ArrayPoints src = {points + 3 * plane * img, width};
    pick_normal(src, y1, x1, y2, x2, r, c, n);
  }
  double *out = normals + 3 * (plane * img + p);
  out[0] = n[0]; out[1] = n[1]; out[2] = n[2];
}

__device__ __forceinline__ int isqrt_floor(int64_t v) {
  int64_t s = (int64_t)sqrt((double)v);
  while (s * s > v) --s;
  while ((s + 1) * (s + 1) <= v) ++s;
  return (int)s;
}

__global__ void __launch_bounds__(kThreads) k_pick_grasp(const float *__restrict__ depth,
                                                          const int32_t *__restrict__ instance,
                                                          const int32_t *__restrict__ item_id,
                                                          const int32_t *__restrict__ box, int height, int width,
                                                          double fx, double fy, double cx, double cy,
                                                          int32_t *__restrict__ cell, double *__restrict__ translation,
                                                          double *__restrict__ normal) {
  __shared__ int32_t s_cnt[kMaxCells];
  __shared__ u64 s_row[kMaxCells], s_col[kMaxCells];
  __shared__ double s_sum[7][kThreads];  // point x y z, normal x y z, pixels with a normal
  __shared__ int32_t s_pix[kThreads];
  __shared__ int s_best;
  const int item = blockIdx.x, t = threadIdx.x;
  const int64_t plane = (int64_t)height * width;
  const float *dimg = depth + (int64_t)(1 + item) * plane;
  const int32_t *mimg = instance + (int64_t)(1 + item) * plane;
  const int32_t id = item_id[item];
  const int y1 = max(box[4 * item], 0), x1 = max(box[4 * item + 1], 0);
  const int y2 = min(box[4 * item + 2], height), x2 = min(box[4 * item + 3], width);
  const int h = y2 - y1, w = x2 - x1;
  int S = 1, gh = 0, gw = 0;
  if (h > 0 && w > 0) {
    S = max(1, isqrt_floor(((int64_t)h * w) / 30));
    gh = (h + S - 1) / S;
    gw = (w + S - 1) / S;
  }
  const int cells = (int64_t)gh * gw <= kMaxCells ? gh * gw : 0;  // (everything here is uniform over the workgroup)
  for (int k = t; k < cells; k += kThreads) { s_cnt[k] = 0; s_row[k] = 0; s_col[k] = 0; }
  if (t == 0) s_best = -1;
  __syncthreads();
  if (cells) {
    for (int64_t q = t; q < (int64_t)h * w; q += kThreads) {
      const int r = y1 + (int)(q / w), c = x1 + (int)(q % w);
      if (mimg[(int64_t)r * width + c] != id) continue;
      const int k = ((r - y1) / S) * gw + (c - x1) / S;
      atomicAdd(&s_cnt[k], 1);
      atomicAdd(&s_row[k], (u64)r);
      atomicAdd(&s_col[k], (u64)c);
    }
  }
  __syncthreads();
  if (t == 0 && cells) {  // regions in cell order: the mean centroid, then the first region nearest to it
    double sr = 0.0, sc = 0.0;
    int regions = 0;
    for (int k = 0; k < cells; ++k)
      if (s_cnt[k] > 0) {
        sr += (double)s_row[k] / (double)s_cnt[k];
        sc += (double)s_col[k] / (double)s_cnt[k];
        ++regions;
      }
    if (regions) {
      const double ar = sr / (double)regions, ac = sc / (double)regions;
      double best = 0.0;
      int arg = -1;
      for (int k = 0; k < cells; ++k)
        if (s_cnt[k] > 0) {
          const double dr = (double)s_row[k] / (double)s_cnt[k] - ar, dc = (double)s_col[k] / (double)s_cnt[k] - ac;
          const double dist = sqrt(dr * dr + dc * dc);
          if (arg < 0 || dist < best) { arg = k; best = dist; }
        }
      s_best = arg;
    }
  }
  __syncthreads();
  const int best = s_best;
  double acc[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  int pix = 0;
  if (best >= 0) {
    const int cy1 = y1 + (best / gw) * S, cx1 = x1 + (best % gw) * S;
    const int ch = min(S, y2 - cy1), cw = min(S, x2 - cx1);
    const DepthPoints src = {dimg, width, fx, fy, cx, cy};
    for (int64_t q = t; q < (int64_t)ch * cw; q += kThreads) {
      const int r = cy1 + (int)(q / cw), c = cx1 + (int)(q % cw);
      if (mimg[(int64_t)r * width + c] != id) continue;
      double p[3], n[3];
      src(r, c, p);
      acc[0] += p[0]; acc[1] += p[1]; acc[2] += p[2];
      ++pix;
      pick_normal(src, y1, x1, y2, x2, r, c, n);
      if (n[0] == n[0] && n[1] == n[1] && n[2] == n[2]) {
        acc[3] += n[0]; acc[4] += n[1]; acc[5] += n[2];
        acc[6] += 1.0;
      }
    }
  }
  for (int k = 0; k < 7; ++k) s_sum[k][t] = acc[k];
  s_pix[t] = pix;
  __syncthreads();
  for (int half = kThreads / 2; half >= 1; half /= 2) {
    if (t < half) {
      for (int k = 0; k < 7; ++k) s_sum[k][t] += s_sum[k][t + half];
      s_pix[t] += s_pix[t + half];
    }
    __syncthreads();
  }
  if (t == 0) {
    cell[item] = best;
    const double np = (double)s_pix[0], nn = s_sum[6][0];
    for (int a = 0; a < 3; ++a) {
      translation[3 * item + a] = s_pix[0] > 0 ? s_sum[a][0] / np : qnan();
      normal[3 * item + a] = nn > 0.0 ? s_sum[3 + a][0] / nn : qnan();
    }
  }
}

int bad(const char *what) {
  mf::set_last_error(hipErrorInvalidValue, what);
  return -(int)hipErrorInvalidValue;
}

bool bad_images(int64_t n_images, int32_t height, int32_t width) {
  return height < 1 || width < 1 || height > MF_RENDER_MAX_SIDE || width > MF_RENDER_MAX_SIDE ||
         n_images * height * width > MF_RENDER_MAX_PIXELS;
}

}  // namespace

extern "C" int mf_pick_occlusion(const int32_t *instance, const int32_t *item_id, int32_t n_items, int32_t height,
                                 int32_t width, int32_t *whole, int32_t *occluded_by, int32_t *bbox,
                                 mfStream_t stream) {
  if (n_items < 0 || n_items > MF_PICK_MAX_OBJECTS || bad_images((int64_t)n_items + 1, height, width))
    return bad("mf_pick_occlusion: 0..MF_PICK_MAX_OBJECTS items, images within the MF_RENDER_MAX_* caps");
  if (n_items == 0) return 0;
  if (int rc = mf::fill_bytes(whole, 0, 4 * (int64_t)n_items, (hipStream_t)stream)) return rc;
  if (int rc = mf::fill_bytes(occluded_by, 0, 4 * (int64_t)n_items * n_items, (hipStream_t)stream)) return rc;
  if (int rc = mf::fill_bytes(bbox, 0, 16 * (int64_t)n_items, (hipStream_t)stream)) return rc;
  const int64_t per_block = (int64_t)kThreads * kPixPerLane;
  const int64_t blocks = ((int64_t)height * width + per_block - 1) / per_block;
  hipLaunchKernelGGL(k_pick_count, dim3((unsigned)blocks), dim3(kThreads), 0, (hipStream_t)stream, instance, item_id,
                     (int)n_items, (int)height, (int)width, whole, occluded_by, bbox);
  if (int rc = mf::check_launch("mf_pick_occlusion (count)")) return rc;
  hipLaunchKernelGGL(k_pick_finish, dim3(1), dim3(kThreads), 0, (hipStream_t)stream, (int)n_items, (int)height,
                     (int)width, whole, bbox);
  return mf::check_launch("mf_pick_occlusion (finish)");
}

extern "C" int mf_pick_normals(const double *points, const int32_t *rect, int32_t n_images, int32_t height,
                               int32_t width, double *normals, mfStream_t stream) {
  if (n_images < 0 || n_images > 65535 || bad_images(n_images, height, width))
    return bad("mf_pick_normals: 0..65535 images within the MF_RENDER_MAX_* caps");
  if (n_images == 0) return 0;
  const int64_t blocks = ((int64_t)height * width + kThreads - 1) / kThreads;
  hipLaunchKernelGGL(k_pick_normals, dim3((unsigned)blocks, (unsigned)n_images), dim3(kThreads), 0,
                     (hipStream_t)stream, points, rect, (int)height, (int)width, normals);
  return mf::check_launch("mf_pick_normals");
}

extern "C" int mf_pick_grasp(const float *depth, const int32_t *instance, const int32_t *item_id,
                             const int32_t *bbox, int32_t n_items, int32_t height, int32_t width, double fx,
                             double fy, double cx, double cy, int32_t *cell, double *translation, double *normal,
                             mfStream_t stream) {
  if (n_items < 0 || n_items > MF_PICK_MAX_OBJECTS || bad_images((int64_t)n_items + 1, height, width) ||
      !(fx != 0.0) || !(fy != 0.0))
    return bad("mf_pick_grasp: 0..MF_PICK_MAX_OBJECTS items, images within the MF_RENDER_MAX_* caps, fx, fy != 0");
  if (n_items == 0) return 0;
  hipLaunchKernelGGL(k_pick_grasp, dim3((unsigned)n_items), dim3(kThreads), 0, (hipStream_t)stream, depth, instance,
                     item_id, bbox, (int)height, (int)width, fx, fy, cx, cy, cell, translation, normal);
  return mf::check_launch("mf_pick_grasp");
}
