// Depth / instance rasteriser and the dataset's full grids (geometry/render.py) -- gfx950, float64 coverage.
//
// Reference: morefusion/extra/_pybullet.py render_cad (an OpenGL render of one CAD model at its pose, used by
// datasets/rgbd_pose_estimation/base.py get_example for mask_rend) and base.py _get_grid_full.  pybullet is not
// linked: DESIGN.md "Mesh rendering" has the contract, tests/render_ref.py the NumPy mirror this file is pinned to
// bit for bit.
//
// A launch renders N items (mesh, float64 T_cad2cam, target image, instance id); record r = item_rec_off[n] + f is
// face f of item n.
//   k_render_setup   one lane per record.  Vertices to the camera frame, x' = ((T0 x + T1 y) + T2 z) + T3 per row,
//                    and to the image, u = (fx x') / z' + cx, v = (fy y') / z' + cy.  A face with an index outside
//                    its mesh, a vertex at z' <= near or a non-finite u, v is dropped.  Box: columns
//                    max(ceil(min u), 0) .. min(floor(max u), W - 1), rows alike.  Edge k joins corners k and
//                    (k + 1) % 3, taken from A to B with A the corner of smaller (v, u) (canonical: both faces at a
//                    shared edge evaluate the same expression): E(p) = du (pv - vA) - dv (pu - uA) with du = uB - uA,
//                    dv = vB - vA.  s = E(third corner); s == 0 on any edge: zero area, dropped.  Plane: n = (b - a) x
//                    (c - a) in the camera frame, d = n . a.
//   k_render_small   one lane per record whose box holds <= kSmallBox pixels: every pixel of the box.
//   k_render_large   the others, listed by the setup kernel: a workgroup per (listed face, 32 x 32 image tile).
//   Per pixel (row i, col j), p = (j, i): inside edge k iff E(p) has the sign of s, or E(p) == 0 and the edge is a
//   top edge (dv == 0, face on the side of larger v) or a left edge (dv > 0, face on the side of larger u) of the
//   face.  Depth z = d / ((nx rx + ny ry) + nz), rx = (j - cx) / fx, ry = (i - cy) / fy, rounded once to float32;
//   a pixel whose float32 depth is not in (0, inf) is not drawn.  key = depth bits << 32 | r; atomic minimum.
//   k_render_resolve one lane per pixel: the key back to depth / instance / face; pixels per item counted with one
//                    integer atomic per (wave, item).
// Nothing here depends on the order in which lanes or workgroups run: every output is bitwise reproducible.
#include <float.h>
#include <limits.h>
#include <math.h>

#include "mf_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kRecD = 16;        // doubles per record: 3 x (uA, vA, du, dv), nx, ny, nz, d
constexpr int kRecI = 8;         // ints per record: x0, y0, x1, y1 (inclusive; x1 < x0: nothing), flags, target, item, face
constexpr int kSmallBox = 64;    // pixels in a box a single lane walks
constexpr int kTile = 32;        // the large pass: 32 x 32 pixels per workgroup, 4 per lane
constexpr int kLargeSlots = 64;  // workgroups per tile striding over the listed faces
typedef unsigned long long u64;
constexpr u64 kEmpty = ~0ull;

struct Ws {
  u64 *zbuf;
  double *recd;
  int32_t *reci;
  int32_t *n_large;
  int32_t *large;
};

__host__ __device__ inline int64_t align16(int64_t x) { return (x + 15) & ~(int64_t)15; }

__host__ __device__ inline Ws carve(void *ws, int64_t records, int64_t pixels) {
  Ws w;
  unsigned char *p = (unsigned char *)ws;
  w.zbuf = (u64 *)p;
  p += align16(8 * pixels);
  w.recd = (double *)p;
  p += align16((int64_t)sizeof(double) * kRecD * records);
  w.reci = (int32_t *)p;
  p += align16((int64_t)sizeof(int32_t) * kRecI * records);
  w.n_large = (int32_t *)p;
  p += 16;
  w.large = (int32_t *)p;
  return w;
}

__global__ void __launch_bounds__(kThreads) k_render_setup(mfRenderBatch P, int64_t total) {
  const int64_t r = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (r >= total) return;
  const Ws w = carve(P.workspace, total, (int64_t)P.n_targets * P.height * P.width);
  int lo = 0, hi = P.n_items - 1;  // the item n with item_rec_off[n] <= r < item_rec_off[n + 1]
  while (lo < hi) {
    const int mid = (lo + hi + 1) / 2;
    if (P.item_rec_off[mid] <= r) lo = mid; else hi = mid - 1;
  }
  const int item = lo;
  const int64_t f = r - P.item_rec_off[item];
  double *rd = w.recd + r * kRecD;
  int32_t *ri = w.reci + r * kRecI;
  for (int k = 0; k < kRecD; ++k) rd[k] = 0.0;
  ri[0] = 0; ri[1] = 0; ri[2] = -1; ri[3] = -1; ri[4] = 0;
  ri[5] = P.item_target[item]; ri[6] = item; ri[7] = (int32_t)f;
  const int32_t mesh = P.item_mesh[item];
  if (mesh < 0 || mesh >= P.n_meshes || ri[5] < 0 || ri[5] >= P.n_targets) return;
  const int64_t v0 = P.v_off[mesh], nv = P.v_off[mesh + 1] - v0;
  const int64_t f0 = P.f_off[mesh], nf = P.f_off[mesh + 1] - f0;
  if (f >= nf) return;
  const double *T = P.item_T + 16 * (int64_t)item;
  double c[3][3], u[3], v[3];
  for (int k = 0; k < 3; ++k) {
    const int32_t i = P.faces[3 * (f0 + f) + k];
    if (i < 0 || (int64_t)i >= nv) return;
    const double x = P.vertices[3 * (v0 + i)], y = P.vertices[3 * (v0 + i) + 1], z = P.vertices[3 * (v0 + i) + 2];
    for (int a = 0; a < 3; ++a) c[k][a] = ((T[4 * a] * x + T[4 * a + 1] * y) + T[4 * a + 2] * z) + T[4 * a + 3];
    if (!(c[k][2] > P.near)) return;
    u[k] = (P.fx * c[k][0]) / c[k][2] + P.cx;
    v[k] = (P.fy * c[k][1]) / c[k][2] + P.cy;
    if (!(fabs(u[k]) <= DBL_MAX) || !(fabs(v[k]) <= DBL_MAX)) return;
  }
  int flags = 1;
  for (int k = 0; k < 3; ++k) {
    int a = k, b = (k + 1) % 3;
    const int o = (k + 2) % 3;
    if (v[b] < v[a] || (v[b] == v[a] && u[b] < u[a])) { const int t = a; a = b; b = t; }
    const double du = u[b] - u[a], dv = v[b] - v[a];
    const double s = du * (v[o] - v[a]) - dv * (u[o] - u[a]);
    if (s == 0.0 || s != s) return;
    rd[4 * k] = u[a]; rd[4 * k + 1] = v[a]; rd[4 * k + 2] = du; rd[4 * k + 3] = dv;
    const bool pos = s > 0.0;
    const bool owns = dv > 0.0 ? !pos : pos;  // left edge: the face lies where E < 0; top edge: where E > 0
    flags |= (pos ? 1 : 0) << (1 + 2 * k) | (owns ? 1 : 0) << (2 + 2 * k);
  }
  const double e1x = c[1][0] - c[0][0], e1y = c[1][1] - c[0][1], e1z = c[1][2] - c[0][2];
  const double e2x = c[2][0] - c[0][0], e2y = c[2][1] - c[0][1], e2z = c[2][2] - c[0][2];
  const double nx = e1y * e2z - e1z * e2y, ny = e1z * e2x - e1x * e2z, nz = e1x * e2y - e1y * e2x;
  rd[12] = nx; rd[13] = ny; rd[14] = nz;
  rd[15] = (nx * c[0][0] + ny * c[0][1]) + nz * c[0][2];
  const double umin = fmin(fmin(u[0], u[1]), u[2]), umax = fmax(fmax(u[0], u[1]), u[2]);
  const double vmin = fmin(fmin(v[0], v[1]), v[2]), vmax = fmax(fmax(v[0], v[1]), v[2]);
  const double x0 = fmax(ceil(umin), 0.0), x1 = fmin(floor(umax), (double)(P.width - 1));
  const double y0 = fmax(ceil(vmin), 0.0), y1 = fmin(floor(vmax), (double)(P.height - 1));
  if (!(x0 <= x1) || !(y0 <= y1)) return;
  ri[0] = (int32_t)x0; ri[1] = (int32_t)y0; ri[2] = (int32_t)x1; ri[3] = (int32_t)y1;
  ri[4] = flags;
  const int64_t box = (int64_t)(ri[2] - ri[0] + 1) * (ri[3] - ri[1] + 1);
  if (box > kSmallBox) w.large[atomicAdd(w.n_large, 1)] = (int32_t)r;
}

// the pixel (row i, col j) against record (rd, flags): true and the float32 depth bits if the face covers it
__device__ __forceinline__ bool shade(const double *rd, int flags, const mfRenderBatch &P, int i, int j,
                                      uint32_t *bits) {
  const double pu = (double)j, pv = (double)i;
  for (int k = 0; k < 3; ++k) {
    const double e = rd[4 * k + 2] * (pv - rd[4 * k + 1]) - rd[4 * k + 3] * (pu - rd[4 * k]);
    const bool pos = (flags >> (1 + 2 * k)) & 1, owns = (flags >> (2 + 2 * k)) & 1;
    const bool in = e == 0.0 ? owns : (pos ? e > 0.0 : e < 0.0);
    if (!in) return false;
  }
  const double rx = (pu - P.cx) / P.fx, ry = (pv - P.cy) / P.fy;
  const double z = rd[15] / ((rd[12] * rx + rd[13] * ry) + rd[14]);
  const float zf = (float)z;
  if (!(zf > 0.0f) || !(zf <= FLT_MAX)) return false;
  *bits = __float_as_uint(zf);
  return true;
}

__global__ void __launch_bounds__(kThreads) k_render_small(mfRenderBatch P, int64_t total) {
  const int64_t r = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (r >= total) return;
  const int64_t plane = (int64_t)P.height * P.width;
  const Ws w = carve(P.workspace, total, (int64_t)P.n_targets * plane);
  const int32_t *ri = w.reci + r * kRecI;
  const int x0 = ri[0], y0 = ri[1], x1 = ri[2], y1 = ri[3], flags = ri[4];
  if (!(flags & 1) || x1 < x0 || y1 < y0) return;
  if ((int64_t)(x1 - x0 + 1) * (y1 - y0 + 1) > kSmallBox) return;
  double rd[kRecD];
  for (int k = 0; k < kRecD; ++k) rd[k] = w.recd[r * kRecD + k];
  u64 *z = w.zbuf + (int64_t)ri[5] * plane;
  for (int i = y0; i <= y1; ++i)
    for (int j = x0; j <= x1; ++j) {
      uint32_t bits;
      if (shade(rd, flags, P, i, j, &bits)) atomicMin(z + (int64_t)i * P.width + j, ((u64)bits << 32) | (u64)r);
    }
}

__global__ void __launch_bounds__(kThreads) k_render_large(mfRenderBatch P, int64_t total) {
  __shared__ double s_rd[kRecD];
  __shared__ int32_t s_ri[kRecI];
  const int64_t plane = (int64_t)P.height * P.width;
  const Ws w = carve(P.workspace, total, (int64_t)P.n_targets * plane);
  const int n_large = *w.n_large;
  const int tiles_x = (P.width + kTile - 1) / kTile;
  const int tx0 = ((int)blockIdx.y % tiles_x) * kTile, ty0 = ((int)blockIdx.y / tiles_x) * kTile;
  const int t = threadIdx.x;
  for (int k = blockIdx.x; k < n_large; k += gridDim.x) {  // (uniform over the workgroup)
    const int64_t r = w.large[k];
    __syncthreads();  // the previous record is consumed
    if (t < kRecD) s_rd[t] = w.recd[r * kRecD + t];
    if (t >= 64 && t < 64 + kRecI) s_ri[t - 64] = w.reci[r * kRecI + (t - 64)];
    __syncthreads();
    const int x0 = max(s_ri[0], tx0), x1 = min(s_ri[2], tx0 + kTile - 1);
    const int y0 = max(s_ri[1], ty0), y1 = min(s_ri[3], ty0 + kTile - 1);
    if (x1 < x0 || y1 < y0) continue;  // the box misses this tile (uniform)
    const int flags = s_ri[4];
    u64 *z = w.zbuf + (int64_t)s_ri[5] * plane;
    const int j = tx0 + (t & (kTile - 1));
    if (j < x0 || j > x1) continue;
    for (int i = ty0 + (t >> 5); i <= y1; i += kThreads / kTile) {
      if (i < y0) continue;
      uint32_t bits;
      if (shade(s_rd, flags, P, i, j, &bits)) atomicMin(z + (int64_t)i * P.width + j, ((u64)bits << 32) | (u64)r);
    }
  }
}

__global__ void __launch_bounds__(kThreads) k_render_resolve(mfRenderBatch P, int64_t total, int64_t pixels) {
  const int64_t p = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  const Ws w = carve(P.workspace, total, pixels);
  int item = -1;
  if (p < pixels) {
    const u64 key = w.zbuf[p];
    float d = __uint_as_float(0x7fc00000u);
    int32_t id = -1, face = -1;
    if (key != kEmpty) {
      const int64_t r = (int64_t)(key & 0xffffffffull);
      d = __uint_as_float((uint32_t)(key >> 32));
      item = w.reci[r * kRecI + 6];
      face = w.reci[r * kRecI + 7];
      id = P.item_id[item];
    }
    P.depth[p] = d;
    P.instance[p] = id;
    P.face[p] = face;
  }
  // one atomic per (wave, item): the lanes of the first pending item are counted and retired, until none is left
  const int lane = threadIdx.x & 63;
  u64 pending = __ballot(item >= 0);
  while (pending) {
    const int first = __shfl(item, __ffsll(pending) - 1);
    const u64 same = __ballot(item == first);
    if (lane == __ffsll(same) - 1) atomicAdd(P.count + first, __popcll(same));
    if (item == first) item = -1;
    pending = __ballot(item >= 0);
  }
}

// grid.x over the packed points, grid.y = the target example e
__global__ void __launch_bounds__(kThreads) k_full_grids(const double *__restrict__ points,
                                                           const int64_t *__restrict__ p_off,
                                                           const double *__restrict__ T,
                                                           const double *__restrict__ pitch,
                                                           const double *__restrict__ origin, int n, int dim,
                                                           int32_t *__restrict__ target_full,
                                                           int32_t *__restrict__ nontarget_full) {
  const int64_t q = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (q >= p_off[n]) return;
  const int e = blockIdx.y;
  int lo = 0, hi = n - 1;  // the example i whose points hold q
  while (lo < hi) {
    const int mid = (lo + hi + 1) / 2;
    if (p_off[mid] <= q) lo = mid; else hi = mid - 1;
  }
  const int i = lo;
  const double *Ti = T + 16 * (int64_t)i;
  const double x = points[3 * q], y = points[3 * q + 1], z = points[3 * q + 2];
  const double h = pitch[e];
  int idx[3];
  for (int a = 0; a < 3; ++a) {
    const double c = ((Ti[4 * a] * x + Ti[4 * a + 1] * y) + Ti[4 * a + 2] * z) + Ti[4 * a + 3];
    const double g = rint((c - origin[3 * e + a]) / h);  // half to even, as np.round
    if (!(g >= 0.0 && g < (double)dim)) return;
    idx[a] = (int)g;
  }
  const int64_t cell = (((int64_t)e * dim + idx[0]) * dim + idx[1]) * dim + idx[2];
  if (i == e)
    target_full[cell] = 1;
  else
    atomicMax(nontarget_full + cell, (i < e ? i : i - 1) + 1);  // the reference's last writer: the largest label
}

int bad(const char *what) {
  mf::set_last_error(hipErrorInvalidValue, what);
  return -(int)hipErrorInvalidValue;
}

int check_batch(const mfRenderBatch *b, int64_t total, const char *what) {
  if (!b) return bad(what);
  if (b->n_items < 0 || b->n_items > MF_RENDER_MAX_ITEMS || b->n_meshes < 0 || b->n_targets < 0 || b->height < 1 ||
      b->width < 1 || !(b->fx != 0.0) || !(b->fy != 0.0))
    return bad(what);
  if (mf_render_workspace_bytes(total, b->n_targets, b->height, b->width) < 0) return bad(what);
  if (!b->workspace || ((uintptr_t)b->workspace & 15)) return bad(what);
  return 0;
}

}  // namespace

extern "C" int64_t mf_render_workspace_bytes(int64_t total_records, int64_t n_targets, int64_t height,
                                             int64_t width) {
  if (total_records < 0 || total_records > MF_RENDER_MAX_FACES || n_targets < 0 || height < 1 || width < 1 ||
      height > MF_RENDER_MAX_SIDE || width > MF_RENDER_MAX_SIDE || n_targets > MF_RENDER_MAX_PIXELS)
    return -1;
  const int64_t pixels = n_targets * height * width;
  if (pixels > MF_RENDER_MAX_PIXELS) return -1;
  return align16(8 * pixels) + align16((int64_t)sizeof(double) * kRecD * total_records) +
         align16((int64_t)sizeof(int32_t) * kRecI * total_records) + 16 + align16(4 * total_records) + 16;
}

extern "C" int mf_render_setup(const mfRenderBatch *batch, int64_t total_records, mfStream_t stream) {
  if (int rc = check_batch(batch, total_records, "mf_render_setup: bad batch")) return rc;
  const mfRenderBatch &P = *batch;
  const int64_t pixels = (int64_t)P.n_targets * P.height * P.width;
  const Ws w = carve(P.workspace, total_records, pixels);
  if (pixels)
    if (int rc = mf::fill_bytes(w.zbuf, 0xff, 8 * pixels, (hipStream_t)stream)) return rc;
  if (int rc = mf::fill_bytes(w.n_large, 0, 16, (hipStream_t)stream)) return rc;
  if (total_records == 0) return 0;
  const int64_t blocks = (total_records + kThreads - 1) / kThreads;
  hipLaunchKernelGGL(k_render_setup, dim3((unsigned)blocks), dim3(kThreads), 0, (hipStream_t)stream, P,
                     total_records);
  return mf::check_launch("mf_render_setup");
}

extern "C" int mf_render_raster(const mfRenderBatch *batch, int64_t total_records, mfStream_t stream) {
  if (int rc = check_batch(batch, total_records, "mf_render_raster: bad batch")) return rc;
  const mfRenderBatch &P = *batch;
  if (total_records == 0 || P.n_targets == 0) return 0;
  const int64_t blocks = (total_records + kThreads - 1) / kThreads;
  hipLaunchKernelGGL(k_render_small, dim3((unsigned)blocks), dim3(kThreads), 0, (hipStream_t)stream, P,
                     total_records);
  if (int rc = mf::check_launch("mf_render_raster (small)")) return rc;
  const int tiles = ((P.width + kTile - 1) / kTile) * ((P.height + kTile - 1) / kTile);
  const int slots = total_records < kLargeSlots ? (int)total_records : kLargeSlots;
  hipLaunchKernelGGL(k_render_large, dim3((unsigned)slots, (unsigned)tiles), dim3(kThreads), 0, (hipStream_t)stream,
                     P, total_records);
  return mf::check_launch("mf_render_raster (large)");
}

extern "C" int mf_render_resolve(const mfRenderBatch *batch, int64_t total_records, mfStream_t stream) {
  if (int rc = check_batch(batch, total_records, "mf_render_resolve: bad batch")) return rc;
  const mfRenderBatch &P = *batch;
  if (P.n_items)
    if (int rc = mf::fill_bytes(P.count, 0, 4 * (int64_t)P.n_items, (hipStream_t)stream)) return rc;
  const int64_t pixels = (int64_t)P.n_targets * P.height * P.width;
  if (pixels == 0) return 0;
  const int64_t blocks = (pixels + kThreads - 1) / kThreads;
  hipLaunchKernelGGL(k_render_resolve, dim3((unsigned)blocks), dim3(kThreads), 0, (hipStream_t)stream, P,
                     total_records, pixels);
  return mf::check_launch("mf_render_resolve");
}

extern "C" int mf_full_grids(const double *points, const int64_t *p_off, const double *T, const double *pitch,
                             const double *origin, int32_t n_examples, int64_t total_points, int32_t dim,
                             int32_t *target_full, int32_t *nontarget_full, mfStream_t stream) {
  if (n_examples < 0 || n_examples > 65535 || dim < 1 || dim > 256 || total_points < 0 ||
      total_points > ((int64_t)1 << 31) * kThreads - 1)
    return bad("mf_full_grids: 0..65535 examples, 1 <= dim <= 256");
  if (n_examples == 0) return 0;
  const int64_t cells = 4 * (int64_t)n_examples * dim * dim * dim;
  if (int rc = mf::fill_bytes(target_full, 0, cells, (hipStream_t)stream)) return rc;
  if (int rc = mf::fill_bytes(nontarget_full, 0, cells, (hipStream_t)stream)) return rc;
  if (total_points == 0) return 0;
  const int64_t blocks = (total_points + kThreads - 1) / kThreads;
  hipLaunchKernelGGL(k_full_grids, dim3((unsigned)blocks, (unsigned)n_examples), dim3(kThreads), 0,
                     (hipStream_t)stream, points, p_off, T, pitch, origin, (int)n_examples, (int)dim, target_full,
                     nontarget_full);
  return mf::check_launch("mf_full_grids");
}
