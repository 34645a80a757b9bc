// Occupancy grids -> welded, smoothed triangle meshes (geometry/grid_mesh.py) -- gfx950.
//
// What the reference's grid_msg_to_mesh (ros/src/morefusion_ros/nodes/voxel_grids_to_mesh_markers.py:80-97) does
// per grid with marching cubes and trimesh.smoothing.filter_humphrey, for a batch of grids.  The surface is the
// 0.5-level set of the occupancy over the six-tetrahedra (Kuhn) subdivision of the padded lattice (DESIGN.md "Grid
// meshes": trimesh / scikit-image parity unpinned).
//
// Lattice: grid b of X x Y x Z cells padded by one empty layer, P = (X + 2, Y + 2, Z + 2) points.  An edge of the
// subdivision whose ends differ in occupancy is a vertex, numbered by its rank in (x, y, z, direction) order; faces are
// numbered in (cell x, y, z, tetrahedron, triangle) order.  The subdivision itself -- corner codes, the edges a point
// owns, which faces a cell has and how they wind -- is kuhn_mesh.h's, shared with csrc/tsdfmesh.hip; the workgroup scan
// is block_scan.h's.
//
// Launches: k_gm_count (grid, x-slab) -> k_gm_scan -> [host reads the offsets] -> k_gm_emit (grid, x-slab);
// k_gm_adj_fill / k_gm_adj_sort build each vertex's neighbour row (at most 12: an edge of the subdivision lies in at
// most 6 tetrahedra, each with at most 2 triangles at it), sorted; k_gm_lap / k_gm_step are one Humphrey iteration.
// Integer atomics count a row's entries, the sort fixes their order; no float atomics, float64 throughout.
#include <limits.h>
#include <math.h>

#include "block_scan.h"
#include "host_args.h"
#include "kuhn_mesh.h"
#include "mf_common.h"

namespace {

constexpr int kWaves = kThreads / 64;
constexpr int kPad = MF_GRIDMESH_MAX_DIM + 2;  // 34 lattice points per axis at most
constexpr int kLayer = kPad * kPad;            // points of one x-layer
constexpr int kNbr = MF_GRIDMESH_MAX_NEIGHBOURS;

struct Grid {
  int X, Y, Z, Px, Py, Pz;
  int64_t off;
};

__device__ __forceinline__ bool load_grid(const int32_t *__restrict__ dims, const int64_t *__restrict__ g_off, int b,
                                          Grid &g) {
  g.X = dims[3 * b];
  g.Y = dims[3 * b + 1];
  g.Z = dims[3 * b + 2];
  g.off = g_off[b];
  const int m = MF_GRIDMESH_MAX_DIM;
  if (g.X < 1 || g.Y < 1 || g.Z < 1 || g.X > m || g.Y > m || g.Z > m || g.off < 0) return false;
  g.Px = g.X + 2;
  g.Py = g.Y + 2;
  g.Pz = g.Z + 2;
  return true;
}

// occupancy of the lattice layers px .. px + NL - 1 into LDS, one byte per point
template <int NL>
__device__ __forceinline__ void load_layers(const float *__restrict__ grids, const Grid &g, int px,
                                            unsigned char (*s_occ)[kLayer]) {
  const int n = g.Py * g.Pz;
  for (int i = threadIdx.x; i < NL * n; i += kThreads) {
    const int L = i / n, r = i - L * n, y = r / g.Pz, z = r - y * g.Pz, x = px + L;
    unsigned char o = 0;
    if (x >= 1 && x <= g.X && y >= 1 && y <= g.Y && z >= 1 && z <= g.Z)
      o = grids[g.off + ((int64_t)(x - 1) * g.Y + (y - 1)) * g.Z + (z - 1)] > 0.0f;
    s_occ[L][r] = o;
  }
}

__device__ __forceinline__ int occ_at(const unsigned char (*s_occ)[kLayer], const Grid &g, int L, int y, int z) {
  return (y < g.Py && z < g.Pz) ? s_occ[L][y * g.Pz + z] : 0;
}

// the active edges of point (layer L, y, z); layer L + 1 must be loaded
__device__ __forceinline__ unsigned point_mask(const unsigned char (*s_occ)[kLayer], const Grid &g, int L, int y, int z) {
  const int o = occ_at(s_occ, g, L, y, z);
  unsigned m = 0;
  m |= (unsigned)(o != occ_at(s_occ, g, L + 1, y, z)) << 0;
  m |= (unsigned)(o != occ_at(s_occ, g, L, y + 1, z)) << 1;
  m |= (unsigned)(o != occ_at(s_occ, g, L, y, z + 1)) << 2;
  m |= (unsigned)(o != occ_at(s_occ, g, L + 1, y + 1, z)) << 3;
  m |= (unsigned)(o != occ_at(s_occ, g, L + 1, y, z + 1)) << 4;
  m |= (unsigned)(o != occ_at(s_occ, g, L, y + 1, z + 1)) << 5;
  m |= (unsigned)(o != occ_at(s_occ, g, L + 1, y + 1, z + 1)) << 6;
  return m;
}

// the 8 corner occupancies of cell (layer 0, y, z), bit = corner code
__device__ __forceinline__ unsigned cell_corners(const unsigned char (*s_occ)[kLayer], const Grid &g, int y, int z) {
  unsigned c = 0;
  for (int k = 0; k < 8; ++k) c |= (unsigned)occ_at(s_occ, g, k >> 2, y + ((k >> 1) & 1), z + (k & 1)) << k;
  return c;
}

// counts[b][px] = vertices of the layer's points | faces of the layer's cells << 16
__global__ __launch_bounds__(kThreads) void k_gm_count(const float *__restrict__ grids, const int64_t *__restrict__ g_off,
                                                       const int32_t *__restrict__ dims, int32_t *__restrict__ counts) {
  __shared__ unsigned char s_occ[2][kLayer];
  __shared__ int s_w[kWaves];
  const int b = blockIdx.y, px = blockIdx.x;
  Grid g;
  if (!load_grid(dims, g_off, b, g) || px >= g.Px) {
    if (threadIdx.x == 0) counts[b * kPad + px] = 0;
    return;
  }
  load_layers<2>(grids, g, px, s_occ);
  __syncthreads();
  int packed = 0;
  const bool cells = px < g.Px - 1;
  for (int i = threadIdx.x; i < g.Py * g.Pz; i += kThreads) {
    const int y = i / g.Pz, z = i - y * g.Pz;
    packed += __popc(point_mask(s_occ, g, 0, y, z));
    if (cells && y < g.Py - 1 && z < g.Pz - 1) packed += cell_faces(cell_corners(s_occ, g, y, z)) << 16;
  }
  int total;
  block_excl_scan<kWaves>(packed, s_w, total);  // a layer has at most 8092 vertices and 13872 faces: no carry between the halves
  if (threadIdx.x == 0) counts[b * kPad + px] = total;
}

// slab_off[b][px] = (vertices, faces) of grid b before layer px; offs[0][b], offs[1][b] = vertices, faces before grid b
__global__ __launch_bounds__(kThreads) void k_gm_scan(const int32_t *__restrict__ counts, const int32_t *__restrict__ dims,
                                                      int B, int32_t *__restrict__ slab_off, int64_t *__restrict__ offs) {
  for (int b = threadIdx.x; b < B; b += kThreads) {
    int v = 0, f = 0;
    const int X = dims[3 * b];
    const int Px = (X >= 1 && X <= MF_GRIDMESH_MAX_DIM) ? X + 2 : 0;
    for (int px = 0; px < kPad; ++px) {
      slab_off[(b * kPad + px) * 2] = v;
      slab_off[(b * kPad + px) * 2 + 1] = f;
      if (px < Px) {
        const int c = counts[b * kPad + px];
        v += c & 0xffff;
        f += c >> 16;
      }
    }
    offs[b + 1] = v;
    offs[(B + 1) + b + 1] = f;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int64_t v = 0, f = 0;
    offs[0] = 0;
    offs[B + 1] = 0;
    for (int b = 1; b <= B; ++b) {
      v += offs[b];
      f += offs[(B + 1) + b];
      offs[b] = v;
      offs[(B + 1) + b] = f;
    }
  }
}

__global__ __launch_bounds__(kThreads) void k_gm_emit(const float *__restrict__ grids, const int64_t *__restrict__ g_off,
                                                      const int32_t *__restrict__ dims, const double *__restrict__ pitch,
                                                      const double *__restrict__ origin,
                                                      const int32_t *__restrict__ slab_off, const int64_t *__restrict__ offs,
                                                      int B, int64_t n_vertices, int64_t n_faces,
                                                      double *__restrict__ vertices, int32_t *__restrict__ faces) {
  __shared__ unsigned char s_occ[3][kLayer];
  __shared__ unsigned char s_mask[2][kLayer];
  __shared__ int s_vbase[2][kLayer];
  __shared__ int s_w[kWaves];
  const int b = blockIdx.y, px = blockIdx.x;
  Grid g;
  if (!load_grid(dims, g_off, b, g) || px >= g.Px) return;
  load_layers<3>(grids, g, px, s_occ);
  __syncthreads();
  const int n = g.Py * g.Pz;
  const int rounds = (n + kThreads - 1) / kThreads;
  for (int L = 0; L < 2; ++L) {
    int running = px + L < kPad ? slab_off[(b * kPad + px + L) * 2] : 0;
    for (int r = 0; r < rounds; ++r) {
      const int i = r * kThreads + threadIdx.x;
      unsigned m = 0;
      if (i < n) m = point_mask(s_occ, g, L, i / g.Pz, i % g.Pz);
      int total;
      const int excl = block_excl_scan<kWaves>((int)__popc(m), s_w, total);
      if (i < n) {
        s_mask[L][i] = (unsigned char)m;
        s_vbase[L][i] = running + excl;
      }
      running += total;
    }
  }
  __syncthreads();
  const int64_t v0 = offs[b], f0 = offs[(B + 1) + b];
  const int64_t v_end = min(offs[b + 1], n_vertices), f_end = min(offs[(B + 1) + b + 1], n_faces);
  const double h = pitch[b], o[3] = {origin[3 * b], origin[3 * b + 1], origin[3 * b + 2]};
  for (int i = threadIdx.x; i < n; i += kThreads) {
    const unsigned m = s_mask[0][i];
    if (!m) continue;
    const int p[3] = {px, i / g.Pz, i % g.Pz};
    int64_t at = v0 + s_vbase[0][i];
    for (int d = 0; d < 7; ++d) {
      if (!((m >> d) & 1u)) continue;
      const int code = code_of_dir(d);
      const int e[3] = {(code >> 2) & 1, (code >> 1) & 1, code & 1};
      if (at >= v0 && at < v_end)
        for (int a = 0; a < 3; ++a) vertices[3 * at + a] = o[a] + h * ((double)(2 * p[a] + e[a]) / 2.0 - 1.0);
      ++at;
    }
  }
  if (px >= g.Px - 1) return;  // the last layer has no cells (uniform over the workgroup)
  const int cz_n = g.Pz - 1, nc = (g.Py - 1) * cz_n;
  int running = slab_off[(b * kPad + px) * 2 + 1];
  for (int r = 0; r < (nc + kThreads - 1) / kThreads; ++r) {
    const int i = r * kThreads + threadIdx.x;
    const int y = i / cz_n, z = i % cz_n;
    const unsigned corners = i < nc ? cell_corners(s_occ, g, y, z) : 0u;
    int total;
    const int64_t at = f0 + running + block_excl_scan<kWaves>(cell_faces(corners), s_w, total);
    running += total;
    const auto vertex_of = [&](int lo, int d) {
      const int pi = (y + ((lo >> 1) & 1)) * g.Pz + z + (lo & 1), L = lo >> 2;  // the owner's point and layer
      return s_vbase[L][pi] + __popc((unsigned)s_mask[L][pi] & ((1u << d) - 1u));
    };
    emit_cell_faces(corners, at, f0, f_end, faces, vertex_of);
  }
}

__global__ void k_gm_zero(int32_t *p, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = 0;
}

// the mesh that holds packed row i: the last b with off[b] <= i
__device__ __forceinline__ int mesh_of(const int64_t *__restrict__ off, int B, int64_t i) {
  int lo = 0, hi = B - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (off[mid] <= i) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

// every directed half-edge a -> b of a face adds b to a's row
__global__ __launch_bounds__(kThreads) void k_gm_adj_fill(const int32_t *__restrict__ faces,
                                                          const int64_t *__restrict__ offs, int B, int64_t n_vertices,
                                                          int64_t n_faces, int32_t *__restrict__ nbr,
                                                          int32_t *__restrict__ deg) {
  const int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= n_faces) return;
  const int b = mesh_of(offs + (B + 1), B, f);
  const int64_t v0 = offs[b], nv = min(offs[b + 1], n_vertices) - v0;
  const int64_t c[3] = {faces[3 * f], faces[3 * f + 1], faces[3 * f + 2]};
  for (int k = 0; k < 3; ++k)
    if (c[k] < 0 || c[k] >= nv) return;
  for (int k = 0; k < 3; ++k) {
    const int64_t a = v0 + c[k], h = v0 + c[(k + 1) % 3];
    const int slot = atomicAdd(&deg[a], 1);
    if (slot < kNbr) nbr[a * kNbr + slot] = (int32_t)h;
  }
}

__global__ __launch_bounds__(kThreads) void k_gm_adj_sort(int64_t n_vertices, int32_t *__restrict__ nbr,
                                                          const int32_t *__restrict__ deg) {
  const int64_t a = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (a >= n_vertices) return;
  const int d = min(deg[a], kNbr);
  int32_t row[kNbr];
  for (int k = 0; k < kNbr; ++k) row[k] = k < d ? nbr[a * kNbr + k] : INT_MAX;
  for (int i = 1; i < kNbr; ++i) {  // insertion sort; the INT_MAX tail stays behind
    const int32_t x = row[i];
    int j = i - 1;
    while (j >= 0 && row[j] > x) {
      row[j + 1] = row[j];
      --j;
    }
    row[j + 1] = x;
  }
  for (int k = 0; k < kNbr; ++k) nbr[a * kNbr + k] = k < d ? row[k] : -1;
}

__global__ void k_gm_copy(const double *__restrict__ src, double *__restrict__ dst, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) dst[i] = src[i];
}

// mean of x over the row of vertex a, summed in ascending neighbour index
__device__ __forceinline__ void row_mean(const double *__restrict__ x, const int32_t *__restrict__ nbr, int64_t a, int d,
                                         int64_t n_vertices, double (&out)[3]) {
  double s[3] = {0.0, 0.0, 0.0};
  for (int k = 0; k < d; ++k) {
    const int64_t h = nbr[a * kNbr + k];
    if (h < 0 || h >= n_vertices) continue;
    for (int c = 0; c < 3; ++c) s[c] = s[c] + x[3 * h + c];
  }
  for (int c = 0; c < 3; ++c) out[c] = s[c] / (double)d;
}

// lap = L q;  bb = lap - (alpha v0 + (1 - alpha) q)
__global__ __launch_bounds__(kThreads) void k_gm_lap(const double *__restrict__ q, const double *__restrict__ v0,
                                                     const int32_t *__restrict__ nbr, const int32_t *__restrict__ deg,
                                                     int64_t n_vertices, double alpha, double *__restrict__ lap,
                                                     double *__restrict__ bb) {
  const int64_t a = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (a >= n_vertices) return;
  const int d = deg[a];
  double m[3];
  if (d >= 1 && d <= kNbr) row_mean(q, nbr, a, d, n_vertices, m);
  for (int c = 0; c < 3; ++c) {
    const double qa = q[3 * a + c];
    const double l = (d >= 1 && d <= kNbr) ? m[c] : qa;
    lap[3 * a + c] = l;
    bb[3 * a + c] = l - (alpha * v0[3 * a + c] + (1.0 - alpha) * qa);
  }
}

// v = lap - (beta bb + (1 - beta) L bb)
__global__ __launch_bounds__(kThreads) void k_gm_step(const double *__restrict__ lap, const double *__restrict__ bb,
                                                      const int32_t *__restrict__ nbr, const int32_t *__restrict__ deg,
                                                      int64_t n_vertices, double beta, double *__restrict__ v) {
  const int64_t a = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (a >= n_vertices) return;
  const int d = deg[a];
  if (!(d >= 1 && d <= kNbr)) return;  // a vertex without a row stays where it is
  double m[3];
  row_mean(bb, nbr, a, d, n_vertices, m);
  for (int c = 0; c < 3; ++c) v[3 * a + c] = lap[3 * a + c] - (beta * bb[3 * a + c] + (1.0 - beta) * m[c]);
}

// render_voxel_grids.py:66-99
__global__ __launch_bounds__(kThreads) void k_gm_label(const float *__restrict__ depth_rendered,
                                                       const int32_t *__restrict__ instance,
                                                       const float *__restrict__ depth_sensor, int64_t n,
                                                       int32_t *__restrict__ label) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int32_t id = instance[i];
  int32_t l = -2;
  if (id != -1) {
    l = id;
    if (depth_rendered[i] > depth_sensor[i] + 0.01f) l = -2;  // false for a NaN reading
  }
  label[i] = l;
}

int64_t count_bytes(int64_t B) { return align16(B * kPad * 4) + align16(B * kPad * 2 * 4); }

unsigned blocks_for(int64_t n) { return (unsigned)((n + kThreads - 1) / kThreads); }

bool bad_total(int64_t n) { return n < 0 || n > MF_GRIDMESH_MAX_ROWS; }

}  // namespace

extern "C" int64_t mf_gridmesh_workspace_bytes(int64_t n_grids, int64_t n_vertices) {
  if (n_grids < 0 || n_grids > MF_GRIDMESH_MAX_GRIDS || bad_total(n_vertices)) return -1;
  return count_bytes(n_grids) + 3 * align16(n_vertices * 3 * 8);
}

extern "C" int mf_gridmesh_count(const float *grids, const int64_t *grid_off, const int32_t *dims, int32_t n_grids,
                                 void *workspace, int64_t *offsets, mfStream_t stream) {
  if (n_grids < 1 || n_grids > MF_GRIDMESH_MAX_GRIDS) return bad("mf_gridmesh_count: 1 .. MF_GRIDMESH_MAX_GRIDS grids");
  int32_t *counts = (int32_t *)workspace;
  int32_t *slab_off = (int32_t *)((char *)workspace + align16((int64_t)n_grids * kPad * 4));
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(k_gm_count, dim3(kPad, n_grids), dim3(kThreads), 0, s, grids, grid_off, dims, counts);
  hipLaunchKernelGGL(k_gm_scan, dim3(1), dim3(kThreads), 0, s, (const int32_t *)counts, dims, (int)n_grids, slab_off,
                     offsets);
  return mf::check_launch("mf_gridmesh_count");
}

extern "C" int mf_gridmesh_emit(const float *grids, const int64_t *grid_off, const int32_t *dims, const double *pitch,
                                const double *origin, int32_t n_grids, const void *workspace, const int64_t *offsets,
                                int64_t n_vertices, int64_t n_faces, double *vertices, int32_t *faces,
                                mfStream_t stream) {
  if (n_grids < 1 || n_grids > MF_GRIDMESH_MAX_GRIDS) return bad("mf_gridmesh_emit: 1 .. MF_GRIDMESH_MAX_GRIDS grids");
  if (bad_total(n_vertices) || bad_total(n_faces)) return bad("mf_gridmesh_emit: totals outside 0 .. MF_GRIDMESH_MAX_ROWS");
  if (n_vertices == 0 && n_faces == 0) return 0;
  const int32_t *slab_off = (const int32_t *)((const char *)workspace + align16((int64_t)n_grids * kPad * 4));
  hipLaunchKernelGGL(k_gm_emit, dim3(kPad, n_grids), dim3(kThreads), 0, (hipStream_t)stream, grids, grid_off, dims,
                     pitch, origin, slab_off, offsets, (int)n_grids, n_vertices, n_faces, vertices, faces);
  return mf::check_launch("mf_gridmesh_emit");
}

extern "C" int mf_gridmesh_adjacency(const int32_t *faces, const int64_t *offsets, int32_t n_grids, int64_t n_vertices,
                                     int64_t n_faces, int32_t *neighbours, int32_t *degree, mfStream_t stream) {
  if (n_grids < 1 || n_grids > MF_GRIDMESH_MAX_GRIDS) return bad("mf_gridmesh_adjacency: 1 .. MF_GRIDMESH_MAX_GRIDS meshes");
  if (bad_total(n_vertices) || bad_total(n_faces)) return bad("mf_gridmesh_adjacency: totals outside 0 .. MF_GRIDMESH_MAX_ROWS");
  if (n_vertices == 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(k_gm_zero, dim3(blocks_for(n_vertices)), dim3(kThreads), 0, s, degree, n_vertices);
  if (n_faces > 0)
    hipLaunchKernelGGL(k_gm_adj_fill, dim3(blocks_for(n_faces)), dim3(kThreads), 0, s, faces, offsets, (int)n_grids,
                       n_vertices, n_faces, neighbours, degree);
  hipLaunchKernelGGL(k_gm_adj_sort, dim3(blocks_for(n_vertices)), dim3(kThreads), 0, s, n_vertices, neighbours,
                     (const int32_t *)degree);
  return mf::check_launch("mf_gridmesh_adjacency");
}

extern "C" int mf_gridmesh_smooth(double *vertices, const int32_t *neighbours, const int32_t *degree,
                                  int64_t n_vertices, double alpha, double beta, int32_t iterations, void *workspace,
                                  mfStream_t stream) {
  if (bad_total(n_vertices) || iterations < 0) return bad("mf_gridmesh_smooth: bad sizes");
  if (n_vertices == 0 || iterations == 0) return 0;
  const int64_t part = align16(n_vertices * 3 * 8);
  double *v0 = (double *)workspace, *lap = (double *)((char *)workspace + part),
         *bb = (double *)((char *)workspace + 2 * part);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(k_gm_copy, dim3(blocks_for(3 * n_vertices)), dim3(kThreads), 0, s, (const double *)vertices, v0,
                     3 * n_vertices);
  for (int it = 0; it < iterations; ++it) {
    hipLaunchKernelGGL(k_gm_lap, dim3(blocks_for(n_vertices)), dim3(kThreads), 0, s, (const double *)vertices,
                       (const double *)v0, neighbours, degree, n_vertices, alpha, lap, bb);
    hipLaunchKernelGGL(k_gm_step, dim3(blocks_for(n_vertices)), dim3(kThreads), 0, s, (const double *)lap,
                       (const double *)bb, neighbours, degree, n_vertices, beta, vertices);
  }
  return mf::check_launch("mf_gridmesh_smooth");
}

extern "C" int mf_gridmesh_label(const float *depth_rendered, const int32_t *instance, const float *depth_sensor,
                                 int32_t height, int32_t width, int32_t *label, mfStream_t stream) {
  if (height <= 0 || width <= 0 || (int64_t)height * width > INT_MAX) return bad("mf_gridmesh_label: bad image size");
  const int64_t n = (int64_t)height * width;
  hipLaunchKernelGGL(k_gm_label, dim3(blocks_for(n)), dim3(kThreads), 0, (hipStream_t)stream, depth_rendered, instance,
                     depth_sensor, n, label);
  return mf::check_launch("mf_gridmesh_label");
}
