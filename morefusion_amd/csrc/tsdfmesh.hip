// TSDF volume -> welded triangle mesh with normals (contrib/tsdf_volume.py TsdfVolume.extract_mesh) -- gfx950.
//
// include/mfhip.h "TSDF mesh" is the contract -- inside / observed, the vertex and face orders, every formula and its
// association -- and tests/tsdfmesh_ref.py the NumPy mirror this file is pinned to bit for bit; DESIGN.md "TSDF mesh"
// has the cost model.  The triangulation is the six-tetrahedra subdivision of csrc/gridmesh.hip: its tables, face
// count and face emitter are kuhn_mesh.h's, one text for both files, and the workgroup scan is block_scan.h's.  What
// differs is the lattice: a volume far larger than LDS, x fastest, vertices interpolated along their edges, and cells
// the camera never saw left out.
//
//   k_tm_flags  a lane per 4 lattice points: the volume is read once, 32 contiguous bytes per lane, and leaves one
//               byte per point (bit 0 inside, bit 1 observed).  Everything below reads bytes, not the volume.
//   k_tm_count  a workgroup per row (k, j), a lane per point along x in chunks of 256.  A lane folds the 9 rows
//               (k - 1 .. k + 1, j - 1 .. j + 1) of its column into one byte in LDS -- which of the four (y, z) quads
//               around the row are observed, and inside of the four rows (k .. k + 1, j .. j + 1) -- and a point's
//               7-bit mask of vertex-carrying edges and its cell's face count come from the bytes of columns i - 1, i,
//               i + 1.  One mask byte per point and a (vertices, faces) pair per row go to the workspace.
//   k_tm_scan   one workgroup: the row pairs become exclusive offsets in place, the totals go behind them.
//   k_tm_emit   a workgroup per row; a row without vertices and faces returns at once.  A vertex's index is the
//               row's offset plus the prefix popcount of the row's masks: one workgroup scan per chunk carries the four
//               rows a cell touches and the cell's faces in 12-bit fields of one 64-bit word.  Positions and normals
//               read the volume only at the surface.
//
// Integer sums only (no atomics at all), float64 arithmetic on widened float32, nothing contracted.
#include <math.h>

#include "block_scan.h"
#include "host_args.h"
#include "kuhn_mesh.h"
#include "mf_common.h"
#include "tsdf_voxel.h"

namespace {

using mf_tsdf::Grid;

constexpr int kWaves = kThreads / 64;
constexpr int kScanThreads = 1024;

constexpr unsigned kInside = 1u, kObserved = 2u;

__device__ __forceinline__ unsigned flag_of(float f, float w, double min_weight) {
  return (f <= 0.0f ? kInside : 0u) | ((double)w >= min_weight ? kObserved : 0u);
}

__global__ __launch_bounds__(kThreads) void k_tm_flags(const float *__restrict__ vol, int64_t n, double min_weight,
                                                       uint8_t *__restrict__ flags) {
  const int64_t q = ((int64_t)blockIdx.x * kThreads + threadIdx.x) * 4;
  if (q >= n) return;
  if (q + 4 <= n) {
    const float4 a = *(const float4 *)(vol + 2 * q), b = *(const float4 *)(vol + 2 * q + 4);
    *(uint32_t *)(flags + q) = flag_of(a.x, a.y, min_weight) | (flag_of(a.z, a.w, min_weight) << 8) |
                               (flag_of(b.x, b.y, min_weight) << 16) | (flag_of(b.z, b.w, min_weight) << 24);
  } else {
    for (int64_t m = q; m < n; ++m) flags[m] = (uint8_t)flag_of(vol[2 * m], vol[2 * m + 1], min_weight);
  }
}

// Column x of the rows around (k, j), folded into a byte.  Bit (cz + 1) * 2 + (cy + 1), cz, cy in {-1, 0}: the four
// points (x, j + cy + {0, 1}, k + cz + {0, 1}) are all observed.  Bit 4 + dz * 2 + dy: point (x, j + dy, k + dz) is
// inside.  A point outside the lattice is neither.
__device__ __forceinline__ unsigned count_column(const uint8_t *__restrict__ flags, int nx, int ny, int nz, int x, int j,
                                                 int k) {
  if (x < 0 || x >= nx) return 0u;
  unsigned f[3][3];
#pragma unroll
  for (int dz = -1; dz <= 1; ++dz)
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy) {
      const int y = j + dy, z = k + dz;
      f[dz + 1][dy + 1] = (y >= 0 && y < ny && z >= 0 && z < nz) ? flags[((int64_t)z * ny + y) * nx + x] : 0u;
    }
  unsigned c = 0;
#pragma unroll
  for (int cz = 0; cz < 2; ++cz)
#pragma unroll
    for (int cy = 0; cy < 2; ++cy) {
      const unsigned all = f[cz][cy] & f[cz][cy + 1] & f[cz + 1][cy] & f[cz + 1][cy + 1];
      c |= ((all >> 1) & 1u) << (cz * 2 + cy);
      c |= (f[cz + 1][cy + 1] & kInside) << (4 + cz * 2 + cy);
    }
  return c;
}

// the vertex-carrying owned edges of a point from the bytes of its columns i - 1, i, i + 1
__device__ __forceinline__ unsigned point_mask(unsigned cm, unsigned c0, unsigned cp) {
  const unsigned right = c0 & cp & 15u, any = right | (cm & c0 & 15u);  // observed cells at i, and at i - 1 or i
  const unsigned in0 = (c0 >> 4) & 1u;
  auto differs = [&](unsigned col, int dz, int dy) { return ((col >> (4 + dz * 2 + dy)) & 1u) != in0; };
  unsigned m = 0;
  m |= (unsigned)(differs(cp, 0, 0) && right != 0u) << 0;           // (1,0,0): the cells (i, j - s, k - s)
  m |= (unsigned)(differs(c0, 0, 1) && (any & 0xAu) != 0u) << 1;    // (0,1,0): the cells (i - s, j, k - s)
  m |= (unsigned)(differs(c0, 1, 0) && (any & 0xCu) != 0u) << 2;    // (0,0,1): the cells (i - s, j - s, k)
  m |= (unsigned)(differs(cp, 0, 1) && (right & 0xAu) != 0u) << 3;  // (1,1,0): the cells (i, j, k - s)
  m |= (unsigned)(differs(cp, 1, 0) && (right & 0xCu) != 0u) << 4;  // (1,0,1): the cells (i, j - s, k)
  m |= (unsigned)(differs(c0, 1, 1) && (any & 8u) != 0u) << 5;      // (0,1,1): the cells (i - s, j, k)
  m |= (unsigned)(differs(cp, 1, 1) && (right & 8u) != 0u) << 6;    // (1,1,1): the cell (i, j, k)
  return m;
}

// inside of the 8 corners of cell i, bit = corner code, from the inside nibbles (bit dz * 2 + dy) of columns i, i + 1
__device__ __forceinline__ unsigned cell_corners(unsigned in0, unsigned in1) {
  unsigned c = 0;
#pragma unroll
  for (int code = 0; code < 8; ++code) {
    const unsigned col = (code >> 2) ? in1 : in0;
    c |= ((col >> ((code & 1) * 2 + ((code >> 1) & 1))) & 1u) << code;
  }
  return c;
}

// masks[k][j][i] and rows[row] = (vertices, faces) of row = k ny + j
__global__ __launch_bounds__(kThreads) void k_tm_count(const uint8_t *__restrict__ flags, int nx, int ny, int nz,
                                                       uint8_t *__restrict__ masks, int64_t *__restrict__ rows) {
  __shared__ unsigned char s_col[kThreads + 2];
  __shared__ int s_w[kWaves];
  const int64_t row = blockIdx.x;
  const int j = (int)(row % ny), k = (int)(row / ny);
  int packed = 0;  // vertices | faces << 16 of this lane: at most 7 and 12 per chunk
  int nv = 0, nf = 0;
  for (int x0 = 0; x0 < nx; x0 += kThreads) {
    __syncthreads();  // the previous chunk's s_col has been read
    for (int t = threadIdx.x; t < kThreads + 2; t += kThreads)
      s_col[t] = (unsigned char)count_column(flags, nx, ny, nz, x0 - 1 + t, j, k);
    __syncthreads();
    const int i = x0 + (int)threadIdx.x;
    packed = 0;
    if (i < nx) {
      const unsigned cm = s_col[threadIdx.x], c0 = s_col[threadIdx.x + 1], cp = s_col[threadIdx.x + 2];
      const unsigned m = point_mask(cm, c0, cp);
      masks[row * nx + i] = (uint8_t)m;
      packed = __popc(m);
      if (c0 & cp & 8u) packed += cell_faces(cell_corners(c0 >> 4, cp >> 4)) << 16;
    }
    int total;
    block_excl_scan<kWaves>(packed, s_w, total);  // a chunk has at most 1792 vertices and 3072 faces: no carry
    nv += total & 0xffff;
    nf += total >> 16;
  }
  if (threadIdx.x == 0) {
    rows[2 * row] = nv;
    rows[2 * row + 1] = nf;
  }
}

// rows [R][2] of counts -> exclusive offsets in place, rows[R] = totals = the two sums
__global__ __launch_bounds__(kScanThreads) void k_tm_scan(int64_t *__restrict__ rows, int64_t R,
                                                          int64_t *__restrict__ totals) {
  __shared__ int64_t s_w[kScanThreads / 64];
  const int64_t per = (R + kScanThreads - 1) / kScanThreads;
  const int64_t lo = min((int64_t)threadIdx.x * per, R), hi = min(lo + per, R);
  int64_t v = 0, f = 0;
  for (int64_t r = lo; r < hi; ++r) {
    v += rows[2 * r];
    f += rows[2 * r + 1];
  }
  int64_t tv, tf;
  int64_t bv = block_excl_scan<kScanThreads / 64>(v, s_w, tv);
  int64_t bf = block_excl_scan<kScanThreads / 64>(f, s_w, tf);
  for (int64_t r = lo; r < hi; ++r) {
    const int64_t cv = rows[2 * r], cf = rows[2 * r + 1];
    rows[2 * r] = bv;
    rows[2 * r + 1] = bf;
    bv += cv;
    bf += cf;
  }
  if (threadIdx.x == 0) {
    rows[2 * R] = totals[0] = tv;
    rows[2 * R + 1] = totals[1] = tf;
  }
}

struct Lattice {
  const float2 *vol;
  Grid g;
  double min_weight;
};

// the tsdf gradient at lattice point (i, j, k): central, one-sided or 0 per axis, by what the neighbours allow
__device__ __forceinline__ void gradient(const Lattice &L, int i, int j, int k, double (&G)[3]) {
  const int64_t at = L.g.flat(i, j, k);
  const double F = (double)L.vol[at].x;
  const int pos[3] = {i, j, k};
  const int64_t stride[3] = {1, L.g.n[0], (int64_t)L.g.n[0] * L.g.n[1]};
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    bool hp = pos[c] + 1 < L.g.n[c], hm = pos[c] >= 1;
    double Fp = 0.0, Fm = 0.0;
    if (hp) {
      const float2 v = L.vol[at + stride[c]];
      hp = (double)v.y >= L.min_weight;
      Fp = (double)v.x;
    }
    if (hm) {
      const float2 v = L.vol[at - stride[c]];
      hm = (double)v.y >= L.min_weight;
      Fm = (double)v.x;
    }
    G[c] = (hp && hm) ? (Fp - Fm) / 2.0 : hp ? Fp - F : hm ? F - Fm : 0.0;
  }
}

constexpr int kField = 12;  // bits of a field of the emit scan: a chunk has at most 1792 vertices per row, 3072 faces
constexpr unsigned long long kFieldMask = (1ull << kField) - 1ull;

__global__ __launch_bounds__(kThreads) void k_tm_emit(
    const float2 *__restrict__ vol, const uint8_t *__restrict__ flags, const uint8_t *__restrict__ masks,
    const int64_t *__restrict__ rows, Grid G, double min_weight, int64_t n_vertices, int64_t n_faces,
    double *__restrict__ vertices, int32_t *__restrict__ faces, double *__restrict__ normals) {
  // column kThreads is the first column of the next chunk: the + x corners of the chunk's last cell
  __shared__ unsigned char s_mask[4][kThreads + 1];
  __shared__ int s_vbase[4][kThreads + 1];
  __shared__ unsigned char s_col[kThreads + 1];  // bit 0: the four rows observed at this column; bit 4 + r: inside
  __shared__ unsigned long long s_w[kWaves];
  const int nx = G.n[0], ny = G.n[1], nz = G.n[2];
  const int64_t row = blockIdx.x;
  const int j = (int)(row % ny), k = (int)(row / ny);
  const int64_t v_row = rows[2 * row], f_row = rows[2 * row + 1];
  if (rows[2 * (row + 1)] == v_row && rows[2 * (row + 1) + 1] == f_row) return;  // nothing to write (uniform)
  // the four rows a cell of this row touches: r = dz * 2 + dy
  int64_t r_row[4], running[4];
  bool r_ok[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int dz = r >> 1, dy = r & 1;
    r_ok[r] = j + dy < ny && k + dz < nz;
    r_row[r] = row + (int64_t)dz * ny + dy;
    running[r] = r_ok[r] ? rows[2 * r_row[r]] : 0;
  }
  int64_t running_f = f_row;
  const Lattice L = {vol, G, min_weight};
  const int tid = (int)threadIdx.x;
  for (int x0 = 0; x0 < nx; x0 += kThreads) {
    // masks and flags of the chunk's columns, and of the column behind it (lane 0)
    unsigned own[4] = {0u, 0u, 0u, 0u};
    for (int slot = tid; slot <= kThreads; slot += kThreads) {
      const int x = x0 + slot;
      unsigned col = 0u, m[4] = {0u, 0u, 0u, 0u};
      if (x < nx) {
        unsigned seen = kObserved;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          unsigned f = 0u;
          if (r_ok[r]) {
            m[r] = masks[r_row[r] * nx + x];
            f = flags[r_row[r] * nx + x];
          }
          seen &= f;
          col |= (f & kInside) << (4 + r);
        }
        col |= seen >> 1;
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) s_mask[r][slot] = (unsigned char)m[r];
      s_col[slot] = (unsigned char)col;
      if (slot == tid)
        for (int r = 0; r < 4; ++r) own[r] = m[r];
    }
    __syncthreads();
    const int i = x0 + tid;
    const unsigned c0 = s_col[tid], c1 = s_col[tid + 1];
    const bool cell = (c0 & c1 & 1u) != 0u;  // (column kThreads is 0 past the row's end, the rows past the volume's)
    const unsigned corners = cell ? cell_corners(c0 >> 4, c1 >> 4) : 0u;
    unsigned long long packed = (unsigned long long)cell_faces(corners) << (4 * kField);
#pragma unroll
    for (int r = 0; r < 4; ++r) packed |= (unsigned long long)__popc(own[r]) << (r * kField);
    unsigned long long total;
    const unsigned long long excl = block_excl_scan<kWaves>(packed, s_w, total);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      s_vbase[r][tid] = (int)(running[r] + (int64_t)((excl >> (r * kField)) & kFieldMask));
      if (tid == 0) s_vbase[r][kThreads] = (int)(running[r] + (int64_t)((total >> (r * kField)) & kFieldMask));
    }
    __syncthreads();
    // the vertices of this row's points
    if (own[0] != 0u) {
      const int64_t at_a = row * nx + i;
      const double Fa = (double)vol[at_a].x;
      const int pa[3] = {i, j, k};
      double Ga[3] = {0.0, 0.0, 0.0};
      if (normals) gradient(L, i, j, k, Ga);
      int64_t at = s_vbase[0][tid];
      for (int d = 0; d < 7; ++d) {
        if (!((own[0] >> d) & 1u)) continue;
        const int code = code_of_dir(d);
        const int e[3] = {(code >> 2) & 1, (code >> 1) & 1, code & 1};
        if (at >= 0 && at < n_vertices) {
          const double Fb = (double)vol[at_a + G.flat(e[0], e[1], e[2])].x;
          const double r = Fa / (Fa - Fb);
          for (int c = 0; c < 3; ++c) {
            const double p_a = G.centre(c, pa[c]), p_b = G.centre(c, pa[c] + e[c]);
            vertices[3 * at + c] = p_a + r * (p_b - p_a);
          }
          if (normals) {
            double Gb[3], g[3];
            gradient(L, i + e[0], j + e[1], k + e[2], Gb);
            for (int c = 0; c < 3; ++c) g[c] = Ga[c] + r * (Gb[c] - Ga[c]);
            const double s = (g[0] * g[0] + g[1] * g[1]) + g[2] * g[2];
            const bool ok = s > 0.0;
            const double len = sqrt(s);
            for (int c = 0; c < 3; ++c) normals[3 * at + c] = ok ? g[c] / len : 0.0;
          }
        }
        ++at;
      }
    }
    // the faces of this row's cells
    const auto vertex_of = [&](int lo, int d) {
      const int r = (lo & 1) * 2 + ((lo >> 1) & 1), col = tid + (lo >> 2);  // the owner's row and column
      return s_vbase[r][col] + __popc((unsigned)s_mask[r][col] & ((1u << d) - 1u));
    };
    emit_cell_faces(corners, running_f + (int64_t)((excl >> (4 * kField)) & kFieldMask), 0, n_faces, faces, vertex_of);
#pragma unroll
    for (int r = 0; r < 4; ++r) running[r] += (int64_t)((total >> (r * kField)) & kFieldMask);
    running_f += (int64_t)((total >> (4 * kField)) & kFieldMask);
    __syncthreads();  // the chunk's LDS has been read
  }
}

struct Parts {
  uint8_t *flags, *masks;
  int64_t *rows;
};

Parts parts_of(const void *workspace, int64_t n) {
  char *base = (char *)workspace;
  return {(uint8_t *)base, (uint8_t *)(base + align16(n)), (int64_t *)(base + 2 * align16(n))};
}

}  // namespace

extern "C" int64_t mf_tsdfmesh_workspace_bytes(int32_t nx, int32_t ny, int32_t nz) {
  if (bad_volume(nx, ny, nz)) return -1;
  return 2 * align16((int64_t)nx * ny * nz) + ((int64_t)ny * nz + 1) * 16;
}

extern "C" int mf_tsdfmesh_count(const float *volume, int32_t nx, int32_t ny, int32_t nz, double min_weight,
                                 void *workspace, int64_t *totals, mfStream_t stream) {
  if (bad_volume(nx, ny, nz) || !(min_weight > 0.0))
    return bad("mf_tsdfmesh_count: nx, ny, nz >= 2 with fewer than 2^31 voxels, min_weight > 0");
  if (!volume || !workspace || !totals) return bad("mf_tsdfmesh_count: null volume, workspace or totals");
  if (misaligned(volume) || misaligned(workspace)) return bad("mf_tsdfmesh_count: volume and workspace 16-byte aligned");
  const int64_t n = (int64_t)nx * ny * nz, R = (int64_t)ny * nz;
  const Parts p = parts_of(workspace, n);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(k_tm_flags, lanes((n + 3) / 4), dim3(kThreads), 0, s, volume, n, min_weight, p.flags);
  hipLaunchKernelGGL(k_tm_count, dim3((unsigned)R), dim3(kThreads), 0, s, (const uint8_t *)p.flags, (int)nx, (int)ny,
                     (int)nz, p.masks, p.rows);
  hipLaunchKernelGGL(k_tm_scan, dim3(1), dim3(kScanThreads), 0, s, p.rows, R, totals);
  return mf::check_launch("mf_tsdfmesh_count");
}

extern "C" int mf_tsdfmesh_emit(const float *volume, int32_t nx, int32_t ny, int32_t nz, double origin_x,
                                double origin_y, double origin_z, double pitch, double min_weight,
                                const void *workspace, int64_t n_vertices, int64_t n_faces, double *vertices,
                                int32_t *faces, double *normals, mfStream_t stream) {
  const int64_t cap = (int64_t)1 << 31;
  if (bad_volume(nx, ny, nz) || !(pitch > 0.0) || !(min_weight > 0.0) || n_vertices < 0 || n_vertices >= cap ||
      n_faces < 0 || n_faces >= cap)
    return bad("mf_tsdfmesh_emit: nx, ny, nz >= 2 with fewer than 2^31 voxels, pitch > 0, min_weight > 0, "
               "0 <= n_vertices, n_faces < 2^31");
  if (!volume || !workspace || !vertices || !faces) return bad("mf_tsdfmesh_emit: null volume, workspace, vertices or faces");
  if (misaligned(volume) || misaligned(workspace)) return bad("mf_tsdfmesh_emit: volume and workspace 16-byte aligned");
  const Grid G = grid_of(nx, ny, nz, origin_x, origin_y, origin_z, pitch);
  const Parts p = parts_of(workspace, G.voxels());
  hipLaunchKernelGGL(k_tm_emit, dim3((unsigned)((int64_t)ny * nz)), dim3(kThreads), 0, (hipStream_t)stream,
                     (const float2 *)volume, (const uint8_t *)p.flags, (const uint8_t *)p.masks,
                     (const int64_t *)p.rows, G, min_weight, n_vertices, n_faces, vertices, faces, normals);
  return mf::check_launch("mf_tsdfmesh_emit");
}
