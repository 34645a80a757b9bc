// The pieces of the TSDF ray march (include/mfhip.h "TSDF fusion", mf_tsdf_raycast), shared by k_tsdf_raycast
// (csrc/tsdf.hip) and k_tsdf_render (csrc/tsdfrender.hip): one text, so the depth and code bytes of the two kernels
// cannot differ.  The loops stay in the kernels -- the render's has the summary byte and the jump -- and call these
// bodies.  float64, + - * / and floor only, every expression associated as the header writes it; nothing is contracted.
#pragma once
#include <math.h>

#include "mf_common.h"
#include "tsdf_voxel.h"

namespace mf_tsdf {

// two x-neighbours of the volume: (tsdf, weight) of voxel i and of voxel i + 1 -- 16 bytes at an 8-byte aligned address
struct __attribute__((aligned(8))) VoxelPair {
  float f0, w0, f1, w1;
};

// The ray of camera point (q0, q1, 1): its direction d in the map frame and the depths [enter, leave] at which it is
// inside both [min_depth, max_depth] and the box of the voxel centres -> MF_TSDF_RAY_MISS for a ray that is never
// inside, -1 (no code yet) for one to march.
__device__ __forceinline__ int ray_setup(const Pose &P, double q0, double q1, const Grid &G, const March &march,
                                         double (&d)[3], double &enter, double &leave) {
#pragma unroll
  for (int a = 0; a < 3; ++a) d[a] = (P.R[3 * a] * q0 + P.R[3 * a + 1] * q1) + P.R[3 * a + 2];
  enter = march.min_depth, leave = march.max_depth;
  int code = -1;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const double lo = G.o[a], hi = G.centre(a, G.n[a] - 1), o = P.t[a];
    if (d[a] < 0.0 || d[a] > 0.0) {
      const double t1 = (lo - o) / d[a], t2 = (hi - o) / d[a];
      const double tn = t1 < t2 ? t1 : t2, tf = t1 < t2 ? t2 : t1;
      enter = tn <= enter ? enter : tn;
      leave = tf >= leave ? leave : tf;
    } else if (!(d[a] == 0.0 && o >= lo && o <= hi)) {
      code = MF_TSDF_RAY_MISS;
    }
  }
  if (!(enter <= leave)) code = MF_TSDF_RAY_MISS;
  return code;
}

// the sample at depth s along the ray, in voxel units: g = ((t + s d) - o) / pitch
__device__ __forceinline__ void grid_pos(const Pose &P, const double (&d)[3], double s, const Grid &G, double (&g)[3]) {
#pragma unroll
  for (int a = 0; a < 3; ++a) g[a] = ((P.t[a] + s * d[a]) - G.o[a]) / G.pitch;
}

// b = floor(g) -> true iff b is a cell of the volume: the eight voxels b .. b + 1 exist
__device__ __forceinline__ bool cell_of(const double (&g)[3], const Grid &G, double (&b)[3]) {
#pragma unroll
  for (int a = 0; a < 3; ++a) b[a] = floor(g[a]);
  return b[0] >= 0.0 && b[0] <= (double)(G.n[0] - 2) && b[1] >= 0.0 && b[1] <= (double)(G.n[1] - 2) && b[2] >= 0.0 &&
         b[2] <= (double)(G.n[2] - 2);
}

// the eight voxels of cell b: 4 loads of 16 bytes, v[dz][dy] = the x-neighbours (b0, b1 + dy, b2 + dz), (b0 + 1, ..)
struct Cell {
  VoxelPair v[2][2];
};

__device__ __forceinline__ Cell load_cell(const float *vol, const Grid &G, const double (&b)[3]) {
  const int64_t sy = G.n[0], sz = (int64_t)G.n[0] * G.n[1];
  const float *base = vol + 2 * G.flat((int)b[0], (int)b[1], (int)b[2]);
  return {{{*(const VoxelPair *)base, *(const VoxelPair *)(base + 2 * sy)},
           {*(const VoxelPair *)(base + 2 * sz), *(const VoxelPair *)(base + 2 * (sz + sy))}}};
}

// a sample is valid where all eight weights are > 0
__device__ __forceinline__ bool all_seen(const Cell &c) {
  const VoxelPair &v00 = c.v[0][0], &v10 = c.v[0][1], &v01 = c.v[1][0], &v11 = c.v[1][1];
  return v00.w0 > 0.0f && v00.w1 > 0.0f && v10.w0 > 0.0f && v10.w1 > 0.0f && v01.w0 > 0.0f && v01.w1 > 0.0f &&
         v11.w0 > 0.0f && v11.w1 > 0.0f;
}

// the trilinear tsdf at g inside cell b = floor(g): along x, then y, then z
__device__ __forceinline__ double trilinear(const Cell &c, const double (&g)[3], const double (&b)[3]) {
  const VoxelPair &v00 = c.v[0][0], &v10 = c.v[0][1], &v01 = c.v[1][0], &v11 = c.v[1][1];
  const double r0 = g[0] - b[0], r1 = g[1] - b[1], r2 = g[2] - b[2];
  const double c00 = (double)v00.f0 + r0 * ((double)v00.f1 - (double)v00.f0);
  const double c10 = (double)v10.f0 + r0 * ((double)v10.f1 - (double)v10.f0);
  const double c01 = (double)v01.f0 + r0 * ((double)v01.f1 - (double)v01.f0);
  const double c11 = (double)v11.f0 + r0 * ((double)v11.f1 - (double)v11.f0);
  const double c0 = c00 + r1 * (c10 - c00), c1 = c01 + r1 * (c11 - c01);
  return c0 + r2 * (c1 - c0);
}

// Sample k gave F <= 0: a HIT at the interpolated crossing where sample k - 1 was valid (`have`) with prev = F > 0 in
// front of the surface, else the ray came from behind or out of the unseen -> the ray's code, `out` = the hit depth.
__device__ __forceinline__ int ray_crossing(bool have, double prev, double F, double enter, double step, int k,
                                            float &out) {
  if (have && prev > 0.0) {
    out = (float)((enter + (double)(k - 1) * step) + step * (prev / (prev - F)));
    return MF_TSDF_RAY_HIT;
  }
  return MF_TSDF_RAY_BACKFACE;
}

}  // namespace mf_tsdf
