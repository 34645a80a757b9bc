// What the TSDF kernels say about one voxel, one text each so that the bytes of two kernels cannot differ:
//   Grid, Camera, Fuse, March  what a call says about the volume, the image, the update and the march: the kernels and
//                    every helper below them take these by value or reference, never as loose scalars;
//   voxel_body<false>  the requirements of TSDF integration (include/mfhip.h "TSDF fusion"): which voxels a frame
//                    writes, their pixel and sdf -- voxel_body<true> and k_tsdf_integrate_colors (csrc/tsdfcolor.hip);
//   voxel_body<true>  the voxel body of TSDF integration: k_tsdf_integrate (csrc/tsdf.hip) and k_tsdf_integrate_labels
//                    (csrc/tsdflabel.hip) store the same (tsdf, weight);
//   pixel_point      the map point of a depth pixel: label_at and k_tsdf_color_image (csrc/tsdfcolor.hip);
//   voxel_of         the voxel a map point falls into ("TSDF labels"): k_tsdf_label_image, k_tsdf_publish_grids
//                    (csrc/tsdflabel.hip) and, through label_at, k_tsdf_render (csrc/tsdfrender.hip);
//   label_at         the label of the voxel a depth pixel falls into: k_tsdf_label_image and k_tsdf_render's label_out.
// float64, + - * / and floor only, every expression associated as the header writes it; nothing is contracted.
#pragma once
#include <math.h>

#include "mf_common.h"

namespace mf_tsdf {

struct Pose {
  double R[9], t[3];
};

__device__ __forceinline__ Pose load_pose(const double *__restrict__ T) {
  Pose p;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
#pragma unroll
    for (int b = 0; b < 3; ++b) p.R[3 * a + b] = T[4 * a + b];
    p.t[a] = T[4 * a + 3];
  }
  return p;
}

// The volume's geometry: n voxels per axis, x fastest, voxel (i, j, k) centred at o + pitch * (i, j, k).
struct Grid {
  int n[3];
  double o[3], pitch;
  __host__ __device__ __forceinline__ int64_t voxels() const { return (int64_t)n[0] * n[1] * n[2]; }
  __device__ __forceinline__ void unflatten(int64_t m, int (&ijk)[3]) const {
    ijk[0] = (int)(m % n[0]);
    const int64_t rest = m / n[0];
    ijk[1] = (int)(rest % n[1]), ijk[2] = (int)(rest / n[1]);
  }
  __device__ __forceinline__ int64_t flat(int i, int j, int k) const { return ((int64_t)k * n[1] + j) * n[0] + i; }
  __device__ __forceinline__ double centre(int a, int i) const { return o[a] + pitch * (double)i; }
};

// The pinhole camera of an H x W image.
struct Camera {
  int H, W;
  double fx, fy, cx, cy;
  // the camera ray (q0, q1, 1) of pixel (col, row)
  __device__ __forceinline__ void ray(int col, int row, double &q0, double &q1) const {
    q0 = ((double)col - cx) / fx, q1 = ((double)row - cy) / fy;
  }
  __device__ __forceinline__ int64_t pixel(int col, int row) const { return (int64_t)row * W + col; }
};

struct Fuse { double truncation, max_weight; };

struct March { double step, min_depth, max_depth; int max_steps; };

// Voxel n of the volume against one depth frame: the requirements of mf_tsdf_integrate and, with kWrite, the update of
// the voxel's (tsdf, weight) -> true iff the voxel passed every requirement (with kWrite: and was written); then
// `pixel` = row * W + col of the pixel it projects to and `sdf` = depth - z (before the clamp).  Without kWrite `vol`
// is not touched (pass nullptr; max_weight is not read): the requirements read the depth image alone.
template <bool kWrite>
__device__ __forceinline__ bool voxel_body(float2 *__restrict__ vol, int64_t n, const Grid &G, const Fuse &fuse,
                                           const float *__restrict__ depth, const Camera &cam, const Pose &P,
                                           int64_t &pixel, double &sdf) {
  int ijk[3];
  G.unflatten(n, ijk);
  const double e0 = G.centre(0, ijk[0]) - P.t[0];
  const double e1 = G.centre(1, ijk[1]) - P.t[1];
  const double e2 = G.centre(2, ijk[2]) - P.t[2];
  const double x = (P.R[0] * e0 + P.R[3] * e1) + P.R[6] * e2;
  const double y = (P.R[1] * e0 + P.R[4] * e1) + P.R[7] * e2;
  const double z = (P.R[2] * e0 + P.R[5] * e1) + P.R[8] * e2;
  if (!(z > 0.0)) return false;
  const double col = floor((cam.fx * (x / z) + cam.cx) + 0.5);
  const double row = floor((cam.fy * (y / z) + cam.cy) + 0.5);
  if (!(col >= 0.0 && col <= (double)(cam.W - 1) && row >= 0.0 && row <= (double)(cam.H - 1))) return false;
  pixel = cam.pixel((int)col, (int)row);
  const double D = (double)depth[pixel];
  if (!(D > 0.0)) return false;
  sdf = D - z;
  if (!(sdf >= -fuse.truncation)) return false;
  if constexpr (kWrite) {
    double f = sdf / fuse.truncation;
    if (f > 1.0) f = 1.0;
    const float2 old = vol[n];
    const double F_old = (double)old.x, W_old = (double)old.y;
    double w = W_old + 1.0;
    const double F = (F_old * W_old + f) / w;
    if (w > fuse.max_weight) w = fuse.max_weight;
    vol[n] = make_float2((float)F, (float)w);
  }
  return true;
}

// floor((m - o) / pitch + 0.5) per axis -> the flat voxel index, or -1 outside the volume (or for a NaN)
__device__ __forceinline__ int64_t voxel_of(const double (&m)[3], const Grid &G) {
  const double g0 = floor((m[0] - G.o[0]) / G.pitch + 0.5);
  const double g1 = floor((m[1] - G.o[1]) / G.pitch + 0.5);
  const double g2 = floor((m[2] - G.o[2]) / G.pitch + 0.5);
  if (!(g0 >= 0.0 && g0 <= (double)(G.n[0] - 1) && g1 >= 0.0 && g1 <= (double)(G.n[1] - 1) && g2 >= 0.0 &&
        g2 <= (double)(G.n[2] - 1)))
    return -1;
  return G.flat((int)g0, (int)g1, (int)g2);
}

// the map-frame point of the pixel of camera ray (q0, q1, 1) at depth d: m = T (q0 d, q1 d, d)
__device__ __forceinline__ void pixel_point(const Pose &P, double q0, double q1, double d, double (&m)[3]) {
  const double x = q0 * d, y = q1 * d;
#pragma unroll
  for (int a = 0; a < 3; ++a) m[a] = ((P.R[3 * a] * x + P.R[3 * a + 1] * y) + P.R[3 * a + 2] * d) + P.t[a];
}

// The label of the voxel that the pixel of camera ray (q0, q1, 1) falls into at depth d > 0 (the caller's test: a pixel
// without a depth has label 0): 0 outside the volume and where the voxel's count is below min_count.
__device__ __forceinline__ int label_at(const int2 *__restrict__ labels, const Grid &G, double q0, double q1, double d,
                                        const Pose &P, int min_count) {
  double m[3];
  pixel_point(P, q0, q1, d, m);
  const int64_t n = voxel_of(m, G);
  if (n < 0) return 0;
  const int2 lc = labels[n];
  return lc.y >= min_count ? lc.x : 0;
}

}  // namespace mf_tsdf
