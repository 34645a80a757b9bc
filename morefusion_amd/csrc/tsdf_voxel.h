// What the TSDF kernels say about one voxel, one text each so that the bytes of two kernels cannot differ:
//   project_voxel    the requirements of TSDF integration (include/mfhip.h "TSDF fusion"): which voxels a frame writes,
//                    their pixel and sdf -- integrate_voxel and k_tsdf_integrate_colors (csrc/tsdfcolor.hip);
//   integrate_voxel  the voxel body of TSDF integration: k_tsdf_integrate (csrc/tsdf.hip) and k_tsdf_integrate_labels
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

// Voxel n of the volume against one depth frame: the requirements of mf_tsdf_integrate and, with kWrite, the update of
// the voxel's (tsdf, weight) -> true iff the voxel passed every requirement (with kWrite: and was written); then
// `pixel` = row * W + col of the pixel it projects to and `sdf` = depth - z (before the clamp).  Without kWrite `vol`
// is not touched: the requirements read the depth image alone.
template <bool kWrite>
__device__ __forceinline__ bool voxel_body(float2 *__restrict__ vol, int64_t n, int nx, int ny, double ox, double oy,
                                           double oz, double pitch, double truncation, double max_weight,
                                           const float *__restrict__ depth, int H, int W, double fx, double fy,
                                           double cx, double cy, const Pose &P, int64_t &pixel, double &sdf) {
  const int i = (int)(n % nx);
  const int64_t rest = n / nx;
  const int j = (int)(rest % ny), k = (int)(rest / ny);
  const double e0 = (ox + pitch * (double)i) - P.t[0];
  const double e1 = (oy + pitch * (double)j) - P.t[1];
  const double e2 = (oz + pitch * (double)k) - P.t[2];
  const double x = (P.R[0] * e0 + P.R[3] * e1) + P.R[6] * e2;
  const double y = (P.R[1] * e0 + P.R[4] * e1) + P.R[7] * e2;
  const double z = (P.R[2] * e0 + P.R[5] * e1) + P.R[8] * e2;
  if (!(z > 0.0)) return false;
  const double col = floor((fx * (x / z) + cx) + 0.5);
  const double row = floor((fy * (y / z) + cy) + 0.5);
  if (!(col >= 0.0 && col <= (double)(W - 1) && row >= 0.0 && row <= (double)(H - 1))) return false;
  pixel = (int64_t)(int)row * W + (int)col;
  const double D = (double)depth[pixel];
  if (!(D > 0.0)) return false;
  sdf = D - z;
  if (!(sdf >= -truncation)) return false;
  if constexpr (kWrite) {
    double f = sdf / truncation;
    if (f > 1.0) f = 1.0;
    const float2 old = vol[n];
    const double F_old = (double)old.x, W_old = (double)old.y;
    double w = W_old + 1.0;
    const double F = (F_old * W_old + f) / w;
    if (w > max_weight) w = max_weight;
    vol[n] = make_float2((float)F, (float)w);
  }
  return true;
}

// the voxel body of TSDF integration -> true iff the voxel passed every requirement and was written
__device__ __forceinline__ bool integrate_voxel(float2 *__restrict__ vol, int64_t n, int nx, int ny, double ox,
                                                double oy, double oz, double pitch, double truncation,
                                                double max_weight, const float *__restrict__ depth, int H, int W,
                                                double fx, double fy, double cx, double cy, const Pose &P,
                                                int64_t &pixel, double &sdf) {
  return voxel_body<true>(vol, n, nx, ny, ox, oy, oz, pitch, truncation, max_weight, depth, H, W, fx, fy, cx, cy, P,
                          pixel, sdf);
}

// the requirements alone -> true iff mf_tsdf_integrate of the same arguments writes voxel n
__device__ __forceinline__ bool project_voxel(int64_t n, int nx, int ny, double ox, double oy, double oz, double pitch,
                                              double truncation, const float *__restrict__ depth, int H, int W,
                                              double fx, double fy, double cx, double cy, const Pose &P,
                                              int64_t &pixel, double &sdf) {
  return voxel_body<false>(nullptr, n, nx, ny, ox, oy, oz, pitch, truncation, 0.0, depth, H, W, fx, fy, cx, cy, P,
                           pixel, sdf);
}

// floor((m - o) / pitch + 0.5) per axis -> the flat voxel index, or -1 outside the volume (or for a NaN)
__device__ __forceinline__ int64_t voxel_of(const double (&m)[3], double ox, double oy, double oz, double pitch, int nx,
                                            int ny, int nz) {
  const double g0 = floor((m[0] - ox) / pitch + 0.5);
  const double g1 = floor((m[1] - oy) / pitch + 0.5);
  const double g2 = floor((m[2] - oz) / pitch + 0.5);
  if (!(g0 >= 0.0 && g0 <= (double)(nx - 1) && g1 >= 0.0 && g1 <= (double)(ny - 1) && g2 >= 0.0 &&
        g2 <= (double)(nz - 1)))
    return -1;
  return ((int64_t)(int)g2 * ny + (int)g1) * nx + (int)g0;
}

// the map-frame point of the pixel of camera ray (q0, q1, 1) at depth d: m = T (q0 d, q1 d, d)
__device__ __forceinline__ void pixel_point(const Pose &P, double q0, double q1, double d, double (&m)[3]) {
  const double x = q0 * d, y = q1 * d;
#pragma unroll
  for (int a = 0; a < 3; ++a) m[a] = ((P.R[3 * a] * x + P.R[3 * a + 1] * y) + P.R[3 * a + 2] * d) + P.t[a];
}

// The label of the voxel that the pixel of camera ray (q0, q1, 1) falls into at depth d > 0 (the caller's test: a pixel
// without a depth has label 0): 0 outside the volume and where the voxel's count is below min_count.
__device__ __forceinline__ int label_at(const int2 *__restrict__ labels, int nx, int ny, int nz, double ox, double oy,
                                        double oz, double pitch, double q0, double q1, double d, const Pose &P,
                                        int min_count) {
  double m[3];
  pixel_point(P, q0, q1, d, m);
  const int64_t n = voxel_of(m, ox, oy, oz, pitch, nx, ny, nz);
  if (n < 0) return 0;
  const int2 lc = labels[n];
  return lc.y >= min_count ? lc.x : 0;
}

}  // namespace mf_tsdf
