// The voxel body of TSDF integration (include/mfhip.h "TSDF fusion"), shared by k_tsdf_integrate (csrc/tsdf.hip) and
// k_tsdf_integrate_labels (csrc/tsdflabel.hip): one text, so the (tsdf, weight) bytes of the two kernels cannot differ.
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

// Voxel n of the volume against one depth frame -> true iff the voxel passed every requirement and was written; then
// `pixel` = row * W + col of the pixel it projects to and `sdf` = depth - z (before the clamp).
__device__ __forceinline__ bool integrate_voxel(float2 *__restrict__ vol, int64_t n, int nx, int ny, double ox,
                                                double oy, double oz, double pitch, double truncation,
                                                double max_weight, const float *__restrict__ depth, int H, int W,
                                                double fx, double fy, double cx, double cy, const Pose &P,
                                                int64_t &pixel, double &sdf) {
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
  double f = sdf / truncation;
  if (f > 1.0) f = 1.0;
  const float2 old = vol[n];
  const double F_old = (double)old.x, W_old = (double)old.y;
  double w = W_old + 1.0;
  const double F = (F_old * W_old + f) / w;
  if (w > max_weight) w = max_weight;
  vol[n] = make_float2((float)F, (float)w);
  return true;
}

}  // namespace mf_tsdf
