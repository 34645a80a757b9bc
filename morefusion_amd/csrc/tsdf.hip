// TSDF fusion: integrate depth frames into a truncated-signed-distance volume and ray-cast it into a depth image
// (contrib/tsdf_volume.py) -- gfx950, float64 arithmetic on float32 storage.
//
// The mapping half of KinectFusion (Newcombe et al., ISMAR 2011, sections 3.3 and 3.4): the model that
// contrib.ModelTracker aligns every frame to.  include/mfhip.h "TSDF fusion" is the contract -- the layout, every
// formula and its association -- and tests/tsdf_ref.py the NumPy mirror this file is pinned to bit for bit; DESIGN.md
// "TSDF fusion" has the cost model.
//
//   k_tsdf_integrate  a lane per voxel, x fastest: a wave reads 64 (tsdf, weight) pairs = 512 contiguous bytes, and
//                     stores only the voxels the frame touches.  The pose and the skip word are read from the device.
//                     The voxel body is tsdf_voxel.h's, shared with the labelled integrate of csrc/tsdflabel.hip.
//   k_tsdf_raycast    a lane per pixel in 16 x 16 tiles: neighbouring rays sample the same voxels (L2 / L1 hits).
//                     The ray set-up, the sample and the hit rule are tsdf_ray.h's, shared with k_tsdf_render of
//                     csrc/tsdfrender.hip; the march itself is this kernel's.
//
// No atomics, no LDS, no cross-lane traffic: every output byte is a function of the inputs alone.  Nothing is
// contracted (-ffp-contract=off); only + - * / and floor are used.
#include <math.h>

#include "host_args.h"
#include "mf_common.h"
#include "tsdf_ray.h"
#include "tsdf_voxel.h"

namespace {

constexpr int kThreads = 256;
constexpr int kTile = 16;

using mf_tsdf::Pose;
using mf_tsdf::load_pose;

__global__ void __launch_bounds__(kThreads) k_tsdf_integrate(
    float2 *__restrict__ vol, int nx, int ny, int64_t n_voxels, double ox, double oy, double oz, double pitch,
    double truncation, double max_weight, const float *__restrict__ depth, int H, int W, double fx, double fy,
    double cx, double cy, const double *__restrict__ T, const int32_t *__restrict__ skip_flag) {
  if (skip_flag && *skip_flag != 0) return;
  const int64_t n = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (n >= n_voxels) return;
  const Pose P = load_pose(T);
  int64_t pixel;
  double sdf;
  mf_tsdf::integrate_voxel(vol, n, nx, ny, ox, oy, oz, pitch, truncation, max_weight, depth, H, W, fx, fy, cx, cy, P,
                           pixel, sdf);
}

__global__ void __launch_bounds__(kTile *kTile) k_tsdf_raycast(
    const float *__restrict__ vol, int nx, int ny, int nz, double ox, double oy, double oz, double pitch, double step,
    double min_depth, double max_depth, int max_steps, int H, int W, double fx, double fy, double cx, double cy,
    const double *__restrict__ T, float *__restrict__ depth_out, uint8_t *__restrict__ code_out) {
  const int col = (int)blockIdx.x * kTile + (int)threadIdx.x, row = (int)blockIdx.y * kTile + (int)threadIdx.y;
  if (col >= W || row >= H) return;
  const Pose P = load_pose(T);
  const double q0 = ((double)col - cx) / fx, q1 = ((double)row - cy) / fy;
  const double org[3] = {ox, oy, oz};
  const int dims[3] = {nx, ny, nz};
  double d[3], enter, leave;
  int code = mf_tsdf::ray_setup(P, q0, q1, org, dims, pitch, min_depth, max_depth, d, enter, leave);
  float out = 0.0f;
  if (code < 0) {
    bool have = false;
    double prev = 0.0;
    for (int k = 0;; ++k) {
      const double s = enter + (double)k * step;
      if (!(s <= leave)) { code = MF_TSDF_RAY_LEFT; break; }
      if (k >= max_steps) { code = MF_TSDF_RAY_CAP; break; }
      double g[3], b[3];
      mf_tsdf::grid_pos(P, d, s, org, pitch, g);
      if (!mf_tsdf::cell_of(g, dims, b)) { have = false; continue; }
      const mf_tsdf::Cell cell = mf_tsdf::load_cell(vol, nx, ny, b);
      if (!mf_tsdf::all_seen(cell)) { have = false; continue; }
      const double F = mf_tsdf::trilinear(cell, g, b);
      if (F <= 0.0) { code = mf_tsdf::ray_crossing(have, prev, F, enter, step, k, out); break; }
      have = true;
      prev = F;
    }
  }
  const int64_t p = (int64_t)row * W + col;
  depth_out[p] = out;
  if (code_out) code_out[p] = (uint8_t)code;
}

}  // namespace

extern "C" int mf_tsdf_integrate(float *volume, int32_t nx, int32_t ny, int32_t nz, double origin_x, double origin_y,
                                 double origin_z, double pitch, double truncation, double max_weight,
                                 const float *depth, int32_t H, int32_t W, double fx, double fy, double cx, double cy,
                                 const double *T_sensor_to_map, const int32_t *skip_flag, mfStream_t stream) {
  if (bad_volume(nx, ny, nz) || !(pitch > 0.0) || !(truncation > 0.0) || !(max_weight >= 1.0) ||
      bad_camera(H, W, fx, fy))
    return bad("mf_tsdf_integrate: nx, ny, nz >= 2 with fewer than 2^31 voxels, pitch > 0, truncation > 0, "
               "max_weight >= 1, 1 <= H, W <= MF_RENDER_MAX_SIDE, fx, fy > 0");
  if (!volume || !depth || !T_sensor_to_map) return bad("mf_tsdf_integrate: null volume, depth or T_sensor_to_map");
  const int64_t n = (int64_t)nx * ny * nz;
  hipLaunchKernelGGL(k_tsdf_integrate, dim3((unsigned)((n + kThreads - 1) / kThreads)), dim3(kThreads), 0,
                     (hipStream_t)stream, (float2 *)volume, (int)nx, (int)ny, n, origin_x, origin_y, origin_z, pitch,
                     truncation, max_weight, depth, (int)H, (int)W, fx, fy, cx, cy, T_sensor_to_map, skip_flag);
  return mf::check_launch("mf_tsdf_integrate");
}

extern "C" int mf_tsdf_raycast(const float *volume, int32_t nx, int32_t ny, int32_t nz, double origin_x,
                               double origin_y, double origin_z, double pitch, double step, double min_depth,
                               double max_depth, int32_t max_steps, int32_t H, int32_t W, double fx, double fy,
                               double cx, double cy, const double *T_sensor_to_map, float *depth_out,
                               uint8_t *code_out, mfStream_t stream) {
  if (bad_volume(nx, ny, nz) || !(pitch > 0.0) || !(step > 0.0) || !(min_depth >= 0.0 && min_depth < max_depth) ||
      max_steps < 1 || max_steps > MF_TSDF_MAX_STEPS || bad_camera(H, W, fx, fy))
    return bad("mf_tsdf_raycast: nx, ny, nz >= 2 with fewer than 2^31 voxels, pitch > 0, step > 0, 0 <= min_depth < "
               "max_depth, 1 <= max_steps <= MF_TSDF_MAX_STEPS, 1 <= H, W <= MF_RENDER_MAX_SIDE, fx, fy > 0");
  if (!volume || !T_sensor_to_map || !depth_out) return bad("mf_tsdf_raycast: null volume, T_sensor_to_map or depth_out");
  hipLaunchKernelGGL(k_tsdf_raycast, dim3((unsigned)((W + kTile - 1) / kTile), (unsigned)((H + kTile - 1) / kTile)),
                     dim3(kTile, kTile), 0, (hipStream_t)stream, volume, (int)nx, (int)ny, (int)nz, origin_x,
                     origin_y, origin_z, pitch, step, min_depth, max_depth, (int)max_steps, (int)H, (int)W, fx, fy,
                     cx, cy, T_sensor_to_map, depth_out, code_out);
  return mf::check_launch("mf_tsdf_raycast");
}
