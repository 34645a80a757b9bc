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

using namespace mf_tsdf;

__global__ void __launch_bounds__(kThreads) k_tsdf_integrate(float2 *__restrict__ vol, Grid G, Fuse fuse,
                                                             const float *__restrict__ depth, Camera cam,
                                                             const double *__restrict__ T,
                                                             const int32_t *__restrict__ skip_flag) {
  if (skip_flag && *skip_flag != 0) return;
  const int64_t n = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (n >= G.voxels()) return;
  const Pose P = load_pose(T);
  int64_t pixel;
  double sdf;
  mf_tsdf::voxel_body<true>(vol, n, G, fuse, depth, cam, P, pixel, sdf);
}

__global__ void __launch_bounds__(kTile *kTile) k_tsdf_raycast(const float *__restrict__ vol, Grid G, March march,
                                                               Camera cam, const double *__restrict__ T,
                                                               float *__restrict__ depth_out,
                                                               uint8_t *__restrict__ code_out) {
  const int col = (int)blockIdx.x * kTile + (int)threadIdx.x, row = (int)blockIdx.y * kTile + (int)threadIdx.y;
  if (col >= cam.W || row >= cam.H) return;
  const Pose P = load_pose(T);
  double q0, q1, d[3], enter, leave;
  cam.ray(col, row, q0, q1);
  int code = mf_tsdf::ray_setup(P, q0, q1, G, march, d, enter, leave);
  float out = 0.0f;
  if (code < 0) {
    bool have = false;
    double prev = 0.0;
    for (int k = 0;; ++k) {
      const double s = enter + (double)k * march.step;
      if (!(s <= leave)) { code = MF_TSDF_RAY_LEFT; break; }
      if (k >= march.max_steps) { code = MF_TSDF_RAY_CAP; break; }
      double g[3], b[3];
      mf_tsdf::grid_pos(P, d, s, G, g);
      if (!mf_tsdf::cell_of(g, G, b)) { have = false; continue; }
      const mf_tsdf::Cell cell = mf_tsdf::load_cell(vol, G, b);
      if (!mf_tsdf::all_seen(cell)) { have = false; continue; }
      const double F = mf_tsdf::trilinear(cell, g, b);
      if (F <= 0.0) { code = mf_tsdf::ray_crossing(have, prev, F, enter, march.step, k, out); break; }
      have = true;
      prev = F;
    }
  }
  const int64_t p = cam.pixel(col, row);
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
  const Grid G = grid_of(nx, ny, nz, origin_x, origin_y, origin_z, pitch);
  hipLaunchKernelGGL(k_tsdf_integrate, lanes(G.voxels()), dim3(kThreads), 0, (hipStream_t)stream, (float2 *)volume, G,
                     Fuse{truncation, max_weight}, depth, camera_of(H, W, fx, fy, cx, cy), T_sensor_to_map, skip_flag);
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
  hipLaunchKernelGGL(k_tsdf_raycast, tiles(H, W), dim3(kTile, kTile), 0, (hipStream_t)stream, volume,
                     grid_of(nx, ny, nz, origin_x, origin_y, origin_z, pitch),
                     March{step, min_depth, max_depth, max_steps}, camera_of(H, W, fx, fy, cx, cy), T_sensor_to_map,
                     depth_out, code_out);
  return mf::check_launch("mf_tsdf_raycast");
}
