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
//                     A sample is 4 loads of 16 bytes (the two x-neighbours are adjacent in memory).
//
// No atomics, no LDS, no cross-lane traffic: every output byte is a function of the inputs alone.  Nothing is
// contracted (-ffp-contract=off); only + - * / and floor are used.
#include <math.h>

#include "mf_common.h"
#include "tsdf_voxel.h"

namespace {

constexpr int kThreads = 256;
constexpr int kTile = 16;

using mf_tsdf::Pose;
using mf_tsdf::load_pose;

// two x-neighbours of the volume: (tsdf, weight) of voxel i and of voxel i + 1 -- 16 bytes at an 8-byte aligned address
struct __attribute__((aligned(8))) VoxelPair {
  float f0, w0, f1, w1;
};

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
  double d[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) d[a] = (P.R[3 * a] * q0 + P.R[3 * a + 1] * q1) + P.R[3 * a + 2];
  double enter = min_depth, leave = max_depth;
  int code = -1;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const double lo = org[a], hi = org[a] + pitch * (double)(dims[a] - 1), o = P.t[a];
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
  float out = 0.0f;
  if (code < 0) {
    const int64_t sy = nx, sz = (int64_t)nx * ny;
    const double mx = (double)(nx - 2), my = (double)(ny - 2), mz = (double)(nz - 2);
    bool have = false;
    double prev = 0.0;
    for (int k = 0;; ++k) {
      const double s = enter + (double)k * step;
      if (!(s <= leave)) { code = MF_TSDF_RAY_LEFT; break; }
      if (k >= max_steps) { code = MF_TSDF_RAY_CAP; break; }
      const double g0 = ((P.t[0] + s * d[0]) - ox) / pitch;
      const double g1 = ((P.t[1] + s * d[1]) - oy) / pitch;
      const double g2 = ((P.t[2] + s * d[2]) - oz) / pitch;
      const double b0 = floor(g0), b1 = floor(g1), b2 = floor(g2);
      if (!(b0 >= 0.0 && b0 <= mx && b1 >= 0.0 && b1 <= my && b2 >= 0.0 && b2 <= mz)) { have = false; continue; }
      const float *base = vol + 2 * (((int64_t)(int)b2 * ny + (int)b1) * nx + (int)b0);
      const VoxelPair v00 = *(const VoxelPair *)base, v10 = *(const VoxelPair *)(base + 2 * sy);
      const VoxelPair v01 = *(const VoxelPair *)(base + 2 * sz), v11 = *(const VoxelPair *)(base + 2 * (sz + sy));
      if (!(v00.w0 > 0.0f && v00.w1 > 0.0f && v10.w0 > 0.0f && v10.w1 > 0.0f && v01.w0 > 0.0f && v01.w1 > 0.0f &&
            v11.w0 > 0.0f && v11.w1 > 0.0f)) { have = false; continue; }
      const double r0 = g0 - b0, r1 = g1 - b1, r2 = g2 - b2;
      const double c00 = (double)v00.f0 + r0 * ((double)v00.f1 - (double)v00.f0);
      const double c10 = (double)v10.f0 + r0 * ((double)v10.f1 - (double)v10.f0);
      const double c01 = (double)v01.f0 + r0 * ((double)v01.f1 - (double)v01.f0);
      const double c11 = (double)v11.f0 + r0 * ((double)v11.f1 - (double)v11.f0);
      const double c0 = c00 + r1 * (c10 - c00), c1 = c01 + r1 * (c11 - c01);
      const double F = c0 + r2 * (c1 - c0);
      if (F <= 0.0) {
        if (have && prev > 0.0) {
          out = (float)((enter + (double)(k - 1) * step) + step * (prev / (prev - F)));
          code = MF_TSDF_RAY_HIT;
        } else {
          code = MF_TSDF_RAY_BACKFACE;
        }
        break;
      }
      have = true;
      prev = F;
    }
  }
  const int64_t p = (int64_t)row * W + col;
  depth_out[p] = out;
  if (code_out) code_out[p] = (uint8_t)code;
}

int bad(const char *what) {
  mf::set_last_error(hipErrorInvalidValue, what);
  return -(int)hipErrorInvalidValue;
}

bool bad_volume(int32_t nx, int32_t ny, int32_t nz, double pitch) {
  if (nx < 2 || ny < 2 || nz < 2 || (int64_t)nx * ny * nz >= ((int64_t)1 << 31)) return true;
  return !(pitch > 0.0);
}

bool bad_camera(int32_t H, int32_t W, double fx, double fy) {
  return H < 1 || W < 1 || H > MF_RENDER_MAX_SIDE || W > MF_RENDER_MAX_SIDE || !(fx > 0.0) || !(fy > 0.0);
}

}  // namespace

extern "C" int mf_tsdf_integrate(float *volume, int32_t nx, int32_t ny, int32_t nz, double origin_x, double origin_y,
                                 double origin_z, double pitch, double truncation, double max_weight,
                                 const float *depth, int32_t H, int32_t W, double fx, double fy, double cx, double cy,
                                 const double *T_sensor_to_map, const int32_t *skip_flag, mfStream_t stream) {
  if (bad_volume(nx, ny, nz, pitch) || !(truncation > 0.0) || !(max_weight >= 1.0) || bad_camera(H, W, fx, fy))
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
  if (bad_volume(nx, ny, nz, pitch) || !(step > 0.0) || !(min_depth >= 0.0 && min_depth < max_depth) ||
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
