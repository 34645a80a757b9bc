// TSDF colour: a per-voxel colour fused next to the TSDF volume, and the colour of renders and of map-frame points from
// it (contrib/tsdf_volume.py) -- gfx950, float64 arithmetic.
//
// include/mfhip.h "TSDF colour" is the contract -- the layout, the update rule, SAMPLE and every formula's association --
// and tests/tsdfcolor_ref.py the NumPy mirror this file is pinned to bit for bit; DESIGN.md "TSDF colour" has the cost
// model.
//
//   k_tsdf_integrate_colors  a lane per voxel, x fastest: the requirements of k_tsdf_integrate (tsdf_voxel.h's
//                            voxel_body<false>, the same text: the voxels that take a colour are among those it writes),
//                            the band sdf <= truncation of k_tsdf_integrate_labels, then one running average on the
//                            voxel's own (r, g, b, weight): a 16-byte load and a 16-byte store, contiguous over a wave.
//                            The (tsdf, weight) volume is not touched.
//   k_tsdf_color_image       a lane per pixel in 16 x 16 tiles: SAMPLE at the map point of a depth pixel (tsdf_voxel.h's
//                            pixel_point, the same text as label_at's).
//   k_tsdf_sample_colors     a lane per point: SAMPLE at a map-frame point.
//
// A lane writes only its own output: no atomics, no LDS.  + - * / and floor only, nothing is contracted
// (-ffp-contract=off).
#include <math.h>

#include "host_args.h"
#include "mf_common.h"
#include "tsdf_ray.h"
#include "tsdf_voxel.h"

namespace {

using namespace mf_tsdf;

// q of the header: floor(x + 0.5) clamped to 0 .. 255, a NaN gives 0
__device__ __forceinline__ uint32_t quantise(double x) {
  double q = floor(x + 0.5);
  if (!(q >= 0.0)) q = 0.0;
  if (q > 255.0) q = 255.0;
  return (uint32_t)q;
}

// SAMPLE of the header at the map point m -> r | g << 8 | b << 16 | a << 24: the four bytes of an rgba element
__device__ __forceinline__ uint32_t sample_color(const float4 *__restrict__ colors, const Grid &G,
                                                 const double (&m)[3]) {
  double g[3], b[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) g[a] = (m[a] - G.o[a]) / G.pitch;
  if (!mf_tsdf::cell_of(g, G, b)) return 0u;
  const double r0 = g[0] - b[0], r1 = g[1] - b[1], r2 = g[2] - b[2];
  const double wx[2] = {1.0 - r0, r0}, wy[2] = {1.0 - r1, r1}, wz[2] = {1.0 - r2, r2};
  const float4 *base = colors + G.flat((int)b[0], (int)b[1], (int)b[2]);
  double S = 0.0, A0 = 0.0, A1 = 0.0, A2 = 0.0;
#pragma unroll
  for (int dx = 0; dx < 2; ++dx) {
#pragma unroll
    for (int dy = 0; dy < 2; ++dy) {
#pragma unroll
      for (int dz = 0; dz < 2; ++dz) {
        const float4 c = base[G.flat(dx, dy, dz)];
        const double w = (wx[dx] * wy[dy]) * wz[dz];
        if (c.w > 0.0f) {
          S = S + w;
          A0 = A0 + w * (double)c.x;
          A1 = A1 + w * (double)c.y;
          A2 = A2 + w * (double)c.z;
        }
      }
    }
  }
  if (!(S > 0.0)) return 0u;
  return quantise(A0 / S) | (quantise(A1 / S) << 8) | (quantise(A2 / S) << 16) | (255u << 24);
}

__global__ void __launch_bounds__(kThreads) k_tsdf_integrate_colors(
    float4 *__restrict__ colors, Grid G, Fuse fuse, const float *__restrict__ depth, const uint8_t *__restrict__ rgb,
    Camera cam, const double *__restrict__ T, const int32_t *__restrict__ skip_flag) {
  if (skip_flag && *skip_flag != 0) return;
  const int64_t n = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (n >= G.voxels()) return;
  const Pose P = load_pose(T);
  int64_t pixel;
  double sdf;
  if (!mf_tsdf::voxel_body<false>(nullptr, n, G, fuse, depth, cam, P, pixel, sdf)) return;
  if (!(sdf <= fuse.truncation)) return;  // far in front of the surface: that pixel's colour belongs to what lies behind
  const uint8_t *px = rgb + 3 * pixel;
  const double p0 = (double)px[0], p1 = (double)px[1], p2 = (double)px[2];
  const float4 c = colors[n];
  const double Wc = (double)c.w;
  double w = Wc + 1.0;
  const double C0 = ((double)c.x * Wc + p0) / w;
  const double C1 = ((double)c.y * Wc + p1) / w;
  const double C2 = ((double)c.z * Wc + p2) / w;
  if (w > fuse.max_weight) w = fuse.max_weight;
  colors[n] = make_float4((float)C0, (float)C1, (float)C2, (float)w);
}

__global__ void __launch_bounds__(kTile *kTile) k_tsdf_color_image(const float4 *__restrict__ colors, Grid G,
                                                                   const float *__restrict__ depth, Camera cam,
                                                                   const double *__restrict__ T,
                                                                   uint32_t *__restrict__ out) {
  const int col = (int)blockIdx.x * kTile + (int)threadIdx.x, row = (int)blockIdx.y * kTile + (int)threadIdx.y;
  if (col >= cam.W || row >= cam.H) return;
  const int64_t p = cam.pixel(col, row);
  const double d = (double)depth[p];
  uint32_t rgba = 0u;
  if (d > 0.0) {
    const Pose P = load_pose(T);
    double q0, q1, m[3];
    cam.ray(col, row, q0, q1);
    mf_tsdf::pixel_point(P, q0, q1, d, m);
    rgba = sample_color(colors, G, m);
  }
  out[p] = rgba;
}

__global__ void __launch_bounds__(kThreads) k_tsdf_sample_colors(const float4 *__restrict__ colors, Grid G,
                                                                 const double *__restrict__ points, int64_t n_points,
                                                                 uint32_t *__restrict__ out) {
  const int64_t n = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (n >= n_points) return;
  const double m[3] = {points[3 * n], points[3 * n + 1], points[3 * n + 2]};
  out[n] = sample_color(colors, G, m);
}

}  // namespace

extern "C" int mf_tsdf_integrate_colors(float *colors, int32_t nx, int32_t ny, int32_t nz, double origin_x,
                                        double origin_y, double origin_z, double pitch, double truncation,
                                        double max_weight, const float *depth, const uint8_t *rgb, int32_t H, int32_t W,
                                        double fx, double fy, double cx, double cy, const double *T_sensor_to_map,
                                        const int32_t *skip_flag, mfStream_t stream) {
  if (bad_volume(nx, ny, nz) || !(pitch > 0.0) || !(truncation > 0.0) || !(max_weight >= 1.0) ||
      bad_camera(H, W, fx, fy))
    return bad("mf_tsdf_integrate_colors: nx, ny, nz >= 2 with fewer than 2^31 voxels, pitch > 0, truncation > 0, "
               "max_weight >= 1, 1 <= H, W <= MF_RENDER_MAX_SIDE, fx, fy > 0");
  if (!colors || !depth || !rgb || !T_sensor_to_map)
    return bad("mf_tsdf_integrate_colors: null colors, depth, rgb or T_sensor_to_map");
  if (misaligned(colors)) return bad("mf_tsdf_integrate_colors: colors must be 16-byte aligned");
  const Grid G = grid_of(nx, ny, nz, origin_x, origin_y, origin_z, pitch);
  hipLaunchKernelGGL(k_tsdf_integrate_colors, lanes(G.voxels()), dim3(kThreads), 0, (hipStream_t)stream,
                     (float4 *)colors, G, Fuse{truncation, max_weight}, depth, rgb, camera_of(H, W, fx, fy, cx, cy),
                     T_sensor_to_map, skip_flag);
  return mf::check_launch("mf_tsdf_integrate_colors");
}

extern "C" int mf_tsdf_color_image(const float *colors, int32_t nx, int32_t ny, int32_t nz, double origin_x,
                                   double origin_y, double origin_z, double pitch, const float *depth, int32_t H,
                                   int32_t W, double fx, double fy, double cx, double cy,
                                   const double *T_sensor_to_map, uint8_t *out, mfStream_t stream) {
  if (bad_volume(nx, ny, nz) || !(pitch > 0.0) || bad_camera(H, W, fx, fy))
    return bad("mf_tsdf_color_image: nx, ny, nz >= 2 with fewer than 2^31 voxels, pitch > 0, 1 <= H, W <= "
               "MF_RENDER_MAX_SIDE, fx, fy > 0");
  if (!colors || !depth || !T_sensor_to_map || !out)
    return bad("mf_tsdf_color_image: null colors, depth, T_sensor_to_map or out");
  if (misaligned(colors) || ((uintptr_t)out & 3u) != 0)
    return bad("mf_tsdf_color_image: colors must be 16-byte aligned, out 4-byte aligned");
  hipLaunchKernelGGL(k_tsdf_color_image, tiles(H, W), dim3(kTile, kTile), 0, (hipStream_t)stream,
                     (const float4 *)colors, grid_of(nx, ny, nz, origin_x, origin_y, origin_z, pitch), depth,
                     camera_of(H, W, fx, fy, cx, cy), T_sensor_to_map, (uint32_t *)out);
  return mf::check_launch("mf_tsdf_color_image");
}

extern "C" int mf_tsdf_sample_colors(const float *colors, int32_t nx, int32_t ny, int32_t nz, double origin_x,
                                     double origin_y, double origin_z, double pitch, const double *points, int64_t N,
                                     uint8_t *out, mfStream_t stream) {
  if (bad_volume(nx, ny, nz) || !(pitch > 0.0) || N < 1 || N >= ((int64_t)1 << 31))
    return bad("mf_tsdf_sample_colors: nx, ny, nz >= 2 with fewer than 2^31 voxels, pitch > 0, 1 <= N < 2^31");
  if (!colors || !points || !out) return bad("mf_tsdf_sample_colors: null colors, points or out");
  if (misaligned(colors) || ((uintptr_t)out & 3u) != 0)
    return bad("mf_tsdf_sample_colors: colors must be 16-byte aligned, out 4-byte aligned");
  hipLaunchKernelGGL(k_tsdf_sample_colors, lanes(N), dim3(kThreads), 0, (hipStream_t)stream, (const float4 *)colors,
                     grid_of(nx, ny, nz, origin_x, origin_y, origin_z, pitch), points, N, (uint32_t *)out);
  return mf::check_launch("mf_tsdf_sample_colors");
}
