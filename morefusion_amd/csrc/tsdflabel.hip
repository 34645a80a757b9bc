// TSDF labels: a per-voxel instance label fused next to (tsdf, weight), and what the pose stages need from it
// (contrib/instance_tsdf_volume.py) -- gfx950, float64 coordinates, int32 label arithmetic.
//
// include/mfhip.h "TSDF labels" is the contract -- the layout, the vote rule, every formula and its association -- and
// tests/tsdflabel_ref.py the NumPy mirror this file is pinned to bit for bit; DESIGN.md "TSDF labels" has the cost model.
//
//   k_tsdf_integrate_labels  a lane per voxel, x fastest: the voxel body of k_tsdf_integrate (tsdf_voxel.h, the same
//                            text: the (tsdf, weight) bytes are those of mf_tsdf_integrate), then one vote on the
//                            voxel's own (label, count) pair.  A lane reads and writes only its own voxel.
//   k_tsdf_label_image       a lane per pixel in 16 x 16 tiles: the label of the voxel a depth pixel falls into
//                            (tsdf_voxel.h's label_at, the same text as the label tail of k_tsdf_render).
//   k_tsdf_stats_init / k_tsdf_instance_stats
//                            a lane per voxel; the id list and a [B, 10] int64 table live in LDS, lanes add to it with
//                            integer LDS atomics and the workgroup adds its non-empty rows to the int64 table in
//                            memory with 64-bit integer atomics.  Integers only: the result has no order.
//   k_tsdf_publish_grids     a lane per voxel of all B grids: D^3 samples in the SENSOR frame, looked up in the volume
//                            (tsdf_voxel.h's voxel_of).
//
// No float atomics.  Coordinates use only + - * / and floor, nothing is contracted (-ffp-contract=off).
#include <limits.h>
#include <math.h>

#include "host_args.h"
#include "mf_common.h"
#include "tsdf_voxel.h"

namespace {

constexpr int kCols = 10;  // {count, sum i, j, k, min i, j, k, max i, j, k}

using namespace mf_tsdf;

__global__ void __launch_bounds__(kThreads) k_tsdf_integrate_labels(
    float2 *__restrict__ vol, int2 *__restrict__ labels, Grid G, Fuse fuse, const float *__restrict__ depth, Camera cam,
    const double *__restrict__ T, const int32_t *__restrict__ label_image, int max_count,
    const int32_t *__restrict__ skip_flag) {
  if (skip_flag && *skip_flag != 0) return;
  const int64_t n = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (n >= G.voxels()) return;
  const Pose P = load_pose(T);
  int64_t pixel;
  double sdf;
  if (!mf_tsdf::voxel_body<true>(vol, n, G, fuse, depth, cam, P, pixel, sdf)) return;
  if (!(sdf <= fuse.truncation)) return;  // far in front of the surface: the tsdf moves, the label does not
  const int v = label_image[pixel];
  if (!(v >= 1 || v == -1)) return;
  int2 lc = labels[n];
  if (lc.y == 0) {
    lc = make_int2(v, 1);
  } else if (lc.x == v) {
    lc.y = lc.y + 1 < max_count ? lc.y + 1 : max_count;
  } else {
    lc.y -= 1;
    if (lc.y == 0) lc.x = 0;
  }
  labels[n] = lc;
}

__global__ void __launch_bounds__(kTile *kTile) k_tsdf_label_image(const int2 *__restrict__ labels, Grid G,
                                                                   const float *__restrict__ depth, Camera cam,
                                                                   const double *__restrict__ T, int min_count,
                                                                   int32_t *__restrict__ out) {
  const int col = (int)blockIdx.x * kTile + (int)threadIdx.x, row = (int)blockIdx.y * kTile + (int)threadIdx.y;
  if (col >= cam.W || row >= cam.H) return;
  const int64_t p = cam.pixel(col, row);
  const double d = (double)depth[p];
  int label = 0;
  if (d > 0.0) {
    const Pose P = load_pose(T);
    double q0, q1;
    cam.ray(col, row, q0, q1);
    label = mf_tsdf::label_at(labels, G, q0, q1, d, P, min_count);
  }
  out[p] = label;
}

__global__ void __launch_bounds__(kThreads) k_tsdf_stats_init(long long *__restrict__ table, int B, Grid G) {
  const int t = (int)blockIdx.x * kThreads + (int)threadIdx.x;
  if (t >= B * kCols) return;
  const int c = t % kCols;
  table[t] = c < 4 ? 0 : (c < 7 ? (long long)G.n[c - 4] : -1);
}

__global__ void __launch_bounds__(kThreads) k_tsdf_instance_stats(
    const float2 *__restrict__ vol, const int2 *__restrict__ labels, Grid G, double min_weight, int min_count,
    const int32_t *__restrict__ ids, int B, long long *__restrict__ table) {
  __shared__ int s_ids[MF_TSDF_MAX_INSTANCES];
  __shared__ long long s_tab[MF_TSDF_MAX_INSTANCES * kCols];  // 64-bit: 256 indices of up to 2^29 do not fit 32
  const int tid = (int)threadIdx.x;
  if (tid < B) s_ids[tid] = ids[tid];
  for (int t = tid; t < B * kCols; t += kThreads) {
    const int c = t % kCols;
    s_tab[t] = c < 4 ? 0 : (c < 7 ? (long long)INT_MAX : -1);
  }
  __syncthreads();
  const int64_t n = (int64_t)blockIdx.x * kThreads + tid;
  if (n < G.voxels()) {
    const float2 fw = vol[n];
    const int2 lc = labels[n];
    if ((double)fw.y >= min_weight && fw.x <= 0.0f && lc.y >= min_count) {
      int lo = 0, hi = B;  // the ids are strictly ascending: the first one >= the label
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (s_ids[mid] < lc.x) lo = mid + 1;
        else hi = mid;
      }
      if (lo < B && s_ids[lo] == lc.x) {
        int idx[3];
        G.unflatten(n, idx);
        long long *row = s_tab + lo * kCols;
        atomicAdd((unsigned long long *)&row[0], 1ull);
#pragma unroll
        for (int a = 0; a < 3; ++a) {
          atomicAdd((unsigned long long *)&row[1 + a], (unsigned long long)idx[a]);
          atomicMin(&row[4 + a], (long long)idx[a]);
          atomicMax(&row[7 + a], (long long)idx[a]);
        }
      }
    }
  }
  __syncthreads();
  for (int t = tid; t < B * kCols; t += kThreads) {
    const int b = t / kCols, c = t % kCols;
    if (s_tab[b * kCols] == 0) continue;  // an empty row adds nothing
    const long long v = s_tab[t];
    if (c < 4) atomicAdd((unsigned long long *)&table[t], (unsigned long long)v);
    else if (c < 7) atomicMin(&table[t], v);
    else atomicMax(&table[t], v);
  }
}

__global__ void __launch_bounds__(kThreads) k_tsdf_publish_grids(
    const float2 *__restrict__ vol, const int2 *__restrict__ labels, Grid G, const int32_t *__restrict__ ids,
    const double *__restrict__ grid_pitch, const double *__restrict__ center_map,
    const double *__restrict__ T_map_to_sensor, const double *__restrict__ T_sensor_to_map, double min_weight,
    int min_count, double empty_above, double ground_z, int flags, int B, int D, double *__restrict__ origin_out,
    float *__restrict__ grid_target, float *__restrict__ grid_noentry, uint8_t *__restrict__ grid_nte) {
  const int64_t nvox = (int64_t)D * D * D;
  const int64_t g = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (g >= nvox * B) return;
  const int b = (int)(g / nvox);
  const int64_t v = g - (int64_t)b * nvox;
  const int idx[3] = {(int)(v / ((int64_t)D * D)), (int)((v / D) % D), (int)(v % D)};
  const double gp = grid_pitch[b];
  const double c0 = center_map[3 * b], c1 = center_map[3 * b + 1], c2 = center_map[3 * b + 2];
  const Pose Pm = load_pose(T_map_to_sensor), Ps = load_pose(T_sensor_to_map);
  double s[3], m[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const double centre = ((Pm.R[3 * a] * c0 + Pm.R[3 * a + 1] * c1) + Pm.R[3 * a + 2] * c2) + Pm.t[a];
    const double origin = centre - ((double)D / 2.0 - 0.5) * gp;
    if (v == 0) origin_out[3 * b + a] = origin;
    s[a] = origin + gp * (double)idx[a];
  }
#pragma unroll
  for (int a = 0; a < 3; ++a) m[a] = ((Ps.R[3 * a] * s[0] + Ps.R[3 * a + 1] * s[1]) + Ps.R[3 * a + 2] * s[2]) + Ps.t[a];
  float gt = 0.0f, ne = 0.0f;
  if ((flags & 1) && m[2] < ground_z) {
    ne = 1.0f;  // below the ground plane
  } else {
    const int64_t n = mf_tsdf::voxel_of(m, G);
    if (n >= 0) {
      const float2 fw = vol[n];
      if ((double)fw.y >= min_weight) {
        if (fw.x <= 0.0f) {  // occupied, as extract_mesh reads it
          const int2 lc = labels[n];
          if (lc.y >= min_count) {
            if (lc.x == ids[b]) gt = 1.0f;
            else if (lc.x != 0) ne = 1.0f;  // another instance, or the background
          }
        } else if ((flags & 2) && (double)fw.x >= empty_above) {
          ne = 1.0f;  // seen free
        }
      }
    }
  }
  grid_target[g] = gt;
  grid_noentry[g] = ne;
  grid_nte[g] = ne != 0.0f;
}

}  // namespace

extern "C" int mf_tsdf_integrate_labels(float *volume, int32_t *labels, int32_t nx, int32_t ny, int32_t nz,
                                        double origin_x, double origin_y, double origin_z, double pitch,
                                        double truncation, double max_weight, const float *depth, int32_t H, int32_t W,
                                        double fx, double fy, double cx, double cy, const double *T_sensor_to_map,
                                        const int32_t *label_image, int32_t max_count, const int32_t *skip_flag,
                                        mfStream_t stream) {
  if (bad_volume(nx, ny, nz) || !(pitch > 0.0) || !(truncation > 0.0) || !(max_weight >= 1.0) ||
      bad_camera(H, W, fx, fy) || max_count < 1)
    return bad("mf_tsdf_integrate_labels: nx, ny, nz >= 2 with fewer than 2^31 voxels, pitch > 0, truncation > 0, "
               "max_weight >= 1, 1 <= H, W <= MF_RENDER_MAX_SIDE, fx, fy > 0, max_count >= 1");
  if (!volume || !labels || !depth || !T_sensor_to_map || !label_image)
    return bad("mf_tsdf_integrate_labels: null volume, labels, depth, T_sensor_to_map or label_image");
  const Grid G = grid_of(nx, ny, nz, origin_x, origin_y, origin_z, pitch);
  hipLaunchKernelGGL(k_tsdf_integrate_labels, lanes(G.voxels()), dim3(kThreads), 0, (hipStream_t)stream,
                     (float2 *)volume, (int2 *)labels, G, Fuse{truncation, max_weight}, depth,
                     camera_of(H, W, fx, fy, cx, cy), T_sensor_to_map, label_image, (int)max_count, skip_flag);
  return mf::check_launch("mf_tsdf_integrate_labels");
}

extern "C" int mf_tsdf_label_image(const int32_t *labels, int32_t nx, int32_t ny, int32_t nz, double origin_x,
                                   double origin_y, double origin_z, double pitch, const float *depth, int32_t H,
                                   int32_t W, double fx, double fy, double cx, double cy,
                                   const double *T_sensor_to_map, int32_t min_count, int32_t *out, mfStream_t stream) {
  if (bad_volume(nx, ny, nz) || !(pitch > 0.0) || bad_camera(H, W, fx, fy) || min_count < 1)
    return bad("mf_tsdf_label_image: nx, ny, nz >= 2 with fewer than 2^31 voxels, pitch > 0, 1 <= H, W <= "
               "MF_RENDER_MAX_SIDE, fx, fy > 0, min_count >= 1");
  if (!labels || !depth || !T_sensor_to_map || !out)
    return bad("mf_tsdf_label_image: null labels, depth, T_sensor_to_map or out");
  hipLaunchKernelGGL(k_tsdf_label_image, tiles(H, W), dim3(kTile, kTile), 0, (hipStream_t)stream, (const int2 *)labels,
                     grid_of(nx, ny, nz, origin_x, origin_y, origin_z, pitch), depth, camera_of(H, W, fx, fy, cx, cy),
                     T_sensor_to_map, (int)min_count, out);
  return mf::check_launch("mf_tsdf_label_image");
}

extern "C" int mf_tsdf_instance_stats(const float *volume, const int32_t *labels, int32_t nx, int32_t ny, int32_t nz,
                                      double min_weight, int32_t min_count, const int32_t *ids, int32_t B,
                                      int64_t *table, mfStream_t stream) {
  if (bad_volume(nx, ny, nz) || !(min_weight > 0.0) || min_count < 1 || B < 1 || B > MF_TSDF_MAX_INSTANCES)
    return bad("mf_tsdf_instance_stats: nx, ny, nz >= 2 with fewer than 2^31 voxels, min_weight > 0, min_count >= 1, "
               "1 <= B <= MF_TSDF_MAX_INSTANCES");
  if (!volume || !labels || !ids || !table) return bad("mf_tsdf_instance_stats: null volume, labels, ids or table");
  const Grid G = grid_of(nx, ny, nz);
  hipLaunchKernelGGL(k_tsdf_stats_init, lanes(B * kCols), dim3(kThreads), 0, (hipStream_t)stream, (long long *)table,
                     (int)B, G);
  hipLaunchKernelGGL(k_tsdf_instance_stats, lanes(G.voxels()), dim3(kThreads), 0, (hipStream_t)stream,
                     (const float2 *)volume, (const int2 *)labels, G, min_weight, (int)min_count, ids, (int)B,
                     (long long *)table);
  return mf::check_launch("mf_tsdf_instance_stats");
}

extern "C" int mf_tsdf_publish_grids(const float *volume, const int32_t *labels, int32_t nx, int32_t ny, int32_t nz,
                                     double origin_x, double origin_y, double origin_z, double pitch,
                                     const int32_t *ids, const double *grid_pitch, const double *center_map,
                                     const double *T_map_to_sensor, const double *T_sensor_to_map, double min_weight,
                                     int32_t min_count, double empty_above, double ground_z, int32_t flags, int32_t B,
                                     int32_t D, double *origin, float *grid_target, float *grid_noentry,
                                     uint8_t *grid_nontarget_empty, mfStream_t stream) {
  if (bad_volume(nx, ny, nz) || !(pitch > 0.0) || !(min_weight > 0.0) || min_count < 1 || B < 1 ||
      B > MF_TSDF_MAX_INSTANCES || D < 1 || D > MF_TSDF_MAX_GRID_DIM || (flags & ~3))
    return bad("mf_tsdf_publish_grids: nx, ny, nz >= 2 with fewer than 2^31 voxels, pitch > 0, min_weight > 0, "
               "min_count >= 1, 1 <= B <= MF_TSDF_MAX_INSTANCES, 1 <= D <= MF_TSDF_MAX_GRID_DIM, flags in 0 .. 3");
  if (!volume || !labels || !ids || !grid_pitch || !center_map || !T_map_to_sensor || !T_sensor_to_map || !origin ||
      !grid_target || !grid_noentry || !grid_nontarget_empty)
    return bad("mf_tsdf_publish_grids: null array");
  const int64_t n = (int64_t)B * D * D * D;  // <= 64 * 256^3 = 2^30
  hipLaunchKernelGGL(k_tsdf_publish_grids, lanes(n), dim3(kThreads), 0, (hipStream_t)stream, (const float2 *)volume,
                     (const int2 *)labels, grid_of(nx, ny, nz, origin_x, origin_y, origin_z, pitch), ids, grid_pitch,
                     center_map, T_map_to_sensor, T_sensor_to_map, min_weight, (int)min_count, empty_above, ground_z,
                     (int)flags, (int)B, (int)D, origin, grid_target, grid_noentry, grid_nontarget_empty);
  return mf::check_launch("mf_tsdf_publish_grids");
}
