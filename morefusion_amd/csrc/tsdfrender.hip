// TSDF render: the ray-cast of csrc/tsdf.hip with empty-space skipping and the label image fused in
// (contrib/tsdf_volume.py TsdfVolume.render, contrib/instance_tsdf_volume.py) -- gfx950, float64 arithmetic on float32
// storage.
//
// include/mfhip.h "TSDF render" is the contract and tests/tsdfrender_ref.py the NumPy mirror this file is pinned to bit
// for bit; DESIGN.md "TSDF render" has the monotonicity argument and the cost model.  depth_out and code_out are the
// bytes of mf_tsdf_raycast and label_out those of mf_tsdf_label_image, whatever the volume holds: a block code only
// replaces eight loads by the value those loads would have given.
//
//   k_tsdf_block_summary  a workgroup per (256 voxels along x, block row J, block layer K); a lane per voxel of the x
//                         run, which walks the (B + 1)^2 rows of the footprint and ORs two bits per voxel ("not free",
//                         "seen").  The last lane of every block also reads the block's halo voxel.  A block is B
//                         consecutive lanes of one wave: two ballots reduce it, its first lane puts the code into LDS,
//                         and the workgroup stores its codes as one run of bytes.  OR has no order.
//   k_tsdf_render         a lane per pixel in 16 x 16 tiles: k_tsdf_raycast's march (the ray set-up, the sample and
//                         the hit rule are tsdf_ray.h's, one text for both kernels), with one summary byte read per
//                         sample in place of the 64 bytes of a FREE or UNKNOWN block, and a verified jump to the last
//                         sample inside such a block.  The label tail is tsdf_voxel.h's label_at, which is all of
//                         k_tsdf_label_image.
//
// No atomics.  Nothing is contracted (-ffp-contract=off); only + - * / and floor are used on coordinates.
#include <math.h>

#include "host_args.h"
#include "mf_common.h"
#include "tsdf_ray.h"
#include "tsdf_voxel.h"

namespace {

using namespace mf_tsdf;

// bit 0: the voxel is not free (not (weight > 0 and tsdf == 1)); bit 1: the voxel was seen (weight > 0)
__device__ __forceinline__ int voxel_bits(const float2 fw) {
  const bool seen = fw.y > 0.0f;
  return (seen && fw.x == 1.0f ? 0 : 1) | (seen ? 2 : 0);
}

__global__ void __launch_bounds__(kThreads) k_tsdf_block_summary(const float2 *__restrict__ vol, int nx, int ny, int nz,
                                                                 int shift, int chunks, int nbx, int nby,
                                                                 uint8_t *__restrict__ summary) {
  __shared__ uint8_t s_code[kThreads / 2];
  const int B = 1 << shift, tid = (int)threadIdx.x;
  const int chunk = (int)(blockIdx.x % (unsigned)chunks);
  const int rest = (int)(blockIdx.x / (unsigned)chunks);
  const int J = rest % nby, K = rest / nby;
  const int64_t i = (int64_t)chunk * kThreads + tid;  // this lane's voxel along x, cell i of block i >> shift
  const bool own = i <= nx - 1 && (i >> shift) < nbx;
  const bool halo = own && ((tid + 1) & (B - 1)) == 0 && i + 1 <= nx - 1;  // the block's last lane: voxel i + 1 too
  const int j0 = J << shift, k0 = K << shift;
  const int j1 = j0 + B < ny - 1 ? j0 + B : ny - 1, k1 = k0 + B < nz - 1 ? k0 + B : nz - 1;
  int bits = 0;
  if (own) {
    for (int k = k0; k <= k1; ++k) {
      const float2 *row = vol + ((int64_t)k * ny + j0) * nx + i;
#pragma unroll 4
      for (int j = j0; j <= j1; ++j, row += nx) {
        bits |= voxel_bits(row[0]);
        if (halo) bits |= voxel_bits(row[1]);
      }
    }
  }
  // lanes past the volume vote "free and unseen": they change neither OR
  const unsigned long long not_free = __ballot(bits & 1), seen = __ballot(bits & 2);
  if (own && (tid & (B - 1)) == 0) {
    const int lane = tid & 63;
    const unsigned long long mask = ((1ull << B) - 1ull) << lane;  // B <= 16: the block's lanes, all in this wave
    s_code[tid >> shift] = (uint8_t)(!(not_free & mask) ? MF_TSDF_BLOCK_FREE
                                                        : (!(seen & mask) ? MF_TSDF_BLOCK_UNKNOWN : MF_TSDF_BLOCK_MIXED));
  }
  __syncthreads();
  const int per_chunk = kThreads >> shift;
  const int I = chunk * per_chunk + tid;
  if (tid < per_chunk && I < nbx) summary[((int64_t)K * nby + J) * nbx + I] = s_code[tid];
}

__global__ void __launch_bounds__(kTile *kTile) k_tsdf_render(
    const float *__restrict__ vol, Grid G, March march, Camera cam, const double *__restrict__ T,
    const uint8_t *__restrict__ summary, int shift, const int2 *__restrict__ labels, int min_count,
    float *__restrict__ depth_out, uint8_t *__restrict__ code_out, int32_t *__restrict__ label_out,
    int2 *__restrict__ stats_out) {
  const int col = (int)blockIdx.x * kTile + (int)threadIdx.x, row = (int)blockIdx.y * kTile + (int)threadIdx.y;
  if (col >= cam.W || row >= cam.H) return;
  const Pose P = load_pose(T);
  const double step = march.step;
  const int max_steps = march.max_steps;
  double q0, q1, d[3], enter, leave;
  cam.ray(col, row, q0, q1);
  int code = mf_tsdf::ray_setup(P, q0, q1, G, march, d, enter, leave);
  float out = 0.0f;
  int sampled = 0, visited = 0;
  if (code < 0) {
    const int nbx = ((G.n[0] - 2) >> shift) + 1, nby = ((G.n[1] - 2) >> shift) + 1;
    bool have = false;
    double prev = 0.0;
    // the jump: `tried` is the block the last attempt started from (a ray meets a block once), (k_pend, pend) a
    // position computed for a sample that the march has yet to reach -- it is used there, not computed again
    int tried = -1, k_pend = -1;
    double pend[3] = {0.0, 0.0, 0.0};
    for (int k = 0;; ++k) {
      const double s = enter + (double)k * step;
      if (!(s <= leave)) { code = MF_TSDF_RAY_LEFT; break; }
      if (k >= max_steps) { code = MF_TSDF_RAY_CAP; break; }
      double g[3], b[3];
      if (k == k_pend) {
        g[0] = pend[0], g[1] = pend[1], g[2] = pend[2];
      } else {
        mf_tsdf::grid_pos(P, d, s, G, g);
        ++visited;
      }
      if (!mf_tsdf::cell_of(g, G, b)) {
        have = false;
        ++sampled;
        continue;
      }
      const int I0 = (int)b[0] >> shift, I1 = (int)b[1] >> shift, I2 = (int)b[2] >> shift;
      const int blk = (I2 * nby + I1) * nbx + I0;
      const int block_code = summary[blk];
      if (block_code != MF_TSDF_BLOCK_MIXED) {
        // FREE: eight voxels of tsdf 1 and weight > 0 give F = 1 + r * (1 - 1) = 1; UNKNOWN: no weight is > 0
        have = block_code == MF_TSDF_BLOCK_FREE;
        prev = 1.0;
        if (blk != tried && k_pend <= k) {
          tried = blk;
          // where the ray leaves the block's cells (an estimate: the sample it gives is checked, not trusted)
          const int I[3] = {I0, I1, I2};
          double s_out = leave;
#pragma unroll
          for (int a = 0; a < 3; ++a) {
            const int top = (I[a] + 1) << shift;
            const double face = d[a] > 0.0 ? (double)(top < G.n[a] - 1 ? top : G.n[a] - 1) : (double)(I[a] << shift);
            const double t = ((G.o[a] + G.pitch * face) - P.t[a]) / d[a];
            if ((d[a] < 0.0 || d[a] > 0.0) && t < s_out) s_out = t;
          }
          double kc = floor((s_out - enter) / step);
          if (kc > (double)(max_steps - 1)) kc = (double)(max_steps - 1);
          if (kc > (double)(k + 1)) {  // (a NaN fails)
            int kj = (int)kc;
            double sj = enter + (double)kj * step;
            if (!(sj <= leave)) {
              --kj;
              sj = enter + (double)kj * step;
            }
            if (kj > k + 1 && sj <= leave) {
              double h[3], c[3];
              mf_tsdf::grid_pos(P, d, sj, G, h);
              ++visited;
              if (mf_tsdf::cell_of(h, G, c) && ((int)c[0] >> shift) == I0 && ((int)c[1] >> shift) == I1 &&
                  ((int)c[2] >> shift) == I2) {
                k = kj;  // floor(g_a) is monotone in k: every sample up to kj lies in this block
              } else {
                k_pend = kj, pend[0] = h[0], pend[1] = h[1], pend[2] = h[2];
              }
            }
          }
        }
        continue;
      }
      ++sampled;
      const mf_tsdf::Cell cell = mf_tsdf::load_cell(vol, G, b);
      if (!mf_tsdf::all_seen(cell)) { have = false; continue; }
      const double F = mf_tsdf::trilinear(cell, g, b);
      if (F <= 0.0) { code = mf_tsdf::ray_crossing(have, prev, F, enter, step, k, out); break; }
      have = true;
      prev = F;
    }
  }
  const int64_t p = cam.pixel(col, row);
  depth_out[p] = out;
  if (code_out) code_out[p] = (uint8_t)code;
  if (stats_out) stats_out[p] = make_int2(sampled, visited);
  if (label_out) {
    // mf_tsdf_label_image on the float32 just stored
    const double dd = (double)out;
    int label = 0;
    if (dd > 0.0) label = mf_tsdf::label_at(labels, G, q0, q1, dd, P, min_count);
    label_out[p] = label;
  }
}

// log2 of an allowed block edge, -1 for any other
int shift_of(int32_t B) { return B == 2 ? 1 : B == 4 ? 2 : B == 8 ? 3 : B == 16 ? 4 : -1; }

}  // namespace

extern "C" int64_t mf_tsdf_summary_bytes(int32_t nx, int32_t ny, int32_t nz, int32_t B) {
  const int shift = shift_of(B);
  if (bad_volume(nx, ny, nz) || shift < 0) return -1;
  return ((int64_t)((nx - 2) >> shift) + 1) * (((ny - 2) >> shift) + 1) * (((nz - 2) >> shift) + 1);
}

extern "C" int mf_tsdf_block_summary(const float *volume, int32_t nx, int32_t ny, int32_t nz, int32_t B,
                                     uint8_t *summary, mfStream_t stream) {
  const int shift = shift_of(B);
  if (bad_volume(nx, ny, nz) || shift < 0)
    return bad("mf_tsdf_block_summary: nx, ny, nz >= 2 with fewer than 2^31 voxels, B one of 2, 4, 8, 16");
  if (!volume || !summary) return bad("mf_tsdf_block_summary: null volume or summary");
  const int nbx = ((nx - 2) >> shift) + 1, nby = ((ny - 2) >> shift) + 1, nbz = ((nz - 2) >> shift) + 1;
  const int per_chunk = kThreads >> shift;
  const int chunks = (nbx + per_chunk - 1) / per_chunk;
  const int64_t groups = (int64_t)chunks * nby * nbz;  // <= the number of blocks < 2^31
  hipLaunchKernelGGL(k_tsdf_block_summary, dim3((unsigned)groups), dim3(kThreads), 0, (hipStream_t)stream,
                     (const float2 *)volume, (int)nx, (int)ny, (int)nz, shift, chunks, nbx, nby, summary);
  return mf::check_launch("mf_tsdf_block_summary");
}

extern "C" int mf_tsdf_render(const float *volume, int32_t nx, int32_t ny, int32_t nz, double origin_x,
                              double origin_y, double origin_z, double pitch, double step, double min_depth,
                              double max_depth, int32_t max_steps, int32_t H, int32_t W, double fx, double fy, double cx,
                              double cy, const double *T_sensor_to_map, const uint8_t *summary, int32_t B,
                              const int32_t *labels, int32_t min_count, float *depth_out, uint8_t *code_out,
                              int32_t *label_out, int32_t *stats_out, mfStream_t stream) {
  const int shift = shift_of(B);
  if (bad_volume(nx, ny, nz) || !(pitch > 0.0) || !(step > 0.0) || !(min_depth >= 0.0 && min_depth < max_depth) ||
      max_steps < 1 || max_steps > MF_TSDF_MAX_STEPS || bad_camera(H, W, fx, fy) || shift < 0 ||
      (labels && min_count < 1))
    return bad("mf_tsdf_render: nx, ny, nz >= 2 with fewer than 2^31 voxels, pitch > 0, step > 0, 0 <= min_depth < "
               "max_depth, 1 <= max_steps <= MF_TSDF_MAX_STEPS, 1 <= H, W <= MF_RENDER_MAX_SIDE, fx, fy > 0, B one of "
               "2, 4, 8, 16, min_count >= 1 with labels");
  if (!volume || !T_sensor_to_map || !summary || !depth_out)
    return bad("mf_tsdf_render: null volume, T_sensor_to_map, summary or depth_out");
  if ((labels != nullptr) != (label_out != nullptr))
    return bad("mf_tsdf_render: labels and label_out are both null or both non-null");
  hipLaunchKernelGGL(k_tsdf_render, tiles(H, W), dim3(kTile, kTile), 0, (hipStream_t)stream, volume,
                     grid_of(nx, ny, nz, origin_x, origin_y, origin_z, pitch),
                     March{step, min_depth, max_depth, max_steps}, camera_of(H, W, fx, fy, cx, cy), T_sensor_to_map, summary, shift, (const int2 *)labels, (int)min_count, depth_out, code_out,
                     label_out, (int2 *)stats_out);
  return mf::check_launch("mf_tsdf_render");
}
