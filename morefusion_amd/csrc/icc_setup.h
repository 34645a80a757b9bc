// ICC kernels that run once per batch or once per call: bounding spheres, scene sums, pose -> R|t and empty
// accumulators, the bin tables.
// A piece of csrc/icc.hip's single translation unit: included there, in the order of that file, nowhere else.
#pragma once
#include "icc_common.h"

namespace {

// ---- setup: bounding spheres, sum(grid_target) per scene, R|t from (q,t) -----------
__global__ __launch_bounds__(256) void k_icc_bound(IccArgs a) {
  __shared__ float s_red[4][4];
  const int o = blockIdx.x;
  const int p0 = a.obj_off[o], p1 = a.obj_off[o + 1];
  float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (int p = p0 + threadIdx.x; p < p1; p += blockDim.x) {
    const float4 m = a.pts4[p];
    lo[0] = fminf(lo[0], m.x); hi[0] = fmaxf(hi[0], m.x);
    lo[1] = fminf(lo[1], m.y); hi[1] = fmaxf(hi[1], m.y);
    lo[2] = fminf(lo[2], m.z); hi[2] = fmaxf(hi[2], m.z);
  }
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  float c[3];
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    const float l = -mf::wave_max(-lo[d]), h = mf::wave_max(hi[d]);
    __syncthreads();
    if (lane == 0) { s_red[wave][0] = l; s_red[wave][1] = h; }
    __syncthreads();
    const float L = fminf(fminf(s_red[0][0], s_red[1][0]), fminf(s_red[2][0], s_red[3][0]));
    const float H = fmaxf(fmaxf(s_red[0][1], s_red[1][1]), fmaxf(s_red[2][1], s_red[3][1]));
    c[d] = 0.5f * (L + H);
  }
  float r2 = 0.0f;
  for (int p = p0 + threadIdx.x; p < p1; p += blockDim.x) {
    const float4 m = a.pts4[p];
    const float dx = m.x - c[0], dy = m.y - c[1], dz = m.z - c[2];
    r2 = fmaxf(r2, dx * dx + dy * dy + dz * dz);
  }
  r2 = mf::wave_max(r2);
  __syncthreads();
  if (lane == 0) s_red[wave][0] = r2;
  __syncthreads();
  if (threadIdx.x == 0) {
    r2 = fmaxf(fmaxf(s_red[0][0], s_red[1][0]), fmaxf(s_red[2][0], s_red[3][0]));
    const bool empty = p1 <= p0;
    a.bound[4 * o + 0] = empty ? 0.0f : c[0];
    a.bound[4 * o + 1] = empty ? 0.0f : c[1];
    a.bound[4 * o + 2] = empty ? 0.0f : c[2];
    a.bound[4 * o + 3] = empty ? -1.0f : sqrtf(r2) * 1.0001f + 1e-6f;
    const int sc = a.obj_scene[o];
    a.meta[o] = make_int4(a.scene_off[sc], a.scene_off[sc + 1], p0, p1);
  }
}

__global__ __launch_bounds__(256) void k_icc_scene_setup(IccArgs a, int32_t step0) {
  __shared__ float s_red[4];
  const int s = blockIdx.x;
  const int V = a.D * a.D * a.D;
  const int64_t b0 = (int64_t)a.scene_off[s] * V, b1 = (int64_t)a.scene_off[s + 1] * V;
  float acc = 0.0f;
  for (int64_t i = b0 + threadIdx.x; i < b1; i += blockDim.x) acc += a.grid_target[i];
  acc = mf::wave_sum(acc);
  if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) a.St[s] = (s_red[0] + s_red[1]) + (s_red[2] + s_red[3]);
}

// Start of a loss evaluation / refinement: R|t from (q, t) (both copies); empty accumulators, per-grid
// maxima and bin counters of every parity; traj[0] = the initial pose.  One workgroup per object.
constexpr int kParities = 2;  // iteration k fills parity k & 1 while the folded step reads (k - 1) & 1 and empties it
__global__ __launch_bounds__(256) void k_icc_pose(IccArgs a, const float *__restrict__ q,
                                                  const float *__restrict__ t, float *traj) {
  const int o = blockIdx.x;
  const int tid = threadIdx.x;
  if (tid == 0) {
    float R[9];
    quat_to_R(q + 4 * o, R);
    for (int cp = 0; cp < 2; ++cp) {
      float *Rt = a.Rt + ((int64_t)cp * a.O + o) * 12;
#pragma unroll
      for (int i = 0; i < 9; ++i) Rt[i] = R[i];
#pragma unroll
      for (int i = 0; i < 3; ++i) Rt[9 + i] = t[3 * o + i];
    }
    if (traj) {
#pragma unroll
      for (int i = 0; i < 4; ++i) traj[7 * o + i] = q[4 * o + i];
#pragma unroll
      for (int i = 0; i < 3; ++i) traj[7 * o + 4 + i] = t[3 * o + i];
    }
  }
  for (int par = 0; par < kParities; ++par) {
    if (tid < 2) a.Mbits[(int64_t)par * 2 * a.O + 2 * o + tid] = 0;
    for (int i = tid; i < 2 * a.nbins; i += blockDim.x) a.bin_cnt[((int64_t)par * 2 * a.O + 2 * o) * a.nbins + i] = 0u;
    for (int i = tid; i < kOwnSlots; i += blockDim.x) a.acc_own[((int64_t)par * a.O + o) * kOwnSlots + i] = 0;
    for (int i = tid; i < a.max_ns * 12; i += blockDim.x) a.acc_oth[((int64_t)par * a.O + o) * a.max_ns * 12 + i] = 0;
  }
}

// First node of mf_icc_refine_converge's graph: fresh loss observers (both copies of every scene's record).
__global__ __launch_bounds__(64) void k_icc_obs_reset(IccObsRec *rec, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  IccObsRec r;
  for (int k = 0; k < kObsMaxWindow; ++k) r.delta[k] = 0.0;
  r.last = 0.0f;
  r.has_last = r.fill = r.head = r.n_passed = r.frozen = r.n_steps = r.pad_ = 0;
  rec[i] = r;
}

// Once per batch: bin capacities/offsets per grid and the (target, source, point chunk) table.
__global__ __launch_bounds__(256) void k_icc_tables(IccArgs a) {
  __shared__ int s_tab_base[1];
  if (threadIdx.x == 0) {
    int64_t rec_off = 0;
    int tab_off = 0;
    for (int o = 0; o < a.O; ++o) {
      const int sc = a.obj_scene[o];
      const int ja = a.scene_off[sc], jb = a.scene_off[sc + 1];
      const int p_own = a.obj_off[o + 1] - a.obj_off[o];
      const int p_all = a.obj_off[jb] - a.obj_off[ja];
      const int nreal = a.nbins - 1;
      a.bin_cap[2 * o] = bin_cap_of(p_own, a.bin_cap_force);
      a.bin_pts[2 * o] = p_own;
      a.bin_base[2 * o] = rec_off;
      rec_off += (int64_t)nreal * a.bin_cap[2 * o] + 2 * (int64_t)p_own;
      a.bin_cap[2 * o + 1] = bin_cap_of(p_all - p_own, a.bin_cap_force);
      a.bin_pts[2 * o + 1] = p_all - p_own;
      a.bin_base[2 * o + 1] = rec_off;
      rec_off += (int64_t)nreal * a.bin_cap[2 * o + 1] + 2 * (int64_t)(p_all - p_own);
      for (int j = ja; j < jb; ++j) {
        const int p0 = a.obj_off[j], p1 = a.obj_off[j + 1];
        // the first chunk of the pair (j, j) is the designated entry of object j: it stores the
        // optimiser step folded into k_icc_bin (exists even for an object without points)
        for (int c = p0; c < p1 || (c == p0 && j == o); c += kBinChunk)
          if (tab_off < a.n_tab) {
            a.tab[tab_off] = make_int4(o, j, c, min(c + kBinChunk, p1));
            a.tab2[tab_off] = make_int4(ja, jb - ja, sc, (j == o && c == p0) ? 1 : 0);
            ++tab_off;
          }
      }
    }
    s_tab_base[0] = tab_off;
  }
  __syncthreads();
  for (int i = s_tab_base[0] + threadIdx.x; i < a.n_tab; i += blockDim.x) a.tab[i] = make_int4(-1, -1, 0, 0);
  for (int i = threadIdx.x; i < kParities * 2 * a.O * a.nbins; i += blockDim.x) a.bin_cnt[i] = 0u;
}

}  // namespace
