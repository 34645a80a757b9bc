// k_icc_bin: launch 1 of an ICC iteration -- the previous iteration's optimiser step, then the x-plane binning.
// A piece of csrc/icc.hip's single translation unit: included there, in the order of that file, nowhere else.
#pragma once
#include "icc_common.h"
#include "icc_step.h"

namespace {

// What the designated workgroup of object j empties, all lanes together (one lane storing ~300 words in a row
// measured 4 us): this object's accumulators and maxima of the parity the coming iteration adds into, and the bins
// of its two grids that the NEXT iteration fills.
__device__ __forceinline__ void icc_bin_empties(const IccArgs &a, const IccStepArgs &sp, int j, int nb) {
  if (threadIdx.x < 2) a.Mbits[(int64_t)(sp.par ^ 1) * 2 * a.O + 2 * j + threadIdx.x] = 0;
  long long *own = a.acc_own + ((int64_t)(sp.par ^ 1) * a.O + j) * kOwnSlots;
  for (int i = threadIdx.x; i < kOwnSlots; i += kBinThreads) own[i] = 0;
  long long *oth = a.acc_oth + ((int64_t)(sp.par ^ 1) * a.O + j) * a.max_ns * 12;
  for (int i = threadIdx.x; i < a.max_ns * 12; i += kBinThreads) oth[i] = 0;
  for (int i = threadIdx.x; i < 2 * nb; i += kBinThreads)
    a.bin_cnt[((int64_t)(sp.cpar ^ 1) * 2 * a.O + 2 * j) * nb + i] = 0u;
}

// launch 1: one workgroup per (target grid, source object, chunk of <= 1024 points)
// OBS (mf_icc_refine_converge): the step carries the scene's loss observer (icc_step.h), and the workgroups of a
// frozen scene neither step nor bin.  Everything of it sits behind `if constexpr`: k_icc_bin<false> is the kernel
// the fixed loop always had.
template <bool OBS>
__global__ __launch_bounds__(kBinThreads) void k_icc_bin(IccArgs a, IccStepArgs sp, typename IccObsOf<OBS>::type ob) {
  __shared__ int s_cnt[kMaxBins], s_base[kMaxBins];
  __shared__ float s_sum[kStepSums], s_state[kStateFloats];
  __shared__ __attribute__((aligned(16))) float s_Rt12[16];
  __shared__ float s_x[kStepLaneWords];
  __shared__ long long s_raw[kStepRawWords];
  auto stamp = [&](int i) {  // tuning aid (MF_ICC_DEBUG & 32)
    if (MF_DBG(a, 32) && threadIdx.x == 0 && blockIdx.x < 1024)
      g_dbg_stamps[(3072 + blockIdx.x) * 8 + i] = wall_clock64();
  };
  stamp(0);
  // (batches of >= 32 objects: the same XCD-contiguous logical order as k_icc_fused -- the workgroups that bin for a
  // grid run on the XCD whose L2 its tiles will read the records from)
  int bi = blockIdx.x;
  if (a.xcd_order && (gridDim.x & 7) == 0) bi = (bi & 7) * (int)(gridDim.x >> 3) + (bi >> 3);
  const int4 e = a.tab[bi];
  const int o = e.x, j = e.y;
  if (o < 0) return;  // block-uniform
  const int D = a.D, nb = a.nbins, hmax = a.hmax;
  const int g = 2 * o + (j != o ? 1 : 0);
  // everything below depends on the table entries only: one memory round trip
  const int4 e2 = a.tab2[bi];  // {scene first object, objects in scene, scene, designated}
  float4 r0, r1, r2;
  float S_t = 1.0f;
  if (sp.mode == 0) {
    r0 = *reinterpret_cast<const float4 *>(a.Rt + 12 * j);
    r1 = *reinterpret_cast<const float4 *>(a.Rt + 12 * j + 4);
    r2 = *reinterpret_cast<const float4 *>(a.Rt + 12 * j + 8);
  } else {
    // its optimiser state; the reduced sums are gathered below, in the same round trip
    if (threadIdx.x >= 224 && threadIdx.x < 224 + kStateFloats) {
      const int i = threadIdx.x - 224;
      s_state[i] = i < 4 ? sp.q_in[4 * j + i] : i < 7 ? sp.t_in[3 * j + i - 4]
                   : i < 14 ? sp.m_in[7 * j + i - 7] : sp.v_in[7 * j + i - 14];
    }
    S_t = a.St[e2.z];
  }
  bool frozen = false;
  if constexpr (OBS) frozen = sp.mode != 0 && ob.rec[(int64_t)ob.in * a.S + e2.z].frozen != 0;  // block-uniform
  const float4 bnd = *reinterpret_cast<const float4 *>(a.bound + 4 * j);
  const float pitch = a.pitch[o];
  const float ox = a.origin[3 * o], oy = a.origin[3 * o + 1], oz = a.origin[3 * o + 2];
  const int cap = a.bin_cap[g];
  const int ovf_cap = 2 * a.bin_pts[g];
  const int64_t base_g = a.bin_base[g];
  const int nbr = nb - 1;  // real bins; counter nbr = the grid's overflow records
  float4 m[kBinPPT];
#pragma unroll
  for (int u = 0; u < kBinPPT; ++u) {
    const int p = e.z + u * kBinThreads + (int)threadIdx.x;
    m[u] = p < e.w ? a.pts4[p] : make_float4(0, 0, 0, 0);
  }
  for (int i = threadIdx.x; i < nbr; i += kBinThreads) s_cnt[i] = 0;
  if constexpr (OBS) {
    if (frozen) {
      // A frozen scene: (q, t, m, v) of its objects pass through with the bits of the last applied step -- the
      // designated workgroup stores them into the output copy, so the ping-pong stays consistent -- and a.Rt keeps
      // that step's R|t.  No losses / traj row, no points binned: the tiles of its grids find empty bins.  What the
      // sum kernels then leave in the accumulators and maxima of its objects (1 / M of an empty grid is not finite)
      // is never read: a frozen scene gathers nothing, and scenes share no accumulator row, maximum or bin.
      if (e2.w == 0) return;
      __syncthreads();  // s_state
      if (threadIdx.x < kStateFloats) {
        const int i = threadIdx.x;
        const float x = s_state[i];
        if (i < 4) sp.q_out[4 * j + i] = x;
        else if (i < 7) sp.t_out[3 * j + i - 4] = x;
        else if (i < 14) sp.m_out[7 * j + i - 7] = x;
        else sp.v_out[7 * j + i - 14] = x;
      }
      if (threadIdx.x == 0 && j == e2.x) icc_obs_keep(ob, a.S, e2.z);
      icc_bin_empties(a, sp, j, nb);
      return;
    }
  }
  if (sp.mode != 0) {
    // the previous iteration's reduced sums of object j (fixed point)
    if (sp.fused)
      icc_step_gather_fused<kBinThreads>(a, sp.par, j, e2.x, e2.y, s_raw, s_sum);
    else
      icc_step_gather<kBinThreads>(a, sp.par, j, e2.x, e2.y, s_raw, s_sum);
    stamp(4);
    // The step on the first 16 lanes (icc_step_lanes: gradient components, Adam updates and rotation on different
    // lanes), R|t to the others through LDS.  (Rounds 2-4: every lane of every wave evaluated the serial step --
    // 850 dependent instructions, 1.5 us of the critical path and of every SIMD's issue time.)
    if (threadIdx.x < 16) {
      float Rt[12], loss, gq[4], gt[3];
      icc_step_lanes(s_sum, S_t, s_state, sp, (int)threadIdx.x, s_x, Rt, loss, gq, gt);
      if (threadIdx.x < 12) {
        float rv = Rt[0];
#pragma unroll
        for (int i = 1; i < 12; ++i) rv = (int)threadIdx.x == i ? Rt[i] : rv;
        s_Rt12[threadIdx.x] = rv;
      }
      if (threadIdx.x == 0) s_Rt12[12] = loss;
    }
    __syncthreads();
    stamp(5);
    r0 = *reinterpret_cast<const float4 *>(&s_Rt12[0]);
    r1 = *reinterpret_cast<const float4 *>(&s_Rt12[4]);
    r2 = *reinterpret_cast<const float4 *>(&s_Rt12[8]);
    const float *st_new = s_x + 12;
    const float loss = s_Rt12[12];
    const float Rt[12] = {r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r1.w, r2.x, r2.y, r2.z, r2.w};
    if (e2.w != 0 && threadIdx.x == 0) {  // the designated workgroup of object j stores the step
#pragma unroll
      for (int i = 0; i < 4; ++i) sp.q_out[4 * j + i] = st_new[i];
#pragma unroll
      for (int i = 0; i < 3; ++i) sp.t_out[3 * j + i] = st_new[4 + i];
#pragma unroll
      for (int i = 0; i < 7; ++i) { sp.m_out[7 * j + i] = st_new[7 + i]; sp.v_out[7 * j + i] = st_new[14 + i]; }
#pragma unroll
      for (int i = 0; i < 12; ++i) a.Rt[12 * j + i] = Rt[i];
      bool stops = false;  // (a scene that freezes with this step has no traj row for it: the fixed loop of as many steps has none)
      if constexpr (OBS) stops = icc_obs_advance(ob, a.S, e2.z, loss, sp.it, j == e2.x);
      if (sp.traj && !stops) {
        float *tr = sp.traj + ((int64_t)sp.it * a.O + j) * 7;
#pragma unroll
        for (int i = 0; i < 7; ++i) tr[i] = st_new[i];
      }
      if (sp.loss_out && j == e2.x) sp.loss_out[e2.z] = loss;
    }
    if (e2.w != 0) icc_bin_empties(a, sp, j, nb);  // ... and empties
  }
  const float R0 = r0.x, R1 = r0.y, R2 = r0.z, R3 = r0.w, R4 = r1.x, R5 = r1.y, R6 = r1.z,
              R7 = r1.w, R8 = r2.x, T0 = r2.y, T1 = r2.z, T2 = r2.w;
  const int h = min(ksize_of(a.thr, pitch) / 2, hmax);
  const float fh = (float)h, inv_pitch = 1.0f / pitch;
  {
    // whole-object rejection with the model's bounding sphere (conservative, block-uniform)
    const float glo = -fh - 0.51f, ghi = (float)(D - 1) + fh + 0.51f;
    const float cx = (((R0 * bnd.x + R1 * bnd.y) + R2 * bnd.z) + T0 - ox) * inv_pitch;
    const float cy = (((R3 * bnd.x + R4 * bnd.y) + R5 * bnd.z) + T1 - oy) * inv_pitch;
    const float cz = (((R6 * bnd.x + R7 * bnd.y) + R8 * bnd.z) + T2 - oz) * inv_pitch;
    const float r = bnd.w * inv_pitch + 0.05f + 1e-4f * (fabsf(cx) + fabsf(cy) + fabsf(cz));
    const bool hit = bnd.w >= 0.0f && !(cx + r < glo || cx - r > ghi || cy + r < glo ||
                                         cy - r > ghi || cz + r < glo || cz - r > ghi);
    if (!hit) return;
  }
  __syncthreads();
  // A survivor goes to the bin of its rounded x-plane, in the y-half (or both halves) its
  // ks rows touch: the tile of a half then finds exactly its own records, dense.
  float fx[kBinPPT], fy[kBinPPT], fz[kBinPPT];
  int bin[kBinPPT][kHalves], slot[kBinPPT][kHalves];
  const int Dh = (D + 1) / 2;
#pragma unroll
  for (int u = 0; u < kBinPPT; ++u) {
    const int p = e.z + u * kBinThreads + (int)threadIdx.x;
#pragma unroll
    for (int hf = 0; hf < kHalves; ++hf) { bin[u][hf] = -1; slot[u][hf] = 0; }
    if (p < e.w) {
      // transform_points: ((R0 x + R1 y) + R2 z) + t, un-fused (oracle order), then
      // (p - origin) / pitch with a correctly rounded divide (voxelization_3d index rule)
      const float wx = ((R0 * m[u].x + R1 * m[u].y) + R2 * m[u].z) + T0;
      const float wy = ((R3 * m[u].x + R4 * m[u].y) + R5 * m[u].z) + T1;
      const float wz = ((R6 * m[u].x + R7 * m[u].y) + R8 * m[u].z) + T2;
      fx[u] = (wx - ox) / pitch; fy[u] = (wy - oy) / pitch; fz[u] = (wz - oz) / pitch;
      const float rx = roundf(fx[u]), ry = roundf(fy[u]), rz = roundf(fz[u]);
      const bool surv = rx + fh >= 0.0f && rx - fh < (float)D && ry + fh >= 0.0f &&
                        ry - fh < (float)D && rz + fh >= 0.0f && rz - fh < (float)D;
      if (surv) {
        const int plane = (int)rx + hmax;  // in [0, D + 2 hmax)
        const int iry = (int)ry;
        if (iry - h < Dh) {
          bin[u][0] = plane * kHalves;
          slot[u][0] = atomicAdd(&s_cnt[bin[u][0]], 1);
        }
        if (iry + h >= Dh) {
          bin[u][1] = plane * kHalves + 1;
          slot[u][1] = atomicAdd(&s_cnt[bin[u][1]], 1);
        }
      }
    }
  }
  __syncthreads();
  stamp(1);
  for (int i = threadIdx.x; i < nbr; i += kBinThreads) {
    const int c = s_cnt[i];
    s_base[i] = c > 0 ? (int)atomicAdd(&a.bin_cnt[((int64_t)sp.cpar * 2 * a.O + g) * nb + i], (uint32_t)c) : 0;
  }
  __syncthreads();
  stamp(2);
#pragma unroll
  for (int u = 0; u < kBinPPT; ++u) {
    const int p = e.z + u * kBinThreads + (int)threadIdx.x;
#pragma unroll
    for (int hf = 0; hf < kHalves; ++hf) {
      if (bin[u][hf] < 0) continue;
      const int idx = s_base[bin[u][hf]] + slot[u][hf];
      const float4 r = make_float4(fx[u], fy[u], fz[u], __uint_as_float((uint32_t)p));
      if (idx < cap) {
        a.rec[base_g + (int64_t)bin[u][hf] * cap + idx] = r;
      } else {  // bin full: the grid's overflow list (its tiles find the record by the membership test)
        const uint32_t k = atomicAdd(&a.bin_cnt[((int64_t)sp.cpar * 2 * a.O + g) * nb + nbr], 1u);
        if ((int)k < ovf_cap) a.rec[base_g + (int64_t)nbr * cap + k] = r;  // (k < 2 P_g always: a point adds <= 2 records)
      }
    }
  }
  stamp(3);
}

}  // namespace
