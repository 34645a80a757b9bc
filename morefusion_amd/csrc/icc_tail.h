// The two ICC kernels the host launches outside an iteration: the optimiser step as a kernel of its own and the
// (points, sdf) -> float4 pack.  Last in the translation unit, where they always were: the device code of the
// library keeps its order.
// A piece of csrc/icc.hip's single translation unit: included there, in the order of that file, nowhere else.
#pragma once
#include "icc_common.h"
#include "icc_step.h"

namespace {

// ---- the step as a kernel of its own: one 64-lane workgroup per object ----------------
// mode 1: after the last iteration of mf_icc_refine.  mode 2: mf_icc_loss_grad (loss, gq, gt).
// OBS: the last step of mf_icc_refine_converge -- observer as in k_icc_bin<true>, and the scene's step count goes out.
template <bool OBS>
__global__ __launch_bounds__(64) void k_icc_step(IccArgs a, IccStepArgs sp, typename IccObsOf<OBS>::type ob) {
  __shared__ float s_sum[kStepSums], s_state[kStateFloats];
  __shared__ long long s_raw[kStepRawWords];
  const int j = blockIdx.x;
  const int4 meta = a.meta[j];
  const int ja = meta.x, Ns = meta.y - meta.x;
  const int sc = a.obj_scene[j];
  if (threadIdx.x < kStateFloats) {
    const int i = threadIdx.x;
    s_state[i] = i < 4 ? sp.q_in[4 * j + i] : i < 7 ? sp.t_in[3 * j + i - 4]
                 : (sp.mode == 1 ? (i < 14 ? sp.m_in[7 * j + i - 7] : sp.v_in[7 * j + i - 14]) : 0.0f);
  }
  const float S_t = a.St[sc];
  if constexpr (OBS) {
    const IccObsRec *rec = ob.rec + (int64_t)ob.in * a.S + sc;
    if (rec->frozen != 0) {  // block-uniform: the state passes through (see k_icc_bin), a.Rt stays
      __syncthreads();
      if (threadIdx.x < kStateFloats) {
        const int i = threadIdx.x;
        const float x = s_state[i];
        if (i < 4) sp.q_out[4 * j + i] = x;
        else if (i < 7) sp.t_out[3 * j + i - 4] = x;
        else if (i < 14) sp.m_out[7 * j + i - 7] = x;
        else sp.v_out[7 * j + i - 14] = x;
      }
      if (threadIdx.x == 0 && j == ja) {
        icc_obs_keep(ob, a.S, sc);
        ob.n_steps[sc] = rec->n_steps;
      }
      return;
    }
  }
  if (sp.fused)
    icc_step_gather_fused<64>(a, sp.par, j, ja, Ns, s_raw, s_sum);
  else
    icc_step_gather<64>(a, sp.par, j, ja, Ns, s_raw, s_sum);
  if (threadIdx.x >= 16) return;
  __shared__ float s_x[kStepLaneWords];
  float Rt[12], loss, gq[4], gt[3];
  icc_step_lanes(s_sum, S_t, s_state, sp, (int)threadIdx.x, s_x, Rt, loss, gq, gt);
  __builtin_amdgcn_wave_barrier();
  if (threadIdx.x != 0) return;
  const float *st_new = s_x + 12;
  if (sp.loss_out && j == ja) sp.loss_out[sc] = loss;
  if constexpr (OBS) {
    if (j == ja) {
      icc_obs_advance(ob, a.S, sc, loss, sp.it, true);
      ob.n_steps[sc] = sp.it;
    }
  }
  if (sp.mode == 1) {
#pragma unroll
    for (int i = 0; i < 4; ++i) sp.q_out[4 * j + i] = st_new[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) sp.t_out[3 * j + i] = st_new[4 + i];
#pragma unroll
    for (int i = 0; i < 7; ++i) { sp.m_out[7 * j + i] = st_new[7 + i]; sp.v_out[7 * j + i] = st_new[14 + i]; }
#pragma unroll
    for (int i = 0; i < 12; ++i) a.Rt[(int64_t)j * 12 + i] = Rt[i];
    if (sp.traj) {
      float *tr = sp.traj + ((int64_t)sp.it * a.O + j) * 7;
#pragma unroll
      for (int i = 0; i < 7; ++i) tr[i] = st_new[i];
    }
  } else if (sp.gq_out) {
#pragma unroll
    for (int i = 0; i < 4; ++i) sp.gq_out[4 * j + i] = gq[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) sp.gt_out[3 * j + i] = gt[i];
  }
}

__global__ void k_pack(const float *__restrict__ points, const float *__restrict__ sdf, int64_t n,
                       float4 *__restrict__ out) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = make_float4(points[3 * i], points[3 * i + 1], points[3 * i + 2], sdf[i]);
}

}  // namespace
