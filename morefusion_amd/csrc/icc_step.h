// The optimiser step of ICC: gathering the reduced sums of an iteration (two-kernel and single-pass form), the
// step on 16 lanes -- device functions of k_icc_bin (icc_bin.h) and of k_icc_step (icc_tail.h).
// A piece of csrc/icc.hip's single translation unit: included there, in the order of that file, nowhere else.
#pragma once
#include "icc_common.h"

namespace {

// ---- the optimiser step of ONE object from the reduced sums of an iteration ------------
// (iterative_collision_check_link.py:91-98 loss; chain rule through transformation_matrix /
// quaternion_matrix.py:36-78; chainer.optimizers.Adam v7 in float32).  A pure function of global
// memory: every workgroup that needs object j's next pose evaluates it and gets the same bits.
// `sv` = 52 sums gathered by the caller (LDS or registers): [0..2] RN, S_in, PN of the scene,
// [3..38] the 3 x 12 own-gradient moments of j, [39..50] collision moments onto j, [51] != 0 if
// any block sum of the scene was not finite.
constexpr int kStepSums = 52;

// The calling workgroup (NT lanes) gathers the kStepSums sums of object j into s_sum.  Every
// accumulator word is fetched by its own lane -- ONE memory round trip (a lane walking the
// scene's objects serially costs a dependent load per object: measured 9 us at 8 objects) --
// staged in LDS, then summed in object order.  s_raw: >= (16 * max_ns + kNumOwn) 64-bit words.
// Contains two barriers: call it from uniform control flow.
constexpr int kStepRawWords = 20 * 64 + 60;  // 64-bit words: the single-pass path stages 20 Ns + 60 FLOATS in them
static_assert(20 * kMaxSceneObjects + 60 <= 2 * kStepRawWords, "staged floats of the single-pass step");
static_assert(16 * kMaxSceneObjectsGeneral + 36 <= kStepRawWords, "staged words of the two-kernel path's step");

template <int NT>
__device__ __forceinline__ void icc_step_gather(const IccArgs &a, int par, int j, int ja, int Ns,
                                                long long *s_raw, float *s_sum) {
  const long long *own = a.acc_own + (int64_t)par * a.O * kOwnSlots;
  const long long *oth = a.acc_oth + (int64_t)par * a.O * a.max_ns * 12;
  // items: [0, 4 Ns): own slots {RN, S_in, PN, non-finite count} of every scene object;
  // [4 Ns, 16 Ns): the 12 collision moments onto j from every scene object's grid;
  // [16 Ns, 16 Ns + 36): the own-gradient moments of j
  const int n_items = 16 * Ns + (kNumOwn - 3);
  for (int i = threadIdx.x; i < n_items; i += NT) {
    long long x;
    if (i < 4 * Ns) {
      const int jo = i >> 2, l = i & 3;
      x = own[(int64_t)(ja + jo) * kOwnSlots + (l < 3 ? l : kNumOwn)];
    } else if (i < 16 * Ns) {
      const int k = i - 4 * Ns, jo = k / 12, c = k - 12 * jo;
      x = oth[((int64_t)(ja + jo) * a.max_ns + (j - ja)) * 12 + c];
    } else {
      x = own[(int64_t)j * kOwnSlots + 3 + (i - 16 * Ns)];
    }
    s_raw[i] = x;
  }
  __syncthreads();
  if (threadIdx.x < kStepSums) {
    const int l = threadIdx.x;
    float r;
    if (l < 3) {  // scene sums, objects in order
      r = 0.0f;
      for (int jo = 0; jo < Ns; ++jo) r += (float)((double)s_raw[4 * jo + l] * (1.0 / kFixOwn));
    } else if (l < kNumOwn) {
      r = (float)((double)s_raw[16 * Ns + (l - 3)] * (1.0 / kFixOwn));
    } else if (l < kNumOwn + 12) {  // exact integer sum over the scene's grids
      long long x = 0;
      for (int jo = 0; jo < Ns; ++jo) x += s_raw[4 * Ns + 12 * jo + (l - kNumOwn)];
      r = (float)((double)x * (1.0 / kFixOth));
    } else {
      long long bad = 0;
      for (int jo = 0; jo < Ns; ++jo) bad |= s_raw[4 * jo + 3];
      r = bad != 0 ? 1.0f : 0.0f;
    }
    s_sum[l] = r;
  }
  __syncthreads();
}

// The same for the single-pass path (k_icc_fused): the accumulators hold the monomial sums, the
// per-grid maxima M_own / M_oth give a = 1/M_own, b = 1/M_oth (b = 0 where the "other" grid is
// empty or absent: iterative_collision_check_link.py:62-63,82), and the lanes form the sums the
// step expects (see the table above k_icc_fused).  Staged words, all converted to float by the lane that
// fetched them (fixed point -> float, M -> 1/M: the conversions and the IEEE reciprocals run in parallel):
//   sA[8 jo + l]   per scene object jo: {5 scene sums, non-finite flag, a = 1/M_own, b = 1/M_oth}
//   sB[12 jo + c]  the 12 collision moments onto object j from the grid of scene object jo
//   sC[i]          the 5 x 12 own-gradient moments of j
__device__ __forceinline__ float fused_item_scene(const long long *own, const uint32_t *Mb, int obj, int l, int Ns) {
  if (l < 5) return (float)((double)own[(int64_t)obj * kOwnSlots + l] * (1.0 / kFixOwn));
  if (l == 5) return own[(int64_t)obj * kOwnSlots + kNumF] != 0 ? 1.0f : 0.0f;
  const float M = __uint_as_float(Mb[2 * obj + (l - 6)]);  // a = 1/M_own, b = 1/M_oth (b = 0 where the "other" grid is empty)
  return l == 6 ? 1.0f / M : ((Ns > 1 && M != 0.0f) ? 1.0f / M : 0.0f);
}
__device__ __forceinline__ float fused_item_oth(const long long *oth, int grid_obj, int max_ns, int jj, int c) {
  return (float)((double)oth[((int64_t)grid_obj * max_ns + jj) * 12 + c] * (1.0 / kFixOth));
}
__device__ __forceinline__ float fused_item_own(const long long *own, int obj, int i) {
  return (float)((double)own[(int64_t)obj * kOwnSlots + 5 + i] * (1.0 / kFixOwn));
}
// sum l (< kStepSums) of scene-local object jj from the staged words
__device__ __forceinline__ float fused_sum(const int l, const int Ns, const int jj, const float *sA, const float *sB,
                                           const float *sC) {
  auto a_of = [&](int jo) { return sA[8 * jo + 6]; };
  auto b_of = [&](int jo) { return sA[8 * jo + 7]; };
  float r = 0.0f;
  if (l == 0) {  // RN
#pragma unroll 8
    for (int jo = 0; jo < Ns; ++jo) r += sA[8 * jo + 0] - a_of(jo) * sA[8 * jo + 1];
  } else if (l == 1) {  // S_in
#pragma unroll 8
    for (int jo = 0; jo < Ns; ++jo) r += a_of(jo) * sA[8 * jo + 2];
  } else if (l == 2) {  // PN
#pragma unroll 8
    for (int jo = 0; jo < Ns; ++jo) r += a_of(jo) * (sA[8 * jo + 3] + b_of(jo) * sA[8 * jo + 4]);
  } else if (l < 15) {  // reward moments
    const int c = l - 3;
    r = sC[c] - a_of(jj) * sC[12 + c];
  } else if (l < 27) {  // penalty numerator moments
    const int c = l - 15;
    r = a_of(jj) * (sC[24 + c] + b_of(jj) * sC[36 + c]);
  } else if (l < 39) {  // penalty denominator moments
    r = a_of(jj) * sC[48 + (l - 27)];
  } else if (l < 51) {  // collision moments of every grid of the scene onto j
#pragma unroll 8
    for (int jo = 0; jo < Ns; ++jo) r += (a_of(jo) * b_of(jo)) * sB[12 * jo + (l - 39)];
  } else {
#pragma unroll 8
    for (int jo = 0; jo < Ns; ++jo) r = sA[8 * jo + 5] != 0.0f ? 1.0f : r;
  }
  return r;
}

template <int NT>
__device__ __forceinline__ void icc_step_gather_fused(const IccArgs &a, int par, int j, int ja, int Ns,
                                                      long long *s_raw, float *s_sum) {
  const long long *own = a.acc_own + (int64_t)par * a.O * kOwnSlots;
  const long long *oth = a.acc_oth + (int64_t)par * a.O * a.max_ns * 12;
  const uint32_t *Mb = a.Mbits + (int64_t)par * 2 * a.O;
  // items: [0, 8 Ns) sA; [8 Ns, 20 Ns) sB; [20 Ns, 20 Ns + 60) sC
  const int n_items = 20 * Ns + 60;
  float *s_f = reinterpret_cast<float *>(s_raw);
  for (int i0 = 0; i0 < n_items; i0 += NT) {
    const int i = i0 + (int)threadIdx.x;
    float fv = 0.0f;
    if (i < n_items) {
      if (i < 8 * Ns) {
        fv = fused_item_scene(own, Mb, ja + (i >> 3), i & 7, Ns);
      } else if (i < 20 * Ns) {
        const int k = i - 8 * Ns, jo = k / 12, c = k - 12 * jo;
        fv = fused_item_oth(oth, ja + jo, a.max_ns, j - ja, c);
      } else {
        fv = fused_item_own(own, j, i - 20 * Ns);
      }
    }
    if (i < n_items) s_f[i] = fv;
  }
  __syncthreads();
  if constexpr (NT >= 256) {
    // the three scene sums are loops over the scene's objects: one wave each, the other 49 sums on a fourth (as 52
    // lanes of one wave the loops ran one after the other)
    const int w = threadIdx.x >> 6, ln = threadIdx.x & 63;
    const int l = w < 3 ? (ln == 0 ? w : -1) : (w == 3 && ln < kStepSums - 3 ? 3 + ln : -1);
    if (l >= 0) s_sum[l] = fused_sum(l, Ns, j - ja, s_f, s_f + 8 * Ns, s_f + 20 * Ns);
  } else {
    if (threadIdx.x < kStepSums) s_sum[threadIdx.x] = fused_sum((int)threadIdx.x, Ns, j - ja, s_f, s_f + 8 * Ns, s_f + 20 * Ns);
  }
  __syncthreads();
}

// The optimiser step of one object spread over the 16 lanes `c` of a lane group (sv: the gathered sums; st: (q, t,
// m, v) before the step): the twelve gradient components, the seven Adam updates (chainer.optimizers.Adam v7 rule in
// float32) and the rotation are evaluated by different lanes -- a third of the dependent instruction chain of one
// lane doing all of it (that chain was 1.5 us of every iteration; the one-lane form is gone, the bits are its).
// xg: kStepLaneWords floats of LDS scratch owned by the group; the state after the step is left
// in xg[12 ..] (q, t, m, v); every lane returns R|t and the loss, and the gradients in (gq, gt).
// Call from wave-uniform control flow (contains wave-level LDS hand-overs).
constexpr int kStepLaneWords = 12 + kStateFloats;
__device__ __forceinline__ void icc_step_lanes(const float *sv, float S_t, const float *st, const IccStepArgs &sp,
                                               const int c, float *xg, float *Rt_out, float &loss, float *gq,
                                               float *gt) {
  const float RN = sv[0], S_in = sv[1], PN = sv[2];
  const float reward = RN / S_t, penalty = PN / S_in;
  loss = sv[51] != 0.0f ? __builtin_nanf("") : penalty - reward;
  const float c0 = 1.0f / S_t, c1 = 1.0f / S_in, c2 = PN / (S_in * S_in);
  if (c < 12) xg[c] = ((c0 * sv[3 + c] - c1 * sv[15 + c]) + c2 * sv[27 + c]) - c1 * sv[39 + c];
  __builtin_amdgcn_wave_barrier();
  float gR[9];
#pragma unroll
  for (int d = 0; d < 3; ++d)
#pragma unroll
    for (int cc = 0; cc < 4; ++cc) {
      const float G = xg[4 * d + cc];
      if (cc < 3) gR[3 * d + cc] = G; else gt[d] = G;
    }
  float qq[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) qq[i] = st[i];
  quat_backward(qq, gR, gq);
  if (sv[51] != 0.0f) {
#pragma unroll
    for (int i = 0; i < 4; ++i) gq[i] = loss;
#pragma unroll
    for (int i = 0; i < 3; ++i) gt[i] = loss;
  }
  float *so = xg + 12;
  if (c < 7) {
    float th = st[c];
    if (sp.mode == 1) {
      // chainer.optimizers.Adam (v7) update rule in float32, parameter c
      const float omb1 = (float)(1.0 - 0.9), omb2 = (float)(1.0 - 0.999), eps = 1e-8f;
      const float gi = c == 0 ? gq[0] : c == 1 ? gq[1] : c == 2 ? gq[2] : c == 3 ? gq[3] : c == 4 ? gt[0] : c == 5 ? gt[1] : gt[2];
      float mm = st[7 + c], vv = st[14 + c];
      mm += omb1 * (gi - mm);
      vv += omb2 * (gi * gi - vv);
      so[7 + c] = mm;
      so[14 + c] = vv;
      const float upd = (c < 4 ? sp.aq : sp.at) * mm / (sqrtf(vv) + eps);
      th -= upd;
    }
    so[c] = th;
  }
  __builtin_amdgcn_wave_barrier();
  float qn[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) qn[i] = so[i];
  quat_to_R(qn, Rt_out);
#pragma unroll
  for (int i = 0; i < 3; ++i) Rt_out[9 + i] = so[4 + i];
}

// ---- the loss observer of a scene, advanced by the loss of the step just applied (mf_icc_refine_converge) --------
// The node's rule: from the second loss on |last - loss| (in double, of the two float32 losses) enters a window of the
// `window` most recent deltas; while the window is not empty a step passes when every delta in it is below max_delta,
// n_passed counts passes in a row, and the scene is frozen once n_passed >= n_pass.  A non-finite delta in the window
// fails the step (Python's max() over a list holding a NaN depends on the order; this rule does not).
// A pure function of the record launch k - 1 left and of the loss, which every workgroup of the scene computes with
// the same bits: every designated workgroup evaluates it (a scene that freezes with this step writes no traj row for
// it), the one of the scene's first object (`store`) writes the record of the other copy.  Returns the new flag.
__device__ __forceinline__ bool icc_obs_advance(const IccObsArgs &ob, int S, int sc, float loss, int steps, bool store) {
  const IccObsRec *in = ob.rec + (int64_t)ob.in * S + sc;
  IccObsRec *out = ob.rec + (int64_t)(ob.in ^ 1) * S + sc;
  int fill = in->fill, head = in->head, n_passed = in->n_passed;
  int put = -1;
  double delta = 0.0;
  if (in->has_last) {
    delta = fabs((double)in->last - (double)loss);
    put = head;
    head = head + 1 < ob.window ? head + 1 : 0;
    fill = min(fill + 1, ob.window);
  }
  bool pass = true;
  for (int i = 0; i < kObsMaxWindow; ++i) {
    const double d = i == put ? delta : in->delta[i];
    if (i < fill) pass = pass && fabs(d) <= 1.7976931348623157e308 && d < ob.max_delta;  // (finite, below)
    if (store) out->delta[i] = d;
  }
  if (fill > 0) n_passed = pass ? n_passed + 1 : 0;
  const bool frozen = n_passed >= ob.n_pass;
  if (store) {
    out->last = loss;
    out->has_last = 1;
    out->fill = fill;
    out->head = head;
    out->n_passed = n_passed;
    out->frozen = frozen ? 1 : 0;
    out->n_steps = steps;
    out->pad_ = 0;
  }
  return frozen;
}

// a frozen scene's record goes to the other copy as it is
__device__ __forceinline__ void icc_obs_keep(const IccObsArgs &ob, int S, int sc) {
  const IccObsRec *in = ob.rec + (int64_t)ob.in * S + sc;
  IccObsRec *out = ob.rec + (int64_t)(ob.in ^ 1) * S + sc;
  *out = *in;
}

}  // namespace
