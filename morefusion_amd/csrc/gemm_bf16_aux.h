// Operand preparation of the bf16 GEMMs: cast, pack and ReLU-mask kernels, and the split-K finish passes.
// A piece of csrc/gemm_bf16.hip's single translation unit: included there, in the order of that file, nowhere else.
#pragma once
#include "mf_common.h"

namespace {

// ---- operand preparation ---------------------------------------------------------------------------------
// fp32 [rows][src_ld] -> bf16 [rows][dst_ld] (zero columns beyond ``cols``), 8 elements per lane
__global__ __launch_bounds__(256) void k_cast_rows_bf16(const float *__restrict__ src, int64_t src_ld,
                                                        uint16_t *__restrict__ dst, int64_t dst_ld, int64_t rows,
                                                        int cols) {
  const int per_row = (int)(dst_ld / 8);
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= rows * per_row) return;
  const int64_t r = i / per_row;
  const int c0 = (int)(i - r * per_row) * 8;
  float v[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) v[j] = c0 + j < cols ? src[r * src_ld + c0 + j] : 0.0f;
  *reinterpret_cast<uint4 *>(dst + r * dst_ld + c0) =
      make_uint4(mf::pack_bf16x2(v[0], v[1]), mf::pack_bf16x2(v[2], v[3]), mf::pack_bf16x2(v[4], v[5]),
                 mf::pack_bf16x2(v[6], v[7]));
}

// W [Cout][w_cin][ks][ks][ks] fp32 (input channels c_off .. c_off + Cin; channels past w_cin read as zero) ->
//   fwd   [Cout][tap][Cin]            (k = tap * Cin + cin)                                  taps = ks^3
//   dgrad [class p][Cin][slot][Cout]  (k4 / s2 / p1 only: k = slot * Cout + cout; tap = (1 - p) + 2 s per axis)
//   flipT [Cin][tap][Cout]            the forward operand of the DATA-GRADIENT convolution of a stride-1 layer:
//                                     dx = conv(dy, flipT), flipT[ci][tap][co] = W[co][ci][ks^3 - 1 - tap]
// Tiled transposes through LDS (round 4's first, element-wise pack read 4-byte values ``taps`` floats apart: 0.1 ms
// for conv4's 8.4 M weights, every training step):
//   k_conv_pack_fwd_tile   workgroup (ci block, co): W[co][c_off + ci ..][taps] -> fwd[co][tap][ci ..]
//   k_conv_pack_cof_tile   workgroup (co block, ci): W[co ..][c_off + ci][taps] -> flipT[ci][tap][co ..] and / or
//                          dgrad[p][ci][slot][co ..]   (the layouts with the OUTPUT channel fastest)
__global__ __launch_bounds__(256) void k_conv_pack_fwd_tile(const float *__restrict__ W, int Cin, int w_cin, int c_off,
                                                            int taps, uint16_t *__restrict__ fwd) {
  __shared__ float s_t[kPackTile][kPackTile + 1];
  const int ci0 = blockIdx.x * kPackTile, co = blockIdx.y;
  const int nci = min(kPackTile, Cin - ci0), live = max(0, min(nci, w_cin - c_off - ci0));
  const float *src = W + ((int64_t)co * w_cin + c_off + ci0) * taps;  // [ci][tap], contiguous
  for (int i = threadIdx.x; i < nci * taps; i += 256) {
    const int cl = i / taps, tap = i - cl * taps;
    s_t[cl][tap] = cl < live ? src[i] : 0.0f;
  }
  __syncthreads();
  uint16_t *dst = fwd + (int64_t)co * taps * Cin + ci0;
  for (int i = threadIdx.x; i < taps * kPackTile; i += 256) {
    const int tap = i >> 6, cl = i & 63;
    if (cl < nci) dst[(int64_t)tap * Cin + cl] = (uint16_t)mf::bf16_bits(s_t[cl][tap]);
  }
}

__global__ __launch_bounds__(256) void k_conv_pack_cof_tile(const float *__restrict__ W, int Cout, int Cin, int w_cin,
                                                            int c_off, int ks, uint16_t *__restrict__ dgrad,
                                                            uint16_t *__restrict__ flipT) {
  __shared__ float s_t[kPackTile][kPackTile + 1];
  const int taps = ks * ks * ks;
  const int co0 = blockIdx.x * kPackTile, ci = blockIdx.y;
  const int nco = min(kPackTile, Cout - co0);
  const bool live = c_off + ci < w_cin;
  for (int i = threadIdx.x; i < nco * taps; i += 256) {
    const int cl = i / taps, tap = i - cl * taps;
    s_t[cl][tap] = live ? W[((int64_t)(co0 + cl) * w_cin + c_off + ci) * taps + tap] : 0.0f;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < taps * kPackTile; i += 256) {
    const int t = i >> 6, cl = i & 63;
    if (cl >= nco) continue;
    if (flipT) flipT[((int64_t)ci * taps + t) * Cout + co0 + cl] = (uint16_t)mf::bf16_bits(s_t[cl][taps - 1 - t]);
    if (dgrad) {  // t = 8 p + slot (k4 / s2 / p1 only: 64 taps)
      const int p = t >> 3, slot = t & 7;
      const int kx = (1 - (p & 1)) + 2 * (slot & 1), ky = (1 - ((p >> 1) & 1)) + 2 * ((slot >> 1) & 1),
                kz = (1 - (p >> 2)) + 2 * (slot >> 2);
      dgrad[(((int64_t)p * Cin + ci) * 8 + slot) * Cout + co0 + cl] = (uint16_t)mf::bf16_bits(s_t[cl][kx * 16 + ky * 4 + kz]);
    }
  }
}

// dz = dy where y > 0 else 0 (the ReLU behind a fused GEMM epilogue), bf16 in / out, 8 elements per lane.
// ``dy32``: an fp32 gradient instead (the accumulated gradient of a sampled grid).
__global__ __launch_bounds__(256) void k_relu_mask_bf16(const uint16_t *__restrict__ y, const uint16_t *__restrict__ dy,
                                                        const float *__restrict__ dy32, uint16_t *__restrict__ dz,
                                                        int64_t n8) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n8) return;
  const uint4 yv = reinterpret_cast<const uint4 *>(y)[i];
  const uint32_t yw[4] = {yv.x, yv.y, yv.z, yv.w};
  uint32_t ow[4];
  if (dy32) {
    const float4 g0 = reinterpret_cast<const float4 *>(dy32)[2 * i], g1 = reinterpret_cast<const float4 *>(dy32)[2 * i + 1];
    const float g[8] = {g0.x, g0.y, g0.z, g0.w, g1.x, g1.y, g1.z, g1.w};
#pragma unroll
    for (int d = 0; d < 4; ++d)
      ow[d] = mf::pack_bf16x2(mf::bf16_lo(yw[d]) > 0.0f ? g[2 * d] : 0.0f, mf::bf16_hi(yw[d]) > 0.0f ? g[2 * d + 1] : 0.0f);
  } else {
    const uint4 gv = reinterpret_cast<const uint4 *>(dy)[i];
    const uint32_t gw[4] = {gv.x, gv.y, gv.z, gv.w};
#pragma unroll
    for (int d = 0; d < 4; ++d)
      ow[d] = (mf::bf16_lo(yw[d]) > 0.0f ? gw[d] & 0xffffu : 0u) | (mf::bf16_hi(yw[d]) > 0.0f ? gw[d] & 0xffff0000u : 0u);
  }
  reinterpret_cast<uint4 *>(dz)[i] = make_uint4(ow[0], ow[1], ow[2], ow[3]);
}

// out[m][n] = act(sum_s slab[s][m][n] + bias[n]) (increasing s: deterministic), bf16 or fp32 rows of pitch ldo: the
// second half of a split-K launch of k_gemm_nt_bf16_pp.  Eight columns per lane (N % 8 == 0).
__global__ __launch_bounds__(256) void k_splitk_finish(const float *__restrict__ slab, const float *__restrict__ bias,
                                                       void *__restrict__ out, int64_t M, int N, int S, int ldo,
                                                       int relu, int out_f32) {
  const int n8 = N >> 3;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= M * n8) return;
  const int64_t m = i / n8;
  const int n = (int)(i - m * n8) * 8;
  const float4 *src = reinterpret_cast<const float4 *>(slab + m * N + n);
  float4 a0 = src[0], a1 = src[1];
  for (int s = 1; s < S; ++s) {
    const float4 *p = reinterpret_cast<const float4 *>(slab + (int64_t)s * M * N + m * N + n);
    const float4 b0 = p[0], b1 = p[1];
    a0.x += b0.x; a0.y += b0.y; a0.z += b0.z; a0.w += b0.w;
    a1.x += b1.x; a1.y += b1.y; a1.z += b1.z; a1.w += b1.w;
  }
  float v[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    if (bias) v[j] += bias[n + j];
    if (relu) v[j] = v[j] > 0.0f ? v[j] : 0.0f;
  }
  if (out_f32) {
    float *o = reinterpret_cast<float *>(out) + m * ldo + n;
    if ((ldo & 3) == 0 && ((uintptr_t)o & 15) == 0) {
      reinterpret_cast<float4 *>(o)[0] = make_float4(v[0], v[1], v[2], v[3]);
      reinterpret_cast<float4 *>(o)[1] = make_float4(v[4], v[5], v[6], v[7]);
    } else {
      for (int j = 0; j < 8; ++j) o[j] = v[j];
    }
  } else {
    uint16_t *o = reinterpret_cast<uint16_t *>(out) + m * ldo + n;
    if ((ldo & 7) == 0 && ((uintptr_t)o & 15) == 0) {
      *reinterpret_cast<uint4 *>(o) = make_uint4(mf::pack_bf16x2(v[0], v[1]), mf::pack_bf16x2(v[2], v[3]),
                                                 mf::pack_bf16x2(v[4], v[5]), mf::pack_bf16x2(v[6], v[7]));
    } else {
      for (int j = 0; j < 8; ++j) o[j] = (uint16_t)mf::bf16_bits(v[j]);
    }
  }
}

// The same sum for a split-K launch of the 2-D split-bf16 convolution, through its epilogue (conv2_store8).
__global__ __launch_bounds__(256) void k_splitk_finish_conv2(NtArgs a) {
  const int n8 = a.N >> 3;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)a.M * n8) return;
  const int64_t m = i / n8;
  const int n = (int)(i - m * n8) * 8;
  const float4 *src = reinterpret_cast<const float4 *>(a.slab + m * a.N + n);
  float4 a0 = src[0], a1 = src[1];
  for (int s = 1; s < a.S; ++s) {
    const float4 *p = reinterpret_cast<const float4 *>(a.slab + (int64_t)s * a.M * a.N + m * a.N + n);
    const float4 b0 = p[0], b1 = p[1];
    a0.x += b0.x; a0.y += b0.y; a0.z += b0.z; a0.w += b0.w;
    a1.x += b1.x; a1.y += b1.y; a1.z += b1.z; a1.w += b1.w;
  }
  float v[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
  conv2_store8(a, m, n, v);
}

// W [Cout][w_cin][taps] fp32 (framework layout: [ks][ks] or [ks][ks][ks] taps), input channels c_off .. c_off + Cin - 1
// -> wp bf16 [Cout][tap][3 Cin] = [w_hi | w_hi | w_lo] per tap, the operand of the split-bf16 convolutions
// (w_hi = bf16(w), w_lo = bf16(w - w_hi)).
__global__ __launch_bounds__(256) void k_conv2_pack_split(const float *__restrict__ W, int Cout, int Cin, int w_cin,
                                                          int c_off, int taps, uint16_t *__restrict__ wp) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int K3 = 3 * Cin;
  if (i >= (int64_t)Cout * taps * K3) return;
  const int j = (int)(i % K3);
  const int64_t r = i / K3;
  const int tap = (int)(r % taps), n = (int)(r / taps);
  const int seg = j / Cin, c = j - seg * Cin;
  const float w = W[((int64_t)n * w_cin + c_off + c) * taps + tap];
  const uint32_t hb = mf::bf16_bits(w);
  wp[i] = (uint16_t)(seg < 2 ? hb : mf::bf16_bits(w - mf::bf16_lo(hb)));
}

// W [G][N][K] fp32 (row pitch ldw, group stride w_gs) -> wp bf16 [G][Np][3 Kp] = [w_hi | w_hi | w_lo] per row, zero
// rows N .. Np - 1 and zero columns K .. Kp - 1 of every segment: the operand of mf_linear_split_fwd.
__global__ __launch_bounds__(256) void k_rows_pack_split(const float *__restrict__ W, int64_t w_gs, int ldw, int N, int K,
                                                         int Np, int Kp, int G, uint16_t *__restrict__ wp) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int K3 = 3 * Kp;
  if (i >= (int64_t)G * Np * K3) return;
  const int j = (int)(i % K3);
  const int64_t r = i / K3;
  const int n = (int)(r % Np), g = (int)(r / Np);
  const int seg = j / Kp, k = j - seg * Kp;
  const float w = n < N && k < K ? W[g * w_gs + (int64_t)n * ldw + k] : 0.0f;
  const uint32_t hb = mf::bf16_bits(w);
  wp[i] = (uint16_t)(seg < 2 ? hb : mf::bf16_bits(w - mf::bf16_lo(hb)));
}

}  // namespace
