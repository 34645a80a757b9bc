// The 3 x 3 x 3 convolution between narrow layers (k_conv_k3_narrow_bf16) and its weight pack.
// A piece of csrc/gemm_bf16.hip's single translation unit: included there, in the order of that file, nowhere else.
#pragma once
#include "mf_common.h"

namespace {

// ---- 3 x 3 x 3 convolutions between NARROW layers (round 6): the occupancy branch ----------------------------------
// conv1_occ (1 -> 8, fed as 8 channels), conv2_occ (8 -> 16, dilation 2) and conv2_occ's data gradient (16 -> 8)
// (model.py:69-72,120-124) went through k_gemm_nt_bf16<conv forward>: 8 or 16 valid columns of a 128-column tile,
// 92-99 us each at 16 objects for 8-16 MB of operands.  Here the convolution is out^T = W (x) im2col with the VOXELS as
// the MFMA's columns: a wave owns 32 voxels, its B operand of k-step s is one 16-byte global load per lane -- the 8
// channels [c0, c0 + 8) of tap (16 s + 8 (lane / 32)) / CI of the voxel lane % 32, a masked (out-of-range) buffer load
// for padding taps -- with no LDS stage at all (neighbouring voxels re-read the same 16 bytes from L1 / L2); the A
// operand, the weights [n][k = tap * CI + ci] of <= 32 output channels, stays in registers for all the tiles a wave
// walks (KS x 16 bytes per lane).  The accumulator's rows are channels: lane (voxel v, half h) ends up with channels
// {0..3, 8..11} + 4 h of its voxel -> two 8-byte stores.
template <int CI, int KS>  // KS = ceil(27 CI / 16) k-steps
__global__ __launch_bounds__(256) void k_conv_k3_narrow_bf16(const uint16_t *__restrict__ x, const uint16_t *__restrict__ wp,
                                                            const float *__restrict__ bias, uint16_t *__restrict__ out,
                                                            int B, int D, int dlog, int CO, int dil, int relu,
                                                            int tiles_per_wave) {
  const int lane = threadIdx.x & 63, wave_g = (int)(((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6);
  const int n = lane & 31, h = lane >> 5;
  // the weights: row n of wp [32][KS * 16] (rows >= CO are zero), k = 16 s + 8 h .. + 7
  uint4 wf[KS];
#pragma unroll
  for (int s = 0; s < KS; ++s) wf[s] = *reinterpret_cast<const uint4 *>(wp + (size_t)n * (KS * 16) + 16 * s + 8 * h);
  float bn[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int row = (e & 3) + 8 * (e >> 2) + 4 * h;
    bn[e] = bias && row < CO ? bias[row] : 0.0f;
  }
  const mf::BufRsrc xrs = mf::make_rsrc(x);
  const int64_t total = (int64_t)B << (3 * dlog);
  for (int it = 0; it < tiles_per_wave; ++it) {
    const int64_t v = ((int64_t)wave_g * tiles_per_wave + it) * 32 + n;  // this lane's voxel (columns of the MFMA)
    if (v - n >= total) break;  // wave-uniform
    const bool vok = v < total;
    const int iz = (int)(v & (D - 1)), iy = (int)((v >> dlog) & (D - 1)), ix = (int)((v >> (2 * dlog)) & (D - 1));
    const int64_t vb = v - (((int64_t)ix << (2 * dlog)) + ((int64_t)iy << dlog) + iz);  // b * D^3
    mf_f32x16 acc;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.0f;
    uint4 xf[KS];
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      const int k0 = 16 * s + 8 * h;
      const int tap = k0 / CI, c0 = k0 - tap * CI;  // (CI = 8: tap = 2 s + h; CI = 16: tap = s, c0 = 8 h)
      const int kx = tap / 9, ky = (tap - 9 * kx) / 3, kz = tap - 9 * kx - 3 * ky;
      const int jx = ix + (kx - 1) * dil, jy = iy + (ky - 1) * dil, jz = iz + (kz - 1) * dil;
      const bool ok = vok && tap < 27 && (unsigned)jx < (unsigned)D && (unsigned)jy < (unsigned)D && (unsigned)jz < (unsigned)D;
      const int64_t src = (vb + (((int64_t)jx << (2 * dlog)) + ((int64_t)jy << dlog) + jz)) * CI + c0;
      xf[s] = mf::buf_load16(xrs, ok ? 2u * (uint32_t)src : mf::kBufMasked);
    }
#pragma unroll
    for (int s = 0; s < KS; ++s) acc = mf::mfma_bf16_32x32x16(wf[s], xf[s], acc);
    if (!vok) continue;
    // rows of the accumulator = output channels (e & 3) + 8 (e >> 2) + 4 h; columns = this lane's voxel
#pragma unroll
    for (int g = 0; g < 2; ++g) {
      if (8 * g + 4 * h >= CO) continue;
      float o4[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float val = acc[4 * g + j] + bn[4 * g + j];
        if (relu) val = val > 0.0f ? val : 0.0f;
        o4[j] = val;
      }
      *reinterpret_cast<uint2 *>(out + v * CO + 8 * g + 4 * h) = make_uint2(mf::pack_bf16x2(o4[0], o4[1]), mf::pack_bf16x2(o4[2], o4[3]));
    }
  }
}

// W [Cout][w_cin][3][3][3] fp32 (framework layout) -> wp bf16 [32 rows][KS * 16]:
//   forward        row n = output channel, k = tap * CI + ci:   W[n][c_off + ci][tap]          (CI = the layer's Cin)
//   data gradient  row n = INPUT channel of the layer, k = tap * CI + co:  W[co][c_off + n][26 - tap]   (CI = Cout)
// rows >= the valid count, k beyond 27 CI and channels at or beyond w_cin are zero.
__global__ __launch_bounds__(256) void k_conv_k3_narrow_pack(const float *__restrict__ W, int Cout, int Cin, int w_cin,
                                                            int c_off, int transpose, int CI, int Kp,
                                                            uint16_t *__restrict__ wp) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= 32 * Kp) return;
  const int nrow = i / Kp, k = i - nrow * Kp;
  const int tap = k / CI, c = k - tap * CI;
  float v = 0.0f;
  if (tap < 27) {
    if (!transpose) {
      if (nrow < Cout && c < Cin && c_off + c < w_cin) v = W[((int64_t)nrow * w_cin + c_off + c) * 27 + tap];
    } else {
      if (nrow < Cin && c < Cout && c_off + nrow < w_cin) v = W[((int64_t)c * w_cin + c_off + nrow) * 27 + (26 - tap)];
    }
  }
  wp[i] = (uint16_t)mf::bf16_bits(v);
}

}  // namespace
