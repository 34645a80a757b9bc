// Element-wise pieces of the 2-D backbone's decoder, forward and backward, for gfx950 (round 4).
//
// Reference: morefusion/models/dense_fusion/pspnet.py:10-35,40-73 -- PSPNet's decoder is three times
// `F.resize_images(x, 2x)` (bilinear, align_corners) -> Convolution2D 3x3 -> PReLU, and the pooling pyramid
// up-samples four pooled maps back to the feature size.  The convolutions stay MIOpen's; the bilinear resize and
// the single-parameter PReLU are memory-bound maps that the stock kernels run far below the HBM roofline:
// measured on the bf16 training step (profiles/r04_train_bf16_steady_step_kernel_stats.csv, 16 objects):
// upsample_bilinear2d_backward 2.8 ms for ~600 MB (0.2 TB/s: a float-atomic scatter), prelu_backward 1.3 ms for
// ~400 MB (0.3 TB/s: the gradient of the ONE slope is a whole-tensor reduction), the forward resize 0.7 ms.
//
// MI355X design: channels-LAST tensors ([B][H][W][C]: what MIOpen's NHWC convolutions on either side consume), a lane
// takes one pixel x 8 channels (bf16: one 16-byte access; fp32: two) -> every load and store is a full coalesced row
// segment.  The resize backward is a GATHER: an input pixel sums the <= ~4 x 4 output pixels whose bilinear footprint
// contains it, in increasing (oy, ox) -- no atomics, deterministic (torch's scatter is neither).  The PReLU
// backward writes dx and block-partial sums of dy * x over the negative side; a second launch adds the partials in
// block order.
#include "mf_common.h"

namespace {

// torch's area_pixel_compute_scale / source index for align_corners = true, in float
__device__ __forceinline__ float up_scale(int in, int out) { return out > 1 ? (float)(in - 1) / (float)(out - 1) : 0.0f; }

// Source taps of output pixel (oy, ox) of an align_corners resize [H][W] -> [Ho][Wo]: rows y0 / y0 + yp with weights
// h0 / h1, columns x0 / x0 + xp with weights w0 / w1 (torch's arithmetic, in float)
struct UpSrc { int y0, x0, yp, xp; float h0, h1, w0, w1; };
__device__ __forceinline__ UpSrc up_src(int oy, int ox, int H, int W, int Ho, int Wo) {
  UpSrc s;
  const float sy = up_scale(H, Ho) * (float)oy, sx = up_scale(W, Wo) * (float)ox;
  s.y0 = (int)sy; s.x0 = (int)sx;
  s.yp = s.y0 < H - 1 ? 1 : 0; s.xp = s.x0 < W - 1 ? 1 : 0;
  s.h1 = sy - (float)s.y0; s.h0 = 1.0f - s.h1; s.w1 = sx - (float)s.x0; s.w0 = 1.0f - s.w1;
  return s;
}

template <bool BF16>
__device__ __forceinline__ void load8(const void *p, int64_t idx, float v[8]) {
  if (BF16) {
    const uint4 w = *reinterpret_cast<const uint4 *>(reinterpret_cast<const uint16_t *>(p) + idx);
    const uint32_t d[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) { v[2 * i] = mf::bf16_lo(d[i]); v[2 * i + 1] = mf::bf16_hi(d[i]); }
  } else {
    const float4 a = *reinterpret_cast<const float4 *>(reinterpret_cast<const float *>(p) + idx);
    const float4 b = *reinterpret_cast<const float4 *>(reinterpret_cast<const float *>(p) + idx + 4);
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
  }
}

template <bool BF16>
__device__ __forceinline__ void store8(void *p, int64_t idx, const float v[8]) {
  if (BF16) {
    *reinterpret_cast<uint4 *>(reinterpret_cast<uint16_t *>(p) + idx) =
        make_uint4(mf::pack_bf16x2(v[0], v[1]), mf::pack_bf16x2(v[2], v[3]), mf::pack_bf16x2(v[4], v[5]),
                   mf::pack_bf16x2(v[6], v[7]));
  } else {
    *reinterpret_cast<float4 *>(reinterpret_cast<float *>(p) + idx) = make_float4(v[0], v[1], v[2], v[3]);
    *reinterpret_cast<float4 *>(reinterpret_cast<float *>(p) + idx + 4) = make_float4(v[4], v[5], v[6], v[7]);
  }
}

// y [B][Ho][Wo][C] = bilinear(x [B][H][W][C]), align_corners = true; the sum order of torch's kernel:
// h0 (w0 x00 + w1 x01) + h1 (w0 x10 + w1 x11)
template <bool BF16>
__global__ __launch_bounds__(256) void k_up_fwd(const void *__restrict__ x, void *__restrict__ y, int B, int H, int W,
                                                int Ho, int Wo, int C8) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t total = (int64_t)B * Ho * Wo * C8;
  if (i >= total) return;
  const int c8 = (int)(i % C8);
  const int64_t pix = i / C8;
  const int ox = (int)(pix % Wo), oy = (int)((pix / Wo) % Ho), b = (int)(pix / ((int64_t)Wo * Ho));
  const UpSrc s = up_src(oy, ox, H, W, Ho, Wo);
  const int yp = s.yp, xp = s.xp;
  const float h0 = s.h0, h1 = s.h1, w0 = s.w0, w1 = s.w1;
  const int C = 8 * C8;
  const int64_t base = (((int64_t)b * H + s.y0) * W + s.x0) * C + 8 * c8;
  float a00[8], a01[8], a10[8], a11[8], o[8];
  load8<BF16>(x, base, a00);
  load8<BF16>(x, base + (int64_t)xp * C, a01);
  load8<BF16>(x, base + (int64_t)yp * W * C, a10);
  load8<BF16>(x, base + ((int64_t)yp * W + xp) * C, a11);
#pragma unroll
  for (int k = 0; k < 8; ++k) o[k] = h0 * (w0 * a00[k] + w1 * a01[k]) + h1 * (w0 * a10[k] + w1 * a11[k]);
  store8<BF16>(y, pix * C + 8 * c8, o);
}

// hi / lo of eight fp32 values -> y[idx ..] and y[idx + los ..] (the split-bf16 form of csrc/gemm_bf16.hip
// mf_conv2d_split_fwd: hi = bf16(v), lo = bf16(v - hi), round to nearest even)
__device__ __forceinline__ void store8_split(uint16_t *y, int64_t idx, int64_t los, const float v[8]) {
  uint32_t h[8], l[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    h[k] = mf::bf16_bits(v[k]);
    l[k] = mf::bf16_bits(v[k] - mf::bf16_lo(h[k]));
  }
  *reinterpret_cast<uint4 *>(y + idx) = make_uint4(h[0] | h[1] << 16, h[2] | h[3] << 16, h[4] | h[5] << 16, h[6] | h[7] << 16);
  *reinterpret_cast<uint4 *>(y + idx + los) =
      make_uint4(l[0] | l[1] << 16, l[2] | l[3] << 16, l[4] | l[5] << 16, l[6] | l[7] << 16);
}

// k_up_fwd<false> with a split output: the resize of fp32 x [B][H][W][C] is taken in fp32 (same arithmetic), then
// split into y [B][Ho][Wo] rows of pitch ldy: hi at channel c, lo at channel los + c.
__global__ __launch_bounds__(256) void k_up_fwd_split(const float *__restrict__ x, uint16_t *__restrict__ y, int B, int H,
                                                      int W, int Ho, int Wo, int C8, int ldy, int los) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t total = (int64_t)B * Ho * Wo * C8;
  if (i >= total) return;
  const int c8 = (int)(i % C8);
  const int64_t pix = i / C8;
  const int ox = (int)(pix % Wo), oy = (int)((pix / Wo) % Ho), b = (int)(pix / ((int64_t)Wo * Ho));
  const UpSrc s = up_src(oy, ox, H, W, Ho, Wo);
  const int yp = s.yp, xp = s.xp;
  const float h0 = s.h0, h1 = s.h1, w0 = s.w0, w1 = s.w1;
  const int C = 8 * C8;
  const int64_t base = (((int64_t)b * H + s.y0) * W + s.x0) * C + 8 * c8;
  float a00[8], a01[8], a10[8], a11[8], o[8];
  load8<false>(x, base, a00);
  load8<false>(x, base + (int64_t)xp * C, a01);
  load8<false>(x, base + (int64_t)yp * W * C, a10);
  load8<false>(x, base + ((int64_t)yp * W + xp) * C, a11);
#pragma unroll
  for (int k = 0; k < 8; ++k) o[k] = h0 * (w0 * a00[k] + w1 * a01[k]) + h1 * (w0 * a10[k] + w1 * a11[k]);
  store8_split(y, pix * ldy + 8 * c8, los, o);
}

// The x2 resize + 3 x 3 convolution of PSPUpsample with the convolution taken first: z [B][H][W][9 C]
// fp32 holds the nine per-tap 1 x 1 convolutions z_t = W_t x of the LOW-resolution map (column t C + c, t = ky 3 + kx).
// Output pixel p = (oy, ox) of the [2H][2W] map, channel c:
//   v = act(bias[c] + sum over t = 0 .. 8 with q = p + (ky - 1, kx - 1) inside the map of bilinear(z_t)(q))
// -- a tap that leaves the up-sampled map is the convolution's zero padding.  The bilinear term is k_up_fwd's
// (same source arithmetic, same order of its four products), the taps are added in increasing t, all in fp32.  A lane
// takes one pixel x 8 channels; v goes to y32 (pitch ld32) and / or to the split rows ys (pitch lds, lo plane at los).
__global__ __launch_bounds__(256) void k_up_tapsum(const float *__restrict__ z, const float *__restrict__ bias,
                                                   const float *__restrict__ slope, int act, float *__restrict__ y32,
                                                   int ld32, uint16_t *__restrict__ ys, int lds, int los, int B, int H,
                                                   int W, int C8) {
  const int G = gridDim.x;
  int64_t blk = blockIdx.x;
  // XCD-contiguous logical order (as k_gemm_nt_bf16): an XCD's workgroups walk neighbouring output rows, so the z rows
  // they share (each is read by ~6 output rows) are fetched into that XCD's L2 once
  if ((G & 7) == 0) blk = (int64_t)(blockIdx.x & 7) * (G >> 3) + (blockIdx.x >> 3);
  const int64_t i = blk * blockDim.x + threadIdx.x;
  const int Ho = 2 * H, Wo = 2 * W;
  if (i >= (int64_t)B * Ho * Wo * C8) return;
  const int c8 = (int)(i % C8);
  const int64_t pix = i / C8;
  const int ox = (int)(pix % Wo), oy = (int)((pix / Wo) % Ho), b = (int)(pix / ((int64_t)Wo * Ho));
  const int C = 8 * C8;
  const int64_t ldz = 9 * (int64_t)C;
  const float *zb = z + (int64_t)b * H * W * ldz + 8 * c8;
  float acc[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
  for (int ky = 0; ky < 3; ++ky) {
    const int qy = oy + ky - 1;
    if (qy < 0 || qy >= Ho) continue;
#pragma unroll
    for (int kx = 0; kx < 3; ++kx) {
      const int qx = ox + kx - 1;
      if (qx < 0 || qx >= Wo) continue;
      const UpSrc s = up_src(qy, qx, H, W, Ho, Wo);
      const float *p = zb + ((int64_t)s.y0 * W + s.x0) * ldz + (ky * 3 + kx) * C;
      float a00[8], a01[8], a10[8], a11[8];
      load8<false>(p, 0, a00);
      load8<false>(p, s.xp * ldz, a01);
      load8<false>(p, s.yp * W * ldz, a10);
      load8<false>(p, ((int64_t)s.yp * W + s.xp) * ldz, a11);
#pragma unroll
      for (int k = 0; k < 8; ++k)
        acc[k] += s.h0 * (s.w0 * a00[k] + s.w1 * a01[k]) + s.h1 * (s.w0 * a10[k] + s.w1 * a11[k]);
    }
  }
  float bv[8];
  load8<false>(bias, 8 * c8, bv);
  const float sl = act == 2 ? *slope : 0.0f;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    acc[k] += bv[k];
    if (act) acc[k] = acc[k] > 0.0f ? acc[k] : sl * acc[k];
  }
  if (y32) store8<false>(y32, pix * ld32 + 8 * c8, acc);
  if (ys) store8_split(ys, pix * lds + 8 * c8, los, acc);
}

// x [B][C][H][W] fp32 at any element strides (channels-first or channels-last) -> the split form y [B][H][W] rows of
// pitch ldy: hi at channel c, lo at channel los + c.  A lane takes one pixel x 8 channels.
__global__ __launch_bounds__(256) void k_split_bf16(const float *__restrict__ x, int64_t sb, int64_t sc, int64_t sh,
                                                    int64_t sw, int B, int C8, int H, int W, uint16_t *__restrict__ y,
                                                    int ldy, int los) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)B * H * W * C8) return;
  const int c8 = (int)(i % C8);
  const int64_t pix = i / C8;
  const int px = (int)(pix % W), py = (int)((pix / W) % H), b = (int)(pix / ((int64_t)W * H));
  const float *src = x + b * sb + py * sh + px * sw + 8 * c8 * sc;
  float v[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) v[k] = src[k * sc];
  store8_split(y, pix * ldy + 8 * c8, los, v);
}

// ResNet18's stem tail: max_pool2d(3, 2, 1) of x [B][C][H][W] fp32 at any element strides (what MIOpen left of conv1:
// channels-first) -> the pooled map channels-last in fp32, y32 [B][Ho][Wo][C] (res2.0's identity shortcut), and in split
// form, ys [B][Ho][Wo][2C] (res2.0's GEMM operand), both from the same value.  Padding is -inf: nothing clamps the
// map in front of the pool, negative maxima are real.  A workgroup takes 16 output pixels of a row x 64 channels:
// the 3 x 3 windows are read with the lanes along the source's unit stride (x for channels-first, c for channels-last),
// turned through LDS, and written as whole channels-last rows.
constexpr int kMpPix = 16, kMpCh = 64, kMpPitch = kMpCh + 1;

__global__ __launch_bounds__(256) void k_maxpool3s2_split(const float *__restrict__ x, int64_t sb, int64_t sc, int64_t sh,
                                                          int64_t sw, int C, int H, int W, int Ho, int Wo, int strips,
                                                          float *__restrict__ y32, uint16_t *__restrict__ ys) {
  __shared__ float s_t[kMpPix * kMpPitch];
  const int strip = blockIdx.x % strips, oy = blockIdx.x / strips;
  const int c0 = blockIdx.y * kMpCh, b = blockIdx.z;
  const float *xb = x + b * sb;
  for (int i = threadIdx.x; i < kMpPix * kMpCh; i += 256) {
    int p, c;
    if (sc == 1) { c = i % kMpCh; p = i / kMpCh; }
    else { p = i % kMpPix; c = i / kMpPix; }
    const int ox = strip * kMpPix + p;
    float m = -INFINITY;
    if (ox < Wo && c0 + c < C) {
      const float *xc = xb + (c0 + c) * sc;
#pragma unroll
      for (int ky = 0; ky < 3; ++ky) {
        const int iy = 2 * oy + ky - 1;
        if (iy < 0 || iy >= H) continue;
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
          const int ix = 2 * ox + kx - 1;
          if (ix < 0 || ix >= W) continue;
          const float v = xc[iy * sh + ix * sw];
          if (v > m || v != v) m = v;  // (torch's update rule: a NaN wins)
        }
      }
    }
    s_t[p * kMpPitch + c] = m;
  }
  __syncthreads();
  if (threadIdx.x < kMpPix * (kMpCh / 8)) {
    const int c8 = threadIdx.x % (kMpCh / 8), p = threadIdx.x / (kMpCh / 8);
    const int ox = strip * kMpPix + p, ch = c0 + 8 * c8;
    if (ox < Wo && ch < C) {
      float v[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) v[k] = s_t[p * kMpPitch + 8 * c8 + k];
      const int64_t pix = ((int64_t)b * Ho + oy) * Wo + ox;
      if (y32) store8<false>(y32, pix * C + ch, v);
      if (ys) store8_split(ys, pix * 2 * C + ch, C, v);
    }
  }
}

// gx [B][H][W][C] = sum over the output pixels whose footprint contains (iy, ix), increasing (oy, ox)
template <bool BF16>
__global__ __launch_bounds__(256) void k_up_bwd(const void *__restrict__ gy, void *__restrict__ gx, int B, int H, int W,
                                                int Ho, int Wo, int C8) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t total = (int64_t)B * H * W * C8;
  if (i >= total) return;
  const int c8 = (int)(i % C8);
  const int64_t pix = i / C8;
  const int ix = (int)(pix % W), iy = (int)((pix / W) % H), b = (int)(pix / ((int64_t)W * H));
  const float ssy = up_scale(H, Ho), ssx = up_scale(W, Wo);
  // candidate output rows / columns: those with y0 in {iy - 1, iy} (generous bounds, exact test inside)
  int oy_lo = 0, oy_hi = Ho - 1, ox_lo = 0, ox_hi = Wo - 1;
  if (ssy > 0.0f) {
    oy_lo = max(0, (int)floorf((float)(iy - 1) / ssy));   // one row of slack on each side for the float quotient
    oy_hi = min(Ho - 1, (int)ceilf((float)(iy + 1) / ssy));
  }
  if (ssx > 0.0f) {
    ox_lo = max(0, (int)floorf((float)(ix - 1) / ssx));
    ox_hi = min(Wo - 1, (int)ceilf((float)(ix + 1) / ssx));
  }
  const int C = 8 * C8;
  float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int oy = oy_lo; oy <= oy_hi; ++oy) {
    const float sy = ssy * (float)oy;
    const int y0 = (int)sy;
    const int yp = y0 < H - 1 ? 1 : 0;
    const float h1 = sy - (float)y0, h0 = 1.0f - h1;
    if (!(y0 == iy || y0 + yp == iy)) continue;
    float wy = 0.0f;
    if (y0 == iy) wy += h0;
    if (y0 + yp == iy) wy += h1;
    for (int ox = ox_lo; ox <= ox_hi; ++ox) {
      const float sx = ssx * (float)ox;
      const int x0 = (int)sx;
      const int xp = x0 < W - 1 ? 1 : 0;
      const float w1 = sx - (float)x0, w0 = 1.0f - w1;
      if (!(x0 == ix || x0 + xp == ix)) continue;
      float wx = 0.0f;
      if (x0 == ix) wx += w0;
      if (x0 + xp == ix) wx += w1;
      float g[8];
      load8<BF16>(gy, (((int64_t)b * Ho + oy) * Wo + ox) * C + 8 * c8, g);
      const float w = wy * wx;
#pragma unroll
      for (int k = 0; k < 8; ++k) acc[k] += w * g[k];
    }
  }
  store8<BF16>(gx, pix * C + 8 * c8, acc);
}


// The channels-last bf16 backward through an LDS tile: a workgroup owns 8 x 8 input pixels x 64 channels, stages
// the output-gradient patch their footprints cover (~20 x 20 pixels for a x2 resize: 51 KB) with coalesced 16-byte
// loads, and the 512 lanes (pixel, 8-channel chunk) gather from LDS -- the direct kernel re-reads every output
// pixel ~6x from L2 (measured 0.37 ms for [16,256,64,64] <- [16,256,128,128]; the patch is read 1.6x).
constexpr int kUpT = 8;
__device__ __forceinline__ int up_lo(int i, float s) { return s > 0.0f ? max(0, (int)floorf((float)(i - 1) / s)) : 0; }
__device__ __forceinline__ int up_hi(int i, float s, int n_out) {
  return s > 0.0f ? min(n_out - 1, (int)ceilf((float)(i + 1) / s)) : n_out - 1;
}

__global__ __launch_bounds__(512) void k_up_bwd_tile_bf16(const uint16_t *__restrict__ gy, uint16_t *__restrict__ gx,
                                                          int H, int W, int Ho, int Wo, int C, int tiles_x) {
  MF_DYN_LDS(uint4, s_patch);  // [rows][cols][8 chunks]
  const int ty0 = (blockIdx.x / tiles_x) * kUpT, tx0 = (blockIdx.x % tiles_x) * kUpT;
  const int c0 = blockIdx.y * 64, b = blockIdx.z;
  const float ssy = up_scale(H, Ho), ssx = up_scale(W, Wo);
  const int r_lo = up_lo(ty0, ssy), r_hi = up_hi(min(ty0 + kUpT - 1, H - 1), ssy, Ho);
  const int q_lo = up_lo(tx0, ssx), q_hi = up_hi(min(tx0 + kUpT - 1, W - 1), ssx, Wo);
  const int R = r_hi - r_lo + 1, S = q_hi - q_lo + 1;
  for (int i = threadIdx.x; i < R * S * 8; i += 512) {
    const int ch = i & 7, pix = i >> 3, r = pix / S, q = pix - r * S;
    s_patch[i] = *reinterpret_cast<const uint4 *>(gy + (((int64_t)b * Ho + r_lo + r) * Wo + q_lo + q) * C + c0 + 8 * ch);
  }
  __syncthreads();
  const int ch = threadIdx.x & 7, p = threadIdx.x >> 3;
  const int iy = ty0 + p / kUpT, ix = tx0 + p % kUpT;
  if (iy >= H || ix >= W) return;
  float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  const int oy_lo = up_lo(iy, ssy), oy_hi = up_hi(iy, ssy, Ho), ox_lo = up_lo(ix, ssx), ox_hi = up_hi(ix, ssx, Wo);
  for (int oy = oy_lo; oy <= oy_hi; ++oy) {
    const float sy = ssy * (float)oy;
    const int y0 = (int)sy;
    const int yp = y0 < H - 1 ? 1 : 0;
    if (!(y0 == iy || y0 + yp == iy)) continue;
    const float h1 = sy - (float)y0, h0 = 1.0f - h1;
    float wy = 0.0f;
    if (y0 == iy) wy += h0;
    if (y0 + yp == iy) wy += h1;
    for (int ox = ox_lo; ox <= ox_hi; ++ox) {
      const float sx = ssx * (float)ox;
      const int x0 = (int)sx;
      const int xp = x0 < W - 1 ? 1 : 0;
      if (!(x0 == ix || x0 + xp == ix)) continue;
      const float w1 = sx - (float)x0, w0 = 1.0f - w1;
      float wx = 0.0f;
      if (x0 == ix) wx += w0;
      if (x0 + xp == ix) wx += w1;
      const uint4 g = s_patch[((oy - r_lo) * S + (ox - q_lo)) * 8 + ch];
      const uint32_t d[4] = {g.x, g.y, g.z, g.w};
      const float w = wy * wx;
#pragma unroll
      for (int k = 0; k < 4; ++k) { acc[2 * k] += w * mf::bf16_lo(d[k]); acc[2 * k + 1] += w * mf::bf16_hi(d[k]); }
    }
  }
  store8<true>(gx, (((int64_t)b * H + iy) * W + ix) * C + c0 + 8 * ch, acc);
}

// Channels-last backward when the INPUT map is small (PSPNet's pooled 1x1 .. 6x6 maps resized to 32 x 32): an input
// pixel's footprint is hundreds of output pixels -- walking it with one lane (the direct kernel) measured 0.37 ms for
// 17 MB.  One workgroup per (input pixel, 64 channels, image): 64 lanes share the footprint's output pixels, 8 lanes
// the channel chunks; partial sums meet in LDS in a fixed order.
template <bool BF16>
__global__ __launch_bounds__(512) void k_up_bwd_small(const void *__restrict__ gy, void *__restrict__ gx, int H, int W,
                                                      int Ho, int Wo, int C) {
  __shared__ float s_part[64][8][9];
  const int ix = blockIdx.x % W, iy = blockIdx.x / W;
  const int c0 = blockIdx.y * 64, b = blockIdx.z;
  const int ch = threadIdx.x & 7, pl = threadIdx.x >> 3;
  const float ssy = up_scale(H, Ho), ssx = up_scale(W, Wo);
  const int oy_lo = up_lo(iy, ssy), oy_hi = up_hi(iy, ssy, Ho), ox_lo = up_lo(ix, ssx), ox_hi = up_hi(ix, ssx, Wo);
  const int nx = ox_hi - ox_lo + 1, n = (oy_hi - oy_lo + 1) * nx;
  float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int k = pl; k < n; k += 64) {
    const int oy = oy_lo + k / nx, ox = ox_lo + k % nx;
    const float sy = ssy * (float)oy, sx = ssx * (float)ox;
    const int y0 = (int)sy, x0 = (int)sx;
    const int yp = y0 < H - 1 ? 1 : 0, xp = x0 < W - 1 ? 1 : 0;
    if (!(y0 == iy || y0 + yp == iy) || !(x0 == ix || x0 + xp == ix)) continue;
    const float h1 = sy - (float)y0, h0 = 1.0f - h1, w1 = sx - (float)x0, w0 = 1.0f - w1;
    float wy = 0.0f, wx = 0.0f;
    if (y0 == iy) wy += h0;
    if (y0 + yp == iy) wy += h1;
    if (x0 == ix) wx += w0;
    if (x0 + xp == ix) wx += w1;
    float g[8];
    load8<BF16>(gy, (((int64_t)b * Ho + oy) * Wo + ox) * C + c0 + 8 * ch, g);
    const float w = wy * wx;
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] += w * g[j];
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) s_part[pl][ch][j] = acc[j];
  __syncthreads();
  if (threadIdx.x < 64) {  // lane = (chunk, element): add the 64 partials in lane order
    const int cc = threadIdx.x >> 3, j = threadIdx.x & 7;
    float t = 0.0f;
    for (int q = 0; q < 64; ++q) t += s_part[q][cc][j];
    const int64_t o = (((int64_t)b * H + iy) * W + ix) * C + c0 + threadIdx.x;
    if (BF16) reinterpret_cast<uint16_t *>(gx)[o] = (uint16_t)mf::bf16_bits(t);
    else reinterpret_cast<float *>(gx)[o] = t;
  }
}

// The same maps for channels-FIRST tensors [B][C][H][W] (what MIOpen's fp32 NCHW solvers leave behind at inference):
// one lane per element, coalesced along x.
template <bool BF16>
__device__ __forceinline__ float load1(const void *p, int64_t i) {
  return BF16 ? __uint_as_float((uint32_t)reinterpret_cast<const uint16_t *>(p)[i] << 16) : reinterpret_cast<const float *>(p)[i];
}
template <bool BF16>
__device__ __forceinline__ void store1(void *p, int64_t i, float v) {
  if (BF16) reinterpret_cast<uint16_t *>(p)[i] = (uint16_t)mf::bf16_bits(v);
  else reinterpret_cast<float *>(p)[i] = v;
}

template <bool BF16>
__global__ __launch_bounds__(256) void k_up_fwd_cf(const void *__restrict__ x, void *__restrict__ y, int64_t BC, int H,
                                                   int W, int Ho, int Wo) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= BC * Ho * Wo) return;
  const int ox = (int)(i % Wo), oy = (int)((i / Wo) % Ho);
  const int64_t bc = i / ((int64_t)Wo * Ho);
  const float sy = up_scale(H, Ho) * (float)oy, sx = up_scale(W, Wo) * (float)ox;
  const int y0 = (int)sy, x0 = (int)sx;
  const int yp = y0 < H - 1 ? 1 : 0, xp = x0 < W - 1 ? 1 : 0;
  const float h1 = sy - (float)y0, h0 = 1.0f - h1, w1 = sx - (float)x0, w0 = 1.0f - w1;
  const int64_t base = (bc * H + y0) * W + x0;
  const float a00 = load1<BF16>(x, base), a01 = load1<BF16>(x, base + xp), a10 = load1<BF16>(x, base + (int64_t)yp * W),
              a11 = load1<BF16>(x, base + (int64_t)yp * W + xp);
  store1<BF16>(y, i, h0 * (w0 * a00 + w1 * a01) + h1 * (w0 * a10 + w1 * a11));
}

template <bool BF16>
__global__ __launch_bounds__(256) void k_up_bwd_cf(const void *__restrict__ gy, void *__restrict__ gx, int64_t BC, int H,
                                                   int W, int Ho, int Wo) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= BC * H * W) return;
  const int ix = (int)(i % W), iy = (int)((i / W) % H);
  const int64_t bc = i / ((int64_t)W * H);
  const float ssy = up_scale(H, Ho), ssx = up_scale(W, Wo);
  int oy_lo = 0, oy_hi = Ho - 1, ox_lo = 0, ox_hi = Wo - 1;
  if (ssy > 0.0f) { oy_lo = max(0, (int)floorf((float)(iy - 1) / ssy)); oy_hi = min(Ho - 1, (int)ceilf((float)(iy + 1) / ssy)); }
  if (ssx > 0.0f) { ox_lo = max(0, (int)floorf((float)(ix - 1) / ssx)); ox_hi = min(Wo - 1, (int)ceilf((float)(ix + 1) / ssx)); }
  float acc = 0.0f;
  for (int oy = oy_lo; oy <= oy_hi; ++oy) {
    const float sy = ssy * (float)oy;
    const int y0 = (int)sy;
    const int yp = y0 < H - 1 ? 1 : 0;
    if (!(y0 == iy || y0 + yp == iy)) continue;
    const float h1 = sy - (float)y0, h0 = 1.0f - h1;
    float wy = 0.0f;
    if (y0 == iy) wy += h0;
    if (y0 + yp == iy) wy += h1;
    for (int ox = ox_lo; ox <= ox_hi; ++ox) {
      const float sx = ssx * (float)ox;
      const int x0 = (int)sx;
      const int xp = x0 < W - 1 ? 1 : 0;
      if (!(x0 == ix || x0 + xp == ix)) continue;
      const float w1 = sx - (float)x0, w0 = 1.0f - w1;
      float wx = 0.0f;
      if (x0 == ix) wx += w0;
      if (x0 + xp == ix) wx += w1;
      acc += (wy * wx) * load1<BF16>(gy, (bc * Ho + oy) * Wo + ox);
    }
  }
  store1<BF16>(gx, i, acc);
}

// PReLU with ONE slope: y = x > 0 ? x : a x
template <bool BF16>
__global__ __launch_bounds__(256) void k_prelu_fwd(const void *__restrict__ x, const float *__restrict__ slope,
                                                   void *__restrict__ y, int64_t n8) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n8) return;
  const float a = slope[0];
  float v[8];
  load8<BF16>(x, 8 * i, v);
#pragma unroll
  for (int k = 0; k < 8; ++k) v[k] = v[k] > 0.0f ? v[k] : a * v[k];
  store8<BF16>(y, 8 * i, v);
}

// BatchNorm in inference mode (+ residual add) (+ ReLU) of ResNet18Extractor (models/resnet.py:44: the statistics are
// never updated): y = relu?((x - mean) * (weight * invstd) + bias (+ identity)), invstd = 1 / sqrt(var + eps) -- torch's
// own operation order.  torch: one elementwise launch for the normalisation, one for the add, one for the ReLU.
// CL: channels-last (8 consecutive elements = 8 consecutive channels); otherwise NCHW with HW % 8 == 0 (8 consecutive
// elements = one channel).
template <bool BF16, bool CL>
__global__ __launch_bounds__(256) void k_bn_act(const void *__restrict__ x, const void *__restrict__ identity,
                                                const float *__restrict__ mean, const float *__restrict__ var,
                                                const float *__restrict__ weight, const float *__restrict__ bias,
                                                float eps, void *__restrict__ y, int64_t n8, int C, int64_t HW, int relu) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n8) return;
  float v[8], r[8];
  load8<BF16>(x, 8 * i, v);
  if (identity) load8<BF16>(identity, 8 * i, r);
  const int c0 = CL ? (int)((8 * i) % C) : (int)(((8 * i) / HW) % C);
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int c = CL ? c0 + k : c0;
    const float invstd = 1.0f / sqrtf(var[c] + eps);
    float o = (v[k] - mean[c]) * (weight[c] * invstd) + bias[c];
    if (identity) o += r[k];
    v[k] = relu ? (o > 0.0f ? o : 0.0f) : o;
  }
  store8<BF16>(y, 8 * i, v);
}

// The channels-last form at ResNet widths (C / 8 = G in {8, 16, 32, 64} channel groups): a lane keeps ONE channel group
// (its 4 x 8 parameters arrive as eight 16-byte loads -- read per element they would be 32 dword loads for 8 elements
// of data, and the kernel would be bound by its own parameter traffic) and walks `ppt` pixels with it.
template <bool BF16>
__global__ __launch_bounds__(256) void k_bn_act_cl(const void *__restrict__ x, const void *__restrict__ identity,
                                                   const float *__restrict__ mean, const float *__restrict__ var,
                                                   const float *__restrict__ weight, const float *__restrict__ bias,
                                                   float eps, void *__restrict__ y, int64_t npix, int G, int ppt, int relu) {
  const int cg = threadIdx.x % G, lp = threadIdx.x / G, ppb = 256 / G;  // pixels per block pass
  float mu[8], sc[8], sh[8], vr[8];
  load8<false>(mean, 8 * cg, mu);
  load8<false>(var, 8 * cg, vr);
  load8<false>(weight, 8 * cg, sc);
  load8<false>(bias, 8 * cg, sh);
#pragma unroll
  for (int k = 0; k < 8; ++k) sc[k] = sc[k] * (1.0f / sqrtf(vr[k] + eps));
  const int64_t p0 = (int64_t)blockIdx.x * ppb * ppt + lp;
  for (int u = 0; u < ppt; ++u) {
    const int64_t pix = p0 + (int64_t)u * ppb;
    if (pix >= npix) break;
    const int64_t e = (pix * G + cg) * 8;
    float v[8], r[8];
    load8<BF16>(x, e, v);
    if (identity) load8<BF16>(identity, e, r);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      float o = (v[k] - mu[k]) * sc[k] + sh[k];
      if (identity) o += r[k];
      v[k] = relu ? (o > 0.0f ? o : 0.0f) : o;
    }
    store8<BF16>(y, e, v);
  }
}

// ResNet18Extractor's input normalisation (models/resnet.py:33-36): (rgb / 255 - mean) / std per channel, torch's
// operation order, on the [B, H, W, 3] image as it arrives (uint8 or float32) -> float32 in the same (channels-last)
// memory order.  torch: cast, divide, subtract, divide = four launches.
template <bool U8>
__global__ __launch_bounds__(256) void k_rgb_norm(const void *__restrict__ rgb, float m0, float m1, float m2, float s0,
                                                  float s1, float s2, float *__restrict__ out, int64_t npix) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= npix) return;
  float r, g, b;
  if (U8) {
    const uint8_t *p = reinterpret_cast<const uint8_t *>(rgb) + 3 * i;
    r = (float)p[0]; g = (float)p[1]; b = (float)p[2];
  } else {
    const float *p = reinterpret_cast<const float *>(rgb) + 3 * i;
    r = p[0]; g = p[1]; b = p[2];
  }
  out[3 * i] = (r / 255.0f - m0) / s0;
  out[3 * i + 1] = (g / 255.0f - m1) / s1;
  out[3 * i + 2] = (b / 255.0f - m2) / s2;
}

// dx = dy (x > 0 ? 1 : a); partial[block] = sum over the block's elements with x <= 0 of dy x
constexpr int kPreluPerThread = 4;  // 8-element chunks per lane: 8192 elements per workgroup

template <bool BF16>
__global__ __launch_bounds__(256) void k_prelu_bwd(const void *__restrict__ x, const void *__restrict__ dy,
                                                   const float *__restrict__ slope, void *__restrict__ dx,
                                                   float *__restrict__ partial, int64_t n8) {
  __shared__ float s_red[4];
  const float a = slope[0];
  float part = 0.0f;
#pragma unroll
  for (int u = 0; u < kPreluPerThread; ++u) {
    const int64_t i = ((int64_t)blockIdx.x * kPreluPerThread + u) * blockDim.x + threadIdx.x;
    if (i >= n8) continue;
    float v[8], g[8];
    load8<BF16>(x, 8 * i, v);
    load8<BF16>(dy, 8 * i, g);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const bool pos = v[k] > 0.0f;
      part += pos ? 0.0f : g[k] * v[k];
      g[k] = pos ? g[k] : a * g[k];
    }
    store8<BF16>(dx, 8 * i, g);
  }
  part = mf::wave_sum(part);
  if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = part;
  __syncthreads();
  if (threadIdx.x == 0) partial[blockIdx.x] = (s_red[0] + s_red[1]) + (s_red[2] + s_red[3]);
}

__global__ __launch_bounds__(256) void k_prelu_finish(const float *__restrict__ partial, int n, float *__restrict__ da) {
  __shared__ float s_red[4];
  float s = 0.0f;
  for (int i = threadIdx.x; i < n; i += 256) s += partial[i];  // fixed assignment of partials to lanes
  s = mf::wave_sum(s);
  if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) da[0] = (s_red[0] + s_red[1]) + (s_red[2] + s_red[3]);
}

// which kernel the last mf_upsample_bilinear_cl_bwd / mf_bn_act_fwd launch of this process took: mf_backbone2d_last_path
enum { kPathUpDirect = 1, kPathUpTile = 2, kPathUpSmall = 3, kPathBnGeneric = 16, kPathBnGroup = 32 /* + ppt */ };
int g_b2d_last_path = 0;

int bad2d(const char *msg) {
  mf::set_last_error(hipErrorInvalidValue, msg);
  return -(int)hipErrorInvalidValue;
}

}  // namespace

/* y [B, Ho, Wo, C] = bilinear resize (align_corners) of x [B, H, W, C], channels-last; bf16 != 0: bfloat16 tensors,
 * else float32.  C % 8 == 0, 16-byte aligned. */
extern "C" int mf_upsample_bilinear_cl_fwd(const void *x, void *y, int32_t B, int32_t H, int32_t W, int32_t Ho,
                                           int32_t Wo, int32_t C, int32_t bf16, mfStream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if ((int64_t)B * Ho * Wo * C == 0) return 0;
  if (C % 8 || H < 1 || W < 1 || (((uintptr_t)x | (uintptr_t)y) & 15)) return bad2d("upsample_bilinear_cl: C % 8 == 0, aligned");
  const int64_t total = (int64_t)B * Ho * Wo * (C / 8);
  const unsigned nb = (unsigned)((total + 255) / 256);
  if (bf16) hipLaunchKernelGGL(k_up_fwd<true>, dim3(nb), dim3(256), 0, stream, x, y, B, H, W, Ho, Wo, C / 8);
  else hipLaunchKernelGGL(k_up_fwd<false>, dim3(nb), dim3(256), 0, stream, x, y, B, H, W, Ho, Wo, C / 8);
  return mf::check_launch("mf_upsample_bilinear_cl_fwd");
}

/* The resize of fp32 x [B, H, W, C] (channels-last, dense) split into y [B, Ho, Wo] rows of pitch ldy: hi(v) at
 * channel c, lo(v) at channel los + c (the split-bf16 operand of mf_conv2d_split_fwd; y may be a channel block of a
 * wider map).  C, ldy, los % 8 == 0, 16-byte aligned. */
extern "C" int mf_upsample_bilinear_cl_split_fwd(const float *x, void *y, int32_t B, int32_t H, int32_t W, int32_t Ho,
                                                 int32_t Wo, int32_t C, int32_t ldy, int32_t los, mfStream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if ((int64_t)B * Ho * Wo * C == 0) return 0;
  if (C % 8 || ldy % 8 || los % 8 || los < C || ldy < los + C || H < 1 || W < 1 ||
      (((uintptr_t)x | (uintptr_t)y) & 15))
    return bad2d("upsample_bilinear_cl_split: C, ldy, los % 8 == 0, los >= C, ldy >= los + C, aligned");
  const int64_t total = (int64_t)B * Ho * Wo * (C / 8);
  hipLaunchKernelGGL(k_up_fwd_split, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, x, (uint16_t *)y, B, H,
                     W, Ho, Wo, C / 8, ldy, los);
  return mf::check_launch("mf_upsample_bilinear_cl_split_fwd");
}

/* PSPUpsample's resize + 3 x 3 convolution from the per-tap 1 x 1 convolutions of the low-resolution map (k_up_tapsum):
 * z fp32 [B, H, W, 9 C] (column t C + c, t = ky 3 + kx) -> v = act(bias + sum of the in-map taps' bilinear terms) on the
 * [B, 2H, 2W] map, written as y32[m * ld32 + c] and / or ys[m * lds + c] = hi(v), ys[m * lds + los + c] = lo(v).
 * act: 0 none, 1 ReLU, 2 PReLU with the single slope *slope (read on the device).  C and the pitches % 8 == 0, 16-byte
 * aligned; fixed summation order, no atomics. */
extern "C" int mf_upsample2x_tapsum_fwd(const float *z, const float *bias, const float *slope, int32_t act, float *y32,
                                        int32_t ld32, void *ys, int32_t lds, int32_t los, int32_t B, int32_t H, int32_t W,
                                        int32_t C, mfStream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if ((int64_t)B * H * W * C == 0) return 0;
  if (C < 8 || C % 8 || H < 1 || W < 1 || B < 0 || !bias || (!y32 && !ys) || act < 0 || act > 2 || (act == 2 && !slope))
    return bad2d("upsample2x_tapsum: C % 8 == 0, a bias, at least one output, act 0 / 1 / 2 (PReLU needs its slope)");
  if ((y32 && (ld32 < C || ld32 % 8)) || (ys && (lds % 8 || los % 8 || los < C || lds < los + C)))
    return bad2d("upsample2x_tapsum: pitches >= C and multiples of 8; lo plane inside the row");
  if (((uintptr_t)z | (uintptr_t)bias | (uintptr_t)y32 | (uintptr_t)ys) & 15 || ((uintptr_t)slope & 3))
    return bad2d("upsample2x_tapsum: 16-byte aligned operands");
  const int64_t total = (int64_t)B * 4 * H * W * (C / 8);
  if ((total + 255) / 256 >= (1ll << 31)) return bad2d("upsample2x_tapsum: too many output elements for one launch");
  hipLaunchKernelGGL(k_up_tapsum, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, z, bias, slope, act, y32,
                     ld32, (uint16_t *)ys, lds, los, B, H, W, C / 8);
  return mf::check_launch("mf_upsample2x_tapsum_fwd");
}

/* fp32 x [B, C, H, W] at element strides (sb, sc, sh, sw) -> its split form y [B, H, W] rows of pitch ldy: hi at
 * channel c, lo at channel los + c.  C, ldy, los % 8 == 0, y 16-byte aligned. */
extern "C" int mf_split_bf16(const float *x, int64_t sb, int64_t sc, int64_t sh, int64_t sw, int32_t B, int32_t C,
                             int32_t H, int32_t W, void *y, int32_t ldy, int32_t los, mfStream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if ((int64_t)B * C * H * W == 0) return 0;
  if (C % 8 || ldy % 8 || los % 8 || los < C || ldy < los + C || ((uintptr_t)y & 15))
    return bad2d("split_bf16: C, ldy, los % 8 == 0, los >= C, ldy >= los + C, aligned output");
  const int64_t total = (int64_t)B * H * W * (C / 8);
  hipLaunchKernelGGL(k_split_bf16, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, x, sb, sc, sh, sw, B,
                     C / 8, H, W, (uint16_t *)y, ldy, los);
  return mf::check_launch("mf_split_bf16");
}

/* max_pool2d(3, 2, 1) (padding -inf) of fp32 x [B, C, H, W] at element strides (sb, sc, sh, sw) -> y32 [B, Ho, Wo, C]
 * channels-last fp32 and / or its split form ys [B, Ho, Wo, 2C] (hi at channel c, lo at C + c), Ho = (H - 1) / 2 + 1.
 * C % 8 == 0, outputs 16-byte aligned; either output may be null. */
extern "C" int mf_maxpool3s2_split_fwd(const float *x, int64_t sb, int64_t sc, int64_t sh, int64_t sw, int32_t B,
                                       int32_t C, int32_t H, int32_t W, float *y32, void *ys, mfStream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if ((int64_t)B * C * H * W == 0) return 0;
  if (B < 0 || B > 65535 || C < 8 || C % 8 || H < 1 || W < 1 || !x || (!y32 && !ys) ||
      (((uintptr_t)y32 | (uintptr_t)ys) & 15))
    return bad2d("maxpool3s2_split: C % 8 == 0, B <= 65535, at least one output, aligned outputs");
  const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1, strips = (Wo + kMpPix - 1) / kMpPix;
  hipLaunchKernelGGL(k_maxpool3s2_split, dim3((unsigned)(strips * Ho), (unsigned)((C + kMpCh - 1) / kMpCh), (unsigned)B),
                     dim3(256), 0, stream, x, sb, sc, sh, sw, C, H, W, Ho, Wo, strips, y32, (uint16_t *)ys);
  return mf::check_launch("mf_maxpool3s2_split_fwd");
}

extern "C" int mf_upsample_bilinear_cl_bwd(const void *gy, void *gx, int32_t B, int32_t H, int32_t W, int32_t Ho,
                                           int32_t Wo, int32_t C, int32_t bf16, mfStream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if ((int64_t)B * H * W * C == 0) return 0;
  if (C % 8 || (((uintptr_t)gx | (uintptr_t)gy) & 15)) return bad2d("upsample_bilinear_cl: C % 8 == 0, aligned");
  const int64_t total = (int64_t)B * H * W * (C / 8);
  const unsigned nb = (unsigned)((total + 255) / 256);
  if (C % 64 == 0 && (int64_t)H * W <= 64 && (int64_t)Ho * Wo >= 16 * (int64_t)H * W) {  // small input, large footprints
    const dim3 grid((unsigned)(H * W), (unsigned)(C / 64), (unsigned)B);
    g_b2d_last_path = kPathUpSmall;
    if (bf16) hipLaunchKernelGGL(k_up_bwd_small<true>, grid, dim3(512), 0, stream, gy, gx, H, W, Ho, Wo, C);
    else hipLaunchKernelGGL(k_up_bwd_small<false>, grid, dim3(512), 0, stream, gy, gx, H, W, Ho, Wo, C);
    return mf::check_launch("mf_upsample_bilinear_cl_bwd");
  }
  if (bf16 && C % 64 == 0 && H >= kUpT && W >= kUpT) {
    // the LDS-tiled gather when the worst tile's output patch fits 64 KB (a x2 resize: 20 x 20 x 128 B = 51 KB)
    const float sy = Ho > 1 ? (float)(H - 1) / (float)(Ho - 1) : 0.0f, sx = Wo > 1 ? (float)(W - 1) / (float)(Wo - 1) : 0.0f;
    const int rows = sy > 0.0f ? (int)ceilf((float)(kUpT + 1) / sy) + 3 : Ho, cols = sx > 0.0f ? (int)ceilf((float)(kUpT + 1) / sx) + 3 : Wo;
    const size_t lds = (size_t)rows * cols * 128;
    if (lds <= 64 * 1024) {
      const int tx = (W + kUpT - 1) / kUpT, ty = (H + kUpT - 1) / kUpT;
      g_b2d_last_path = kPathUpTile;
      hipLaunchKernelGGL(k_up_bwd_tile_bf16, dim3((unsigned)(tx * ty), (unsigned)(C / 64), (unsigned)B), dim3(512), lds, stream,
                         (const uint16_t *)gy, (uint16_t *)gx, H, W, Ho, Wo, C, tx);
      return mf::check_launch("mf_upsample_bilinear_cl_bwd");
    }
  }
  g_b2d_last_path = kPathUpDirect;
  if (bf16) hipLaunchKernelGGL(k_up_bwd<true>, dim3(nb), dim3(256), 0, stream, gy, gx, B, H, W, Ho, Wo, C / 8);
  else hipLaunchKernelGGL(k_up_bwd<false>, dim3(nb), dim3(256), 0, stream, gy, gx, B, H, W, Ho, Wo, C / 8);
  return mf::check_launch("mf_upsample_bilinear_cl_bwd");
}


/* the same for channels-first tensors x [B*C, H, W] -> y [B*C, Ho, Wo] (no alignment or channel-count requirement) */
extern "C" int mf_upsample_bilinear_cf_fwd(const void *x, void *y, int64_t BC, int32_t H, int32_t W, int32_t Ho,
                                           int32_t Wo, int32_t bf16, mfStream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const int64_t total = BC * Ho * Wo;
  if (total == 0) return 0;
  const unsigned nb = (unsigned)((total + 255) / 256);
  if (bf16) hipLaunchKernelGGL(k_up_fwd_cf<true>, dim3(nb), dim3(256), 0, stream, x, y, BC, H, W, Ho, Wo);
  else hipLaunchKernelGGL(k_up_fwd_cf<false>, dim3(nb), dim3(256), 0, stream, x, y, BC, H, W, Ho, Wo);
  return mf::check_launch("mf_upsample_bilinear_cf_fwd");
}

extern "C" int mf_upsample_bilinear_cf_bwd(const void *gy, void *gx, int64_t BC, int32_t H, int32_t W, int32_t Ho,
                                           int32_t Wo, int32_t bf16, mfStream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const int64_t total = BC * H * W;
  if (total == 0) return 0;
  const unsigned nb = (unsigned)((total + 255) / 256);
  if (bf16) hipLaunchKernelGGL(k_up_bwd_cf<true>, dim3(nb), dim3(256), 0, stream, gy, gx, BC, H, W, Ho, Wo);
  else hipLaunchKernelGGL(k_up_bwd_cf<false>, dim3(nb), dim3(256), 0, stream, gy, gx, BC, H, W, Ho, Wo);
  return mf::check_launch("mf_upsample_bilinear_cf_bwd");
}

/* PReLU with one slope (device pointer, fp32) over n elements (n % 8 == 0) */
extern "C" int mf_prelu_fwd(const void *x, const float *slope, void *y, int64_t n, int32_t bf16, mfStream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (n <= 0) return 0;
  if (n % 8 || (((uintptr_t)x | (uintptr_t)y) & 15)) return bad2d("prelu: n % 8 == 0, aligned");
  const unsigned nb = (unsigned)((n / 8 + 255) / 256);
  if (bf16) hipLaunchKernelGGL(k_prelu_fwd<true>, dim3(nb), dim3(256), 0, stream, x, slope, y, n / 8);
  else hipLaunchKernelGGL(k_prelu_fwd<false>, dim3(nb), dim3(256), 0, stream, x, slope, y, n / 8);
  return mf::check_launch("mf_prelu_fwd");
}

extern "C" int64_t mf_prelu_bwd_workspace_floats(int64_t n) { return (n / 8 + 256 * kPreluPerThread - 1) / (256 * kPreluPerThread); }

/* dx = dy * (x > 0 ? 1 : slope); dslope[0] = sum_{x <= 0} dy x (fp32; block partials in ws, added in block order) */
extern "C" int mf_prelu_bwd(const void *x, const void *dy, const float *slope, void *dx, float *dslope, float *ws,
                            int64_t n, int32_t bf16, mfStream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (n <= 0) return 0;
  if (n % 8 || !ws || (((uintptr_t)x | (uintptr_t)dy | (uintptr_t)dx) & 15)) return bad2d("prelu backward: n % 8 == 0, aligned, workspace");
  const int64_t nblk = mf_prelu_bwd_workspace_floats(n);
  if (bf16) hipLaunchKernelGGL(k_prelu_bwd<true>, dim3((unsigned)nblk), dim3(256), 0, stream, x, dy, slope, dx, ws, n / 8);
  else hipLaunchKernelGGL(k_prelu_bwd<false>, dim3((unsigned)nblk), dim3(256), 0, stream, x, dy, slope, dx, ws, n / 8);
  hipLaunchKernelGGL(k_prelu_finish, dim3(1), dim3(256), 0, stream, (const float *)ws, (int)nblk, dslope);
  return mf::check_launch("mf_prelu_bwd");
}

/* BatchNorm (inference statistics) + optional residual add + optional ReLU over a dense [B, C, H, W] tensor, NCHW
 * (channels_last = 0; H * W % 8 == 0) or channels-last (C % 8 == 0); fp32 or bf16 activations, fp32 parameters. */
extern "C" int mf_bn_act_fwd(const void *x, const void *identity, const float *mean, const float *var, const float *weight,
                             const float *bias, float eps, void *y, int64_t n, int32_t C, int64_t HW, int32_t channels_last,
                             int32_t relu, int32_t bf16, mfStream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (n <= 0) return 0;
  if (n % 8 || C <= 0 || HW <= 0 || (channels_last ? C % 8 : HW % 8) ||
      (((uintptr_t)x | (uintptr_t)y | (uintptr_t)identity) & 15))
    return bad2d("bn_act: n % 8 == 0, 8 | C (channels-last) or 8 | H W (NCHW), aligned");
  const int G = C / 8;
  if (channels_last && G <= 256 && 256 % G == 0 &&
      ((((uintptr_t)mean | (uintptr_t)var | (uintptr_t)weight | (uintptr_t)bias) & 15) == 0)) {
    const int64_t npix = n / C, ppb = 256 / G;
    int ppt = 1;  // pixels per lane: as many as still leave >= 2048 workgroups (8 per CU), at most 4
    while (ppt < 4 && npix / (ppb * ppt * 2) >= 2048) ppt *= 2;
    const unsigned nbp = (unsigned)((npix + ppb * ppt - 1) / (ppb * ppt));
    g_b2d_last_path = kPathBnGroup + ppt;
    if (bf16) hipLaunchKernelGGL(k_bn_act_cl<true>, dim3(nbp), dim3(256), 0, stream, x, identity, mean, var, weight, bias,
                                 eps, y, npix, G, ppt, relu);
    else hipLaunchKernelGGL(k_bn_act_cl<false>, dim3(nbp), dim3(256), 0, stream, x, identity, mean, var, weight, bias, eps,
                            y, npix, G, ppt, relu);
    return mf::check_launch("mf_bn_act_fwd");
  }
  const unsigned nb = (unsigned)((n / 8 + 255) / 256);
  g_b2d_last_path = kPathBnGeneric;
#define MF_BN_LAUNCH(BF, CL_)                                                                                   \
  hipLaunchKernelGGL((k_bn_act<BF, CL_>), dim3(nb), dim3(256), 0, stream, x, identity, mean, var, weight, bias, eps, y, \
                     n / 8, C, HW, relu)
  if (bf16) { if (channels_last) MF_BN_LAUNCH(true, true); else MF_BN_LAUNCH(true, false); }
  else { if (channels_last) MF_BN_LAUNCH(false, true); else MF_BN_LAUNCH(false, false); }
#undef MF_BN_LAUNCH
  return mf::check_launch("mf_bn_act_fwd");
}

extern "C" int mf_backbone2d_last_path(void) { return g_b2d_last_path; }

/* (rgb / 255 - mean) / std of a [B, H, W, 3] image, uint8 (u8 = 1) or float32, -> float32 [B, H, W, 3]. */
extern "C" int mf_rgb_normalize(const void *rgb, int32_t u8, const float *mean3, const float *std3, float *out,
                                int64_t npix, mfStream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (npix <= 0) return 0;
  const unsigned nb = (unsigned)((npix + 255) / 256);
  if (u8) hipLaunchKernelGGL(k_rgb_norm<true>, dim3(nb), dim3(256), 0, stream, rgb, mean3[0], mean3[1], mean3[2], std3[0],
                             std3[1], std3[2], out, npix);
  else hipLaunchKernelGGL(k_rgb_norm<false>, dim3(nb), dim3(256), 0, stream, rgb, mean3[0], mean3[1], mean3[2], std3[0],
                          std3[1], std3[2], out, npix);
  return mf::check_launch("mf_rgb_normalize");
}
