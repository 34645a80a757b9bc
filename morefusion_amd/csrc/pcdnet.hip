// Point-cloud baseline pose network (contrib/singleview_pcd): the point-wise kernels around the split-bf16 GEMMs --
// gfx950, inference.
//
// Reference: examples/ycb_video/singleview_pcd/contrib/models/model.py:69-155 (predict) and :299-330
// (PoseNetExtractor): a chain of 1 x 1 Convolution1D over the B * P sampled points.  Rows are points, m = b * P + p.
// DESIGN.md "Point-cloud baseline network" has the layer table; tests/pcdnet_ref.py is the NumPy mirror these kernels
// are pinned to.
//
//   k_pcd_stem        gather of the sampled points, p - center, conv1_rgb (32 -> 64) and conv1_pcd (3 -> 64) with ReLU.
//                     K = 32 and K = 3 are below one MFMA step: VALU, the weights in LDS (k-major, a lane = a channel),
//                     the 16 input rows of a workgroup in LDS (read as broadcasts).  feat1 is written in split form twice:
//                     into its own rows (conv2's operand: rgb hi | rgb lo | pcd hi | pcd lo, 64 each) and into channels
//                     0 .. 127 of the heads' 384-wide rows (hi plane, lo plane 384 further).
//   k_pcd_pool        pooled[b][c] = mean over the P rows of object b (average_pooling_1d over all points): 8 row lanes x
//                     64 channels per workgroup, row lane j adds rows j, j + 8, ... in increasing order, the eight partial
//                     sums are folded as ((0 + 1) + (2 + 3)) + ((4 + 5) + (6 + 7)), divided by P.  No atomics: the order
//                     depends on P alone, results are bit-identical from run to run.
//   k_pcd_bias_split  heads layer 1 after the fold: h = relu(y[m][n] + gbias[m / P][n]) in split form, head g's 640
//                     channels as (hi | lo) at column 1280 g -- the operand layout of the heads' second layer.
//
// The arithmetic (nothing is contracted: -ffp-contract=off): a convolution is s = 0; s += x[k] * w[k] for increasing k;
// v = max(s + bias, 0).  Split form: hi = bf16(v) (round to nearest even), lo = bf16(v - hi).
#include "mf_common.h"

namespace {

constexpr int kStemRows = 16;   // rows of a stem workgroup: 256 lanes = 2 row halves x 128 channels
constexpr int kPoolLanes = 8;   // row lanes of the pool
constexpr int kPoolChans = 64;  // channels of a pool workgroup

int bad(const char *what) {
  mf::set_last_error(hipErrorInvalidValue, what);
  return -(int)hipErrorInvalidValue;
}

__device__ __forceinline__ void store_split(uint16_t *hi_at, int los, float v) {
  const uint32_t h = mf::bf16_bits(v);
  hi_at[0] = (uint16_t)h;
  hi_at[los] = (uint16_t)mf::bf16_bits(v - __uint_as_float(h << 16));
}

__global__ __launch_bounds__(256) void k_pcd_stem(const float *__restrict__ x,       // [M][32]
                                                  const float *__restrict__ pcd,     // [B][HW][3]
                                                  const int64_t *__restrict__ pix,   // [M]
                                                  const float *__restrict__ center,  // [B][3] or null
                                                  const float *__restrict__ w_rgb,   // [64][32]
                                                  const float *__restrict__ b_rgb, const float *__restrict__ w_pcd,  // [64][3]
                                                  const float *__restrict__ b_pcd, int M, int P, int HW,
                                                  float *__restrict__ pts,  // [M][3]: p - center (p without a center)
                                                  uint16_t *__restrict__ f1, int ld1, uint16_t *__restrict__ xs, int ldx,
                                                  int losx) {
  __shared__ float s_w[32][128];  // [k][channel]; rows 0 .. 2 of the pcd half hold conv1_pcd
  __shared__ __attribute__((aligned(16))) float s_x[kStemRows][32];
  __shared__ float s_p[kStemRows][4];
  const int t = threadIdx.x, c = t & 127, half = t >> 7;
  const int m0 = blockIdx.x * kStemRows;
  for (int i = t; i < 32 * 64; i += 256) {
    const int n = i >> 5, k = i & 31;
    s_w[k][n] = w_rgb[i];
  }
  if (t < 3 * 64) s_w[t % 3][64 + t / 3] = w_pcd[t];
  for (int i = t; i < kStemRows * 8; i += 256) {
    const int r = i >> 3, m = m0 + r;
    const float4 v = m < M ? *reinterpret_cast<const float4 *>(x + (int64_t)m * 32 + 4 * (i & 7)) : make_float4(0, 0, 0, 0);
    *reinterpret_cast<float4 *>(&s_x[r][4 * (i & 7)]) = v;
  }
  if (t < kStemRows * 3) {
    const int r = t / 3, a = t - 3 * r, m = m0 + r;
    float v = 0.0f;
    if (m < M) {
      const int b = m / P;
      const int64_t px = pix[m];
      // (a pixel outside the image: NaN, never a read outside the cloud)
      v = (px >= 0 && px < HW) ? pcd[((int64_t)b * HW + px) * 3 + a] : __uint_as_float(0x7fc00000u);
      if (center) v = v - center[3 * b + a];
      pts[(int64_t)m * 3 + a] = v;
    }
    s_p[r][a] = v;
  }
  __syncthreads();
  const bool rgb = c < 64;
  const int K = rgb ? 32 : 3;
  float w[32];
#pragma unroll
  for (int k = 0; k < 32; ++k) w[k] = k < K ? s_w[k][c] : 0.0f;
  const float bias = rgb ? b_rgb[c] : b_pcd[c - 64];
  // feat1's own rows: rgb hi at 0, lo at 64; pcd hi at 128, lo at 192
  const int col1 = rgb ? c : 128 + (c - 64);
  for (int r = half * (kStemRows / 2); r < (half + 1) * (kStemRows / 2); ++r) {
    const int m = m0 + r;
    if (m >= M) break;
    float s = 0.0f;
    if (rgb) {
#pragma unroll
      for (int k = 0; k < 32; ++k) s += s_x[r][k] * w[k];
    } else {
#pragma unroll
      for (int k = 0; k < 3; ++k) s += s_p[r][k] * w[k];
    }
    float v = s + bias;
    v = v > 0.0f ? v : 0.0f;
    store_split(f1 + (int64_t)m * ld1 + col1, 64, v);
    store_split(xs + (int64_t)m * ldx + c, losx, v);
  }
}

__global__ __launch_bounds__(kPoolLanes * kPoolChans) void k_pcd_pool(const float *__restrict__ h, int64_t ldh, int P,
                                                                      int C, float *__restrict__ pooled) {
  __shared__ float s_sum[kPoolLanes][kPoolChans];
  const int b = blockIdx.y, c = blockIdx.x * kPoolChans + (threadIdx.x & (kPoolChans - 1));
  const int j = threadIdx.x / kPoolChans;
  const float *src = h + (int64_t)b * P * ldh + c;
  float acc = 0.0f;
#pragma unroll 4
  for (int p = j; p < P; p += kPoolLanes) acc += src[(int64_t)p * ldh];
  s_sum[j][threadIdx.x & (kPoolChans - 1)] = acc;
  __syncthreads();
  if (j == 0) {
    const int l = threadIdx.x;
    const float s = ((s_sum[0][l] + s_sum[1][l]) + (s_sum[2][l] + s_sum[3][l])) +
                    ((s_sum[4][l] + s_sum[5][l]) + (s_sum[6][l] + s_sum[7][l]));
    pooled[(int64_t)b * C + c] = s / (float)P;
  }
}

__global__ __launch_bounds__(256) void k_pcd_bias_split(const float *__restrict__ y, int64_t ldy,
                                                        const float *__restrict__ gbias, int64_t M, int P, int N, int G,
                                                        uint16_t *__restrict__ out, int64_t ldo) {
  const int n8 = N / 8;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= M * n8) return;
  const int64_t m = i / n8;
  const int n = 8 * (int)(i - m * n8);
  const int b = (int)(m / P);
  const float *yr = y + m * ldy + n, *gb = gbias + (int64_t)b * N + n;
  const float4 y0 = *reinterpret_cast<const float4 *>(yr), y1 = *reinterpret_cast<const float4 *>(yr + 4);
  const float4 g0 = *reinterpret_cast<const float4 *>(gb), g1 = *reinterpret_cast<const float4 *>(gb + 4);
  const float v[8] = {y0.x + g0.x, y0.y + g0.y, y0.z + g0.z, y0.w + g0.w, y1.x + g1.x, y1.y + g1.y, y1.z + g1.z, y1.w + g1.w};
  uint32_t hi[4], lo[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const float a = v[2 * k] > 0.0f ? v[2 * k] : 0.0f, c = v[2 * k + 1] > 0.0f ? v[2 * k + 1] : 0.0f;
    hi[k] = mf::pack_bf16x2(a, c);
    lo[k] = mf::pack_bf16x2(a - mf::bf16_lo(hi[k]), c - mf::bf16_hi(hi[k]));
  }
  const int g = n / G;  // (G % 8 == 0: the eight channels belong to one head)
  uint16_t *dst = out + m * ldo + (int64_t)2 * G * g + (n - g * G);
  *reinterpret_cast<uint4 *>(dst) = make_uint4(hi[0], hi[1], hi[2], hi[3]);
  *reinterpret_cast<uint4 *>(dst + G) = make_uint4(lo[0], lo[1], lo[2], lo[3]);
}

// rows of the network: B objects of P points, at most INT32_MAX in all
bool rows_ok(int32_t B, int32_t P) { return B > 0 && P > 0 && (int64_t)B * P <= INT32_MAX; }

constexpr int kMaxFg = MF_PCDNET_MAX_FG;
int64_t up256(int64_t v) { return (v + 255) & ~(int64_t)255; }

}  // namespace

extern "C" int32_t mf_pcdnet_workspace_offsets(int32_t B, int32_t P, int32_t n_fg, int64_t *offsets) {
  if (!rows_ok(B, P) || n_fg < 1 || n_fg > kMaxFg || !offsets) return -1;
  const int64_t M = (int64_t)B * P, np4 = (4 * (int64_t)n_fg + 7) / 8 * 8;
  const int64_t bytes[MF_PCDNET_WS_BUFFERS] = {
      M * 3 * 4,             // 0 pts     fp32 [M][3]
      M * 256 * 2,           // 1 f1      bf16 [M][256]
      M * 768 * 2,           // 2 xs      bf16 [M][768]
      M * 1024 * 2,          // 3 h3      bf16 [M][1024]
      M * 1024 * 4,          // 4 h4      fp32 [M][1024]
      (int64_t)B * 1024 * 4, // 5 pooled  fp32 [B][1024]
      (int64_t)B * 1920 * 4, // 6 gbias   fp32 [B][1920]
      M * 1920 * 4,          // 7 y       fp32 [M][1920]
      M * 3840 * 2,          // 8 h1      bf16 [M][3840]
      M * 1536 * 2,          // 9 h2      bf16 [M][1536]
      M * 768 * 2,           // 10 h3h    bf16 [M][768]
      M * 3 * np4 * 4,       // 11 o      fp32 [M][3 np4]
  };
  int64_t at = 0;
  for (int i = 0; i < MF_PCDNET_WS_BUFFERS; ++i) {
    offsets[i] = at;
    at += up256(bytes[i]);
  }
  offsets[MF_PCDNET_WS_BUFFERS] = at;
  return MF_PCDNET_WS_BUFFERS;
}

extern "C" int64_t mf_pcdnet_workspace_bytes(int32_t B, int32_t P, int32_t n_fg) {
  int64_t off[MF_PCDNET_WS_BUFFERS + 1];
  if (mf_pcdnet_workspace_offsets(B, P, n_fg, off) < 0) return -1;
  return off[MF_PCDNET_WS_BUFFERS];
}

extern "C" int mf_pcdnet_stem(const float *x_rows, const float *pcd, const int64_t *pix, const float *center,
                              const float *w_rgb, const float *b_rgb, const float *w_pcd, const float *b_pcd, int32_t B,
                              int32_t P, int32_t HW, float *pts, void *f1, int32_t ld1, void *xs, int32_t ldx,
                              int32_t losx, mfStream_t stream) {
  if (!rows_ok(B, P) || HW <= 0) return bad("mf_pcdnet_stem: B, P, HW >= 1 and B * P <= INT32_MAX");
  if (ld1 < 256 || ld1 % 8 || ldx % 8 || losx < 128 || losx % 8 || ldx < losx + 128 ||
      (((uintptr_t)x_rows | (uintptr_t)f1 | (uintptr_t)xs) & 15))
    return bad("mf_pcdnet_stem: pitches multiples of 8, ld1 >= 256, ldx >= losx + 128, losx >= 128; 16-byte aligned rows");
  const int M = B * P;
  hipLaunchKernelGGL(k_pcd_stem, dim3((unsigned)((M + kStemRows - 1) / kStemRows)), dim3(256), 0, (hipStream_t)stream,
                     x_rows, pcd, pix, center, w_rgb, b_rgb, w_pcd, b_pcd, M, (int)P, (int)HW, pts, (uint16_t *)f1,
                     (int)ld1, (uint16_t *)xs, (int)ldx, (int)losx);
  return mf::check_launch("mf_pcdnet_stem");
}

extern "C" int mf_pcdnet_pool(const float *h, int64_t ldh, int32_t B, int32_t P, int32_t C, float *pooled,
                              mfStream_t stream) {
  if (!rows_ok(B, P) || B > 65535) return bad("mf_pcdnet_pool: 1 <= B <= 65535, P >= 1 and B * P <= INT32_MAX");
  if (C <= 0 || C % kPoolChans || ldh < C || ldh % 4)
    return bad("mf_pcdnet_pool: C a multiple of 64, row pitch >= C and a multiple of 4");
  hipLaunchKernelGGL(k_pcd_pool, dim3((unsigned)(C / kPoolChans), (unsigned)B), dim3(kPoolLanes * kPoolChans), 0,
                     (hipStream_t)stream, h, ldh, (int)P, (int)C, pooled);
  return mf::check_launch("mf_pcdnet_pool");
}

extern "C" int mf_pcdnet_bias_relu_split(const float *y, int64_t ldy, const float *gbias, int32_t B, int32_t P,
                                         int32_t N, int32_t G, void *out, int64_t ldo, mfStream_t stream) {
  if (!rows_ok(B, P)) return bad("mf_pcdnet_bias_relu_split: B, P >= 1 and B * P <= INT32_MAX");
  if (N <= 0 || G <= 0 || G % 8 || N % G || ldy < N || ldy % 4 || ldo < 2 * (int64_t)N || ldo % 8 ||
      (((uintptr_t)y | (uintptr_t)gbias | (uintptr_t)out) & 15))
    return bad("mf_pcdnet_bias_relu_split: G % 8 == 0, N a multiple of G, ldy >= N and % 4 == 0, ldo >= 2 N and % 8 == 0, "
               "16-byte aligned operands");
  const int64_t M = (int64_t)B * P, total = M * (N / 8);
  if ((total + 255) / 256 > INT32_MAX) return bad("mf_pcdnet_bias_relu_split: more than 2^31 - 1 workgroups");
  hipLaunchKernelGGL(k_pcd_bias_split, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, y, ldy,
                     gbias, M, (int)P, (int)N, (int)G, (uint16_t *)out, ldo);
  return mf::check_launch("mf_pcdnet_bias_relu_split");
}
