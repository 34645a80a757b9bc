// NT engine of the bf16 GEMMs: NtArgs, the conv2_store8 epilogue, k_gemm_nt_bf16 and its 256 x 256 ping-pong form.
// A piece of csrc/gemm_bf16.hip's single translation unit: included there, in the order of that file, nowhere else.
#pragma once
#include "mf_common.h"

namespace {

using mf::mf_f32x16;

constexpr int kBN = 128, kBK = 64;
constexpr int kPitch = 144;  // bytes per LDS row (64 bf16 + 16 bytes)
template <int MI> constexpr int nt_buf_bytes() { return (64 * MI + kBN) * kPitch; }
template <int MI> constexpr int nt_lds() {
  return 2 * nt_buf_bytes<MI>() > 64 * MI * (kBN + 4) * 4 ? 2 * nt_buf_bytes<MI>() : 64 * MI * (kBN + 4) * 4;
}

enum { kRows = 0, kConvFwd = 1, kConvDgrad = 2, kConv2Fwd = 3, kConvFwdS = 4, kRowsS = 5 };
// kConvFwdS / kRowsS: the 3-D convolution and the rows loader on SPLIT operands (see NtArgs::xc): same addressing as
// their plain forms but for the source-channel wrap, and the kConv2Fwd epilogue (conv2_store8).
constexpr bool nt_conv3(int mode) { return mode == kConvFwd || mode == kConvFwdS; }
constexpr bool nt_rows(int mode) { return mode == kRows || mode == kRowsS; }
constexpr bool nt_split(int mode) { return mode == kConv2Fwd || mode == kConvFwdS || mode == kRowsS; }

struct NtArgs {
  const uint16_t *A;   // bf16 operand (rows / channels-last grid / channels-last output gradient)
  const uint16_t *W;   // bf16 [N][ldw] k-contiguous; group g at W + g * w_gs; dgrad: class p at W + p * N * ldw
  const float *bias;   // fp32 [N] or null; group g at bias + g * b_gs
  void *out;           // bf16 or fp32 rows, pitch ldo (elements); group g at out + g * o_gs
  int64_t a_gs, w_gs, b_gs, o_gs;
  int M, N, K, lda, ldw, ldo, groups;
  int relu, out_f32, accumulate;
  // rows mode only: weight group of every 64-row block of A (device array, -1 = no rows: the tile exits).  Row
  // tiles must not straddle groups (the producer pads each group to a multiple of 128 rows): the compact
  // parity-class rows of the sparse conv3 (csrc/sparseconv_bf16.hip) multiply their class's weight slice.
  const int32_t *tile_group;
  // conv geometry: D = INPUT grid size, Do = OUTPUT grid size = 1 << olog; forward taps ks^3 at x = stride * o - pad
  // + dil * k per axis (dgrad: the k4 / s2 / p1 parity-class form only)
  int B, D, Do, olog, Cin, Cout, ks, stride, pad, dil;
  // k_gemm_nt_bf16_pp only: S > 1 splits the K-tiles into S contiguous ranges; split s writes its fp32 partial
  // sums (no bias / ReLU) to slab + s * M * N (row pitch N), k_splitk_finish adds them in order
  int S;
  float *slab;
  // 2-D split-bf16 convolution (kConv2Fwd, mf_conv2d_split_fwd): the input is [B][D][D][xc] bf16 with xc = 2 C (hi
  // plane, then lo plane); Cin = 3 C is the K length of one tap, whose source channel is k mod xc (segments
  // [hi | lo | hi] against the packed weights [w_hi | w_hi | w_lo]).  Epilogue (conv2_store8):
  //   v = act(acc + bias[n] + res[m][n])   act: 0 none, 1 ReLU, 2 PReLU with the single slope *slope
  //   out32[m][n] = v (pitch ldo32), outs[m][n] = bf16(v), outs[m][los + n] = bf16(v - bf16(v)) (pitch ldos)
  // kConvFwdS (mf_conv3d_k4s2_split_fwd): the same for a grid [B][D^3][xc]; kRowsS (mf_linear_split_fwd): A rows
  // [hi | lo] of xc = 2 Kp columns at pitch lda, K = 3 Kp, chunk k reads column k mod xc.  Both: groups = 1.
  int xc, act, ldr, ldo32, ldos, los;
  const float *res, *slope;
  float *out32;
  uint16_t *outs;
  int dbg;  // k_gemm_nt_bf16_pp ablations (MF_PP_DBG; timing experiments only, results are wrong): see read_knobs
};

// The kConv2Fwd epilogue of eight columns n .. n + 7 of output row m (N % 8 == 0; every pitch a multiple of 8 and every
// pointer 16-byte aligned: checked by mf_conv2d_split_fwd).  hi = bf16(v) and lo = bf16(v - hi), both round-to-nearest-
// even; v - hi is exact in fp32.
__device__ __forceinline__ void conv2_store8(const NtArgs &a, int64_t m, int n, float *v) {
  if (a.bias) {
    const float4 b0 = *reinterpret_cast<const float4 *>(a.bias + n), b1 = *reinterpret_cast<const float4 *>(a.bias + n + 4);
    v[0] += b0.x; v[1] += b0.y; v[2] += b0.z; v[3] += b0.w; v[4] += b1.x; v[5] += b1.y; v[6] += b1.z; v[7] += b1.w;
  }
  if (a.res) {
    const float *r = a.res + m * a.ldr + n;
    const float4 r0 = *reinterpret_cast<const float4 *>(r), r1 = *reinterpret_cast<const float4 *>(r + 4);
    v[0] += r0.x; v[1] += r0.y; v[2] += r0.z; v[3] += r0.w; v[4] += r1.x; v[5] += r1.y; v[6] += r1.z; v[7] += r1.w;
  }
  if (a.act) {
    const float s = a.act == 2 ? *a.slope : 0.0f;
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = v[j] > 0.0f ? v[j] : s * v[j];
  }
  if (a.out32) {
    float4 *o = reinterpret_cast<float4 *>(a.out32 + m * a.ldo32 + n);
    o[0] = make_float4(v[0], v[1], v[2], v[3]);
    o[1] = make_float4(v[4], v[5], v[6], v[7]);
  }
  if (a.outs) {
    uint32_t h[8], l[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      h[j] = mf::bf16_bits(v[j]);
      l[j] = mf::bf16_bits(v[j] - mf::bf16_lo(h[j]));
    }
    uint16_t *o = a.outs + m * a.ldos + n;
    *reinterpret_cast<uint4 *>(o) = make_uint4(h[0] | h[1] << 16, h[2] | h[3] << 16, h[4] | h[5] << 16, h[6] | h[7] << 16);
    *reinterpret_cast<uint4 *>(o + a.los) =
        make_uint4(l[0] | l[1] << 16, l[2] | l[3] << 16, l[4] | l[5] << 16, l[6] | l[7] << 16);
  }
}

template <int MODE, int MI>
__global__ __launch_bounds__(256, 2) void k_gemm_nt_bf16(NtArgs a) {
  MF_DYN_LDS(unsigned char, s_raw);
  constexpr int kBM = 64 * MI, kBuf = nt_buf_bytes<MI>();
  const int tiles_m = (a.M + kBM - 1) / kBM, tiles_n = (a.N + kBN - 1) / kBN;
  const int per_group = tiles_m * tiles_n;
  const int G = gridDim.x;
  int L = blockIdx.x;
  if ((G & 7) == 0) L = (blockIdx.x & 7) * (G >> 3) + (blockIdx.x >> 3);  // XCD-contiguous logical order
  const int grp = L / per_group;
  const int rem = L - grp * per_group;
  const int m0 = (rem / tiles_n) * kBM, n0 = (rem % tiles_n) * kBN;  // N tile fastest (csrc/linear.hip)
  const int T = (a.K + kBK - 1) / kBK;

  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int wm = wave & 1, wn = wave >> 1;
  const int lrow = lane & 31, lhalf = lane >> 5;
  const int chunk = tid & 7, r0 = tid >> 3;  // this lane stages rows r0 + 32 i, bf16 8 chunk .. + 7 of the K-tile

  const int Do = a.Do, dol = a.olog;
  const uint16_t *A = a.A + grp * a.a_gs;
  const uint16_t *W = a.W + grp * a.w_gs;
  if (MODE == kRows && a.tile_group) {
    const int g = a.tile_group[m0 >> 6];  // (block-uniform)
    if (g < 0) return;
    W += (int64_t)g * a.w_gs;
  }
  int cls = 0;
  if (MODE == kConvDgrad) {  // tile-uniform parity class: its weight slice
    cls = (m0 >> (3 * dol)) & 7;
    W += (int64_t)cls * a.N * a.ldw;
  }
  // per staged row: element offset of its k = 0 chunk and validity bits
  //   rows:        bit 12 = row exists
  //   conv fwd:    bits kx | 4 + ky | 8 + kz = tap coordinate inside the grid (csrc/conv3d.hip)
  //   conv dgrad:  bits sx | 4 + sy | 8 + sz = contributing output voxel h + p - s inside the output grid
  int base[2 * MI], mask[2 * MI];
#pragma unroll
  for (int i = 0; i < 2 * MI; ++i) {
    const int m = m0 + r0 + 32 * i;
    const bool row_ok = m < a.M;
    const int mm = row_ok ? m : 0;
    int mk = row_ok ? 1 << 12 : 0;
    if (nt_rows(MODE)) {
      base[i] = mm * a.lda;
    } else if (MODE == kConv2Fwd) {  // row m = (b, oy, ox); bits ky | 4 + kx = tap row / column inside the map
      const int b = mm >> (2 * dol), o = mm & ((1 << (2 * dol)) - 1);
      const int y0 = a.stride * (o >> dol) - a.pad, x0 = a.stride * (o & (Do - 1)) - a.pad;
      base[i] = ((b * a.D + y0) * a.D + x0) * a.xc;
#pragma unroll
      for (int k = 0; k < 4; ++k) {  // (k >= ks: never asked for)
        mk |= ((unsigned)(y0 + a.dil * k) < (unsigned)a.D ? 1 : 0) << k;
        mk |= ((unsigned)(x0 + a.dil * k) < (unsigned)a.D ? 1 : 0) << (4 + k);
      }
    } else if (nt_conv3(MODE)) {
      const int b = mm >> (3 * dol), o = mm & ((1 << (3 * dol)) - 1);
      const int ox = o >> (2 * dol), oy = (o >> dol) & (Do - 1), oz = o & (Do - 1);
      const int x0 = a.stride * ox - a.pad, y0 = a.stride * oy - a.pad, z0 = a.stride * oz - a.pad;
      base[i] = (((b * a.D + x0) * a.D + y0) * a.D + z0) * (MODE == kConvFwdS ? a.xc : a.Cin);
#pragma unroll
      for (int k = 0; k < 4; ++k) {  // (k >= ks: never asked for)
        mk |= ((unsigned)(x0 + a.dil * k) < (unsigned)a.D ? 1 : 0) << k;
        mk |= ((unsigned)(y0 + a.dil * k) < (unsigned)a.D ? 1 : 0) << (4 + k);
        mk |= ((unsigned)(z0 + a.dil * k) < (unsigned)a.D ? 1 : 0) << (8 + k);
      }
    } else {
      // m = ((b * 8 + p) * Do^3 + h): input voxel x = 2 h + p per axis
      const int h = mm & ((1 << (3 * dol)) - 1), b = mm >> (3 * dol + 3);
      const int hx = h >> (2 * dol), hy = (h >> dol) & (Do - 1), hz = h & (Do - 1);
      const int ux = hx + (cls & 1), uy = hy + ((cls >> 1) & 1), uz = hz + ((cls >> 2) & 1);  // slot (0,0,0)
      base[i] = (((b * Do + ux) * Do + uy) * Do + uz) * a.Cout;
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        mk |= ((unsigned)(ux - s) < (unsigned)Do ? 1 : 0) << s;
        mk |= ((unsigned)(uy - s) < (unsigned)Do ? 1 : 0) << (4 + s);
        mk |= ((unsigned)(uz - s) < (unsigned)Do ? 1 : 0) << (8 + s);
      }
    }
    mask[i] = mk;
  }
  uint32_t wrow[4];  // byte offsets into W (weights: far below 2^32 bytes)
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int n = n0 + r0 + 32 * i;
    wrow[i] = 2u * (uint32_t)((int64_t)(n < a.N ? n : 0) * a.ldw);
  }

  mf_f32x16 acc[MI][2];
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.0f;

  // K-tile kt -> registers.  Nothing touches the loaded data before the stash: a select right behind a load would
  // make the wave wait for its own data at once (s_waitcnt vmcnt(0) in front of the MFMAs) and the prefetch would
  // hide nothing.
  // (Scalars and macros, not arrays in lambdas: behind the "memory" clobber that pins the loads in front of the MFMAs,
  // arrays captured by reference were kept in scratch memory -- every load waited for and stored.)
  // ONE register set, one tile ahead.  (Two sets -- tile t + 2 in flight while t + 1 waits -- were measured twice in
  // round 4, before and after the VALU diet: no gain on any shape, 90 more registers.)
  uint4 ra0P, ra1P, ra2P = make_uint4(0u, 0u, 0u, 0u), ra3P = ra2P, rb0P, rb1P, rb2P, rb3P;
  // This lane's position in K, advanced by one K-tile per fetch (the fetches run over kt = 0, 1, 2, ... in order): the
  // chunk's k offset and, for the convolutions, its (tap, channel) -- tracked incrementally (round 4, first version:
  // two integer divisions per fetch and 64-bit address arithmetic per load, 12 VALU instructions per MFMA by
  // SQ_INSTS_VALU; the MFMA pipe at 0.37).
  int kg = 8 * chunk, tc = 0, tx = 0, ty = 0, tz = 0;  // conv fwd: tap (tx, ty, tz), channel tc; dgrad: slot tx, cout tc
  if (nt_conv3(MODE)) {
    const int tap = kg / a.Cin;
    tc = kg - tap * a.Cin;
    const int kxy = tap / a.ks;
    tz = tap - kxy * a.ks; tx = kxy / a.ks; ty = kxy - tx * a.ks;
  } else if (MODE == kConv2Fwd) {  // tap (ky, kx) = (tx, ty), position tc in the tap's 3 C
    const int tap = kg / a.Cin;
    tc = kg - tap * a.Cin;
    tx = tap / a.ks; ty = tap - tx * a.ks;
  } else if (MODE == kConvDgrad) {
    tx = kg / a.Cout;
    tc = kg - tx * a.Cout;
  }
  // A masked chunk (padding tap, row past the edge, K tail) is a buffer load at an OUT-OF-RANGE offset: the hardware
  // returns zeros (mf_common.h).  No select or AND on the loaded data (that was 44 VALU instructions per K-tile in
  // every wave that touches a border -- nearly all of them in a 16^3 grid), and the stash is eight plain
  // ds_write_b128.  The weight operand needs no mask at all: behind the K tail it re-reads k = 0 (finite; the A chunk
  // there is zero), and a column past N re-reads row 0 into an accumulator column the epilogue never stores.
  const mf::BufRsrc Ars = mf::make_rsrc(A), Wrs = mf::make_rsrc(W);
#define MF_NT_LOAD_A(S, i_, reg_)                                                                     \
  reg_ = mf::buf_load16(Ars, (mask[i_] & bits_) == bits_ ? 2u * (uint32_t)(base[i_] + off_) : mf::kBufMasked);
#define MF_NT_LOAD_B(S, i_, reg_) reg_ = mf::buf_load16(Wrs, wrow[i_] + kofs_);
#define MF_NT_FETCH(S)                                                                                \
  {                                                                                                   \
    const bool kin_ = kg + 8 <= a.K;                                                                  \
    const uint32_t kofs_ = kin_ ? 2u * (uint32_t)kg : 0u;                                             \
    int off_ = MODE == kRowsS && kg >= a.xc ? kg - a.xc : kg, bits_ = 1 << 12;                        \
    if (nt_conv3(MODE)) {                                                                             \
      off_ = ((tx * a.D + ty) * a.D + tz) * a.dil * (MODE == kConvFwdS ? a.xc : a.Cin) +              \
             (MODE == kConvFwdS && tc >= a.xc ? tc - a.xc : tc);                                      \
      bits_ = tx < a.ks ? (1 << tx) | (16 << ty) | (256 << tz) | (1 << 12) : 1 << 13;                 \
    } else if (MODE == kConv2Fwd) {                                                                   \
      off_ = (tx * a.D + ty) * a.dil * a.xc + (tc >= a.xc ? tc - a.xc : tc);                          \
      bits_ = tx < a.ks ? (1 << tx) | (16 << ty) | (1 << 12) : 1 << 13;                               \
    } else if (MODE == kConvDgrad) {                                                                  \
      const int sx = tx & 1, sy = (tx >> 1) & 1, sz = tx >> 2;                                        \
      off_ = tc - ((sx * Do + sy) * Do + sz) * a.Cout;                                                \
      bits_ = (1 << sx) | (16 << sy) | (256 << sz) | (1 << 12);                                       \
    }                                                                                                 \
    if (!kin_) bits_ = 1 << 13; /* (no row has bit 13) */                                             \
    MF_NT_LOAD_A(S, 0, ra0##S) MF_NT_LOAD_A(S, 1, ra1##S)                                             \
    if constexpr (MI == 2) { MF_NT_LOAD_A(S, 2 * MI - 2, ra2##S) MF_NT_LOAD_A(S, 2 * MI - 1, ra3##S) } \
    MF_NT_LOAD_B(S, 0, rb0##S) MF_NT_LOAD_B(S, 1, rb1##S) MF_NT_LOAD_B(S, 2, rb2##S) MF_NT_LOAD_B(S, 3, rb3##S) \
    kg += kBK;                                                                                        \
    if (nt_conv3(MODE)) {                                                                             \
      tc += kBK;                                                                                      \
      while (tc >= a.Cin) {                                                                           \
        tc -= a.Cin;                                                                                  \
        if (++tz == a.ks) { tz = 0; if (++ty == a.ks) { ty = 0; ++tx; } }                             \
      }                                                                                               \
    } else if (MODE == kConv2Fwd) {                                                                   \
      tc += kBK;                                                                                      \
      while (tc >= a.Cin) {                                                                           \
        tc -= a.Cin;                                                                                  \
        if (++ty == a.ks) { ty = 0; ++tx; }                                                           \
      }                                                                                               \
    } else if (MODE == kConvDgrad) {                                                                  \
      tc += kBK;                                                                                      \
      while (tc >= a.Cout) { tc -= a.Cout; ++tx; }                                                    \
    }                                                                                                 \
  }
  // (MF_HOLD: the staged registers stay opaque until here, BEHIND the MFMAs -- and with them the wait for the loads.)
#define MF_NT_STASH(S, buf_)                                                                          \
  {                                                                                                   \
    MF_HOLD(ra0##S); MF_HOLD(ra1##S); MF_HOLD(rb0##S); MF_HOLD(rb1##S); MF_HOLD(rb2##S); MF_HOLD(rb3##S); \
    if constexpr (MI == 2) { MF_HOLD(ra2##S); MF_HOLD(ra3##S); }                                      \
    unsigned char *As_ = s_raw + (buf_) * kBuf + r0 * kPitch + 16 * chunk;                            \
    unsigned char *Bs_ = As_ + kBM * kPitch;                                                          \
    *reinterpret_cast<uint4 *>(As_) = ra0##S; *reinterpret_cast<uint4 *>(As_ + 32 * kPitch) = ra1##S; \
    if constexpr (MI == 2) {                                                                          \
      *reinterpret_cast<uint4 *>(As_ + 64 * kPitch) = ra2##S; *reinterpret_cast<uint4 *>(As_ + 96 * kPitch) = ra3##S; \
    }                                                                                                 \
    *reinterpret_cast<uint4 *>(Bs_) = rb0##S; *reinterpret_cast<uint4 *>(Bs_ + 32 * kPitch) = rb1##S; \
    *reinterpret_cast<uint4 *>(Bs_ + 64 * kPitch) = rb2##S; *reinterpret_cast<uint4 *>(Bs_ + 96 * kPitch) = rb3##S; \
  }
  // NJ_ = 2: both 32-column blocks of the wave's 64 columns; NJ_ = 1: the first only (the second lies past N).
  // The fragments of k-step s + 1 are read while the MFMAs of step s run (round 5: two
  // register sets, the order pinned with sched_group_barrier; MF_NT_PIPE=0: the scheduler's own order).
#ifndef MF_NT_PIPE
#define MF_NT_PIPE 1
#endif
#define MF_NT_FRAGS(set_, s_, NJ_)                                                                    \
  {                                                                                                   \
    fa[set_][0] = *reinterpret_cast<const uint4 *>(As + 32 * (s_));                                   \
    if constexpr (MI == 2) fa[set_][1] = *reinterpret_cast<const uint4 *>(As + 32 * kPitch + 32 * (s_)); \
    fb[set_][0] = *reinterpret_cast<const uint4 *>(Bs + 32 * (s_));                                   \
    if constexpr (NJ_ == 2) fb[set_][1] = *reinterpret_cast<const uint4 *>(Bs + 32 * kPitch + 32 * (s_)); \
  }
#define MF_NT_COMPUTE(buf_, NJ_)                                                                      \
  {                                                                                                   \
    asm volatile("" ::: "memory");                                                                    \
    __builtin_amdgcn_sched_barrier(0);                                                                \
    const unsigned char *As = s_raw + (buf_) * kBuf + (wm * 32 * MI + lrow) * kPitch + 16 * lhalf;    \
    const unsigned char *Bs = s_raw + (buf_) * kBuf + (kBM + wn * 64 + lrow) * kPitch + 16 * lhalf;   \
    if constexpr (MF_NT_PIPE) {                                                                       \
      uint4 fa[2][2], fb[2][2];                                                                       \
      MF_NT_FRAGS(0, 0, NJ_)                                                                          \
      __builtin_amdgcn_sched_group_barrier(0x100, MI + NJ_, 0);                                       \
      _Pragma("unroll") for (int s = 0; s < 4; ++s) {                                                 \
        const int c = s & 1;                                                                          \
        if (s < 3) MF_NT_FRAGS(c ^ 1, s + 1, NJ_)                                                     \
        _Pragma("unroll") for (int mi = 0; mi < MI; ++mi) {                                           \
          acc[mi][0] = mf::mfma_bf16_32x32x16(fa[c][mi], fb[c][0], acc[mi][0]);                       \
          if constexpr (NJ_ == 2) acc[mi][1] = mf::mfma_bf16_32x32x16(fa[c][mi], fb[c][1], acc[mi][1]); \
        }                                                                                             \
        if (s < 3) __builtin_amdgcn_sched_group_barrier(0x100, MI + NJ_, 0);                          \
        __builtin_amdgcn_sched_group_barrier(0x008, MI * NJ_, 0);                                     \
      }                                                                                               \
    } else {                                                                                          \
      _Pragma("unroll") for (int s = 0; s < 4; ++s) {                                                 \
        const uint4 a0 = *reinterpret_cast<const uint4 *>(As + 32 * s);                               \
        const uint4 b0 = *reinterpret_cast<const uint4 *>(Bs + 32 * s);                               \
        acc[0][0] = mf::mfma_bf16_32x32x16(a0, b0, acc[0][0]);                                        \
        if constexpr (NJ_ == 2) {                                                                     \
          const uint4 b1 = *reinterpret_cast<const uint4 *>(Bs + 32 * kPitch + 32 * s);               \
          acc[0][1] = mf::mfma_bf16_32x32x16(a0, b1, acc[0][1]);                                      \
          if constexpr (MI == 2) {                                                                    \
            const uint4 a1 = *reinterpret_cast<const uint4 *>(As + 32 * kPitch + 32 * s);             \
            acc[MI - 1][0] = mf::mfma_bf16_32x32x16(a1, b0, acc[MI - 1][0]);                          \
            acc[MI - 1][1] = mf::mfma_bf16_32x32x16(a1, b1, acc[MI - 1][1]);                          \
          }                                                                                           \
        } else if constexpr (MI == 2) {                                                               \
          const uint4 a1 = *reinterpret_cast<const uint4 *>(As + 32 * kPitch + 32 * s);               \
          acc[MI - 1][0] = mf::mfma_bf16_32x32x16(a1, b0, acc[MI - 1][0]);                            \
        }                                                                                             \
      }                                                                                               \
    }                                                                                                 \
    __builtin_amdgcn_sched_barrier(0);                                                                \
  }
  // Column blocks of this wave that lie past N (the last N-tile of a layer whose width is not a multiple of 128:
  // conv3's data gradient has N = 160 -- its second tile holds 32 columns) are not multiplied: wave-uniform.
  const int ncols = a.N - (n0 + wn * 64);  // columns of this wave's 64 that exist
  // Per K-tile t: the loads of tile t + 1 are issued, tile t is multiplied, the registers go into the other buffer,
  // barrier.  (Stash AFTER the barrier and the next fetch right behind it -- the order the 256^2-tile GEMMs of the
  // programming guide prefer -- measured 3 - 5 % slower here, at 2 workgroups per CU.)  The fetches run over the
  // K-tiles in order, one past the last (k beyond K: every chunk masked, zeros into the buffer nobody reads again) --
  // NOT under "if (t + 1 < T)": behind a branch the compiler copies the loaded registers at the join and waits for
  // the loads right where they are issued (measured: 2x slower).
  MF_NT_FETCH(P);  // tile 0
  MF_NT_STASH(P, 0);
  __syncthreads();
  for (int t = 0; t < T; ++t) {
    MF_NT_FETCH(P);  // tile t + 1 in flight under the MFMAs of tile t
    if (ncols > 32) MF_NT_COMPUTE(t & 1, 2) else if (ncols > 0) MF_NT_COMPUTE(t & 1, 1)
    MF_NT_STASH(P, (t + 1) & 1);
    __syncthreads();
  }
#undef MF_NT_FRAGS
#undef MF_NT_COMPUTE
#undef MF_NT_STASH
#undef MF_NT_FETCH
#undef MF_NT_LOAD_B
#undef MF_NT_LOAD_A

  // epilogue through LDS (the loop ended on a barrier: the operand buffers are free)
  constexpr int kEp = kBN + 4;
  float *s_out = reinterpret_cast<float *>(s_raw);  // [kBM][kEp]
  const float *bias = a.bias && !nt_split(MODE) ? a.bias + grp * a.b_gs : nullptr;  // (conv2: conv2_store8)
#pragma unroll
  for (int mi = 0; mi < MI; ++mi)
#pragma unroll
    for (int ni = 0; ni < 2; ++ni) {
      const int nl = wn * 64 + ni * 32 + lrow;
      const float bn = (bias && n0 + nl < a.N) ? bias[n0 + nl] : 0.0f;
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int ml = wm * 32 * MI + mi * 32 + (e & 3) + 8 * (e >> 2) + 4 * lhalf;
        float v = acc[mi][ni][e] + bn;
        if (a.relu && !nt_split(MODE)) v = v > 0.0f ? v : 0.0f;
        s_out[ml * kEp + nl] = v;
      }
    }
  __syncthreads();
  for (int i = tid; i < kBM * (kBN / 8); i += 256) {
    const int ml = i / (kBN / 8), c8 = i - ml * (kBN / 8);
    const int m = m0 + ml, n = n0 + 8 * c8;
    if (m >= a.M || n >= a.N) continue;
    int64_t orow = m;
    if (MODE == kConvDgrad) {  // class-ordered row -> channels-last voxel row of the input gradient
      const int h = m & ((1 << (3 * dol)) - 1), p = (m >> (3 * dol)) & 7, b = m >> (3 * dol + 3);
      const int x = 2 * (h >> (2 * dol)) + (p & 1), y = 2 * ((h >> dol) & (Do - 1)) + ((p >> 1) & 1),
                z = 2 * (h & (Do - 1)) + (p >> 2);
      orow = (((int64_t)b * a.D + x) * a.D + y) * a.D + z;
    }
    const float4 v0 = *reinterpret_cast<const float4 *>(s_out + ml * kEp + 8 * c8);
    const float4 v1 = *reinterpret_cast<const float4 *>(s_out + ml * kEp + 8 * c8 + 4);
    float v[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
    if (nt_split(MODE)) {
      conv2_store8(a, m, n, v);
      continue;
    }
    const int nv = a.N - n < 8 ? a.N - n : 8;
    if (a.out_f32) {
      float *o = reinterpret_cast<float *>(a.out) + grp * a.o_gs + orow * a.ldo + n;
      if (nv == 8 && (a.ldo & 3) == 0 && ((uintptr_t)o & 15) == 0) {
        float4 *o4 = reinterpret_cast<float4 *>(o);
        if (a.accumulate) {
          const float4 p0 = o4[0], p1 = o4[1];
          v[0] += p0.x; v[1] += p0.y; v[2] += p0.z; v[3] += p0.w;
          v[4] += p1.x; v[5] += p1.y; v[6] += p1.z; v[7] += p1.w;
        }
        o4[0] = make_float4(v[0], v[1], v[2], v[3]);
        o4[1] = make_float4(v[4], v[5], v[6], v[7]);
      } else {
        for (int j = 0; j < nv; ++j) o[j] = a.accumulate ? o[j] + v[j] : v[j];
      }
    } else {
      uint16_t *o = reinterpret_cast<uint16_t *>(a.out) + grp * a.o_gs + orow * a.ldo + n;
      if (nv == 8 && (a.ldo & 7) == 0 && ((uintptr_t)o & 15) == 0) {
        *reinterpret_cast<uint4 *>(o) = make_uint4(mf::pack_bf16x2(v[0], v[1]), mf::pack_bf16x2(v[2], v[3]),
                                                   mf::pack_bf16x2(v[4], v[5]), mf::pack_bf16x2(v[6], v[7]));
      } else {
        for (int j = 0; j < nv; ++j) o[j] = (uint16_t)mf::bf16_bits(v[j]);
      }
    }
  }
}

// ---- the 256 x 256 x 64 tile (round 5: eight waves, each a 128 x 64 corner = 4 x 2 accumulators) --------------------
// A wave of the 128 x 128 tile reads one LDS fragment (ds_read_b128) per MFMA: at the MFMA rate of gfx950 that alone
// keeps the LDS pipe busy all the time (1 KB per wave per 32-cycle MFMA, four SIMDs).  With a 128 x 64 wave tile a
// k-step reads 4 + 2 fragments for 8 MFMAs -- 0.75 per MFMA.  Round 5's form of this tile staged its operands through
// registers (global -> VGPR -> ds_write_b128, one barrier per K-tile: 852 / 961 TFLOP/s on conv3 forward / conv4 data
// gradient, MFMA pipe 0.43 busy); round 6's k_gemm_nt_bf16_pp below replaced it (1019-1059 / 1202-1225 in the same
// measurement) and the register-staged kernel is gone from the source.
constexpr int kBigM = 256, kBigN = 256;

// ---- the 256 x 256 x 64 tile with LDS-DMA operands and two wave groups in ping-pong (round 6) ------------------------
// Round 5's form of this tile moved every operand chunk global -> VGPR -> ds_write_b128 -> barrier, once per K-tile: all
// eight waves met at that barrier, waited out their loads, stored, and started reading fragments at the same moment --
// the MFMA pipe idled through every one of these episodes (0.42-0.43 busy).  Here
//   * operands go global -> LDS directly (buffer_load_dwordx4 ... lds, mf::glds16: 1 KiB = 8 tile rows per wave
//     instruction; masked chunks are out-of-range offsets and land as zeros): no staging registers, no store pass;
//   * the LDS image of an operand is [256 rows][128 bytes] with the 16-byte chunk index XORed with (row >> 1) & 7.  The
//     DMA writes a wave's 1 KiB lane-linear, so the swizzle is applied to the SOURCE: the lane whose slot is chunk
//     position q of row r fetches global chunk q ^ ((r >> 1) & 7); a fragment read (row = lane % 32, chunk
//     2 s + lane / 32) XORs the same value: every 16-lane group of a ds_read_b128 covers all 64 banks once;
//   * a K-tile is two phases of two k-steps: 12 fragment reads and 4 DMA requests in the phase's load section, 16
//     MFMAs in its MFMA section, a barrier behind each.  The waves with the upper and the lower 128 rows of the tile
//     (waves 0-3 / 4-7: one of each per SIMD) run ONE BARRIER APART: while one group multiplies (s_setprio 1) the
//     other reads the fragments of its next phase and issues DMA -- the SIMD's MFMA pipe always has a wave with
//     operands in registers, and the LDS round trip and the DMA issue time (60-180 cycles of the issuing wave per
//     request) are paid beside the other group's MFMAs;
//   * the 160 KiB of LDS are THREE A stages + TWO W stages (the weight panel is shared by every workgroup and comes
//     from L2; the activation rows come from HBM): in tile t, phase 0 requests W(t + 1) into the stage W(t - 1) was
//     read from, phase 1 requests A(t + 2) into the stage of A(t - 1) and then waits with a COUNTED vmcnt(4) --
//     everything but A(t + 2), which stays in flight across the barriers.
// Ordering, in barrier intervals (group 0's load section of phase (t, p) is interval 4 t + 2 p, its MFMA section
// 4 t + 2 p + 1; group 1 one interval later):
//   WAR  the last reads of tile t - 1 are group 1's phase (t - 1, 1) in interval 4 t - 1, retired by lgkmcnt(0) BEFORE
//        the barrier that ends it; the earliest request into a stage of tile t - 1 is group 0's in interval 4 t.
//   RAW  every wave waits for its own requests of A(t + 1) and W(t + 1) in the load section of its phase (t, 1)
//        (intervals 4 t + 2 / 4 t + 3) in front of a barrier; the first read of tile t + 1 is group 0's in 4 t + 4.
// The fragment reads are inline asm (mf::lds_read16_async): the compiler puts s_waitcnt vmcnt(0) in front of any LDS
// read it can see while a DMA is pending.  Same loaders, masks, tile order and epilogue as the kernel above.
constexpr int kPpOp = 256 * 128;             // bytes of one operand stage: [256 rows][128]
constexpr int kPpW0 = 3 * kPpOp;             // A stages at 0, 1, 2 x kPpOp; W stages behind them
constexpr int nt_pp_lds() { return 5 * kPpOp; }  // 160 KiB: all of a CU's LDS (the epilogue's 64 x 260 floats fit inside)

template <int MODE>
__global__ __launch_bounds__(512, 2) void k_gemm_nt_bf16_pp(NtArgs a) {
  MF_DYN_LDS(unsigned char, s_raw);
  constexpr int kBM = kBigM, kBNb = kBigN;
  const int tiles_m = (a.M + kBM - 1) / kBM, tiles_n = (a.N + kBNb - 1) / kBNb;
  const int per_group = tiles_m * tiles_n;
  const int G = gridDim.x;
  int L = blockIdx.x;
  if ((G & 7) == 0) L = (blockIdx.x & 7) * (G >> 3) + (blockIdx.x >> 3);  // XCD-contiguous logical order
  const int split = L / (per_group * a.groups);  // (0 unless a.S > 1: the splits of a tile are S whole rounds apart)
  L -= split * per_group * a.groups;
  const int grp = L / per_group;
  const int rem = L - grp * per_group;
  const int m0 = (rem / tiles_n) * kBM, n0 = (rem % tiles_n) * kBNb;  // N tile fastest (csrc/linear.hip)
  const int Tall = (a.K + kBK - 1) / kBK, Tper = (Tall + a.S - 1) / a.S;
  const int t0 = split * Tper;
  const int T = max(0, min(Tall, t0 + Tper) - t0);  // this workgroup's K-tiles: t0 .. t0 + T - 1

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = mf::wave_uniform(tid >> 6);
  const int wm = wave >> 2, wn = wave & 3;  // wm = the ping-pong group: waves w and w + 4 share a SIMD
  const int lrow = lane & 31, lhalf = lane >> 5;
  // DMA slot of this lane: tile rows r0 + 64 i, chunk position tid & 7 of the row -> global chunk ``chunk``
  const int r0 = tid >> 3;
  const int chunk = (tid & 7) ^ ((r0 >> 1) & 7);

  const int Do = a.Do, dol = a.olog;
  const uint16_t *A = a.A + grp * a.a_gs;
  const uint16_t *W = a.W + grp * a.w_gs;
  int cls = 0;
  if (MODE == kConvDgrad) {  // tile-uniform parity class: its weight slice
    cls = (m0 >> (3 * dol)) & 7;
    W += (int64_t)cls * a.N * a.ldw;
  }
  // per staged row: element offset of its k = 0 chunk and validity bits (as in k_gemm_nt_bf16)
  int base[4], mask[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int m = m0 + r0 + 64 * i;
    const bool row_ok = m < a.M;
    const int mm = row_ok ? m : 0;
    int mk = row_ok ? 1 << 12 : 0;
    if (nt_rows(MODE)) {
      base[i] = mm * a.lda;
    } else if (MODE == kConv2Fwd) {  // row m = (b, oy, ox); bits ky | 4 + kx = tap row / column inside the map
      const int b = mm >> (2 * dol), o = mm & ((1 << (2 * dol)) - 1);
      const int y0 = a.stride * (o >> dol) - a.pad, x0 = a.stride * (o & (Do - 1)) - a.pad;
      base[i] = ((b * a.D + y0) * a.D + x0) * a.xc;
#pragma unroll
      for (int k = 0; k < 4; ++k) {  // (k >= ks: never asked for)
        mk |= ((unsigned)(y0 + a.dil * k) < (unsigned)a.D ? 1 : 0) << k;
        mk |= ((unsigned)(x0 + a.dil * k) < (unsigned)a.D ? 1 : 0) << (4 + k);
      }
    } else if (nt_conv3(MODE)) {
      const int b = mm >> (3 * dol), o = mm & ((1 << (3 * dol)) - 1);
      const int ox = o >> (2 * dol), oy = (o >> dol) & (Do - 1), oz = o & (Do - 1);
      const int x0 = a.stride * ox - a.pad, y0 = a.stride * oy - a.pad, z0 = a.stride * oz - a.pad;
      base[i] = (((b * a.D + x0) * a.D + y0) * a.D + z0) * (MODE == kConvFwdS ? a.xc : a.Cin);
#pragma unroll
      for (int k = 0; k < 4; ++k) {  // (k >= ks: never asked for)
        mk |= ((unsigned)(x0 + a.dil * k) < (unsigned)a.D ? 1 : 0) << k;
        mk |= ((unsigned)(y0 + a.dil * k) < (unsigned)a.D ? 1 : 0) << (4 + k);
        mk |= ((unsigned)(z0 + a.dil * k) < (unsigned)a.D ? 1 : 0) << (8 + k);
      }
    } else {
      const int h = mm & ((1 << (3 * dol)) - 1), b = mm >> (3 * dol + 3);
      const int hx = h >> (2 * dol), hy = (h >> dol) & (Do - 1), hz = h & (Do - 1);
      const int ux = hx + (cls & 1), uy = hy + ((cls >> 1) & 1), uz = hz + ((cls >> 2) & 1);  // slot (0,0,0)
      base[i] = (((b * Do + ux) * Do + uy) * Do + uz) * a.Cout;
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        mk |= ((unsigned)(ux - s) < (unsigned)Do ? 1 : 0) << s;
        mk |= ((unsigned)(uy - s) < (unsigned)Do ? 1 : 0) << (4 + s);
        mk |= ((unsigned)(uz - s) < (unsigned)Do ? 1 : 0) << (8 + s);
      }
    }
    mask[i] = mk;
  }
  uint32_t wrow[4];  // byte offsets into W (weights: far below 2^32 bytes)
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int n = n0 + r0 + 64 * i;
    wrow[i] = 2u * (uint32_t)((int64_t)(n < a.N ? n : 0) * a.ldw);
  }

  mf_f32x16 acc[4][2];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.0f;

  // this lane's position in K, advanced by one K-tile per request (see k_gemm_nt_bf16); the A requests run one tile
  // ahead of the W requests
  int kg = 8 * chunk + kBK * t0, tc = 0, tx = 0, ty = 0, tz = 0, kgw = kg;
  if (nt_conv3(MODE)) {
    const int tap = kg / a.Cin;
    tc = kg - tap * a.Cin;
    const int kxy = tap / a.ks;
    tz = tap - kxy * a.ks; tx = kxy / a.ks; ty = kxy - tx * a.ks;
  } else if (MODE == kConv2Fwd) {  // tap (ky, kx) = (tx, ty), position tc in the tap's 3 C
    const int tap = kg / a.Cin;
    tc = kg - tap * a.Cin;
    tx = tap / a.ks; ty = tap - tx * a.ks;
  } else if (MODE == kConvDgrad) {
    tx = kg / a.Cout;
    tc = kg - tx * a.Cout;
  }
  const mf::BufRsrc Ars = mf::make_rsrc(A), Wrs = mf::make_rsrc(W);
  // the 1 KiB of LDS a DMA instruction of this wave fills: rows 64 i + 8 wave .. + 7 of an operand stage
  unsigned char *const dma0 = s_raw + 8 * wave * 128;
  // requests i0_ .. i1_ - 1 (rows 64 i .. + 63) of A's next K-tile -> A stage sa_; the position advances behind the last
#define MF_PP_REQ_A(sa_, i0_, i1_)                                                                    \
  {                                                                                                   \
    const bool kin_ = kg + 8 <= a.K;                                                                  \
    int off_ = MODE == kRowsS && kg >= a.xc ? kg - a.xc : kg, bits_ = 1 << 12;                        \
    if (nt_conv3(MODE)) {                                                                             \
      off_ = ((tx * a.D + ty) * a.D + tz) * a.dil * (MODE == kConvFwdS ? a.xc : a.Cin) +              \
             (MODE == kConvFwdS && tc >= a.xc ? tc - a.xc : tc);                                      \
      bits_ = tx < a.ks ? (1 << tx) | (16 << ty) | (256 << tz) | (1 << 12) : 1 << 13;                 \
    } else if (MODE == kConv2Fwd) {                                                                   \
      off_ = (tx * a.D + ty) * a.dil * a.xc + (tc >= a.xc ? tc - a.xc : tc);                          \
      bits_ = tx < a.ks ? (1 << tx) | (16 << ty) | (1 << 12) : 1 << 13;                               \
    } else if (MODE == kConvDgrad) {                                                                  \
      const int sx = tx & 1, sy = (tx >> 1) & 1, sz = tx >> 2;                                        \
      off_ = tc - ((sx * Do + sy) * Do + sz) * a.Cout;                                                \
      bits_ = (1 << sx) | (16 << sy) | (256 << sz) | (1 << 12);                                       \
    }                                                                                                 \
    if (!kin_) bits_ = 1 << 13; /* (no row has bit 13) */                                             \
    _Pragma("unroll") for (int i = (i0_); i < (i1_); ++i)                                             \
      mf::glds16(Ars, (mask[i] & bits_) == bits_ ? 2u * (uint32_t)(base[i] + off_) : mf::kBufMasked,  \
                 dma0 + (sa_) * kPpOp + i * 64 * 128);                                                \
    if ((i1_) == 4) {                                                                                 \
      kg += kBK;                                                                                      \
      if (nt_conv3(MODE)) {                                                                           \
        tc += kBK;                                                                                    \
        while (tc >= a.Cin) {                                                                         \
          tc -= a.Cin;                                                                                \
          if (++tz == a.ks) { tz = 0; if (++ty == a.ks) { ty = 0; ++tx; } }                           \
        }                                                                                             \
      } else if (MODE == kConv2Fwd) {                                                                 \
        tc += kBK;                                                                                    \
        while (tc >= a.Cin) {                                                                         \
          tc -= a.Cin;                                                                                \
          if (++ty == a.ks) { ty = 0; ++tx; }                                                         \
        }                                                                                             \
      } else if (MODE == kConvDgrad) {                                                                \
        tc += kBK;                                                                                    \
        while (tc >= a.Cout) { tc -= a.Cout; ++tx; }                                                  \
      }                                                                                               \
    }                                                                                                 \
  }
  // (the weight operand needs no mask: behind the K tail it re-reads k = 0 -- finite, and the A chunk there is zero --
  // and a column past N re-reads row 0 into an accumulator column the epilogue never stores)
#define MF_PP_REQ_W(sw_, i0_, i1_)                                                                    \
  {                                                                                                   \
    const uint32_t kofs_ = kgw + 8 <= a.K ? 2u * (uint32_t)kgw : 0u;                                  \
    _Pragma("unroll") for (int i = (i0_); i < (i1_); ++i)                                             \
      mf::glds16(Wrs, wrow[i] + kofs_, dma0 + kPpW0 + (sw_) * kPpOp + i * 64 * 128);                  \
    if ((i1_) == 4) kgw += kBK;                                                                       \
  }
  // fragment addresses inside a stage: row R = 128 wm + 32 mi + lrow of A (64 wn + 32 ni + lrow of W), chunk
  // (2 s + lhalf) ^ ((lrow >> 1) & 7) = ((s ^ (lrow >> 2 & 3)) << 1) | ((lhalf ^ (lrow >> 1)) & 1)
  const int gh = (lrow >> 2) & 3, c0 = ((lhalf ^ (lrow >> 1)) & 1) << 4;
  const mf::lds_addr_t fragA = mf::lds_addr(s_raw) + (128 * wm + lrow) * 128 + c0;
  const mf::lds_addr_t fragW = mf::lds_addr(s_raw) + kPpW0 + (64 * wn + lrow) * 128 + c0;
  const int ncols = a.N - (n0 + wn * 64);  // columns of this wave's 64 that exist (wave-uniform)
  // A phase = two k-steps of 16: twelve fragment reads and four DMA requests in its load section, sixteen MFMAs
  // (every accumulator twice, eight MFMAs apart) in its MFMA section.  (One k-step per phase -- eight barriers per
  // K-tile -- left the MFMA pipe at 0.55 of its peak even with NO DMA at all, whether the load section waited for its
  // own six reads or they were issued between the previous phase's MFMAs: the barrier hand-over itself, ~100 cycles
  // per 256 cycles of MFMAs.  MF_PP_DBG ablations, tools/ab_gemm.sh.)
  uint4 fa[2][4], fb[2][2];
#define MF_PP_READS(NJ_, kk_, sa_, sw_, s_, r0_, r1_)                                                  \
  if ((NJ_) > 0) {                                                                                    \
    const mf::lds_addr_t va_ = fragA + (sa_) * kPpOp + (((s_) ^ gh) << 5);                            \
    const mf::lds_addr_t vb_ = fragW + (sw_) * kPpOp + (((s_) ^ gh) << 5);                            \
    if ((r0_) <= 0 && 0 < (r1_)) fa[kk_][0] = mf::lds_read16_async<0>(va_);                           \
    if ((r0_) <= 1 && 1 < (r1_)) fb[kk_][0] = mf::lds_read16_async<0>(vb_);                           \
    if ((r0_) <= 2 && 2 < (r1_)) fa[kk_][1] = mf::lds_read16_async<4096>(va_);                        \
    if ((r0_) <= 3 && 3 < (r1_) && (NJ_) > 1) fb[kk_][1] = mf::lds_read16_async<4096>(vb_);           \
    if ((r0_) <= 4 && 4 < (r1_)) fa[kk_][2] = mf::lds_read16_async<8192>(va_);                        \
    if ((r0_) <= 5 && 5 < (r1_)) fa[kk_][3] = mf::lds_read16_async<12288>(va_);                       \
  }
  // NJ_ = the wave's 32-column blocks that exist (2, 1 or 0: wave-uniform, one loop per value).  A fragment that no
  // MFMA uses is NOT read: the compiler takes the asm's result register as written when the statement ends and hands
  // a dead one out again at once -- the data then lands on top of whatever lives there (seen: the offset of the next
  // DMA request, a memory fault).  MF_HOLD behind the wait keeps every fragment register reserved up to there.
  // (the load section alternating three reads and one request, and one or two of a phase's four requests issued
  // between its MFMAs instead, both measured slower: DESIGN.md 4)
#define MF_PP_PHASE(NJ_, p_, REQ_, WAIT_)                                                             \
  {                                                                                                   \
    MF_PP_READS(NJ_, 0, sa, sw, 2 * (p_), 0, 6)                                                       \
    MF_PP_READS(NJ_, 1, sa, sw, 2 * (p_) + 1, 0, 6)                                                   \
    REQ_(0, 4)                                                                                        \
    WAIT_                                                                                             \
    mf::wait_lds_reads();                                                                             \
    if ((NJ_) > 0) {                                                                                  \
      _Pragma("unroll") for (int kk = 0; kk < 2; ++kk) {                                              \
        _Pragma("unroll") for (int mi = 0; mi < 4; ++mi) MF_HOLD(fa[kk][mi]);                         \
        MF_HOLD(fb[kk][0]);                                                                           \
        if ((NJ_) > 1) MF_HOLD(fb[kk][1]);                                                            \
      }                                                                                               \
    }                                                                                                 \
    mf::raw_barrier();                                                                                \
    __builtin_amdgcn_s_setprio(1);                                                                    \
    _Pragma("unroll") for (int q = 0; q < 16; ++q) {                                                  \
      const int kk = q >> 3, mi = q & 3, nj = (q >> 2) & 1;                                           \
      if (nj < (NJ_)) acc[mi][nj] = mf::mfma_bf16_32x32x16(fa[kk][mi], fb[kk][nj], acc[mi][nj]);      \
    }                                                                                                 \
    __builtin_amdgcn_s_setprio(0);                                                                    \
    mf::raw_barrier();                                                                                \
  }
#define MF_PP_RW(i0_, i1_) if (more1) MF_PP_REQ_W(sw ^ 1, i0_, i1_)
#define MF_PP_RA(i0_, i1_) if (more2) MF_PP_REQ_A(sa2, i0_, i1_)
#define MF_PP_LOOP(NJ_)                                                                               \
  for (int t = 0; t < T; ++t) {                                                                       \
    const int sw = t & 1;                                                                             \
    const bool more1 = t + 1 < T && !(a.dbg & 1), more2 = t + 2 < T && !(a.dbg & 1);                  \
    if (a.dbg & 2) { kg = kgw = 8 * chunk; tc = kg; tx = ty = tz = 0; }                               \
    MF_PP_PHASE(NJ_, 0, MF_PP_RW, )                                                                   \
    MF_PP_PHASE(NJ_, 1, MF_PP_RA, if (more2) mf::wait_dma<4>(); else mf::wait_dma<0>();)              \
    sa = sa == 2 ? 0 : sa + 1;                                                                        \
    sa2 = sa2 == 2 ? 0 : sa2 + 1;                                                                     \
  }
  // tiles 0 (A, W) and 1 (A) before the loop; the requests of A(1) stay in flight
  MF_PP_REQ_A(0, 0, 4) MF_PP_REQ_W(0, 0, 4)
  if (T > 1 && !(a.dbg & 1)) {
    MF_PP_REQ_A(1, 0, 4)
    mf::wait_dma<4>();
  } else {
    mf::wait_dma<0>();
  }
  mf::raw_barrier();
  int sa = 0, sa2 = 2;  // A stages of tiles t and t + 2
  if (wm == 1 && !(a.dbg & 4)) mf::raw_barrier();  // the lower half runs one barrier behind from here on
  if (ncols > 32) {
    MF_PP_LOOP(2)
  } else if (ncols > 0) {
    MF_PP_LOOP(1)
  } else {
    MF_PP_LOOP(0)
  }
  if (wm == 0 && !(a.dbg & 4)) mf::raw_barrier();  // the groups meet again: every fragment read is retired, no DMA is pending
#undef MF_PP_LOOP
#undef MF_PP_RW
#undef MF_PP_RA
#undef MF_PP_READS
#undef MF_PP_PHASE
#undef MF_PP_REQ_W
#undef MF_PP_REQ_A

  // epilogue through LDS in four passes of 64 rows (64 x 260 floats)
  constexpr int kEp = kBNb + 4;
  float *s_out = reinterpret_cast<float *>(s_raw);  // [64][kEp]
  const float *bias = a.bias && a.S == 1 && !nt_split(MODE) ? a.bias + grp * a.b_gs : nullptr;  // (conv2: conv2_store8)
  const bool relu = a.relu && a.S == 1 && !nt_split(MODE), out_f32 = a.out_f32 || a.S > 1;
  const int ldo = a.S > 1 ? a.N : a.ldo;
  void *const outp = a.S > 1 ? (void *)(a.slab + (int64_t)split * a.M * a.N) : a.out;
#pragma unroll
  for (int pass = 0; pass < 4; ++pass) {
    if (wm == (pass >> 1)) {
#pragma unroll
      for (int mh = 0; mh < 2; ++mh)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) {
          const int nl = wn * 64 + ni * 32 + lrow;
          const float bn = (bias && n0 + nl < a.N) ? bias[n0 + nl] : 0.0f;
          const mf_f32x16 &c = (pass & 1) ? acc[2 + mh][ni] : acc[mh][ni];
#pragma unroll
          for (int e = 0; e < 16; ++e) {
            const int ml = mh * 32 + (e & 3) + 8 * (e >> 2) + 4 * lhalf;
            float v = c[e] + bn;
            if (relu) v = v > 0.0f ? v : 0.0f;
            s_out[ml * kEp + nl] = v;
          }
        }
    }
    __syncthreads();
    for (int i = tid; i < 64 * (kBNb / 8); i += 512) {
      const int ml = i / (kBNb / 8), c8 = i - ml * (kBNb / 8);
      const int m = m0 + 128 * (pass >> 1) + 64 * (pass & 1) + ml, n = n0 + 8 * c8;
      if (m >= a.M || n >= a.N) continue;
      int64_t orow = m;
      if (MODE == kConvDgrad) {  // class-ordered row -> channels-last voxel row of the input gradient
        const int h = m & ((1 << (3 * dol)) - 1), p = (m >> (3 * dol)) & 7, b = m >> (3 * dol + 3);
        const int x = 2 * (h >> (2 * dol)) + (p & 1), y = 2 * ((h >> dol) & (Do - 1)) + ((p >> 1) & 1),
                  z = 2 * (h & (Do - 1)) + (p >> 2);
        orow = (((int64_t)b * a.D + x) * a.D + y) * a.D + z;
      }
      const float4 v0 = *reinterpret_cast<const float4 *>(s_out + ml * kEp + 8 * c8);
      const float4 v1 = *reinterpret_cast<const float4 *>(s_out + ml * kEp + 8 * c8 + 4);
      float v[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
      if (nt_split(MODE) && a.S == 1) {
        conv2_store8(a, m, n, v);
        continue;
      }
      const int nv = a.N - n < 8 ? a.N - n : 8;
      if (out_f32) {
        float *o = reinterpret_cast<float *>(outp) + grp * a.o_gs + orow * ldo + n;
        if (nv == 8 && (ldo & 3) == 0 && ((uintptr_t)o & 15) == 0) {
          float4 *o4 = reinterpret_cast<float4 *>(o);
          if (a.accumulate && a.S == 1) {
            const float4 p0 = o4[0], p1 = o4[1];
            v[0] += p0.x; v[1] += p0.y; v[2] += p0.z; v[3] += p0.w;
            v[4] += p1.x; v[5] += p1.y; v[6] += p1.z; v[7] += p1.w;
          }
          o4[0] = make_float4(v[0], v[1], v[2], v[3]);
          o4[1] = make_float4(v[4], v[5], v[6], v[7]);
        } else {
          for (int j = 0; j < nv; ++j) o[j] = a.accumulate && a.S == 1 ? o[j] + v[j] : v[j];
        }
      } else {
        uint16_t *o = reinterpret_cast<uint16_t *>(outp) + grp * a.o_gs + orow * ldo + n;
        if (nv == 8 && (ldo & 7) == 0 && ((uintptr_t)o & 15) == 0) {
          *reinterpret_cast<uint4 *>(o) = make_uint4(mf::pack_bf16x2(v[0], v[1]), mf::pack_bf16x2(v[2], v[3]),
                                                     mf::pack_bf16x2(v[4], v[5]), mf::pack_bf16x2(v[6], v[7]));
        } else {
          for (int j = 0; j < nv; ++j) o[j] = (uint16_t)mf::bf16_bits(v[j]);
        }
      }
    }
    __syncthreads();
  }
}

}  // namespace
