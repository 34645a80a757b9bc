// TN engine of the bf16 GEMMs (weight gradients): TnArgs, k_gemm_tn_bf16, its ping-pong form, the finish passes.
// A piece of csrc/gemm_bf16.hip's single translation unit: included there, in the order of that file, nowhere else.
#pragma once
#include "mf_common.h"

namespace {

// ---- TN engine: C[i][j] = sum_m P[m][i] * Q(m, j) -------------------------------------------------------------
// Both operands arrive with the reduction index m as the SLOW dimension (rows of dY, rows of x / of the im2col view),
// the MFMA wants 8 consecutive m per lane.  The LDS image keeps the global order -- 16-byte chunks land with a plain
// ds_write_b128 -- and the fragments come out through gfx950's transposing LDS read (ds_read_b64_tr_b16: a 16-lane
// group reads a [4 m][16 columns] block, lane c receives column c).  Round 4's first version transposed 4 x 8 blocks
// in registers on the way in: 17 VALU instructions per MFMA and LDS bank conflicts on half of the LDS cycles.
//   image of one operand: 8 subtiles of 16 columns, each [64 m][16] bf16 (32 bytes per m) + 128 bytes, so that two
//   neighbouring subtiles -- the two 16-lane groups of a half-wave -- sit 32 banks apart
constexpr int kTnSub = 64 * 32 + 128;
constexpr int kTnOperand = 8 * kTnSub;
constexpr int kTnBuf = 2 * kTnOperand;
constexpr int kTnLds = 2 * kTnBuf > 128 * (128 + 4) * 4 ? 2 * kTnBuf : 128 * (128 + 4) * 4;

struct TnArgs {
  const uint16_t *P;  // bf16 [M][ldp]  (dY), group g at P + g * p_gs
  const uint16_t *Q;  // bf16 rows [M][ldq] (group g at Q + g * q_gs) or a channels-last grid [B][D^3][Cin] (conv)
  float *out;         // S == 1: C [Ni][ldc] (group g at out + g * c_gs); S > 1: slabs [S][groups][Ni][ldc]
  int64_t p_gs, q_gs, c_gs;
  int M, Ni, Nj, ldp, ldq, ldc, groups, S;
  const int32_t *m_range;  // rows mode, S == 1: group g reduces rows [m_range[g], m_range[g + 1]) of P / Q (device array)
  int conv, B, D, Do, olog, Cin, ks, stride, pad, dil;  // conv: Q(m, j = tap * Cin + cin) = x[b][stride o - pad + dil tap][cin], m = (b, o)
};

template <bool CONV>
__global__ __launch_bounds__(256, 2) void k_gemm_tn_bf16(TnArgs a) {
  MF_DYN_LDS(unsigned char, s_raw);
  const int tiles_i = (a.Ni + 127) / 128, tiles_j = (a.Nj + 127) / 128;
  const int per_group = tiles_i * tiles_j;
  const int G = gridDim.x;
  int L = blockIdx.x;
  if ((G & 7) == 0) L = (blockIdx.x & 7) * (G >> 3) + (blockIdx.x >> 3);
  const int split = L / (per_group * a.groups);
  const int rem0 = L - split * per_group * a.groups;
  const int grp = rem0 / per_group;
  const int rem = rem0 - grp * per_group;
  const int i0 = (rem % tiles_i) * 128, j0 = (rem / tiles_i) * 128;  // i tile fastest: neighbours share Q columns
  // this split's rows: K-tiles of 64 rows, contiguous ranges
  int m_lo = 0, M = a.M;
  if (!CONV && a.m_range) {  // (block-uniform)
    m_lo = a.m_range[grp];
    M = a.m_range[grp + 1] - m_lo;
  }
  const int Tall = (M + 63) / 64;
  const int Tper = (Tall + a.S - 1) / a.S;
  const int t0 = split * Tper, t1 = min(Tall, t0 + Tper);

  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int wm = wave & 1, wn = wave >> 1;
  const int lrow = lane & 31, lhalf = lane >> 5;
  // staging: load r (0..3) of this lane goes to LDS row 16 r + 4 wave + kr of the K-tile, columns 16 sub + 8 half .. + 7.  Eight
  // consecutive lanes (the unit a ds_write_b128 is served in) fill 4 rows x 32 bytes = 128 contiguous bytes of one
  // subtile: 32 distinct banks; a wave's load covers 4 rows x 256 contiguous bytes.
  const int half = lane & 1, kr = (lane >> 1) & 3, sub = lane >> 3;
  const int col = 16 * sub + 8 * half;
  const int st_off = sub * kTnSub + (4 * wave + kr) * 32 + 16 * half;  // + 512 r
  const int mrow = 16 * kr + 4 * wave;  // this lane's rows of a K-tile: mrow .. mrow + 3 (see MF_TN_LOAD)

  const uint16_t *P = a.P + grp * a.p_gs + (int64_t)m_lo * a.ldp;
  const uint16_t *Q = a.Q + grp * a.q_gs + (CONV ? 0 : (int64_t)m_lo * a.ldq);
  const int Do = a.Do, dol = a.olog;
  const bool pcol_ok = i0 + col + 8 <= a.Ni;
  // conv: this lane's column chunk is one (tap, cin .. cin + 7) for the whole loop, so per row only the output voxel
  // (b, ox, oy, oz) is decoded: the address is linear in it, and "the tap lies inside the grid" is one range test per
  // axis on the output coordinate (lo <= o <= lo + span, as one unsigned compare); a chunk past the last tap, or a
  // tap no output voxel can reach, is never valid
  const int q_off = j0 + col;
  int tap_const = 0, lo_x = 0, lo_y = 0, lo_z = 0;
  unsigned span_x = 0, span_y = 0, span_z = 0;
  bool qcol_ok = j0 + col + 8 <= a.Nj;
  const int cxs = a.stride * a.D * a.D * a.Cin, cys = a.stride * a.D * a.Cin, czs = a.stride * a.Cin;
  const int cb = a.D * a.D * a.D * a.Cin;
  if (CONV) {
    const int jj = qcol_ok ? j0 + col : 0;
    const int tap = jj / a.Cin, tap_c = jj - tap * a.Cin;
    const int kxy = tap / a.ks, kz = tap - kxy * a.ks, kx = kxy / a.ks, ky = kxy - kx * a.ks;
    const int tx = a.dil * kx - a.pad, ty = a.dil * ky - a.pad, tz = a.dil * kz - a.pad;
    tap_const = ((tx * a.D + ty) * a.D + tz) * a.Cin + tap_c;
    qcol_ok = qcol_ok && kx < a.ks;
    const int t3[3] = {tx, ty, tz};
    int lo3[3];
    unsigned sp3[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {  // 0 <= stride * o + t < D
      const int lo = t3[k] >= 0 ? 0 : (-t3[k] + a.stride - 1) / a.stride;
      const int hi = a.D - 1 - t3[k] >= 0 ? min((a.D - 1 - t3[k]) / a.stride, Do - 1) : -1;
      qcol_ok = qcol_ok && hi >= lo;
      lo3[k] = lo;
      sp3[k] = (unsigned)max(hi - lo, 0);
    }
    lo_x = lo3[0]; lo_y = lo3[1]; lo_z = lo3[2];
    span_x = sp3[0]; span_y = sp3[1]; span_z = sp3[2];
  }

  mf_f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.0f;

  // one register set, one tile ahead; a masked chunk (row past M, column past the edge, padding tap) is a buffer
  // load at an out-of-range offset and comes back as zeros (see the NT kernel)
  const mf::BufRsrc Prs = mf::make_rsrc(P), Qrs = mf::make_rsrc(Q);
  uint4 rp0, rp1, rp2, rp3, rq0, rq1, rq2, rq3;
  // Load r of this lane is row 16 kr + 4 wave + r of the K-tile (it lands in LDS row 16 r + 4 wave + kr: any
  // permutation of the reduction index is fine as long as both operands use it): the lane's four rows are consecutive,
  // so with an output size that is a multiple of 4 they share (b, ox, oy) and differ in oz only -- one voxel decode,
  // two range tests and one address per K-tile, then a z test and an add per load (the per-load decode was 20 of the
  // kernel's 29 VALU instructions per load: 7.3 per MFMA).
#define MF_TN_LOAD(r_, rp_, rq_)                                                                      \
  {                                                                                                   \
    const bool ok_ = mb_ + (r_) < M;                                                                \
    rp_ = mf::buf_load16(Prs, ok_ && pcol_ok ? 2u * (uint32_t)(pb_ + (r_) * a.ldp) : mf::kBufMasked); \
    bool qok_ = ok_ && qrow_ok_;                                                                      \
    if (CONV) qok_ = qok_ && (unsigned)(zrel_ + (r_)) <= span_z;                                      \
    rq_ = mf::buf_load16(Qrs, qok_ ? 2u * (uint32_t)(qb_ + (r_) * (CONV ? czs : a.ldq)) : mf::kBufMasked); \
  }
#define MF_TN_FETCH(tt_)                                                                              \
  {                                                                                                   \
    const int mb_ = (tt_) * 64 + mrow;                                                                \
    const int pb_ = mb_ * a.ldp + i0 + col;                                                           \
    int qb_ = mb_ * a.ldq + q_off, zrel_ = 0;                                                         \
    bool qrow_ok_ = qcol_ok;                                                                          \
    if (CONV) {                                                                                       \
      const int b_ = mb_ >> (3 * dol), ox_ = (mb_ >> (2 * dol)) & (Do - 1), oy_ = (mb_ >> dol) & (Do - 1), \
                oz_ = mb_ & (Do - 1);                                                                 \
      qrow_ok_ = qcol_ok && (unsigned)(ox_ - lo_x) <= span_x && (unsigned)(oy_ - lo_y) <= span_y;     \
      qb_ = tap_const + b_ * cb + ox_ * cxs + oy_ * cys + oz_ * czs;                                  \
      zrel_ = oz_ - lo_z;                                                                             \
    }                                                                                                 \
    MF_TN_LOAD(0, rp0, rq0) MF_TN_LOAD(1, rp1, rq1) MF_TN_LOAD(2, rp2, rq2) MF_TN_LOAD(3, rp3, rq3)   \
  }
#define MF_TN_STASH(buf_)                                                                             \
  {                                                                                                   \
    MF_HOLD(rp0); MF_HOLD(rp1); MF_HOLD(rp2); MF_HOLD(rp3);                                           \
    MF_HOLD(rq0); MF_HOLD(rq1); MF_HOLD(rq2); MF_HOLD(rq3);                                           \
    unsigned char *Ps_ = s_raw + (buf_) * kTnBuf + st_off;                                            \
    *reinterpret_cast<uint4 *>(Ps_) = rp0; *reinterpret_cast<uint4 *>(Ps_ + 512) = rp1;               \
    *reinterpret_cast<uint4 *>(Ps_ + 1024) = rp2; *reinterpret_cast<uint4 *>(Ps_ + 1536) = rp3;       \
    unsigned char *Qs_ = Ps_ + kTnOperand;                                                            \
    *reinterpret_cast<uint4 *>(Qs_) = rq0; *reinterpret_cast<uint4 *>(Qs_ + 512) = rq1;               \
    *reinterpret_cast<uint4 *>(Qs_ + 1024) = rq2; *reinterpret_cast<uint4 *>(Qs_ + 1536) = rq3;       \
  }
  // fragment of a 32-column block at subtile pair (2 n, 2 n + 1), k-step s: lane l = 16 g + c takes column c of
  // subtile 2 n + (g & 1), m = 16 s + 8 (g >> 1) + 0..3 (first read) and + 4..7 (second): the operand layout of
  // v_mfma_f32_32x32x16_bf16 (row l % 32, k = 8 (l / 32) .. + 7)
  const int frag = ((lane >> 4) & 1) * kTnSub + (8 * (lane >> 5) + ((lane & 15) >> 2)) * 32 + 8 * (lane & 3);
#define MF_TN_FRAG(ptr_, s_) mf::lds_read_tr16_b64x2((ptr_) + 512 * (s_), 128)
#define MF_TN_COMPUTE(buf_)                                                                           \
  {                                                                                                   \
    asm volatile("" ::: "memory");                                                                    \
    __builtin_amdgcn_sched_barrier(0);                                                                \
    const unsigned char *Ps = s_raw + (buf_) * kTnBuf + 4 * wm * kTnSub + frag;                       \
    const unsigned char *Qs = s_raw + (buf_) * kTnBuf + kTnOperand + 4 * wn * kTnSub + frag;          \
    _Pragma("unroll") for (int s = 0; s < 4; ++s) {                                                   \
      const uint4 a0 = MF_TN_FRAG(Ps, s), a1 = MF_TN_FRAG(Ps + 2 * kTnSub, s);                        \
      const uint4 b0 = MF_TN_FRAG(Qs, s), b1 = MF_TN_FRAG(Qs + 2 * kTnSub, s);                        \
      acc[0][0] = mf::mfma_bf16_32x32x16(a0, b0, acc[0][0]);                                          \
      acc[0][1] = mf::mfma_bf16_32x32x16(a0, b1, acc[0][1]);                                          \
      acc[1][0] = mf::mfma_bf16_32x32x16(a1, b0, acc[1][0]);                                          \
      acc[1][1] = mf::mfma_bf16_32x32x16(a1, b1, acc[1][1]);                                          \
    }                                                                                                 \
    __builtin_amdgcn_sched_barrier(0);                                                                \
  }
  // (the fetch past this split's last tile reads the next split's rows, or rows past M as zeros, into a buffer nobody
  // reads: unconditional on purpose, see the NT kernel)
  if (t0 < t1) {
    MF_TN_FETCH(t0);
    MF_TN_STASH(0);
  }
  __syncthreads();
  for (int t = t0; t < t1; ++t) {
    MF_TN_FETCH(t + 1);
    MF_TN_COMPUTE((t - t0) & 1);
    MF_TN_STASH((t - t0 + 1) & 1);
    __syncthreads();
  }
#undef MF_TN_COMPUTE
#undef MF_TN_FRAG
#undef MF_TN_STASH
#undef MF_TN_FETCH
#undef MF_TN_LOAD

  constexpr int kEp = 128 + 4;
  float *s_out = reinterpret_cast<float *>(s_raw);
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int ni = 0; ni < 2; ++ni) {
      const int nl = wn * 64 + ni * 32 + lrow;
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int ml = wm * 64 + mi * 32 + (e & 3) + 8 * (e >> 2) + 4 * lhalf;
        s_out[ml * kEp + nl] = acc[mi][ni][e];
      }
    }
  __syncthreads();
  float *dst = a.out + ((int64_t)split * a.groups + grp) * (a.S > 1 ? (int64_t)a.Ni * a.ldc : 0) +
               (a.S > 1 ? 0 : grp * a.c_gs);
  for (int i = tid; i < 128 * 32; i += 256) {
    const int il = i >> 5, c4 = i & 31;
    const int ii = i0 + il, jj = j0 + 4 * c4;
    if (ii >= a.Ni || jj >= a.Nj) continue;
    const float4 v = *reinterpret_cast<const float4 *>(s_out + il * kEp + 4 * c4);
    float *o = dst + (int64_t)ii * a.ldc + jj;
    if (jj + 4 <= a.Nj && (a.ldc & 3) == 0 && ((uintptr_t)o & 15) == 0) {
      *reinterpret_cast<float4 *>(o) = v;
    } else {
      const float vv[4] = {v.x, v.y, v.z, v.w};
      for (int j = 0; j < 4 && jj + j < a.Nj; ++j) o[j] = vv[j];
    }
  }
}

// ---- the TN engine on the 256 x 256 tile with LDS-DMA operands and two wave groups in ping-pong (round 6) -----------
// The structure of k_gemm_nt_bf16_pp (see there: phases of two k-steps, the groups one barrier apart, counted vmcnt,
// inline-asm fragment reads) for C[i][j] = sum_m P[m][i] Q(m, j): a K-tile is 64 rows m of both operands, 256 columns
// each -- [64][512 bytes] per operand and stage, THREE Q stages (the im2col rows: re-read from far away) + TWO P stages
// (dY: shared by every workgroup of a column of tiles).
//   * DMA: one request = two LDS rows (2 x 512 bytes: whole contiguous row segments of the tile).  LDS row
//     rho = 16 i + 2 wave + h (request i of the wave, h = lane / 32) holds global row 64 t + 8 wave + 4 h + i: any
//     permutation of the reduction index is fine as long as both operands use it, and this one gives a lane four
//     CONSECUTIVE rows per K-tile -- for a convolution one voxel decode, an oz test and an add per request.
//   * fragments: ds_read_b64_tr_b16 (a 16-lane group reads a [4 rows][16 columns] block, lane c receives column c):
//     the four rows of a group are 512 bytes apart -- the same banks -- so the 16-byte chunk index of LDS row rho is
//     XORed with 4 (rho & 3) (applied to the SOURCE column of the DMA lane, as in the NT kernel): the four rows of a
//     group land in the four 64-byte quarters of the 256-byte bank row.  rho & 3 is the lane's r = (lane & 15) / 4 in
//     every read, so a lane's address of column block n is (n ^ r) * 64 + const: one address register per block.

template <bool CONV>
__global__ __launch_bounds__(512, 2) void k_gemm_tn_bf16_pp(TnArgs a) {
  MF_DYN_LDS(unsigned char, s_raw);
  const int tiles_i = (a.Ni + 255) / 256, tiles_j = (a.Nj + 255) / 256;
  const int per_group = tiles_i * tiles_j;
  const int G = gridDim.x;
  int L = blockIdx.x;
  if ((G & 7) == 0) L = (blockIdx.x & 7) * (G >> 3) + (blockIdx.x >> 3);
  const int split = L / (per_group * a.groups);
  const int rem0 = L - split * per_group * a.groups;
  const int grp = rem0 / per_group;
  const int rem = rem0 - grp * per_group;
  const int i0 = (rem % tiles_i) * 256, j0 = (rem / tiles_i) * 256;  // i tile fastest: neighbours share Q columns
  int m_lo = 0, M = a.M;
  if (!CONV && a.m_range) {  // (block-uniform)
    m_lo = a.m_range[grp];
    M = a.m_range[grp + 1] - m_lo;
  }
  const int Tall = (M + 63) / 64;
  const int Tper = (Tall + a.S - 1) / a.S;
  const int t0 = split * Tper;
  const int T = max(0, min(Tall, t0 + Tper) - t0);

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = mf::wave_uniform(tid >> 6);
  const int wm = wave >> 2, wn = wave & 3;
  const int lrow = lane & 31, lhalf = lane >> 5;
  // DMA slot: LDS rows 16 i + 2 wave + h, chunk position lane & 31 -> this lane's column chunk (the same for every row)
  const int h = lane >> 5;
  const int cq = (lane & 31) ^ (4 * ((2 * wave + h) & 3));
  const int col = 8 * cq;
  const int mrow = 8 * wave + 4 * h;  // this lane's rows of a K-tile: mrow + i

  const uint16_t *P = a.P + grp * a.p_gs + (int64_t)m_lo * a.ldp;
  const uint16_t *Q = a.Q + grp * a.q_gs + (CONV ? 0 : (int64_t)m_lo * a.ldq);
  const int Do = a.Do, dol = a.olog;
  const bool pcol_ok = i0 + col + 8 <= a.Ni;
  // conv: the lane's column chunk is one (tap, cin .. cin + 7) for the whole loop (see k_gemm_tn_bf16)
  const int q_off = j0 + col;
  int tap_const = 0, lo_x = 0, lo_y = 0, lo_z = 0;
  unsigned span_x = 0, span_y = 0, span_z = 0;
  bool qcol_ok = j0 + col + 8 <= a.Nj;
  const int cxs = a.stride * a.D * a.D * a.Cin, cys = a.stride * a.D * a.Cin, czs = a.stride * a.Cin;
  const int cb = a.D * a.D * a.D * a.Cin;
  if (CONV) {
    const int jj = qcol_ok ? j0 + col : 0;
    const int tap = jj / a.Cin, tap_c = jj - tap * a.Cin;
    const int kxy = tap / a.ks, kz = tap - kxy * a.ks, kx = kxy / a.ks, ky = kxy - kx * a.ks;
    const int tx = a.dil * kx - a.pad, ty = a.dil * ky - a.pad, tz = a.dil * kz - a.pad;
    tap_const = ((tx * a.D + ty) * a.D + tz) * a.Cin + tap_c;
    qcol_ok = qcol_ok && kx < a.ks;
    const int t3[3] = {tx, ty, tz};
    int lo3[3];
    unsigned sp3[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {  // 0 <= stride * o + t < D
      const int lo = t3[k] >= 0 ? 0 : (-t3[k] + a.stride - 1) / a.stride;
      const int hi = a.D - 1 - t3[k] >= 0 ? min((a.D - 1 - t3[k]) / a.stride, Do - 1) : -1;
      qcol_ok = qcol_ok && hi >= lo;
      lo3[k] = lo;
      sp3[k] = (unsigned)max(hi - lo, 0);
    }
    lo_x = lo3[0]; lo_y = lo3[1]; lo_z = lo3[2];
    span_x = sp3[0]; span_y = sp3[1]; span_z = sp3[2];
  }

  mf_f32x16 acc[4][2];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.0f;

  const mf::BufRsrc Prs = mf::make_rsrc(P), Qrs = mf::make_rsrc(Q);
  unsigned char *const dma0 = s_raw + wave * 1024;  // request i of this wave fills LDS rows 16 i + 2 wave, + 1
  constexpr int kQ0 = 0, kP0 = 3 * kPpOp;            // Q stages at 0, 1, 2 x kPpOp; P stages behind them
  int tq = t0, tp = t0;                              // K-tiles the next Q / P requests fetch (Q runs one ahead)
  // requests i0_ .. i1_ - 1 of Q's next K-tile -> Q stage sq_ (rows 64 tq + mrow + i); the tile advances behind the last
#define MF_TP_REQ_Q(sq_, i0_, i1_)                                                                    \
  {                                                                                                   \
    const int mb_ = tq * 64 + mrow;                                                                   \
    int qb_ = mb_ * a.ldq + q_off, zrel_ = 0;                                                         \
    bool qrow_ok_ = qcol_ok;                                                                          \
    if (CONV) {                                                                                       \
      const int b_ = mb_ >> (3 * dol), ox_ = (mb_ >> (2 * dol)) & (Do - 1), oy_ = (mb_ >> dol) & (Do - 1), \
                oz_ = mb_ & (Do - 1);                                                                 \
      qrow_ok_ = qcol_ok && (unsigned)(ox_ - lo_x) <= span_x && (unsigned)(oy_ - lo_y) <= span_y;     \
      qb_ = tap_const + b_ * cb + ox_ * cxs + oy_ * cys + oz_ * czs;                                  \
      zrel_ = oz_ - lo_z;                                                                             \
    }                                                                                                 \
    _Pragma("unroll") for (int i = (i0_); i < (i1_); ++i) {                                           \
      bool ok_ = mb_ + i < M && qrow_ok_;                                                             \
      if (CONV) ok_ = ok_ && (unsigned)(zrel_ + i) <= span_z;                                         \
      mf::glds16(Qrs, ok_ ? 2u * (uint32_t)(qb_ + i * (CONV ? czs : a.ldq)) : mf::kBufMasked,         \
                 dma0 + kQ0 + (sq_) * kPpOp + i * 8192);                                              \
    }                                                                                                 \
    if ((i1_) == 4) ++tq;                                                                             \
  }
#define MF_TP_REQ_P(sp_, i0_, i1_)                                                                    \
  {                                                                                                   \
    const int mb_ = tp * 64 + mrow;                                                                   \
    const int pb_ = mb_ * a.ldp + i0 + col;                                                           \
    _Pragma("unroll") for (int i = (i0_); i < (i1_); ++i)                                             \
      mf::glds16(Prs, mb_ + i < M && pcol_ok ? 2u * (uint32_t)(pb_ + i * a.ldp) : mf::kBufMasked,     \
                 dma0 + kP0 + (sp_) * kPpOp + i * 8192);                                              \
    if ((i1_) == 4) ++tp;                                                                             \
  }
  // fragment addresses inside a stage (k-step s: + s * 8192, second half of a fragment: + 2048)
  const int r = (lane & 15) >> 2, q4 = lane & 3, g = lane >> 4;
  const int rowpart = (8 * (g >> 1) + r) * 512 + (2 * (g & 1) + (q4 >> 1)) * 16 + 8 * (q4 & 1);
  mf::lds_addr_t fragP[4], fragQ[2];
#pragma unroll
  for (int mi = 0; mi < 4; ++mi) fragP[mi] = mf::lds_addr(s_raw) + kP0 + rowpart + ((4 * wm + mi) ^ r) * 64;
#pragma unroll
  for (int ni = 0; ni < 2; ++ni) fragQ[ni] = mf::lds_addr(s_raw) + kQ0 + rowpart + ((2 * wn + ni) ^ r) * 64;
  const int ncols = a.Nj - (j0 + wn * 64);  // columns of this wave's 64 that exist (wave-uniform)
  uint4 fa[2][4], fb[2][2];
  // (a fragment is two 8-byte transposing reads into the halves of one 16-byte register: mf::lds_read_tr16_x2_async)
#define MF_TP_READS(NJ_, kk_, sq_, sp_, s_)                                                           \
  if ((NJ_) > 0) {                                                                                    \
    _Pragma("unroll") for (int mi = 0; mi < 4; ++mi)                                                  \
      fa[kk_][mi] = mf::lds_read_tr16_x2_async<(s_) * 8192>(fragP[mi] + (sp_) * kPpOp);               \
    fb[kk_][0] = mf::lds_read_tr16_x2_async<(s_) * 8192>(fragQ[0] + (sq_) * kPpOp);                   \
    if ((NJ_) > 1) fb[kk_][1] = mf::lds_read_tr16_x2_async<(s_) * 8192>(fragQ[1] + (sq_) * kPpOp);    \
  }
#define MF_TP_PHASE(NJ_, p_, REQ_, WAIT_)                                                             \
  {                                                                                                   \
    MF_TP_READS(NJ_, 0, sq, sp, 2 * (p_))                                                             \
    MF_TP_READS(NJ_, 1, sq, sp, 2 * (p_) + 1)                                                         \
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
    _Pragma("unroll") for (int qq = 0; qq < 16; ++qq) {                                               \
      const int kk = qq >> 3, mi = qq & 3, nj = (qq >> 2) & 1;                                        \
      if (nj < (NJ_)) acc[mi][nj] = mf::mfma_bf16_32x32x16(fa[kk][mi], fb[kk][nj], acc[mi][nj]);      \
    }                                                                                                 \
    __builtin_amdgcn_s_setprio(0);                                                                    \
    mf::raw_barrier();                                                                                \
  }
#define MF_TP_RP(i0_, i1_) if (more1) MF_TP_REQ_P(sp ^ 1, i0_, i1_)
#define MF_TP_RQ(i0_, i1_) if (more2) MF_TP_REQ_Q(sq2, i0_, i1_)
#define MF_TP_LOOP(NJ_)                                                                               \
  for (int t = 0; t < T; ++t) {                                                                       \
    const int sp = t & 1;                                                                             \
    const bool more1 = t + 1 < T, more2 = t + 2 < T;                                                  \
    MF_TP_PHASE(NJ_, 0, MF_TP_RP, )                                                                   \
    MF_TP_PHASE(NJ_, 1, MF_TP_RQ, if (more2) mf::wait_dma<4>(); else mf::wait_dma<0>();)              \
    sq = sq == 2 ? 0 : sq + 1;                                                                        \
    sq2 = sq2 == 2 ? 0 : sq2 + 1;                                                                     \
  }
  // tiles 0 (Q, P) and 1 (Q) before the loop; the requests of Q(1) stay in flight
  MF_TP_REQ_Q(0, 0, 4) MF_TP_REQ_P(0, 0, 4)
  if (T > 1) {
    MF_TP_REQ_Q(1, 0, 4)
    mf::wait_dma<4>();
  } else {
    mf::wait_dma<0>();
  }
  mf::raw_barrier();
  int sq = 0, sq2 = 2;  // Q stages of tiles t and t + 2
  if (wm == 1) mf::raw_barrier();  // the lower half runs one barrier behind from here on
  if (ncols > 32) {
    MF_TP_LOOP(2)
  } else if (ncols > 0) {
    MF_TP_LOOP(1)
  } else {
    MF_TP_LOOP(0)
  }
  if (wm == 0) mf::raw_barrier();  // the groups meet again
#undef MF_TP_LOOP
#undef MF_TP_RQ
#undef MF_TP_RP
#undef MF_TP_PHASE
#undef MF_TP_READS
#undef MF_TP_REQ_P
#undef MF_TP_REQ_Q

  // epilogue through LDS in four passes of 64 rows (fp32 tile rows i, columns j)
  constexpr int kEp = 256 + 4;
  float *s_out = reinterpret_cast<float *>(s_raw);  // [64][kEp]
  float *dst = a.out + ((int64_t)split * a.groups + grp) * (a.S > 1 ? (int64_t)a.Ni * a.ldc : 0) +
               (a.S > 1 ? 0 : grp * a.c_gs);
#pragma unroll
  for (int pass = 0; pass < 4; ++pass) {
    if (wm == (pass >> 1)) {
#pragma unroll
      for (int mh = 0; mh < 2; ++mh)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) {
          const int nl = wn * 64 + ni * 32 + lrow;
          const mf_f32x16 &c = (pass & 1) ? acc[2 + mh][ni] : acc[mh][ni];
#pragma unroll
          for (int e = 0; e < 16; ++e) {
            const int ml = mh * 32 + (e & 3) + 8 * (e >> 2) + 4 * lhalf;
            s_out[ml * kEp + nl] = c[e];
          }
        }
    }
    __syncthreads();
    for (int i = tid; i < 64 * 64; i += 512) {
      const int il = i >> 6, c4 = i & 63;
      const int ii = i0 + 64 * pass + il, jj = j0 + 4 * c4;
      if (ii >= a.Ni || jj >= a.Nj) continue;
      const float4 v = *reinterpret_cast<const float4 *>(s_out + il * kEp + 4 * c4);
      float *o = dst + (int64_t)ii * a.ldc + jj;
      if (jj + 4 <= a.Nj && (a.ldc & 3) == 0 && ((uintptr_t)o & 15) == 0) {
        *reinterpret_cast<float4 *>(o) = v;
      } else {
        const float vv[4] = {v.x, v.y, v.z, v.w};
        for (int j = 0; j < 4 && jj + j < a.Nj; ++j) o[j] = vv[j];
      }
    }
    __syncthreads();
  }
}

// out[g][i][f(j)] = sum_s slab[s][g][i][j] (increasing s); conv: j = tap * Cin + cin -> f(j) = cin * taps + tap
// (the torch / Chainer ConvolutionND weight layout [Cout][w_cin][ks][ks][ks]); channels cin >= cin_keep (the zero
// padding of a narrow layer's input up to 8 channels) are dropped.
__global__ __launch_bounds__(256) void k_wgrad_finish(const float *__restrict__ slabs, float *__restrict__ out,
                                                      int64_t per_slab, int Nj, int ldc, int S, int conv_cin,
                                                      int64_t c_gs, int64_t per_group, int64_t out_row_pitch,
                                                      int taps, int cin_keep) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= per_slab) return;
  const int64_t g = idx / per_group, in_g = idx - g * per_group;
  const int64_t i = in_g / ldc;
  const int j = (int)(in_g - i * ldc);
  if (j >= Nj) return;
  float v = slabs[idx];
  for (int s = 1; s < S; ++s) v += slabs[(int64_t)s * per_slab + idx];
  int64_t o = j;
  if (conv_cin) {
    const int tap = j / conv_cin, ci = j - tap * conv_cin;
    if (ci >= cin_keep) return;
    o = (int64_t)ci * taps + tap;
  }
  out[g * c_gs + i * out_row_pitch + o] = v;
}

// The same sum for MANY slabs of a SMALL result (the occupancy convolutions: a few thousand weights in up to 256
// slabs -- one thread per weight walked 256 dependent-latency loads: 62 us): one WAVE per weight, lane l adds slabs
// l, l + 64, ... in increasing order, the 64 partial sums meet in a fixed butterfly (deterministic).
__global__ __launch_bounds__(256) void k_wgrad_finish_deep(const float *__restrict__ slabs, float *__restrict__ out,
                                                           int64_t per_slab, int Nj, int ldc, int S, int conv_cin,
                                                           int64_t c_gs, int64_t per_group, int64_t out_row_pitch,
                                                           int taps, int cin_keep) {
  const int64_t idx = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (idx >= per_slab) return;  // wave-uniform
  const int lane = threadIdx.x & 63;
  float v = 0.0f;
  for (int s = lane; s < S; s += 64) v += slabs[(int64_t)s * per_slab + idx];
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
  if (lane != 0) return;
  const int64_t g = idx / per_group, in_g = idx - g * per_group;
  const int64_t i = in_g / ldc;
  const int j = (int)(in_g - i * ldc);
  if (j >= Nj) return;
  int64_t o = j;
  if (conv_cin) {
    const int tap = j / conv_cin, ci = j - tap * conv_cin;
    if (ci >= cin_keep) return;
    o = (int64_t)ci * taps + tap;
  }
  out[g * c_gs + i * out_row_pitch + o] = v;
}

// The convolution form of the finish pass as a tiled transpose: workgroup (ci block of 64, co) sums the slabs'
// [tap][cin] tile -- rows of 64 consecutive cin, coalesced -- into LDS and writes it out as [cin][tap], the
// framework's order, contiguous again.  (The element-wise form above would write 4-byte values ``taps`` floats apart:
// 0.3 ms per training step over the six convolution layers.)
constexpr int kPackTile = 64;  // channels per tile; taps <= 64 (kernel 3 or 4)

__global__ __launch_bounds__(256) void k_wgrad_finish_conv(const float *__restrict__ slabs, float *__restrict__ out,
                                                           int64_t per_slab, int S, int Cin, int taps, int w_cin,
                                                           int keep) {
  __shared__ float s_t[kPackTile][kPackTile + 1];
  const int ci0 = blockIdx.x * kPackTile, co = blockIdx.y;
  const float *src = slabs + (int64_t)co * taps * Cin;
  for (int i = threadIdx.x; i < taps * kPackTile; i += 256) {
    const int tap = i >> 6, cl = i & 63;
    float v = 0.0f;
    if (ci0 + cl < Cin) {
      v = src[(int64_t)tap * Cin + ci0 + cl];
      for (int s = 1; s < S; ++s) v += src[(int64_t)s * per_slab + (int64_t)tap * Cin + ci0 + cl];
    }
    s_t[cl][tap] = v;
  }
  __syncthreads();
  float *dst = out + ((int64_t)co * w_cin + ci0) * taps;  // (out already points at channel c_off)
  const int nci = min(kPackTile, keep - ci0);             // channels >= keep: the zero padding of a narrow input
  for (int i = threadIdx.x; i < nci * taps; i += 256) {
    const int cl = i / taps, tap = i - cl * taps;
    dst[i] = s_t[cl][tap];
  }
}

}  // namespace
