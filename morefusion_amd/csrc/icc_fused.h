// The single-pass path of an ICC iteration ({0,1} no-entry grids): k_icc_fused / k_icc_fused_big.
// A piece of csrc/icc.hip's single translation unit: included there, in the order of that file, nowhere else.
#pragma once
#include "icc_common.h"

namespace {

// ---- single-pass path: TDF tiles + weights / sums / moments in ONE kernel -------------
// k_icc_tile -> W -> k_icc_accum exists only because the weights are normalised by the per-grid
// maximum M = max(inside weight), known once every tile of the grid is done.  Every caller of
// the reference passes {0,1} no-entry grids (bool cast to float32:
// check_iterative_collision_check_link.py:36-38, collision_based_pose_refinement.py:162), and
// for those maximum(no-entry, other) is a selection, so the loss and its gradient are POLYNOMIAL
// in a = 1/M_own and b = 1/M_oth.  With gw = g*w (g = 1 - tdf/trunc, w = clamped inside weight),
// go, wo the same of the "other" grid, nb = [sdf + offset >= 0], ne in {0,1}:
//   RN   = sum nb*g*tg          - a   sum gw*tg                  (sums 0, 1)
//   S_in =                        a   sum gw                      (sum 2)
//   PN   =                        a   sum gw*ne + a b sum gw*(1-ne)*go*wo        (sums 3, 4)
//   own gradient moments (u = unit residual of the winner, m its model point; 12 each):
//     U0a: nb*tg/trunc, U0b: w*tg/trunc (coeff -a), U1a: w*ne/trunc (a), U1b: w*(1-ne)*go*wo/trunc
//     (a b), U2: w/trunc (a)
//   collision moments onto the other object e: u_o (x) {m_o,1} * wo*gw/trunc     (coeff a b)
// A workgroup = (object, x-plane, y-half) runs both TDFs of its voxels in LDS (own + other
// records), then one lane per voxel accumulates the 65 monomial sums; the step (icc_step_gather)
// applies a, b from the per-grid maxima.  The winners never leave LDS: no W round trip, no
// second launch, no dependent re-load of what the tile just computed.  Same arithmetic per
// voxel as k_icc_accum up to the association of the normaliser (tests: loss within 2e-5,
// step within 1e-5 of the oracle's).  Grids with other values take the two-kernel path.
// LDS of the voxel phase (k_icc_fused)
struct VoxLds {
  float rows[kTileThreads / 16][kNumF + 1];
  float max[2][kTileThreads / 64];
  // voxels with an own winner, compacted in voxel order: index, (no-entry, target), winner points
  uint16_t list[kTileThreads];
  float2 netg[kTileThreads];
  float4 mown[kTileThreads], moth[kTileThreads];
  int wcnt[kTileThreads / 64];
};
// static LDS of k_icc_fused (declared once in the kernel: the body is instantiated per kernel size)
// (MAXNS = 64: the kernel every scene of <= 64 objects runs, unchanged since round 3; 128: k_icc_fused_big)
template <int MAXNS>
struct FusedLds {
  VoxLds v;
  float Rt[MAXNS][12];
  int off[MAXNS + 1];
};

// Constants of one padded half-plane tile (k_icc_fused, kernel size 3).
struct Tile3 {
  int Wp, rows_p, y0;
  float fxp, pitch, trunc, d2_in;
  uint32_t in_bits, hi_bits;
};

// The two-pass (min, arg-min) of k_icc_tile on the LDS arrays of one grid, kernel size 3.  The tile
// carries a margin of kPad cells on every side: all nine (y, z) candidates of a record of this half's
// bins (rounded y in [y0 - 1, y1], z in [-1, D]) address cells of the padded tile, the ones
// outside the half land in margin cells nobody reads.  ks = 3 therefore needs NO predicate:
// pass 1 = nine fire-and-forget ds_min at constant offsets from one base address (a peek at
// the current minimum first, or range / radius tests per candidate, cost more instructions
// than the atomics they save: 19.9 -> 18.4 us without the peek alone), pass 2 = the nine
// FINAL minima in one batch of reads, the exact test only where this record is within a few
// ulp.  A minimum beyond the truncation radius simply finds no winner in pass 2.
// (sx, sy, sz) = voxel-frame coordinates of the point, pid its id, rb = its plane's offset in x-1 .. x+1.
__device__ __forceinline__ void icc_visit3(const int pass, uint32_t *dist, uint32_t *id, const Tile3 &tl,
                                           const float sx, const float sy, const float sz, const uint32_t pid,
                                           const int rb) {
  const int Wp = tl.Wp;
  const int iry = (int)roundf(sy), irz = (int)roundf(sz);
  const uint32_t idb = pid * 27u;
  const int bb = 2 - rb;
  const float dx = sx - tl.fxp;
  const float dx2 = dx * dx;
  // cell of candidate (aa, cc) = (0, 0): row iry - 1, column irz - 1; clamped so that a
  // corrupt record cannot leave the tile
  const int r0 = min(max(iry - 1 - tl.y0 + kPad, 0), tl.rows_p - 3);
  const int c0 = min(max(irz - 1 + kPad, 0), Wp - 3);
  const int cbase = r0 * Wp + c0;
  uint32_t db[9];
#pragma unroll
  for (int aa = 0; aa < 3; ++aa) {
    const float dy = sy - (float)(iry + aa - 1);
    const float dxy = dx2 + dy * dy;
#pragma unroll
    for (int cc = 0; cc < 3; ++cc) {
      const float dz = sz - (float)(irz + cc - 1);
      db[aa * 3 + cc] = __float_as_uint(dxy + dz * dz);
    }
  }
  if (pass == 1) {
#pragma unroll
    for (int k = 0; k < 9; ++k) atomicMin(&dist[cbase + (k / 3) * Wp + (k % 3)], db[k]);
  } else {
    uint32_t cur[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) cur[k] = dist[cbase + (k / 3) * Wp + (k % 3)];
    // fast: this record IS the minimum, certainly inside the truncation radius -> candidate
    // for the arg-min.  slow (rare): within a few ulp of the minimum or near the radius ->
    // the exact float test, in a ROLLED loop behind one branch that recomputes what it
    // needs.  (Inlined next to the fast path the compiler speculated both square roots into
    // every candidate: pass 2 took 4-5 us in every tile; unrolled behind the branch it was
    // still 900 instructions of code per record.)
    const uint32_t cid0 = idb + (uint32_t)(bb * 3);
    bool any_slow = false;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
      const bool f = db[k] == cur[k] && db[k] < tl.in_bits;
      // (issuing it unconditionally with a neutral value instead: measured slower, 2.3 vs 1.6 us)
      if (f) atomicMin(&id[cbase + (k / 3) * Wp + (k % 3)], cid0 + (uint32_t)((k / 3) * 9 + (k % 3)));
      any_slow |= !f && db[k] <= min(cur[k] + 8u, tl.hi_bits);
    }
    if (any_slow) {
#pragma nounroll
      for (int k = 0; k < 9; ++k) {
        const int aa = k / 3, cc = k - 3 * aa;
        const float dy = sy - (float)(iry + aa - 1), dz = sz - (float)(irz + cc - 1);
        const uint32_t dbk = __float_as_uint((dx2 + dy * dy) + dz * dz);
        const int ad = cbase + aa * Wp + cc;
        const uint32_t curk = dist[ad];
        const bool f = dbk == curk && dbk < tl.in_bits;
        if (!f && dbk <= min(curk + 8u, tl.hi_bits)) {
          // candidate at squared distance bits dbk against the final minimum curk of its voxel
          bool win = dbk == curk && __uint_as_float(dbk) < tl.d2_in;
          if (!win) {
            const float dd = tl.pitch * sqrtf(__uint_as_float(dbk));
            const float dmin = tl.pitch * sqrtf(__uint_as_float(curk));
            win = dd == dmin && dd < tl.trunc;
          }
          if (win) atomicMin(&id[ad], cid0 + (uint32_t)(aa * 9 + cc));
        }
      }
    }
  }
}

// ---- voxel phase of a half-plane tile whose (min distance, arg-min) arrays are final.  Only a voxel
// WITH an own winner adds to any sum (without one g = 0 and w = 0), and those are the few voxels of
// the surface shell, scattered over most waves of the tile: compact them, so that ceil(n / 64) waves
// pay the arithmetic and the 65 row reductions instead of every wave the shell touches.  The maximum
// of the OTHER grid's weights needs every voxel with an other-winner: taken here in the
// voxel-per-lane layout, its gather is in flight during the compaction.
// V.rows and s_rows2 must be zero on entry (a wave writes only the sets / objects it meets).
struct TileGeom {
  int o, ja, Ns, x, y0, nvox, nvh, Wp, D, K;
  float pitch, trunc, ox, oy, oz;
};

// NSU > 0 (the specialised forms): the scene holds at most NSU <= 16 objects -- the object of a colliding point is
// found by NSU - 1 unrolled compares, and the collision moments are reduced in one trip without a loop.
template <bool BIG, int NSU, class Stamp>
__device__ __forceinline__ void icc_voxel_phase(const IccArgs &a, const int par, const TileGeom &tg_, const float ne0,
                                                const float tg0, uint32_t *s_dist, uint32_t *s_id, float *s_rows2,
                                                VoxLds &Vx, const float (*s_Rt)[12], const int *s_off, Stamp stamp) {
  auto &s_rows = Vx.rows;
  auto &s_max = Vx.max;
  auto &s_list = Vx.list;
  auto &s_netg = Vx.netg;
  auto &s_mown = Vx.mown;
  auto &s_moth = Vx.moth;
  auto &s_wcnt = Vx.wcnt;
  const int o = tg_.o, ja = tg_.ja, Ns = tg_.Ns, x = tg_.x, y0 = tg_.y0, nvox = tg_.nvox, nvh = tg_.nvh, Wp = tg_.Wp,
            D = tg_.D, K = tg_.K;
  const float pitch = tg_.pitch, trunc = tg_.trunc, ox = tg_.ox, oy = tg_.oy, oz = tg_.oz;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // voxel -> (row, column) without an integer divide: exact for vi < 1024, D <= 64
  const uint32_t rcpD = (65536u + (uint32_t)D - 1u) / (uint32_t)D;  // (scalar)
  const int my_r = (int)(((uint32_t)tid * rcpD) >> 16), my_c = tid - my_r * D;
  const int my_cell = tid < nvox ? (my_r + kPad) * Wp + (my_c + kPad) : 0;
  const uint32_t my_id = tid < nvox ? s_id[my_cell] : kNoCand;
  const uint32_t my_ido = tid < nvox ? s_id[nvh + my_cell] : kNoCand;
  // both winner gathers of this voxel in flight during the compaction; the lane that takes the
  // voxel reads them from LDS (no second dependent global round trip)
  const bool act = my_id != kNoCand;
  const float4 g_own = act ? a.pts4[my_id / (uint32_t)K] : make_float4(0, 0, 0, -1.0f);
  const float4 g_oth = my_ido != kNoCand ? a.pts4[my_ido / (uint32_t)K] : make_float4(0, 0, 0, -1.0f);
  const unsigned long long bal = __ballot(act);
  if (lane == 0) s_wcnt[wave] = __popcll(bal);
  __syncthreads();
  int before = 0, total = 0;
#pragma unroll
  for (int w = 0; w < kTileThreads / 64; ++w) {
    const int cw = s_wcnt[w];
    before += w < wave ? cw : 0;
    total += cw;
  }
  if (act) {
    const int slot = before + __popcll(bal & ((1ull << lane) - 1ull));
    s_list[slot] = (uint16_t)((my_r << 8) | my_c);
    s_mown[slot] = g_own;
    s_moth[slot] = g_oth;
    s_netg[slot] = make_float2(ne0, tg0);
  }
  __syncthreads();
  stamp(5);
  const float *Rt_o = s_Rt[o - ja];
  float wmax_own = 0.0f;
  float wmax_oth = fmaxf(g_oth.w + 0.0f, 0.0f);
  constexpr int kRows = kTileThreads / 16;
  const int n_rows = (total + 15) / 16;
  int ecol_keep = -1;  // (BIG only: the collision terms of the later chunks of a scene of > kRows2Chunk objects)
  float cv_keep[12];
  if constexpr (BIG) {
#pragma unroll
    for (int cc = 0; cc < 12; ++cc) cv_keep[cc] = 0.0f;
  }
  if ((tid & ~63) < total) {  // wave-uniform
    const bool live = tid < total;
    const int rc = live ? (int)s_list[tid] : 0;
    const int vr = rc >> 8, vc = rc & 255;
    const int pc = (vr + kPad) * Wp + (vc + kPad);
    const uint32_t lo = live ? s_id[pc] : kNoCand;
    const uint32_t lo_o = live ? s_id[nvh + pc] : kNoCand;
    const float4 m_own = live ? s_mown[tid] : make_float4(0, 0, 0, -1.0f);
    const float4 m_oth = live ? s_moth[tid] : make_float4(0, 0, 0, -1.0f);
    const float2 netg = s_netg[tid];
    const float ne = live ? netg.x : 0.0f, tg = live ? netg.y : 0.0f;
    const bool has = lo != kNoCand, has_o = lo_o != kNoCand;
    // Winners (arg-min) are exact; from here on the weights use reciprocal multiplies
    // (x * (1/trunc), x * (1/pitch), d * rsq(|d|^2)) instead of IEEE divides: <= 2 ulp per factor,
    // far inside the tolerance of the sums (which are re-associated anyway), and ~200 fewer
    // instructions on the one wave whose issue time is this phase.
    const float inv_trunc = 1.0f / trunc, inv_pitch = 1.0f / pitch;
    const float dist_o = has ? pitch * sqrtf(__uint_as_float(s_dist[pc])) : trunc;
    const float dist_k = has_o ? pitch * sqrtf(__uint_as_float(s_dist[nvh + pc])) : trunc;
    const int iy = y0 + vr, iz = vc;
    const float g = has ? fmaxf(1.0f - dist_o * inv_trunc, 0.0f) : 0.0f;  // 1 - tdf/trunc
    float w = m_own.w + a.sdf_offset;
    const bool neg = w < 0.0f;
    if (neg) w = 0.0f;
    const float go = has_o ? fmaxf(1.0f - dist_k * inv_trunc, 0.0f) : 0.0f;
    float wo = m_oth.w + 0.0f;
    if (wo < 0.0f) wo = 0.0f;
    if (live) wmax_own = w;
    const float gw = g * w;
    const float gwo = (1.0f - ne) * (go * wo);  // (1 - ne) * go * wo: the part that needs b
    const int row = tid >> 4;
    const bool row_lead = (tid & 15) == 0;
    {
      const float v5[5] = {live && !neg ? g * tg : 0.0f, live ? gw * tg : 0.0f, live ? gw : 0.0f,
                           live ? gw * ne : 0.0f, live ? gw * gwo : 0.0f};
      float r5[5];
#pragma unroll
      for (int k = 0; k < 5; ++k) r5[k] = mf::row16_sum(v5[k]);
      if (row_lead) {
#pragma unroll
        for (int k = 0; k < 5; ++k) s_rows[row][k] = r5[k];
      }
    }
    // own-gradient moments, set by set; a set no lane of the wave contributes to is skipped
    // (s_rows starts zeroed): target-free or no-entry-free regions drop 24 of the 60 reductions
    {
      float uu[3] = {0.0f, 0.0f, 0.0f};
      bool ok = false;
      if (live && has) {
        world_frac_r(Rt_o, m_own, ox, oy, oz, inv_pitch, x, iy, iz, uu[0], uu[1], uu[2], ok);
        if (!ok) uu[0] = uu[1] = uu[2] = 0.0f;
      }
      const float wt = ok ? w * inv_trunc : 0.0f;
      const float kk[5] = {ok && !neg ? tg * inv_trunc : 0.0f, wt * tg, wt * ne, wt * gwo, wt};
      const float mc[4] = {m_own.x, m_own.y, m_own.z, 1.0f};
#pragma unroll
      for (int sset = 0; sset < 5; ++sset) {
        if (__ballot(kk[sset] != 0.0f) == 0ull) continue;  // wave-uniform
        // the 12 chains in one block (independent DPP chains interleave: no wait-state nops),
        // one predicated burst of stores
        float r12[12];
#pragma unroll
        for (int d = 0; d < 3; ++d) {
          const float sc = uu[d] * kk[sset];
#pragma unroll
          for (int cc = 0; cc < 4; ++cc) r12[4 * d + cc] = mf::row16_sum(sc * mc[cc]);
        }
        if (row_lead) {
#pragma unroll
          for (int i = 0; i < 12; ++i) s_rows[row][5 + 12 * sset + i] = r12[i];
        }
      }
    }
    // collision term: gradient flows to the OTHER object's pose
    int ecol = -1;
    float cv[12];
    if (live && ne == 0.0f && has_o && go * wo > 0.0f && gw != 0.0f) {
      const int pp = (int)(lo_o / (uint32_t)K);
      int e = 0;  // scene object of the point: independent LDS reads, no dependent search loop
      if constexpr (NSU > 0) {
#pragma unroll
        for (int k = 1; k < NSU; ++k) e += (k < Ns && pp >= s_off[k]) ? 1 : 0;
      } else {
        for (int k = 1; k < Ns; ++k) e += pp >= s_off[k] ? 1 : 0;
      }
      float ux, uy, uz;
      bool ok;
      world_frac_r(s_Rt[e], m_oth, ox, oy, oz, inv_pitch, x, iy, iz, ux, uy, uz, ok);
      const float B = wo * gw * inv_trunc;
      if (ok && isfinite(B)) {
        const float uu[3] = {ux, uy, uz};
        ecol = e;
#pragma unroll
        for (int d = 0; d < 3; ++d) {
          const float sB = uu[d] * B;
          cv[4 * d + 0] = sB * m_oth.x;
          cv[4 * d + 1] = sB * m_oth.y;
          cv[4 * d + 2] = sB * m_oth.z;
          cv[4 * d + 3] = sB;
        }
      }
    }
    // the 12 collision moments per other object some lane of this wave collides with (rows2
    // starts zeroed: a wave writes only the objects it meets); objects beyond the first chunk: below
    if (__ballot(ecol >= 0) != 0ull) {
      const int e1 = BIG ? min(Ns, kRows2Chunk) : Ns;
      for (int e = 0; e < e1; ++e) {
        if (__ballot(ecol == e) == 0ull) continue;  // wave-uniform
        float r12[12];
#pragma unroll
        for (int cc = 0; cc < 12; ++cc) r12[cc] = mf::row16_sum(ecol == e ? cv[cc] : 0.0f);
        if (row_lead) {
#pragma unroll
          for (int cc = 0; cc < 12; ++cc) s_rows2[(e * kRows + row) * 13 + cc] = r12[cc];
        }
      }
    }
    if constexpr (BIG) {  // kept for the later chunks of a scene of more than kRows2Chunk objects
      ecol_keep = ecol;
#pragma unroll
      for (int cc = 0; cc < 12; ++cc) cv_keep[cc] = ecol >= 0 ? cv[cc] : 0.0f;
    }
  }
  stamp(7);
  // per-grid maxima of the raw inside weights (the normalisers a, b of the step)
  wmax_own = mf::wave_max(wmax_own);
  wmax_oth = mf::wave_max(wmax_oth);
  if (lane == 0) { s_max[0][wave] = wmax_own; s_max[1][wave] = wmax_oth; }
  __syncthreads();
  if (tid >= kTileThreads - 2) {  // (lanes away from the ones that reduce the sums below)
    const int kd = tid - (kTileThreads - 2);
    float m = s_max[kd][0];
#pragma unroll
    for (int i = 1; i < kTileThreads / 64; ++i) m = fmaxf(m, s_max[kd][i]);
    if (m > 0.0f) atomicMax(&a.Mbits[(int64_t)par * 2 * a.O + 2 * o + kd], __float_as_uint(m));
  }
  if (total == 0) return;  // block-uniform: no own winner here, nothing to add
  // ONE reduction phase: lane k < 65 adds the rows of own sum k, the next 12 Ns lanes the rows of
  // a collision moment (zero rows where no wave met that object); fixed order, fixed point
  if (tid < kNumF) {
    long long *own = a.acc_own + ((int64_t)par * a.O + o) * kOwnSlots;
    float sacc = 0.0f;
    for (int r = 0; r < n_rows; ++r) sacc += s_rows[r][tid];
    if (isfinite(sacc)) {
      const long long xq = __double2ll_rn((double)sacc * kFixOwn);
      if (xq != 0) atomicAdd(reinterpret_cast<unsigned long long *>(own + tid), (unsigned long long)xq);
    } else {
      atomicAdd(reinterpret_cast<unsigned long long *>(own + kNumF), 1ull);  // -> NaN loss
    }
  } else if constexpr (NSU > 0) {  // (12 NSU <= kTileThreads - kNumF lanes: one trip, no loop)
    static_assert(12 * NSU <= kTileThreads - kNumF, "one trip of the collision reduction");
    long long *po = a.acc_oth + ((int64_t)par * a.O + o) * a.max_ns * 12;
    const int i = tid - kNumF;
    if (i < 12 * Ns) {
      const int e = i / 12, cc = i - 12 * e;
      float sacc = 0.0f;
      for (int r = 0; r < n_rows; ++r) sacc += s_rows2[(e * kRows + r) * 13 + cc];
      const long long xq = isfinite(sacc) ? __double2ll_rn((double)sacc * kFixOth) : 0;
      if (xq != 0) atomicAdd(reinterpret_cast<unsigned long long *>(po + i), (unsigned long long)xq);
    }
  } else {  // (one trip up to 37 scene objects; a 64-object scene takes two)
    long long *po = a.acc_oth + ((int64_t)par * a.O + o) * a.max_ns * 12;
    for (int i = tid - kNumF; i < 12 * (BIG ? min(Ns, kRows2Chunk) : Ns); i += kTileThreads - kNumF) {
      const int e = i / 12, cc = i - 12 * e;
      float sacc = 0.0f;
      for (int r = 0; r < n_rows; ++r) sacc += s_rows2[(e * kRows + r) * 13 + cc];
      const long long xq = isfinite(sacc) ? __double2ll_rn((double)sacc * kFixOth) : 0;
      if (xq != 0) atomicAdd(reinterpret_cast<unsigned long long *>(po + i), (unsigned long long)xq);
    }
  }
  // Scene objects kRows2Chunk .. Ns - 1 (a scene of more than 64 objects, block-uniform): the same row sums and the
  // same reduction on the SAME LDS rows, chunk by chunk -- zero the rows, the waves write the objects of the chunk
  // they met (their collision terms waited in registers), all lanes add the rows.  Fixed order, fixed point: what a
  // single pass over 1664 Ns bytes of rows would give, in 106 KB.
  if constexpr (BIG)
  for (int eb = kRows2Chunk; eb < Ns; eb += kRows2Chunk) {
    const int ne_ = min(Ns - eb, kRows2Chunk);
    __syncthreads();
    for (int i = tid; i < ne_ * kRows * 13; i += kTileThreads) s_rows2[i] = 0.0f;
    __syncthreads();
    if ((tid & ~63) < total && __ballot(ecol_keep >= eb && ecol_keep < eb + ne_) != 0ull) {  // wave-uniform
      const int row = tid >> 4;
      const bool row_lead = (tid & 15) == 0;
      for (int e = eb; e < eb + ne_; ++e) {
        if (__ballot(ecol_keep == e) == 0ull) continue;  // wave-uniform
        float r12[12];
#pragma unroll
        for (int cc = 0; cc < 12; ++cc) r12[cc] = mf::row16_sum(ecol_keep == e ? cv_keep[cc] : 0.0f);
        if (row_lead) {
#pragma unroll
          for (int cc = 0; cc < 12; ++cc) s_rows2[((e - eb) * kRows + row) * 13 + cc] = r12[cc];
        }
      }
    }
    __syncthreads();
    long long *po = a.acc_oth + ((int64_t)par * a.O + o) * a.max_ns * 12 + 12 * eb;
    for (int i = tid; i < 12 * ne_; i += kTileThreads) {
      const int e = i / 12, cc = i - 12 * e;
      float sacc = 0.0f;
      for (int r = 0; r < n_rows; ++r) sacc += s_rows2[(e * kRows + r) * 13 + cc];
      const long long xq = isfinite(sacc) ? __double2ll_rn((double)sacc * kFixOth) : 0;
      if (xq != 0) atomicAdd(reinterpret_cast<unsigned long long *>(po + i), (unsigned long long)xq);
    }
  }
}

// SPEC = false: the body of k_icc_fused / k_icc_fused_big as it always was (every kernel size, scenes of any size).
// SPEC = true (KS = 3 only; k_icc_fused3 below): what the host decided once for the batch is a constant here -- the
// prefix table of a grid's bins has KS + 1 entries and fetch selects among KS bins, MAXNS <= 16 sizes the scene tables
// and unrolls the scene loops of the voxel phase, and scenes of one size take Ns from the arguments, so that the loads
// of the bin counters do not wait for the scene table's.  Same arithmetic in the same order: the same bits.
template <int KS, int MAXNS, bool SPEC = false>
__device__ __forceinline__ void icc_fused_body(const IccArgs &a, const int ks_rt, const int par, FusedLds<MAXNS> &L,
                                               const int o, const int tile_) {
  MF_DYN_LDS(uint32_t, s_tile);  // dist[2][nvh] | id[2][nvh] | rows2[max_ns][32][13] floats
  auto &s_rows = L.v.rows;
  auto &s_Rt = L.Rt;
  auto &s_off = L.off;
  const int ks = KS > 0 ? KS : ks_rt;
  const int h = ks / 2, K = ks * ks * ks;
  const int D = a.D, nb = a.nbins, hmax = a.hmax, V = D * D * D;
  const int x = tile_ / kHalves, half = tile_ % kHalves;
  const int Dh = (D + 1) / 2;
  const int y0 = half * Dh, y1 = half == 0 ? Dh : D;
  const int Wp = D + 2 * kPad, rows_p = Dh + 2 * kPad;  // padded tile (see icc_visit3)
  const int nvh = rows_p * Wp;          // LDS stride of one (dist | id) array
  const int nvox = (y1 - y0) * D;
  uint32_t *s_dist = s_tile, *s_id = s_tile + 2 * nvh;
  float *s_rows2 = reinterpret_cast<float *>(s_tile + 4 * nvh);
  const int4 meta = a.meta[o];
  static_assert(!SPEC || KS == 3, "the specialised forms are the 3-cell kernel's");
  constexpr int NBK = SPEC ? KS : 7;  // bins of a grid a tile reads: entries of the prefix table c[kd][]
  const int ja = meta.x, Ns = (SPEC && a.uniform_ns > 0) ? a.uniform_ns : meta.y - meta.x;
  // independent loads: bin counts of both grids, capacities, offsets, scalars, scene tables
  int c[2][NBK + 1];
  int cap[2], nov[2], tot[2];
  int64_t base_g[2];
  const float pitch = a.pitch[o];
  const int bin0 = x + hmax - h;  // plane x - h
  const int nbr = nb - 1;
#pragma unroll
  for (int kd = 0; kd < 2; ++kd) {
    const int g = 2 * o + kd;
    cap[kd] = a.bin_cap[g];
    base_g[kd] = a.bin_base[g];
    nov[kd] = (kd == 0 || Ns > 1)
                  ? min((int)a.bin_cnt[((int64_t)par * 2 * a.O + g) * nb + nbr], 2 * a.bin_pts[g]) : 0;
    c[kd][0] = 0;
#pragma unroll
    for (int b = 0; b < NBK; ++b) {
      int n = 0;
      if (b < ks && (kd == 0 || Ns > 1))
        n = min((int)a.bin_cnt[((int64_t)par * 2 * a.O + g) * nb + (bin0 + b) * kHalves + half], cap[kd]);
      c[kd][b + 1] = c[kd][b] + n;
    }
    tot[kd] = c[kd][NBK] + nov[kd];  // the tile's bins, then the grid's overflow list (filtered by fetch)
  }
  if (tot[0] + tot[1] == 0) return;  // block-uniform: no record of either grid reaches this tile
  const float ox = a.origin[3 * o], oy = a.origin[3 * o + 1], oz = a.origin[3 * o + 2];
  for (int i = threadIdx.x; i < Ns * 12; i += blockDim.x) s_Rt[i / 12][i % 12] = a.Rt[12 * ja + i];  // Ns up to 64: 768 words
  if (threadIdx.x <= Ns) s_off[threadIdx.x] = a.obj_off[ja + threadIdx.x];
  const float trunc = a.thr * pitch;
  for (int i = threadIdx.x; i < 2 * nvh; i += kTileThreads) { s_dist[i] = 0x7f800000u; s_id[i] = kNoCand; }
  for (int i = threadIdx.x; i < (MAXNS > kRows2Chunk ? min(Ns, kRows2Chunk) : Ns) * (kTileThreads / 16) * 13; i += kTileThreads)
    s_rows2[i] = 0.0f;  // (the rows of the first chunk; MAXNS = 64: Ns <= 64)
  for (int i = threadIdx.x; i < (kTileThreads / 16) * (kNumF + 1); i += kTileThreads) (&s_rows[0][0])[i] = 0.0f;
  const int wg = blockIdx.y * gridDim.x + blockIdx.x;
  auto stamp = [&](int i) {  // tuning aid (MF_ICC_DEBUG & 32)
    if (MF_DBG(a, 32) && threadIdx.x == 0 && wg < 2048) g_dbg_stamps[wg * 8 + i] = wall_clock64();
  };
  stamp(0);
  if (MF_DBG(a, 32) && threadIdx.x == 0 && wg < 2048) g_dbg_stamps[wg * 8 + 6] = (unsigned long long)(c[0][NBK] + c[1][NBK]);
#if MF_ICC_DEBUG_BUILD && defined(__HIP_DEVICE_COMPILE__)  // (GCN registers: not in a host build of this source)
  if (MF_DBG(a, 32) && threadIdx.x == 0 && wg < 2048) {  // where did this workgroup run? (HW_ID: CU / SH / SE; XCC_ID)
    unsigned hw, xcc;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
    g_dbg_stamps[(2048 + wg) * 8 + 0] = hw;
    g_dbg_stamps[(2048 + wg) * 8 + 1] = xcc;
  }
#endif
  // the voxel phase's first-level loads, issued now: this lane's voxel of the two input grids
  float ne0 = 0.0f, tg0 = 0.0f;
  if ((int)threadIdx.x < nvox) {
    const int64_t gv = (int64_t)o * V + ((int64_t)x * D + y0) * D + (int)threadIdx.x;
    ne0 = a.grid_ne[gv];
    tg0 = a.grid_target[gv];
  }
  __syncthreads();
  const float d2_hi = a.thr * a.thr * 1.00002f;  // conservative inclusion; exact test in pass 2
  const float d2_in = a.thr * a.thr * 0.999f;    // certainly inside the truncation radius
  const float fxp = (float)x;
  Tile3 tl;
  tl.Wp = Wp; tl.rows_p = rows_p; tl.y0 = y0; tl.fxp = fxp; tl.pitch = pitch; tl.trunc = trunc; tl.d2_in = d2_in;
  tl.hi_bits = __float_as_uint(d2_hi) - 1u;  // d2 < d2_hi on the bit patterns (d2 >= 0)
  tl.in_bits = __float_as_uint(d2_in);       // d2 < d2_in  <=>  bits < in_bits

  // record i of grid kd's concatenated bins -> (plane offset b, record); rb < 0: none
  auto fetch = [&](const int kd, const int i, float4 &rv, int &rb) {
    rb = -1;
    if (i >= tot[kd]) return;
    if (i >= c[kd][NBK]) {  // overflow record: this tile's iff its plane is in x-h..x+h and its rows touch the half
      rv = a.rec[base_g[kd] + (int64_t)nbr * cap[kd] + (i - c[kd][NBK])];
      const int pl = (int)roundf(rv.x) - (x - h), iry_ = (int)roundf(rv.y);
      const bool in_half = half == 0 ? (iry_ - h < Dh) : (iry_ + h >= Dh);
      rb = (pl >= 0 && pl < ks && in_half) ? pl : -1;
      return;
    }
    int b = 0;
#pragma unroll
    for (int k = 1; k < NBK; ++k) b += (k < ks && i >= c[kd][k]) ? 1 : 0;
    int cb = 0;
#pragma unroll
    for (int k = 1; k < NBK; ++k) cb = (k == b) ? c[kd][k] : cb;
    rb = b;
    rv = a.rec[base_g[kd] + (int64_t)((bin0 + b) * kHalves + half) * cap[kd] + (i - cb)];
  };
  // candidate `cid` at squared distance bits `db` against the final minimum `cur` of its voxel
  auto settle_at = [&](uint32_t *id, const int ad, const uint32_t db, const uint32_t cur, const uint32_t cid) {
    bool win = db == cur && __uint_as_float(db) < d2_in;
    if (!win) {
      const float dd = pitch * sqrtf(__uint_as_float(db));
      const float dmin = pitch * sqrtf(__uint_as_float(cur));
      win = dd == dmin && dd < trunc;
    }
    if (win) atomicMin(&id[ad], cid);
  };
  auto visit = [&](const int pass, const int kd, const float4 sv, const int rb) {
    uint32_t *dist = s_dist + kd * nvh, *id = s_id + kd * nvh;
    if constexpr (KS == 3) {
      icc_visit3(pass, dist, id, tl, sv.x, sv.y, sv.z, __float_as_uint(sv.w), rb);
    } else {
      const int iry = (int)roundf(sv.y), irz = (int)roundf(sv.z);
      const uint32_t idb = __float_as_uint(sv.w) * (uint32_t)K;
      const int bb = ks - 1 - rb;
      const float dx = sv.x - fxp;
      const float dx2 = dx * dx;
      for (int aa = 0; aa < ks; ++aa) {
        const int iy = iry + aa - h;
        if (iy < y0 || iy >= y1) continue;
        const float dy = sv.y - (float)iy;
        const float dxy = dx2 + dy * dy;
        const int lrow = (iy - y0 + kPad) * Wp + kPad;
        for (int cc = 0; cc < ks; ++cc) {
          const int iz = irz + cc - h;
          if (iz < 0 || iz >= D) continue;
          const float dz = sv.z - (float)iz;
          const float d2 = dxy + dz * dz;
          if (!(d2 < d2_hi)) continue;
          const uint32_t db = __float_as_uint(d2);
          if (pass == 1) {
            atomicMin(&dist[lrow + iz], db);
          } else {
            const uint32_t cur = dist[lrow + iz];
            if (db <= cur + 8u) settle_at(id, lrow + iz, db, cur, idb + (uint32_t)((aa * ks + bb) * ks + cc));
          }
        }
      }
    }
  };

  // kept records: kFusedKeepOwn per lane of the own grid, kFusedKeepOth of the other grid, all
  // loads in flight at once (ONE memory round trip); more crowded tiles stream the rest twice
  float4 rvo[kFusedKeepOwn], rvk[kFusedKeepOth];
  int rbo[kFusedKeepOwn], rbk[kFusedKeepOth];
#pragma unroll
  for (int u = 0; u < kFusedKeepOwn; ++u) fetch(0, u * kTileThreads + (int)threadIdx.x, rvo[u], rbo[u]);
#pragma unroll
  for (int u = 0; u < kFusedKeepOth; ++u) fetch(1, u * kTileThreads + (int)threadIdx.x, rvk[u], rbk[u]);
  stamp(1);
  auto pass_over = [&](const int pass) {
#pragma unroll
    for (int u = 0; u < kFusedKeepOwn; ++u)
      if (rbo[u] >= 0) visit(pass, 0, rvo[u], rbo[u]);
#pragma unroll
    for (int u = 0; u < kFusedKeepOth; ++u)
      if (rbk[u] >= 0) visit(pass, 1, rvk[u], rbk[u]);
#pragma unroll
    for (int kd = 0; kd < 2; ++kd) {
      const int first = kTileThreads * (kd == 0 ? kFusedKeepOwn : kFusedKeepOth);
      for (int base = first; base < tot[kd]; base += kTileThreads * kTileR) {
        float4 xv[kTileR];
        int xb[kTileR];
#pragma unroll
        for (int u = 0; u < kTileR; ++u) fetch(kd, base + u * kTileThreads + (int)threadIdx.x, xv[u], xb[u]);
#pragma unroll
        for (int u = 0; u < kTileR; ++u)
          if (xb[u] >= 0) visit(pass, kd, xv[u], xb[u]);
      }
    }
  };
  if (!MF_DBG(a, 128)) pass_over(1);  // (MF_ICC_DEBUG & 128 / 256 / 512: skip a phase to time the others; results invalid)
  __syncthreads();
  stamp(2);
  if (!MF_DBG(a, 256)) pass_over(2);
  __syncthreads();
  stamp(3);
  if (MF_DBG(a, 512)) return;

  TileGeom tg_;
  tg_.o = o; tg_.ja = ja; tg_.Ns = Ns; tg_.x = x; tg_.y0 = y0; tg_.nvox = nvox; tg_.nvh = nvh; tg_.Wp = Wp; tg_.D = D;
  tg_.K = K; tg_.pitch = pitch; tg_.trunc = trunc; tg_.ox = ox; tg_.oy = oy; tg_.oz = oz;
  icc_voxel_phase<(MAXNS > kRows2Chunk), (SPEC && MAXNS <= 16 ? MAXNS : 0)>(a, par, tg_, ne0, tg0, s_dist, s_id, s_rows2, L.v, s_Rt, s_off, stamp);
  stamp(4);
}

#ifndef MF_ICC_FUSED_WPE
#define MF_ICC_FUSED_WPE 4  // waves per SIMD the register budget is cut for (4: 128 VGPRs; 5: 96; 6: 80; 8: 64)
#endif
// (a macro, not a wrapper function: through a wrapper the standard kernel compiled to seven more SGPR spills)
  // Workgroup b runs on XCD b % 8 (observed dispatch order, MI355X_MICROARCH.md): with the plain (tile, object)
  // numbering the 64 tiles of a grid are spread over all eight L2s and each of them fetches the grid's records,
  // points and voxels over the fabric.  XCD-contiguous logical order (a.dbg bit 2048 for now): XCD k takes the logical
  // workgroups [k G/8, (k + 1) G/8) -- whole objects -- and inside an XCD workgroups i and i + 32 share a CU: planes x
  // and x + 16, a central with an outer one.  *Measured* (round 5): 8 scenes x 8 objects 96.6 -> 89.5 us per
  // iteration (the working set of a grid stays in one L2), but ONE scene 23.0 -> 24.2 us: eight objects of different
  // size on eight XCDs, the largest one's XCD is the straggler, while the plain order spreads every object over all
  // of them.  Hence by batch size: a.xcd_order is set for >= 32 objects (MF_ICC_DEBUG bit 2048 forces it on, 4096
  // off).  Two other placements for ONE scene, both measured slower than the plain order (22.6-22.9 us) and removed:
  // planes rotated by D / 2 in every other block of 256 workgroups (a central next to an outer plane on a CU:
  // 23.9-24.1), centre-out dispatch with the objects rotating over the XCDs (23.3); profiles/r05_icc_xcd_order_ab.log.
#define MF_ICC_FUSED_KERNEL_BODY(MAXNS_) \
  __shared__ FusedLds<MAXNS_> L; \
  int lin = blockIdx.y * gridDim.x + blockIdx.x; \
  const int G_ = gridDim.x * gridDim.y; \
  if (a.xcd_order && (G_ & 7) == 0) lin = (lin & 7) * (G_ >> 3) + (lin >> 3); \
  const int o = lin / (int)gridDim.x; \
  const int tile_ = lin - o * (int)gridDim.x; \
  const int ks = min(ksize_of(a.thr, a.pitch[o]), 2 * a.hmax + 1); \
  if (ks == 3) \
    icc_fused_body<3>(a, 3, par, L, o, tile_); \
  else \
    icc_fused_body<0>(a, ks, par, L, o, tile_);
__global__ __launch_bounds__(kTileThreads, MF_ICC_FUSED_WPE) void k_icc_fused(IccArgs a, int par) {  // 2 workgroups per CU
  MF_ICC_FUSED_KERNEL_BODY(kRows2Chunk)
}
// scenes of 65 .. 128 objects: the scene tables for 128, the collision rows re-used chunk by chunk (round 6)
__global__ __launch_bounds__(kTileThreads, MF_ICC_FUSED_WPE) void k_icc_fused_big(IccArgs a, int par) {
  MF_ICC_FUSED_KERNEL_BODY(kMaxSceneObjects)
}

// The specialised forms: every grid of the batch has kernel size 3 (proved on the host, icc_plan: threshold 2, what
// every caller of the reference passes) and scenes of at most MAXNS objects.  Only icc_fused_body<3> is compiled in;
// nothing is selected per workgroup.  The two kernels above stay as they were: every other batch, and
// MF_ICC_FUSED_FORM=generic, run them.
template <int MAXNS>
__global__ __launch_bounds__(kTileThreads, MF_ICC_FUSED_WPE) void k_icc_fused3(IccArgs a, int par) {
  __shared__ FusedLds<MAXNS> L;
  int lin = blockIdx.y * gridDim.x + blockIdx.x;
  const int G_ = gridDim.x * gridDim.y;
  if (a.xcd_order && (G_ & 7) == 0) lin = (lin & 7) * (G_ >> 3) + (lin >> 3);
  const int o = lin / (int)gridDim.x;
  const int tile_ = lin - o * (int)gridDim.x;
  icc_fused_body<3, MAXNS, true>(a, 3, par, L, o, tile_);
}

}  // namespace
