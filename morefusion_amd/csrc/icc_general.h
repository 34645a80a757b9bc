// The two-kernel path of an ICC iteration (any no-entry grid values): k_icc_tile -> W -> k_icc_accum.
// A piece of csrc/icc.hip's single translation unit: included there, in the order of that file, nowhere else.
#pragma once
#include "icc_common.h"

namespace {

// launch 2: TDF of one half of an x-plane (rows [y0, y1)) of one grid, fed from the bins of
// planes x-h..x+h of that half.
//  pass 1 works on SQUARED distances in voxel units (no sqrt, no pitch): 32-bit atomicMin of
//         the d2 bits behind a batched peek.  dist = pitch*sqrt(d2) is monotone in d2.  A lane
//         remembers, per record, WHICH of its candidates were within a few ulp of the minimum
//         it saw (9-bit mask): minima only decrease, so no other candidate can end up minimal.
//  pass 2 re-derives, only for those candidates (~ln n of the n candidates of a voxel), the EXACT
//         float distance and, where it equals the exact minimum and is < truncation, takes
//         atomicMin of the candidate id: the same winners as the oracle (lowest id among
//         equal ROUNDED distances).
// Measured alternatives (profiles/): a single pass with a 64-bit (d2, id) LDS
// atomicMin per improving candidate is slower (ds_min_u64 processes lanes serially); splitting
// a crowded plane over 4 workgroups that each scan all its records is slower (every stripe
// pays for every record, and 2048 workgroups no longer fit the chip at once) -- hence the
// halves are made by the binning kernel, where it costs one extra append for 1 point in 8.

template <int KS>
__device__ __forceinline__ void icc_tile_body(const IccArgs &a, const int ks_rt, const int par) {
  MF_DYN_LDS(uint32_t, s_tile);  // dist[rows*D], id[rows*D]
  __shared__ float s_max[kTileThreads / 64];
  const int ks = KS > 0 ? KS : ks_rt;
  const int h = ks / 2, K = ks * ks * ks;
  const int D = a.D, nb = a.nbins, hmax = a.hmax;
  const int g = blockIdx.y, o = g >> 1, other = g & 1;
  const int x = blockIdx.x / kHalves, half = blockIdx.x % kHalves;
  const int Dh = (D + 1) / 2;
  const int y0 = half * Dh, y1 = half == 0 ? Dh : D;
  const int nvox = (y1 - y0) * D;
  uint32_t *s_dist = s_tile, *s_id = s_tile + Dh * D;
  // independent loads: the <= 7 bin counts of this tile, capacity, offset
  int c[8];
  c[0] = 0;
  const int cap = a.bin_cap[g];
  const int64_t base_g = a.bin_base[g];
  const float pitch = a.pitch[o];
  const int bin0 = x + hmax - h;  // plane x - h
  const int nbr = nb - 1;
  const int nov = min((int)a.bin_cnt[((int64_t)par * 2 * a.O + g) * nb + nbr], 2 * a.bin_pts[g]);
#pragma unroll
  for (int b = 0; b < 7; ++b) {
    int n = 0;
    if (b < ks) n = min((int)a.bin_cnt[((int64_t)par * 2 * a.O + g) * nb + (bin0 + b) * kHalves + half], cap);
    c[b + 1] = c[b] + n;
  }
  const int T = c[7] + nov;  // the tile's bins, then the grid's overflow list (filtered by fetch)
  const int wg = blockIdx.y * gridDim.x + blockIdx.x;
  auto stamp = [&](int i) {  // tuning aid (MF_ICC_DEBUG & 32)
    if (MF_DBG(a, 32) && threadIdx.x == 0 && wg < 2048) g_dbg_stamps[wg * 8 + i] = wall_clock64();
  };
  stamp(0);
  if (MF_DBG(a, 32) && threadIdx.x == 0 && wg < 2048) g_dbg_stamps[wg * 8 + 6] = (unsigned long long)T;
  const float trunc = a.thr * pitch;
  for (int i = threadIdx.x; i < nvox; i += kTileThreads) { s_dist[i] = 0x7f800000u; s_id[i] = kNoCand; }
  __syncthreads();
  const float d2_hi = a.thr * a.thr * 1.00002f;  // conservative inclusion; exact test in pass 2
  const float d2_in = a.thr * a.thr * 0.999f;    // certainly inside the truncation radius
  const float4 *recs = a.rec + base_g;
  const float fxp = (float)x;

  // record i of this tile's concatenated bins -> (plane offset b, record); rb < 0: none
  auto fetch = [&](const int i, float4 &rv, int &rb) {
    rb = -1;
    if (i >= T) return;
    if (i >= c[7]) {  // overflow record: belongs to this tile iff its plane is in x-h..x+h and its rows touch the half
      rv = recs[(int64_t)nbr * cap + (i - c[7])];
      const int pl = (int)roundf(rv.x) - (x - h), iry_ = (int)roundf(rv.y);
      const bool in_half = half == 0 ? (iry_ - h < Dh) : (iry_ + h >= Dh);
      rb = (pl >= 0 && pl < ks && in_half) ? pl : -1;
      return;
    }
    int b = 0;
#pragma unroll
    for (int k = 1; k < 7; ++k) b += (k < ks && i >= c[k]) ? 1 : 0;
    int cb = 0;
#pragma unroll
    for (int k = 1; k < 7; ++k) cb = (k == b) ? c[k] : cb;
    rb = b;
    rv = recs[(int64_t)((bin0 + b) * kHalves + half) * cap + (i - cb)];
  };
  // exact tie-break of ONE candidate against the final minimum of its voxel
  auto settle = [&](const int ad, const uint32_t db, const uint32_t cid) {
    const uint32_t cur = s_dist[ad];
    if (db <= cur + 8u) {  // within a few ulp of the minimal d2
      // dist == dmin is certain for equal bits; dist < trunc is certain well inside the
      // truncation radius (pitch*sqrt(d2) <= 0.9995 thr pitch (1 + 2^-22) < trunc)
      bool win = db == cur && __uint_as_float(db) < d2_in;
      if (!win) {
        const float dist = pitch * sqrtf(__uint_as_float(db));
        const float dmin = pitch * sqrtf(__uint_as_float(cur));
        win = dist == dmin && dist < trunc;
      }
      if (win) atomicMin(&s_id[ad], cid);
    }
  };
  // One record against its ks x ks (y, z) candidates in plane x.  pass 1 returns the mask of
  // candidates that may still win (KS == 3: one bit per candidate; else bit 0 = "any"); pass 2
  // visits the candidates of `mask`.  All peeks of a record are issued together, then the
  // non-returning atomics.  A peek may be stale (another lane lowered the voxel meanwhile):
  // values only decrease, so a stale peek only lets MORE candidates through.
  auto visit = [&](const int pass, const float4 sv, const int rb, const unsigned mask) -> unsigned {
    const int iry = (int)roundf(sv.y), irz = (int)roundf(sv.z);
    const uint32_t idb = __float_as_uint(sv.w) * (uint32_t)K;
    const int bb = ks - 1 - rb;  // x offset of plane x inside this point's neighbourhood
    const float dx = sv.x - fxp;
    const float dx2 = dx * dx;
    unsigned out = 0u;
    if constexpr (KS == 3) {
      if (pass == 1) {
        uint32_t db[9], cur[9];
        int ad[9];
#pragma unroll
        for (int aa = 0; aa < 3; ++aa) {
          const int iy = iry + aa - 1;
          const float dy = sv.y - (float)iy;
          const float dxy = dx2 + dy * dy;  // (dx^2 + dy^2) + dz^2: the oracle's order
#pragma unroll
          for (int cc = 0; cc < 3; ++cc) {
            const int iz = irz + cc - 1;
            const float dz = sv.z - (float)iz;
            const float d2 = dxy + dz * dz;
            const bool ok = iy >= y0 && iy < y1 && iz >= 0 && iz < D && d2 < d2_hi;
            db[aa * 3 + cc] = __float_as_uint(d2);
            ad[aa * 3 + cc] = ok ? (iy - y0) * D + iz : -1;
          }
        }
#pragma unroll
        for (int k = 0; k < 9; ++k) cur[k] = s_dist[ad[k] < 0 ? 0 : ad[k]];
#pragma unroll
        for (int k = 0; k < 9; ++k) {
          if (ad[k] < 0) continue;
          if (db[k] <= cur[k]) atomicMin(&s_dist[ad[k]], db[k]);
          if (db[k] <= cur[k] + 8u) out |= 1u << k;
        }
      } else {
#pragma unroll
        for (int k = 0; k < 9; ++k) {
          if (!((mask >> k) & 1u)) continue;  // in range and near-minimal when pass 1 saw it
          const int aa = k / 3, cc = k % 3;
          const int iy = iry + aa - 1, iz = irz + cc - 1;
          const float dy = sv.y - (float)iy, dz = sv.z - (float)iz;
          const float d2 = (dx2 + dy * dy) + dz * dz;
          settle((iy - y0) * D + iz, __float_as_uint(d2), idb + (uint32_t)((aa * 3 + bb) * 3 + cc));
        }
      }
    } else {
      for (int aa = 0; aa < ks; ++aa) {
        const int iy = iry + aa - h;
        if (iy < y0 || iy >= y1) continue;
        const float dy = sv.y - (float)iy;
        const float dxy = dx2 + dy * dy;
        const int lrow = (iy - y0) * D;
        for (int cc = 0; cc < ks; ++cc) {
          const int iz = irz + cc - h;
          if (iz < 0 || iz >= D) continue;
          const float dz = sv.z - (float)iz;
          const float d2 = dxy + dz * dz;
          if (!(d2 < d2_hi)) continue;
          const uint32_t db = __float_as_uint(d2);
          if (pass == 1) {
            const uint32_t cur = s_dist[lrow + iz];
            if (db <= cur) atomicMin(&s_dist[lrow + iz], db);
            if (db <= cur + 8u) out = 1u;
          } else {
            settle(lrow + iz, db, idb + (uint32_t)((aa * ks + bb) * ks + cc));
          }
        }
      }
    }
    return out;
  };

  // The first kTileThreads * kTileKeep records stay in registers over both passes (all loads
  // in flight at once: ONE memory round trip); a more crowded tile streams the rest again.
  float4 rv[kTileKeep];
  int rb[kTileKeep];
  unsigned long long keep = 0ull;  // 9 bits per kept record: candidates that may still win
#pragma unroll
  for (int u = 0; u < kTileKeep; ++u) fetch(u * kTileThreads + (int)threadIdx.x, rv[u], rb[u]);
  stamp(1);
#pragma unroll
  for (int u = 0; u < kTileKeep; ++u)
    if (rb[u] >= 0) keep |= (unsigned long long)visit(1, rv[u], rb[u], 0u) << (9 * u);
  for (int base = kTileThreads * kTileKeep; base < T; base += kTileThreads * kTileR) {
    float4 xv[kTileR];
    int xb[kTileR];
#pragma unroll
    for (int u = 0; u < kTileR; ++u) fetch(base + u * kTileThreads + (int)threadIdx.x, xv[u], xb[u]);
#pragma unroll
    for (int u = 0; u < kTileR; ++u)
      if (xb[u] >= 0) visit(1, xv[u], xb[u], 0u);
  }
  __syncthreads();
  stamp(2);
#pragma unroll
  for (int u = 0; u < kTileKeep; ++u) {
    const unsigned m9 = (unsigned)(keep >> (9 * u)) & 0x1ffu;
    if (m9 != 0u) visit(2, rv[u], rb[u], m9);
  }
  for (int base = kTileThreads * kTileKeep; base < T; base += kTileThreads * kTileR) {
    float4 xv[kTileR];
    int xb[kTileR];
#pragma unroll
    for (int u = 0; u < kTileR; ++u) fetch(base + u * kTileThreads + (int)threadIdx.x, xv[u], xb[u]);
#pragma unroll
    for (int u = 0; u < kTileR; ++u) {
      if (xb[u] < 0) continue;
      // streamed records carry no mask: every in-range candidate within the window is examined
      if constexpr (KS == 3) {
        const int iry = (int)roundf(xv[u].y), irz = (int)roundf(xv[u].z);
        unsigned m9 = 0u;
#pragma unroll
        for (int k = 0; k < 9; ++k) {
          const int iy = iry + k / 3 - 1, iz = irz + k % 3 - 1;
          const float dxs = xv[u].x - fxp, dy = xv[u].y - (float)iy, dz = xv[u].z - (float)iz;
          const float d2 = (dxs * dxs + dy * dy) + dz * dz;
          if (iy >= y0 && iy < y1 && iz >= 0 && iz < D && d2 < d2_hi) m9 |= 1u << k;
        }
        if (m9 != 0u) visit(2, xv[u], xb[u], m9);
      } else {
        visit(2, xv[u], xb[u], 1u);
      }
    }
  }
  __syncthreads();
  stamp(3);
  // epilogue: winners out (coalesced 8 B/lane) + max raw inside weight of this tile
  // (truncated_distance_function.py:198-204: -1 where no winner, + offset, clamp at 0)
  const float offset = other ? 0.0f : a.sdf_offset;
  unsigned long long *Wg = a.W + (int64_t)g * D * D * D + ((int64_t)x * D + y0) * D;
  float wmax = 0.0f;
  for (int i0 = threadIdx.x; i0 < nvox; i0 += kTileThreads * 2) {
    uint32_t lo[2];
    float sd[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int i = i0 + u * kTileThreads;
      lo[u] = i < nvox ? s_id[i] : kNoCand;  // set only where pitch*sqrt(min d2) < trunc
      sd[u] = lo[u] != kNoCand ? a.pts4[lo[u] / (uint32_t)K].w : -1.0f;
    }
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int i = i0 + u * kTileThreads;
      if (i >= nvox) continue;
      const float dist = lo[u] != kNoCand ? pitch * sqrtf(__uint_as_float(s_dist[i])) : trunc;
      Wg[i] = ((unsigned long long)__float_as_uint(dist) << 32) | lo[u];
      float w = sd[u] + offset;
      w = w < 0.0f ? 0.0f : w;
      wmax = fmaxf(wmax, w);
    }
  }
  wmax = mf::wave_max(wmax);
  if ((threadIdx.x & 63) == 0) s_max[threadIdx.x >> 6] = wmax;
  __syncthreads();
  if (threadIdx.x == 0) {
    float m = s_max[0];
#pragma unroll
    for (int i = 1; i < kTileThreads / 64; ++i) m = fmaxf(m, s_max[i]);
    if (m > 0.0f) atomicMax(&a.Mbits[(int64_t)par * 2 * a.O + g], __float_as_uint(m));  // m >= 0: uint order == float order
  }
  stamp(4);
}

__global__ __launch_bounds__(kTileThreads) void k_icc_tile(IccArgs a, int par) {
  const int ks = min(ksize_of(a.thr, a.pitch[blockIdx.y >> 1]), 2 * a.hmax + 1);  // block-uniform
  if (ks == 3)
    icc_tile_body<3>(a, 3, par);
  else
    icc_tile_body<0>(a, ks, par);
}

// ---- launch 2: weights, sums, gradient moments ------------------------------------
constexpr int kVPT = kVoxPerBlock / kAccThreads;  // voxels per thread

__global__ __launch_bounds__(kAccThreads) void k_icc_accum(IccArgs a, int par) {
  __shared__ float s_rows[kAccThreads / 16][kNumOwn + 1];  // 16-lane row sums (+1: bank spread)
  // Collision moments (gradient of this grid's penalty onto ANOTHER object's pose): each lane
  // keeps the 12 moments of its colliding voxels in registers; after the voxel loop the block
  // reduces them per other object in a fixed order (DPP row sums + ordered row adds), exactly
  // like its own moments.  (Round 1 / early round 2 pushed every colliding voxel through 36
  // fixed-point LDS atomics behind float64 conversions: ~600 instructions per colliding voxel,
  // 3-5 us in the crowded blocks.)
  MF_DYN_LDS(float, s_rows2);   // [max_ns][kAccThreads / 16][12 + 1] row sums per other object
  __shared__ unsigned long long s_emask;  // scene objects some voxel of this block collides with (<= 64 per scene)
  __shared__ float s_Rt[kMaxSceneObjectsGeneral][12];
  __shared__ int s_off[kMaxSceneObjectsGeneral + 1];
  const int o = blockIdx.y;
  const int wg2 = 2048 + blockIdx.y * gridDim.x + blockIdx.x;
  auto stamp = [&](int i) {
    if (MF_DBG(a, 32) && threadIdx.x == 0 && wg2 < 4096) g_dbg_stamps[wg2 * 8 + i] = wall_clock64();
  };
  stamp(0);
  const int D = a.D, V = D * D * D;
  const int4 meta = a.meta[o];
  const int ja = meta.x, jb = meta.y;
  const int Ns = jb - ja;
  // all independent loads first: scene tables, scalars, and this thread's voxels
  for (int i = threadIdx.x; i < Ns * 12; i += blockDim.x) s_Rt[i / 12][i % 12] = a.Rt[12 * ja + i];  // Ns up to 64: 768 words
  if (threadIdx.x <= Ns) s_off[threadIdx.x] = a.obj_off[ja + threadIdx.x];
  if (threadIdx.x == 0) s_emask = 0ull;
  const float pitch = a.pitch[o];
  // candidate ids are point * K + offset with this grid's own kernel size
  const int ks_o = ksize_of(a.thr, pitch);
  const int K = ks_o * ks_o * ks_o;
  const float ox = a.origin[3 * o], oy = a.origin[3 * o + 1], oz = a.origin[3 * o + 2];
  const float M_own = __uint_as_float(a.Mbits[(int64_t)par * 2 * a.O + 2 * o]);
  const float M_oth = __uint_as_float(a.Mbits[(int64_t)par * 2 * a.O + 2 * o + 1]);
  const float trunc = a.thr * pitch;
  // iterative_collision_check_link.py:82: skip the max() when grid_other has NaN,
  // which happens iff its normaliser max(weight) is 0 (0/0 everywhere).
  const bool use_oth = (Ns > 1) && (M_oth != 0.0f);
  const unsigned long long *W_own = a.W + (int64_t)(2 * o) * V;
  const unsigned long long *W_oth = a.W + (int64_t)(2 * o + 1) * V;
  const float *tgt = a.grid_target + (int64_t)o * V;
  const float *gne = a.grid_ne + (int64_t)o * V;

  unsigned long long ko[kVPT], kk[kVPT];
  float ne_[kVPT], tg_[kVPT];
  float4 m_own[kVPT], m_oth[kVPT];
#pragma unroll
  for (int it = 0; it < kVPT; ++it) {
    const int v = blockIdx.x * kVoxPerBlock + it * kAccThreads + threadIdx.x;
    const bool in = v < V;
    ko[it] = in ? W_own[v] : (((unsigned long long)__float_as_uint(trunc) << 32) | kNoCand);
    kk[it] = (in && use_oth) ? W_oth[v] : (unsigned long long)kNoCand;
    ne_[it] = in ? gne[v] : 0.0f;
    tg_[it] = in ? tgt[v] : 0.0f;
  }
#pragma unroll
  for (int it = 0; it < kVPT; ++it) {  // second level: winner gathers
    const uint32_t lo = (uint32_t)ko[it], lo_o = (uint32_t)kk[it];
    m_own[it] = lo != kNoCand ? a.pts4[lo / (uint32_t)K] : make_float4(0, 0, 0, -1.0f);
    m_oth[it] = lo_o != kNoCand ? a.pts4[lo_o / (uint32_t)K] : make_float4(0, 0, 0, -1.0f);
  }
  __syncthreads();
  stamp(1);
  const float *Rt_o = s_Rt[o - ja];

  float acc[kNumOwn];
#pragma unroll
  for (int i = 0; i < kNumOwn; ++i) acc[i] = 0.0f;
  int ecol[kVPT];
  float cv[kVPT][12];
#pragma unroll
  for (int it = 0; it < kVPT; ++it) ecol[it] = -1;

#pragma unroll
  for (int it = 0; it < kVPT; ++it) {
    const int v = blockIdx.x * kVoxPerBlock + it * kAccThreads + threadIdx.x;
    if (v >= V) continue;
    const int iz = v % D, iy = (v / D) % D, ix = v / (D * D);
    const uint32_t lo = (uint32_t)ko[it];
    const bool has = lo != kNoCand;
    const float g = 1.0f - __uint_as_float((uint32_t)(ko[it] >> 32)) / trunc;  // 1 - tdf/trunc
    float w = m_own[it].w + a.sdf_offset;
    const bool neg = w < 0.0f;
    if (neg) w = 0.0f;
    const float win = w / M_own;
    const float wsurf = neg ? win : 1.0f - win;
    const float surf = g * wsurf, ins = g * win;
    const float ne = ne_[it], tg = tg_[it];
    float ne_eff = ne;
    bool oth_wins = false;
    float wo_in = 0.0f;
    const uint32_t lo_o = (uint32_t)kk[it];
    if (use_oth) {
      const float go = 1.0f - __uint_as_float((uint32_t)(kk[it] >> 32)) / trunc;
      float wo = m_oth[it].w + 0.0f;
      if (wo < 0.0f) wo = 0.0f;
      wo_in = wo / M_oth;
      const float oth = go * wo_in;
      // F.maximum(grid_nontarget_empty, grid_other): gradient to `other` only if larger
      oth_wins = !(ne >= oth);
      if (oth_wins) ne_eff = oth;
    }
    acc[0] += surf * tg;
    acc[1] += ins;
    acc[2] += ins * ne_eff;
    if (has) {
      float ux, uy, uz;
      bool ok;
      world_frac(Rt_o, m_own[it], ox, oy, oz, pitch, ix, iy, iz, ux, uy, uz, ok);
      if (ok) {
        const float A[3] = {wsurf * tg / trunc, win * ne_eff / trunc, win / trunc};
        const float u[3] = {ux, uy, uz};
#pragma unroll
        for (int k = 0; k < 3; ++k)
#pragma unroll
          for (int d = 0; d < 3; ++d) {
            const float s = u[d] * A[k];
            acc[3 + 12 * k + 4 * d + 0] += s * m_own[it].x;
            acc[3 + 12 * k + 4 * d + 1] += s * m_own[it].y;
            acc[3 + 12 * k + 4 * d + 2] += s * m_own[it].z;
            acc[3 + 12 * k + 4 * d + 3] += s;
          }
      }
    }
    if (oth_wins && lo_o != kNoCand && ins != 0.0f) {
      // collision term: gradient flows to the OTHER object's pose
      const uint32_t p = lo_o / (uint32_t)K;
      int e = 0;
      while (e + 1 < Ns && (int)p >= s_off[e + 1]) ++e;
      const float4 m = m_oth[it];  // fetched with the second-level gathers above
      float ux, uy, uz;
      bool ok;
      world_frac(s_Rt[e], m, ox, oy, oz, pitch, ix, iy, iz, ux, uy, uz, ok);
      const float B = wo_in * ins / trunc;
      if (ok && isfinite(B)) {
        const float u[3] = {ux, uy, uz};
        ecol[it] = e;
#pragma unroll
        for (int d = 0; d < 3; ++d) {
          const float sB = u[d] * B;
          cv[it][4 * d + 0] = sB * m.x;
          cv[it][4 * d + 1] = sB * m.y;
          cv[it][4 * d + 2] = sB * m.z;
          cv[it][4 * d + 3] = sB;
        }
      }
    }
  }
#pragma unroll
  for (int it = 0; it < kVPT; ++it)
    if (ecol[it] >= 0) atomicOr(&s_emask, 1ull << ecol[it]);
  // fixed-order block reduction: every component is summed over each 16-lane row on DPP (4 VALU
  // steps, no LDS), the 32 row sums go through LDS, one lane per component adds them in order.
  stamp(2);
#pragma unroll
  for (int i = 0; i < kNumOwn; ++i) {
    const float r = mf::row16_sum(acc[i]);
    if ((threadIdx.x & 15) == 0) s_rows[threadIdx.x >> 4][i] = r;
  }
  __syncthreads();
  // The block sums join the object's accumulators as 64-bit fixed point: integer atomics are
  // exact and order-independent, so the iteration's reduced sums (~200 words per scene) are
  // bitwise reproducible and the optimiser step needs no reduction pass of its own.
  long long *own = a.acc_own + ((int64_t)par * a.O + o) * kOwnSlots;
  if (threadIdx.x < kNumOwn) {
    float sacc = 0.0f;
#pragma unroll
    for (int r = 0; r < kAccThreads / 16; ++r) sacc += s_rows[r][threadIdx.x];
    if (isfinite(sacc)) {
      const long long x = __double2ll_rn((double)sacc * kFixOwn);
      if (x != 0) atomicAdd(reinterpret_cast<unsigned long long *>(own + threadIdx.x), (unsigned long long)x);
    } else {
      atomicAdd(reinterpret_cast<unsigned long long *>(own + kNumOwn), 1ull);  // -> NaN loss
    }
  }
  stamp(3);
  // collision moments: row sums of every other object this block collides with (block-uniform
  // loop over the set bits, no barrier inside), ONE barrier, then 12 lanes per object add the
  // rows in order
  long long *po = a.acc_oth + ((int64_t)par * a.O + o) * a.max_ns * 12;
  const unsigned long long em0 = s_emask;  // complete: every atomicOr precedes the barrier above
  constexpr int kRows = kAccThreads / 16;
  for (unsigned long long em = em0; em != 0ull; em &= em - 1ull) {
    const int e = __ffsll((long long)em) - 1;
#pragma unroll
    for (int c = 0; c < 12; ++c) {
      float v = 0.0f;
#pragma unroll
      for (int it = 0; it < kVPT; ++it) v += ecol[it] == e ? cv[it][c] : 0.0f;
      const float r = mf::row16_sum(v);
      if ((threadIdx.x & 15) == 0) s_rows2[(e * kRows + (threadIdx.x >> 4)) * 13 + c] = r;
    }
  }
  if (em0 == 0ull) return;  // block-uniform
  __syncthreads();
  for (int i = threadIdx.x; i < a.max_ns * 12; i += kAccThreads) {
    const int e = i / 12, c = i - 12 * e;
    if (!((em0 >> e) & 1ull)) continue;
    float sacc = 0.0f;
#pragma unroll
    for (int r = 0; r < kRows; ++r) sacc += s_rows2[(e * kRows + r) * 13 + c];
    const long long x = isfinite(sacc) ? __double2ll_rn((double)sacc * kFixOth) : 0;
    if (x != 0) atomicAdd(reinterpret_cast<unsigned long long *>(po + i), (unsigned long long)x);
  }
}

}  // namespace
