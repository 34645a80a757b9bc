// bf16 MFMA GEMM engines (fp32 accumulate) for the 3-D CNN and the per-point 1x1 convolutions, forward AND
// backward, for gfx950 -- the kernels BASELINE config 5 (bf16 training) and `--dtype bf16` inference run on.
//
// Reference: contrib/singleview_3d/models/model.py:114-139 (conv3 / conv4: `L.Convolution3D(.., 4, 2, pad=1)`),
// :239-258 (the three heads' Convolution1D chains), :59-66,101-111 (point MLP), trained by
// examples/ycb_video/singleview_3d/train.py:342-369 (cuDNN forward + backward-data + backward-filter).
//
// Two engines on v_mfma_f32_32x32x16_bf16 (16x the fp32-MFMA rate of csrc/conv3d.hip / linear.hip):
//
//   NT   C[m][n] = sum_k A(m, k) * W[n][k]        both operands k-contiguous in memory
//        A loaders:  rows          a row-major activation matrix with a row pitch   (linear forward / dgrad)
//                    conv forward  im2col rows of a channels-last grid, k = (tap, cin)
//                    conv dgrad    rows = INPUT voxels grouped by parity class, k = (slot, cout): an input
//                                  voxel x receives from the 2 x 2 x 2 output voxels o = h + p - s with tap
//                                  (1 - p) + 2 s per axis (x = 2 h + p); a tile of 128 rows is class-homogeneous
//                                  and multiplies that class's [Cin][8 Cout] weight slice
//   TN   C[i][j] = sum_m P[m][i] * Q(m, j)        the reduction index is the ROW index of both operands
//        (weight gradients: P = dY, Q = the layer's input rows / im2col rows).  Rows land in LDS in the global order
//        (plain ds_write_b128); the MFMA fragments come out through gfx950's transposing LDS read
//        ds_read_b64_tr_b16.  Split over m into fp32 slabs (mf_wgrad_split: a cost model over rounds of workgroup
//        slots), summed in slab order by k_wgrad_finish / k_wgrad_finish_conv (deterministic, no float atomics).
//
// Tile: 128 x 128 x 64 per 256-lane workgroup (4 waves, each a 64 x 64 corner = 2 x 2 accumulators of 32 x 32).
// NT: LDS rows of 64 bf16 at a pitch of 144 bytes (36 dwords: the sixteen rows a ds_read_b128 phase touches start
// 4 dwords apart modulo 64 banks -- conflict-free).  Register-staged double buffering with the next tile's global
// loads issued in front of this tile's 16 MFMAs and kept opaque until behind them, one barrier per K-tile,
// 2 workgroups per CU.  Masked operand chunks (padding taps, tails) are buffer loads at an out-of-range offset: the
// hardware returns zeros, nothing touches the loaded data (mf_common.h).  The epilogue goes through LDS: bias +
// ReLU on the way in, 16-byte row segments out (bf16 or fp32, optionally accumulating into an fp32 tensor).
//
// This file: the launch plans (which form of an engine a problem takes: nt_plan / tn_plan, pure host arithmetic over
// the problem size and the MF_* knobs, answered to the outside by mf_gemm_bf16_nt_plan / _tn_plan), the launchers and
// the C entry points.  The kernels, in the order of the translation unit: gemm_bf16_nt.h (NT engine and its ping-pong
// form), gemm_bf16_tn.h (TN engine, weight-gradient finishes), gemm_bf16_aux.h (pack / cast / mask / split-K finish),
// gemm_bf16_narrow.h (3 x 3 x 3 between narrow layers).
#include <cstdlib>

#include "mf_common.h"

#include "gemm_bf16_nt.h"
#include "gemm_bf16_tn.h"
#include "gemm_bf16_aux.h"
#include "gemm_bf16_narrow.h"

namespace {

// ---- knobs and plans: no device call, no HIP type -----------------------------------------------------------------
// The environment, read once per entry-point call (who honours what: DESIGN.md, "Knobs and plans of the bf16 engines").
// MF_NT_BIG: 0 = never the 256 x 256 forms, 1 = by problem size (the default), 2 = wherever their structure allows
// (tests of small problems); MF_TN_PP=0: never the TN engine's ping-pong form; MF_NT_SPLITK: S > 0 = that split of K
// wherever one may run and K has S tiles (tests); MF_NT_HALF_MAX: the largest count of 128-row tiles that still takes
// the half-height tile (tuning).  MF_PP_DBG, -DMF_PP_ABLATE builds only (timing ablations of k_gemm_nt_bf16_pp, WRONG
// results): 1 = no operand requests after tile 0, 2 = every request re-reads K-tile 0 (cache hits), 4 = the two wave
// groups in lockstep instead of one barrier apart.
struct Knobs { int nt_big, nt_splitk, tn_pp, nt_half_max, pp_dbg; };
Knobs read_knobs() {
  auto num = [](const char *name, int unset) { const char *e = getenv(name); return e ? atoi(e) : unset; };
  Knobs k = {num("MF_NT_BIG", -1), num("MF_NT_SPLITK", 0), num("MF_TN_PP", 1), num("MF_NT_HALF_MAX", 255), 0};
#ifdef MF_PP_ABLATE
  k.pp_dbg = num("MF_PP_DBG", 0);
#endif
  return k;
}

// An NT problem: C [M][N] per group over K; ``table``: rows come with a group table (mf_linear_bf16_tiles);
// ``dgrad_rows``: rows of one parity class of the k4 / s2 data gradient (Do^3), 0 for every other mode; ``may_split``:
// the entry point can split K (the _ws / split forwards) into the ``ws_bytes`` it was given for the slabs.
constexpr int64_t kAnyWs = INT64_MAX;
struct NtShape { int mode; int64_t M; int N, K, groups; bool table; int64_t dgrad_rows; bool may_split; int64_t ws_bytes; };
// rows of the tile (64 / 128: k_gemm_nt_bf16, 256: k_gemm_nt_bf16_pp), splits of K, the ping-pong form's ablation bits
struct NtPlan { int tile, S, dbg; };

NtPlan nt_plan(const NtShape &p, const Knobs &k) {
  const int64_t full = ((p.M + 127) / 128) * ((p.N + kBN - 1) / kBN) * p.groups;
  const int64_t big = ((p.M + kBigM - 1) / kBigM) * ((p.N + kBigN - 1) / kBigN) * p.groups;
  // the 256-row form's structure: no group table, a data gradient only with class-homogeneous tiles (256 | Do^3)
  const bool dgrad = p.mode == kConvDgrad, can_big = !p.table && !(dgrad && (p.dgrad_rows & (kBigM - 1)));
  // Split of K for a forward GEMM with too few 256 x 256 tiles to fill the chip (conv4's forward at 16 objects: 32 x 2
  // tiles for 256 CUs): S workgroups per tile, each over a contiguous range of >= 16 K-tiles, fp32 partial sums in S
  // slabs, added in order by k_splitk_finish (deterministic).  1 = no split.
  int S = 1;
  if (p.may_split && p.ws_bytes > 0 && can_big && p.N >= 192 && p.N % 8 == 0 && k.nt_big != 0) {
    const int T = (p.K + kBK - 1) / kBK;
    if (k.nt_splitk > 0) S = k.nt_splitk <= T ? k.nt_splitk : 1;
    else if (big >= 16 && big < 160)
      for (S = (int)(256 / big); S > 1 && T / S < 16;) --S;
    if (S > 1 && p.ws_bytes < S * p.M * p.N * 4) S = 1;
  }
  // (N >= 160: dense conv3's data gradient, N = 160 -- one tile of 256 columns, the waves of its last 96 columns idle --
  // measured 551 -> 778 TFLOP/s on the ping-pong form against the 128 x 128 tile's two column tiles)
  bool use_big = (big >= 224 && p.N >= 160 && can_big) || S > 1;  // (a split runs on the ping-pong form only)
  if (k.nt_big == 2)  // (tests: the big tile wherever its structure allows, whatever the tile count)
    use_big = can_big;
  else if (k.nt_big >= 0)  // (a value other than 0 / 1 / 2 keeps S and drops the tile, which then ignores S)
    use_big = use_big && k.nt_big == 1;
  if (use_big) return {kBigM, S, k.pp_dbg};
  // 64-row tiles when the 128-row ones would leave CUs with fewer than two workgroups
  const bool half = full <= k.nt_half_max && !dgrad;  // (dgrad tiles must stay class-homogeneous: 128 | Do^3)
  return {half ? 64 : 128, S, 0};
}

int64_t nt_workspace_bytes(int mode, int64_t M, int N, int K) {
  const NtPlan p = nt_plan({mode, M, N, K, 1, false, 0, true, kAnyWs}, read_knobs());
  return p.S > 1 ? p.S * M * N * 4 : 0;
}

int wgrad_split_model(int64_t tiles, int64_t ktiles, int64_t slab_bytes, int slots) {
  if (tiles <= 0 || ktiles <= 0) return 1;
  const double per_slab = slab_bytes / 3.0e6 > 0.05 ? slab_bytes / 3.0e6 : 0.05;  // us at ~3 TB/s, launch floor
  int best = 1;
  double best_cost = 1e30;
  for (int S = 1; S <= 512; ++S) {
    if (S > 1 && ktiles / S < 8) break;
    const int64_t rounds = (tiles * S + slots - 1) / slots;
    const double cost = (double)rounds * (double)((ktiles + S - 1) / S + 8) + (S > 1 ? S * per_slab : 0.0);
    if (cost < best_cost) { best_cost = cost; best = S; }
  }
  return best;
}

// A weight gradient [Ni][Nj] (row pitch ldc) reduced over ``ktiles`` row tiles of 64, ``groups`` results side by side;
// ``ranges``: the rows of a group come from a device table (mf_linear_wgrad_bf16_ranges); ``conv``: the result goes
// through the (tap, cin) -> (cin, tap) finish even unsplit; ``split``: the caller's, <= 0 = ask for the default.
struct TnShape { int Ni, Nj, ldc; int64_t ktiles; int groups; bool ranges, conv; int split; };
enum { kFinishNone = 0, kFinishPlain = 1, kFinishDeep = 2, kFinishConv = 3 };  // k_wgrad_finish / _deep / _conv
struct TnPlan { bool pp; int split, finish; };

TnPlan tn_plan(const TnShape &p, const Knobs &k) {
  // The 256 x 256 ping-pong form of the TN engine (k_gemm_tn_bf16_pp) takes the weight gradients whose result has at
  // least 192 rows and columns AND whose reduction is long enough that a split filling the 256 CUs still leaves every
  // workgroup >= 48 K-tiles (its prologue / epilogue -- 256 KB of fp32 tile through LDS -- weigh on shorter ones: the
  // heads' first layer, 32 tiles x 250 K-tiles, measured 570 TFLOP/s on it against 670 on the 128 x 128 form).
  // MF_TN_PP=0: never; MF_NT_BIG=2, the tests' switch: wherever the shape allows.
  const int64_t tiles_pp = (int64_t)((p.Ni + 255) / 256) * ((p.Nj + 255) / 256) * p.groups;
  bool pp = k.tn_pp != 0 && k.nt_big != 0 && !p.ranges;
  if (pp && k.nt_big != 2)  // (256 / tiles, rounded up: the splits that fill the chip)
    pp = p.Ni >= 192 && p.Nj >= 192 && p.ktiles >= 48 * (tiles_pp >= 256 ? 1 : (256 + tiles_pp - 1) / tiles_pp);
  // the default split: the cost model on the tile / workgroup-slot counts of the form that will run (the pp form: one
  // 256 x 256 tile per CU and K-tiles of twice the work)
  const int64_t tiles = (int64_t)((p.Ni + 127) / 128) * ((p.Nj + 127) / 128) * p.groups, slab_bytes = 4ll * p.Ni * p.Nj * p.groups;
  const int split = p.split > 0 ? p.split : pp ? wgrad_split_model(tiles_pp, 2 * p.ktiles, slab_bytes, 256)
                                               : wgrad_split_model(tiles, p.ktiles, slab_bytes, 512);
  // big layers: the tiled transpose; small ones (the occupancy convolutions: a few thousand weights in up to 256
  // slabs) stay element-wise -- one thread per weight walks the slabs, where a tile's 256 threads would walk them
  // seven elements each (measured: 0.42 ms for conv2_occ's 3456 weights) -- or, from 32 slabs, one wave per weight
  const int64_t per_slab = (int64_t)p.Ni * p.ldc * p.groups;
  int finish = split >= 32 && per_slab <= (1 << 16) ? kFinishDeep : kFinishPlain;
  if (p.conv && per_slab >= (1 << 20)) finish = kFinishConv;
  if (!p.conv && split == 1) finish = kFinishNone;
  return {pp, split, finish};
}

// ---- launchers ----------------------------------------------------------------------------------------------------
int g_nt_last_tile = 0;  // rows of the tile the last NT launch used (64 / 128 / 256): mf_gemm_bf16_last_tile

template <int MODE, int MI>
int launch_nt_tile(const NtArgs &a, hipStream_t stream) {
  if (int e = mf::allow_big_lds((const void *)k_gemm_nt_bf16<MODE, MI>, nt_lds<MI>())) return e;
  const int64_t grid = (int64_t)((a.M + 64 * MI - 1) / (64 * MI)) * ((a.N + kBN - 1) / kBN) * a.groups;
  hipLaunchKernelGGL((k_gemm_nt_bf16<MODE, MI>), dim3((unsigned)grid), dim3(256), nt_lds<MI>(), stream, a);
  return 0;
}
template <int MODE>
int launch_nt(const NtArgs &a, const NtPlan &p, hipStream_t stream, const char *what) {
  g_nt_last_tile = p.tile;
  if (p.tile == kBigM) {
    const int64_t big = (int64_t)((a.M + kBigM - 1) / kBigM) * ((a.N + kBigN - 1) / kBigN) * a.groups;
    if (int e = mf::allow_big_lds((const void *)k_gemm_nt_bf16_pp<MODE>, nt_pp_lds())) return e;
    hipLaunchKernelGGL((k_gemm_nt_bf16_pp<MODE>), dim3((unsigned)(big * a.S)), dim3(512), nt_pp_lds(), stream, a);
    const dim3 finish((unsigned)(((int64_t)a.M * (a.N / 8) + 255) / 256));
    if (a.S > 1 && nt_split(MODE))
      hipLaunchKernelGGL(k_splitk_finish_conv2, finish, dim3(256), 0, stream, a);
    else if (a.S > 1)
      hipLaunchKernelGGL(k_splitk_finish, finish, dim3(256), 0, stream, (const float *)a.slab, a.bias, a.out,
                         (int64_t)a.M, a.N, a.S, a.ldo, a.relu, a.out_f32);
  } else if (int e = p.tile == 64 ? launch_nt_tile<MODE, 1>(a, stream) : launch_nt_tile<MODE, 2>(a, stream))
    return e;
  return mf::check_launch(what);
}

template <bool CONV>
int launch_tn(const TnArgs &a, const TnPlan &p, hipStream_t stream) {
  if (p.pp) {
    if (int e = mf::allow_big_lds((const void *)k_gemm_tn_bf16_pp<CONV>, 5 * kPpOp)) return e;
    const int64_t grid = (int64_t)((a.Ni + 255) / 256) * ((a.Nj + 255) / 256) * a.groups * a.S;
    hipLaunchKernelGGL(k_gemm_tn_bf16_pp<CONV>, dim3((unsigned)grid), dim3(512), 5 * kPpOp, stream, a);
    return 0;
  }
  if (int e = mf::allow_big_lds((const void *)k_gemm_tn_bf16<CONV>, kTnLds)) return e;
  const int64_t grid = (int64_t)((a.Ni + 127) / 128) * ((a.Nj + 127) / 128) * a.groups * a.S;
  hipLaunchKernelGGL(k_gemm_tn_bf16<CONV>, dim3((unsigned)grid), dim3(256), kTnLds, stream, a);
  return 0;
}

// the slabs a.out [S][groups][Ni][ldc] summed in order into dW; conv: [Ni][w_cin][taps], input channels < ``keep``
void launch_wgrad_finish(int finish, const TnArgs &a, float *dW, int w_cin, int keep, hipStream_t stream) {
  const int taps = a.conv ? a.ks * a.ks * a.ks : 0, cin = a.conv ? a.Cin : 0;
  const int64_t per_group = (int64_t)a.Ni * a.ldc, per_slab = per_group * a.groups;
  const int64_t pitch = a.conv ? (int64_t)w_cin * taps : a.ldc;
  if (finish == kFinishConv)
    hipLaunchKernelGGL(k_wgrad_finish_conv, dim3((keep + kPackTile - 1) / kPackTile, a.Ni), dim3(256), 0, stream,
                       (const float *)a.out, dW, per_slab, a.S, a.Cin, taps, w_cin, keep);
  else if (finish == kFinishDeep)
    hipLaunchKernelGGL(k_wgrad_finish_deep, dim3((unsigned)((per_slab + 3) / 4)), dim3(256), 0, stream,
                       (const float *)a.out, dW, per_slab, a.Nj, a.ldc, a.S, cin, a.c_gs, per_group, pitch, taps, keep);
  else if (finish == kFinishPlain)
    hipLaunchKernelGGL(k_wgrad_finish, dim3((unsigned)((per_slab + 255) / 256)), dim3(256), 0, stream,
                       (const float *)a.out, dW, per_slab, a.Nj, a.ldc, a.S, cin, a.c_gs, per_group, pitch, taps, keep);
}

// ---- argument checks and the fields of NtArgs ---------------------------------------------------------------------
constexpr int64_t kMaxBf16Elems = 1ll << 30;  // 2^31 bytes: the span of a buffer resource (mf_common.h kBufSpan)
int bad(const char *msg) {
  mf::set_last_error(hipErrorInvalidValue, msg);
  return -(int)hipErrorInvalidValue;
}

int ilog2_exact(int x) {
  int l = 0;
  while ((1 << l) < x) ++l;
  return (1 << l) == x ? l : -1;
}

/* Convolution3D on channels-last bf16 grids: kernel ks in {3, 4}, stride in {1, 2}, any pad / dilation whose output
 * size Do = (D + 2 pad - dil (ks - 1) - 1) / stride + 1 is a power of two.  W: fp32 in the framework layout
 * [Cout][w_cin][ks][ks][ks]. */
struct Geom { int Do, olog, taps; };
int conv_geom(int B, int Cin, int Cout, int D, int ks, int stride, int pad, int dil, Geom *g) {
  const int span = dil * (ks - 1) + 1;
  if ((ks != 3 && ks != 4) || (stride != 1 && stride != 2) || dil < 1 || pad < 0 || D + 2 * pad < span)
    return bad("conv3d (bf16): kernel 3 or 4, stride 1 or 2");
  g->Do = (D + 2 * pad - span) / stride + 1;
  g->olog = ilog2_exact(g->Do);
  g->taps = ks * ks * ks;
  // operands are addressed with 32-bit BYTE offsets from a buffer resource of 2^31 bytes (mf_common.h: an offset
  // >= 2^31 is the masked value and reads zeros): every bf16 tensor must stay below 2^30 ELEMENTS
  if (g->olog < 1 || Cin % 8 || Cout % 8 || (int64_t)B * D * D * D * Cin >= kMaxBf16Elems ||
      (int64_t)B * g->Do * g->Do * g->Do * Cout >= kMaxBf16Elems || (int64_t)Cout * g->taps * Cin >= kMaxBf16Elems)
    return bad("conv3d (bf16): output size a power of two, Cin % 8 == 0, Cout % 8 == 0, tensors < 2^30 elements (2^31 bytes)");
  return 0;
}

int conv2_geom(int B, int Cin, int Cout, int D, int ks, int stride, int pad, int dil, Geom *g) {
  const int span = dil * (ks - 1) + 1;
  if ((ks != 1 && ks != 3) || (stride != 1 && stride != 2) || dil < 1 || dil > 4 || pad < 0 || D + 2 * pad < span)
    return bad("conv2d_split: kernel 1 or 3, stride 1 or 2, dilation 1 .. 4");
  g->Do = (D + 2 * pad - span) / stride + 1;
  g->olog = ilog2_exact(g->Do);
  g->taps = ks * ks;
  if (g->olog < 0 || Cin % 8 || Cout % 8 || (int64_t)B * D * D * 2 * Cin >= kMaxBf16Elems ||
      (int64_t)B * g->Do * g->Do >= (1ll << 31) || (int64_t)Cout * g->taps * 3 * Cin >= kMaxBf16Elems)
    return bad("conv2d_split: output side a power of two, Cin % 8 == 0, Cout % 8 == 0, operands < 2^30 elements");
  return 0;
}

// a split-bf16 forward's outputs (conv2d: and residual): one at least, pitches >= N, % 8, lo plane in the row, aligned
int split_out_check(const char *what, const float *bias, float *out32, int ldo32, void *outs, int ldos, int los, int N,
                    const float *res = nullptr, int ldr = 0) {
  if ((!out32 && !outs) || N % 8 || (out32 && (ldo32 < N || ldo32 % 8)) ||
      (outs && (ldos < N || ldos % 8 || los < N || los % 8 || ldos < los + N)) || (res && (ldr < N || ldr % 8)))
    return bad(what);
  if (((uintptr_t)bias | (uintptr_t)out32 | (uintptr_t)outs | (uintptr_t)res) & 15) return bad(what);
  return 0;
}

// NtArgs is filled by these and nowhere else: operands and problem, conv geometry, one of the two output forms
NtArgs nt_operands(const void *A, int lda, int64_t a_gs, const void *W, int ldw, int64_t w_gs, const float *bias,
                   int64_t b_gs, int64_t M, int N, int K, int groups, const int32_t *tile_group = nullptr) {
  NtArgs a = {};
  a.A = (const uint16_t *)A; a.W = (const uint16_t *)W; a.bias = bias;
  a.a_gs = a_gs; a.w_gs = w_gs; a.b_gs = b_gs;
  a.M = (int)M; a.N = N; a.K = K; a.lda = lda; a.ldw = ldw; a.groups = groups;
  a.tile_group = tile_group;
  return a;
}
void nt_conv_geom(NtArgs &a, int B, int D, const Geom &g, int Cin, int Cout, int ks, int stride, int pad, int dil) {
  // (Cin: the K length of one tap -- 3 C for the split operands)
  a.B = B; a.D = D; a.Do = g.Do; a.olog = g.olog; a.Cin = Cin; a.Cout = Cout;
  a.ks = ks; a.stride = stride; a.pad = pad; a.dil = dil;
}
void nt_plain_out(NtArgs &a, void *out, int64_t o_gs, int ldo, int relu, int out_f32, int accumulate, const NtPlan &p,
                  void *ws = nullptr) {
  a.out = out; a.o_gs = o_gs; a.ldo = ldo; a.relu = relu; a.out_f32 = out_f32; a.accumulate = accumulate;
  a.S = p.S; a.slab = p.S > 1 ? (float *)ws : nullptr; a.dbg = p.dbg;
}
template <int MODE>
int launch_nt_split(NtArgs a, int xc, int act, float *out32, int ldo32, void *outs, int ldos, int los, void *ws,
                    int64_t ws_bytes, mfStream_t stream, const char *what, const float *res = nullptr, int ldr = 0,
                    const float *slope = nullptr) {
  const NtPlan p = nt_plan({MODE, a.M, a.N, a.K, 1, false, 0, true, ws ? ws_bytes : 0}, read_knobs());
  a.xc = xc; a.act = act; a.ldo32 = ldo32; a.ldos = ldos; a.los = los; a.out32 = out32; a.outs = (uint16_t *)outs;
  a.res = res; a.ldr = ldr; a.slope = slope;
  a.S = p.S; a.slab = p.S > 1 ? (float *)ws : nullptr; a.dbg = p.dbg;
  return launch_nt<MODE>(a, p, (hipStream_t)stream, what);
}

}  // namespace

/* nt_plan / tn_plan for the outside (include/mfhip.h): no device call */
extern "C" int mf_gemm_bf16_nt_plan(int32_t mode, int64_t M, int32_t N, int32_t K, int32_t groups, int32_t table,
                                    int64_t dgrad_rows, int32_t may_split, int32_t have_ws, int32_t *tile, int32_t *S) {
  if (mode < kRows || mode > kRowsS || M <= 0 || N <= 0 || K <= 0 || groups <= 0 || !tile || !S)
    return bad("gemm_bf16_nt_plan: a mode 0 .. 5, a problem, somewhere to answer");
  const NtShape s = {mode, M, N, K, groups, table != 0, dgrad_rows, may_split != 0, have_ws ? kAnyWs : 0};
  const NtPlan p = nt_plan(s, read_knobs());
  *tile = p.tile; *S = p.S;
  return 0;
}

extern "C" int mf_gemm_bf16_tn_plan(int32_t Ni, int32_t Nj, int32_t ldc, int64_t rows, int32_t groups, int32_t ranges,
                                    int32_t conv, int32_t split, int32_t *form, int32_t *default_split, int32_t *finish) {
  if (Ni <= 0 || Nj <= 0 || ldc < Nj || rows < 0 || groups <= 0 || !form || !default_split || !finish)
    return bad("gemm_bf16_tn_plan: a problem with ldc >= Nj, somewhere to answer");
  const Knobs k = read_knobs();
  TnShape s = {Ni, Nj, ldc, (rows + 63) / 64, groups, ranges != 0, conv != 0, 0};
  *default_split = s.split = tn_plan(s, k).split;
  if (split > 0) s.split = split;
  const TnPlan p = tn_plan(s, k);
  *form = p.pp ? 256 : 128; *finish = p.finish;
  return 0;
}

/* Tile height (64 / 128 / 256 rows) of the NT engine's most recent launch in this process: lets tests and the
 * timing tools see which form of the engine a problem was given to (nt_plan's choice, MF_NT_BIG). */
extern "C" int mf_gemm_bf16_last_tile(void) { return g_nt_last_tile; }

extern "C" int mf_cast_rows_bf16(const float *src, int64_t src_ld, void *dst, int64_t dst_ld, int64_t rows,
                                 int32_t cols, mfStream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (rows <= 0) return 0;
  if (dst_ld % 8 || cols > dst_ld || src_ld < cols || ((uintptr_t)dst & 15)) return bad("cast_rows_bf16: dst_ld % 8 == 0, cols <= dst_ld");
  const int64_t n = rows * (dst_ld / 8);
  hipLaunchKernelGGL(k_cast_rows_bf16, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, src, src_ld,
                     (uint16_t *)dst, dst_ld, rows, cols);
  return mf::check_launch("mf_cast_rows_bf16");
}

extern "C" int mf_relu_mask_bf16(const void *y, const void *dy, const float *dy32, void *dz, int64_t n,
                                 mfStream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (n <= 0) return 0;
  if (n % 8 || (!dy == !dy32)) return bad("relu_mask_bf16: n % 8 == 0 and exactly one of dy / dy32");
  hipLaunchKernelGGL(k_relu_mask_bf16, dim3((unsigned)((n / 8 + 255) / 256)), dim3(256), 0, stream,
                     (const uint16_t *)y, (const uint16_t *)dy, dy32, (uint16_t *)dz, n / 8);
  return mf::check_launch("mf_relu_mask_bf16");
}

/* out = act(A W^T + bias): A bf16 [M][lda], W bf16 [N][ldw] (k-contiguous rows), bias fp32; out bf16 or fp32
 * [M][ldo] (accumulate: out += , fp32 only); ``groups`` independent problems at the given element strides. */
extern "C" int mf_linear_bf16(const void *A, int64_t a_gs, int32_t lda, const void *W, int64_t w_gs, int32_t ldw,
                              const float *bias, int64_t b_gs, void *out, int64_t o_gs, int32_t ldo, int32_t M,
                              int32_t N, int32_t K, int32_t groups, int32_t relu, int32_t out_f32,
                              int32_t accumulate, mfStream_t stream_) {
  if (M <= 0 || N <= 0 || groups <= 0) return 0;
  if (K <= 0 || K % 8 || lda % 8 || ldw % 8 || a_gs % 8 || w_gs % 8 || lda < K || ldw < K || ldo < N ||
      (((uintptr_t)A | (uintptr_t)W) & 15) || (accumulate && !out_f32))
    return bad("linear_bf16: K, lda, ldw, group strides % 8 == 0, 16-byte aligned A / W, accumulate needs fp32 out");
  if ((int64_t)M * lda >= kMaxBf16Elems || (int64_t)N * ldw >= kMaxBf16Elems)
    return bad("linear_bf16: an operand of one group spans >= 2^31 bytes (32-bit byte offsets: split the rows)");
  NtArgs a = nt_operands(A, lda, a_gs, W, ldw, w_gs, bias, b_gs, M, N, K, groups);
  const NtPlan p = nt_plan({kRows, M, N, K, groups, false, 0, false, 0}, read_knobs());
  nt_plain_out(a, out, o_gs, ldo, relu, out_f32, accumulate, p);
  return launch_nt<kRows>(a, p, (hipStream_t)stream_, "mf_linear_bf16");
}

/* Weight gradient of out = A W^T: dW[n][k] (fp32, row pitch ldc) = sum_m dY[m][n] A[m][k]; ``split`` > 1: partial
 * sums over row ranges in ws (split * groups * N * ldc floats), added in order. */
extern "C" int mf_linear_wgrad_bf16(const void *dY, int64_t y_gs, int32_t ldy, const void *A, int64_t a_gs, int32_t lda,
                                    float *dW, int64_t w_gs, int32_t ldc, void *ws, int32_t M, int32_t N, int32_t K,
                                    int32_t groups, int32_t split, mfStream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (M <= 0 || N <= 0 || K <= 0 || groups <= 0) return 0;
  if (N % 8 || K % 8 || ldy % 8 || lda % 8 || y_gs % 8 || a_gs % 8 || split < 1 || (split > 1 && !ws) || ldc < K ||
      (((uintptr_t)dY | (uintptr_t)A) & 15))
    return bad("linear_wgrad_bf16: N, K, ldy, lda, group strides % 8 == 0, 16-byte aligned operands");
  if ((int64_t)M * ldy >= kMaxBf16Elems || (int64_t)M * lda >= kMaxBf16Elems)
    return bad("linear_wgrad_bf16: an operand of one group spans >= 2^31 bytes (32-bit byte offsets: split the rows)");
  TnArgs a = {};
  a.P = (const uint16_t *)dY; a.Q = (const uint16_t *)A; a.out = split > 1 ? (float *)ws : dW;
  a.p_gs = y_gs; a.q_gs = a_gs; a.c_gs = w_gs;
  a.M = M; a.Ni = N; a.Nj = K; a.ldp = ldy; a.ldq = lda; a.ldc = ldc; a.groups = groups; a.S = split;
  const TnPlan p = tn_plan({N, K, ldc, ((int64_t)M + 63) / 64, groups, false, false, split}, read_knobs());
  if (int e = launch_tn<false>(a, p, stream)) return e;
  launch_wgrad_finish(p.finish, a, dW, 0, 0, stream);
  return mf::check_launch("mf_linear_wgrad_bf16");
}

/* mf_linear_bf16 for rows that come in GROUPS with their own weights, the group of every 64-row block read from a
 * device table (``tile_group`` [ceil(M / 64)], -1 = empty block; groups are padded to multiples of 128 rows by the
 * producer): out[m][:] = A[m][:] W[group(m)]^T.  W: [n_groups][N][ldw] at group stride ``w_gs``.  No bias / ReLU. */
extern "C" int mf_linear_bf16_tiles(const void *A, int32_t lda, const void *W, int64_t w_gs, int32_t ldw,
                                    const int32_t *tile_group, void *out, int32_t ldo, int32_t M, int32_t N, int32_t K,
                                    int32_t out_f32, mfStream_t stream_) {
  if (M <= 0 || N <= 0) return 0;
  if (K <= 0 || K % 8 || lda % 8 || ldw % 8 || w_gs % 8 || lda < K || ldw < K || ldo < N || M % 128 || !tile_group ||
      (((uintptr_t)A | (uintptr_t)W) & 15))
    return bad("linear_bf16_tiles: K, lda, ldw, w_gs % 8 == 0, M % 128 == 0, 16-byte aligned A / W, a group table");
  if ((int64_t)M * lda >= kMaxBf16Elems || (int64_t)N * ldw >= kMaxBf16Elems)
    return bad("linear_bf16_tiles: an operand spans >= 2^31 bytes");
  NtArgs a = nt_operands(A, lda, 0, W, ldw, w_gs, nullptr, 0, M, N, K, 1, tile_group);
  const NtPlan p = nt_plan({kRows, M, N, K, 1, true, 0, false, 0}, read_knobs());
  nt_plain_out(a, out, 0, ldo, 0, out_f32, 0, p);
  return launch_nt<kRows>(a, p, (hipStream_t)stream_, "mf_linear_bf16_tiles");
}

/* mf_linear_wgrad_bf16 over row RANGES read from the device: dW[g][n][k] = sum over rows m in
 * [m_range[g], m_range[g + 1]) of dY[m][n] A[m][k] for g < groups (ranges are multiples of 64 rows; rows of a range
 * that hold no data must be zero in one operand).  dW fp32 [groups][N][ldc] at group stride ``w_gs``. */
extern "C" int mf_linear_wgrad_bf16_ranges(const void *dY, int32_t ldy, const void *A, int32_t lda, float *dW,
                                           int64_t w_gs, int32_t ldc, const int32_t *m_range, int32_t groups, int32_t N,
                                           int32_t K, mfStream_t stream_) {
  if (N <= 0 || K <= 0 || groups <= 0) return 0;
  if (N % 8 || K % 8 || ldy % 8 || lda % 8 || ldc < K || !m_range || (((uintptr_t)dY | (uintptr_t)A) & 15))
    return bad("linear_wgrad_bf16_ranges: N, K, ldy, lda % 8 == 0, 16-byte aligned operands, a range table");
  TnArgs a = {};
  a.P = (const uint16_t *)dY; a.Q = (const uint16_t *)A; a.out = dW;
  a.c_gs = w_gs;
  a.M = 0; a.Ni = N; a.Nj = K; a.ldp = ldy; a.ldq = lda; a.ldc = ldc; a.groups = groups; a.S = 1;
  a.m_range = m_range;
  if (int e = launch_tn<false>(a, tn_plan({N, K, ldc, 0, groups, true, false, 1}, read_knobs()), (hipStream_t)stream_))
    return e;
  return mf::check_launch("mf_linear_wgrad_bf16_ranges");
}

extern "C" int64_t mf_conv3d_bf16_fwd_workspace_bytes(int32_t B, int32_t Cin, int32_t Cout, int32_t D, int32_t ks,
                                                      int32_t stride, int32_t pad, int32_t dil) {
  Geom g;
  if (B <= 0 || conv_geom(B, Cin, Cout, D, ks, stride, pad, dil, &g)) return 0;
  return nt_workspace_bytes(kConvFwd, (int64_t)B * g.Do * g.Do * g.Do, Cout, g.taps * Cin);
}

extern "C" int mf_conv3d_bf16_pack(const float *W, int32_t Cout, int32_t Cin, int32_t w_cin, int32_t c_off, int32_t ks,
                                   void *fwd, void *dgrad_k4s2, void *flipT, mfStream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if ((ks != 3 && ks != 4) || (dgrad_k4s2 && ks != 4)) return bad("conv3d_bf16_pack: kernel 3 or 4 (parity-class dgrad: 4)");
  const int taps = ks * ks * ks;
  if (fwd)
    hipLaunchKernelGGL(k_conv_pack_fwd_tile, dim3((Cin + kPackTile - 1) / kPackTile, Cout), dim3(256), 0, stream, W, Cin,
                       w_cin, c_off, taps, (uint16_t *)fwd);
  if (dgrad_k4s2 || flipT)
    hipLaunchKernelGGL(k_conv_pack_cof_tile, dim3((Cout + kPackTile - 1) / kPackTile, Cin), dim3(256), 0, stream, W,
                       Cout, Cin, w_cin, c_off, ks, (uint16_t *)dgrad_k4s2, (uint16_t *)flipT);
  return mf::check_launch("mf_conv3d_bf16_pack");
}

/* out [B][Do^3][ldo >= Cout] = act(conv(x [B][D^3][Cin]) + bias): x, wt ([Cout][ks^3][Cin]) bf16; out bf16 / fp32.
 * ws: mf_conv3d_bf16_fwd_workspace_bytes(...) bytes (0: none needed, ws may be null): a layer with too few output
 * tiles for the chip splits its reduction over the workspace's fp32 slabs; without a workspace it runs unsplit. */
extern "C" int mf_conv3d_bf16_fwd_ws(const void *x, const void *wt, const float *bias, void *out, void *ws,
                                     int64_t ws_bytes, int32_t B, int32_t Cin, int32_t Cout, int32_t D, int32_t ks,
                                     int32_t stride, int32_t pad, int32_t dil, int32_t relu, int32_t out_f32,
                                     int32_t ldo, mfStream_t stream_) {
  if (B <= 0) return 0;
  Geom g;
  if (int e = conv_geom(B, Cin, Cout, D, ks, stride, pad, dil, &g)) return e;
  if (ldo < Cout) return bad("conv3d_bf16_fwd / _ws: ldo >= Cout");
  const int64_t M = (int64_t)B * g.Do * g.Do * g.Do;
  const NtPlan p = nt_plan({kConvFwd, M, Cout, g.taps * Cin, 1, false, 0, true, ws ? kAnyWs : 0}, read_knobs());
  if (p.S > 1 && (ws_bytes < p.S * M * Cout * 4 || ((uintptr_t)ws & 15))) return bad("conv3d_bf16_fwd_ws: workspace too small / unaligned");
  NtArgs a = nt_operands(x, 0, 0, wt, g.taps * Cin, 0, bias, 0, M, Cout, g.taps * Cin, 1);
  nt_conv_geom(a, B, D, g, Cin, Cout, ks, stride, pad, dil);
  nt_plain_out(a, out, 0, ldo, relu, out_f32, 0, p, ws);
  return launch_nt<kConvFwd>(a, p, (hipStream_t)stream_, "mf_conv3d_bf16_fwd");
}

extern "C" int mf_conv3d_bf16_fwd(const void *x, const void *wt, const float *bias, void *out, int32_t B, int32_t Cin,
                                  int32_t Cout, int32_t D, int32_t ks, int32_t stride, int32_t pad, int32_t dil,
                                  int32_t relu, int32_t out_f32, int32_t ldo, mfStream_t stream) {
  return mf_conv3d_bf16_fwd_ws(x, wt, bias, out, nullptr, 0, B, Cin, Cout, D, ks, stride, pad, dil, relu, out_f32, ldo, stream);
}

/* dx [B][D^3][Cin] (+)= conv^T(dy [B][(D/2)^3][Cout]) of the k4 / s2 / p1 layers: dy, wd (packed parity-class layout)
 * bf16; dx bf16, or fp32 with ``accumulate`` (dx already holds another consumer's gradient).  (Stride-1 layers take
 * their data gradient through mf_conv3d_bf16_fwd on the flipT operand.) */
extern "C" int mf_conv3d_k4s2_bf16_dgrad(const void *dy, const void *wd, void *dx, int32_t B, int32_t Cin,
                                         int32_t Cout, int32_t D, int32_t out_f32, int32_t accumulate,
                                         mfStream_t stream_) {
  if (B <= 0) return 0;
  Geom g;
  if (int e = conv_geom(B, Cin, Cout, D, 4, 2, 1, 1, &g)) return e;
  const int64_t Do3 = (int64_t)g.Do * g.Do * g.Do, M = (int64_t)B * D * D * D;
  if (Do3 % 128 || (accumulate && !out_f32)) return bad("conv3d_k4s2 dgrad: (D/2)^3 % 128 == 0; accumulate needs fp32");
  NtArgs a = nt_operands(dy, 0, 0, wd, 8 * Cout, 0, nullptr, 0, M, Cin, 8 * Cout, 1);
  nt_conv_geom(a, B, D, g, Cin, Cout, 4, 2, 1, 1);
  const NtPlan p = nt_plan({kConvDgrad, M, Cin, 8 * Cout, 1, false, Do3, false, 0}, read_knobs());
  nt_plain_out(a, dx, 0, Cin, 0, out_f32, accumulate, p);
  return launch_nt<kConvDgrad>(a, p, (hipStream_t)stream_, "mf_conv3d_k4s2_bf16_dgrad");
}

extern "C" int64_t mf_conv3d_bf16_wgrad_workspace_bytes(int32_t Cin, int32_t Cout, int32_t ks, int32_t split) {
  return (int64_t)(split > 1 ? split : 1) * Cout * ks * ks * ks * Cin * 4;
}

/* Split of the reduction (rows) of a weight-gradient GEMM over S workgroups per output tile, S fp32 slabs summed by
 * the finish pass.  ``tiles`` output tiles of 128 x 128, ``ktiles`` row tiles of 64, ``slab_bytes`` = size of one
 * slab.  Cost model in units of one K-tile of one workgroup (~1 us at two workgroups per CU, 512 slots on the chip):
 *   ceil(tiles S / 512) rounds x (ceil(ktiles / S) + 8 K-tiles of prologue / epilogue)  +  S slabs read by the finish
 * -- the first version doubled S until tiles * S >= 512, which put conv3 (160 tiles) at S = 4: 640 workgroups, a
 * second round a quarter full; S = 3 fills one round.  (The 128 x 128 form's model; mf_linear_wgrad_bf16_default_split
 * / mf_conv3d_bf16_wgrad_default_split answer for the form that will actually run.) */
extern "C" int32_t mf_wgrad_split(int64_t tiles, int64_t ktiles, int64_t slab_bytes) {
  return wgrad_split_model(tiles, ktiles, slab_bytes, 512);
}

extern "C" int32_t mf_linear_wgrad_bf16_default_split(int64_t M, int32_t N, int32_t K, int32_t groups) {
  return tn_plan({N, K, K, (M + 63) / 64, groups, false, false, 0}, read_knobs()).split;
}

extern "C" int32_t mf_conv3d_bf16_wgrad_default_split(int32_t B, int32_t Cin, int32_t Cout, int32_t Do, int32_t ks) {
  const int Nj = ks * ks * ks * Cin;
  return tn_plan({Cout, Nj, Nj, ((int64_t)B * Do * Do * Do + 63) / 64, 1, false, true, 0}, read_knobs()).split;
}

/* dW [Cout][w_cin][ks][ks][ks] (input channels c_off .., those below w_cin: fp32, the framework layout) = sum over
 * output voxels of dy (x) im2col(x); ws: mf_conv3d_bf16_wgrad_workspace_bytes. */
extern "C" int mf_conv3d_bf16_wgrad(const void *dy, const void *x, float *dW, void *ws, int32_t B, int32_t Cin,
                                    int32_t Cout, int32_t D, int32_t ks, int32_t stride, int32_t pad, int32_t dil,
                                    int32_t w_cin, int32_t c_off, int32_t split, mfStream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (B <= 0) return 0;
  Geom g;
  if (int e = conv_geom(B, Cin, Cout, D, ks, stride, pad, dil, &g)) return e;
  if (split < 1 || !ws) return bad("conv3d wgrad: workspace required");
  if (g.olog < 2) return bad("conv3d wgrad: output size >= 4 per axis");
  TnArgs a = {};
  a.P = (const uint16_t *)dy; a.Q = (const uint16_t *)x; a.out = (float *)ws;
  a.M = B * g.Do * g.Do * g.Do; a.Ni = Cout; a.Nj = g.taps * Cin; a.ldp = Cout; a.ldc = g.taps * Cin; a.groups = 1;
  a.S = split;
  a.conv = 1; a.B = B; a.D = D; a.Do = g.Do; a.olog = g.olog; a.Cin = Cin;
  a.ks = ks; a.stride = stride; a.pad = pad; a.dil = dil;
  // (S == 1 also goes through the workspace: the finish pass permutes (tap, cin) -> (cin, tap))
  const TnPlan p = tn_plan({a.Ni, a.Nj, a.ldc, ((int64_t)a.M + 63) / 64, 1, false, true, split}, read_knobs());
  if (int e = launch_tn<true>(a, p, stream)) return e;
  const int keep = w_cin - c_off < Cin ? w_cin - c_off : Cin;
  if (keep > 0) launch_wgrad_finish(p.finish, a, dW + (int64_t)c_off * g.taps, w_cin, keep, stream);
  return mf::check_launch("mf_conv3d_bf16_wgrad");
}

/* 3 x 3 x 3 convolutions (stride 1, pad = dil) between narrow layers -- Cin in {8, 16}, Cout <= 16 -- on channels-last
 * bf16 grids whose size D is a power of two: the occupancy branch's conv1_occ / conv2_occ and conv2_occ's data
 * gradient (``transpose`` at pack time).  wp: 32 x ceil(27 CI / 16) x 16 bf16 from mf_conv3d_k3_narrow_bf16_pack
 * (CI = the channels of the tensor the convolution READS: Cin forward, Cout for the data gradient). */
extern "C" int64_t mf_conv3d_k3_narrow_bf16_pack_elems(int32_t CI) { return (int64_t)32 * ((27 * CI + 15) / 16) * 16; }

extern "C" int mf_conv3d_k3_narrow_bf16_pack(const float *W, int32_t Cout, int32_t Cin, int32_t w_cin, int32_t c_off,
                                             int32_t transpose, void *wp, mfStream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const int CI = transpose ? Cout : Cin, NO = transpose ? Cin : Cout;
  if ((CI != 8 && CI != 16) || NO < 1 || NO > 16 || (NO & 3)) return bad("conv3d_k3_narrow pack: read channels 8 or 16, written channels 4 .. 16 (% 4)");
  const int Kp = ((27 * CI + 15) / 16) * 16;
  hipLaunchKernelGGL(k_conv_k3_narrow_pack, dim3((32 * Kp + 255) / 256), dim3(256), 0, stream, W, Cout, Cin, w_cin, c_off,
                     transpose, CI, Kp, (uint16_t *)wp);
  return mf::check_launch("mf_conv3d_k3_narrow_bf16_pack");
}

extern "C" int mf_conv3d_k3_narrow_bf16(const void *x, const void *wp, const float *bias, void *out, int32_t B,
                                        int32_t CI, int32_t CO, int32_t D, int32_t dil, int32_t relu,
                                        mfStream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (B <= 0) return 0;
  const int dlog = ilog2_exact(D);
  if ((CI != 8 && CI != 16) || CO < 1 || CO > 16 || (CO & 3) || dlog < 1 || dil < 1 ||
      (int64_t)B * D * D * D * 16 >= kMaxBf16Elems || (((uintptr_t)x | (uintptr_t)wp | (uintptr_t)out) & 15))
    return bad("conv3d_k3_narrow: read channels 8 or 16, written channels 4 .. 16 (% 4), D a power of two, 16-byte aligned");
  const int64_t tiles = ((int64_t)B * D * D * D + 31) / 32;
  // a wave walks a few tiles with its weights in registers; enough workgroups (4 waves) for every CU
  int tpw = 1;
  while (tpw < 8 && tiles / (4 * tpw * 2) >= 2048) tpw *= 2;
  const unsigned blocks = (unsigned)((tiles + 4 * tpw - 1) / (4 * tpw));
  if (CI == 8)
    hipLaunchKernelGGL((k_conv_k3_narrow_bf16<8, 14>), dim3(blocks), dim3(256), 0, stream, (const uint16_t *)x,
                       (const uint16_t *)wp, bias, (uint16_t *)out, B, D, dlog, CO, dil, relu, tpw);
  else
    hipLaunchKernelGGL((k_conv_k3_narrow_bf16<16, 27>), dim3(blocks), dim3(256), 0, stream, (const uint16_t *)x,
                       (const uint16_t *)wp, bias, (uint16_t *)out, B, D, dlog, CO, dil, relu, tpw);
  return mf::check_launch("mf_conv3d_k3_narrow_bf16");
}

/* the k4 / s2 / p1 forms (conv3, conv4) under their round-4 names */
extern "C" int mf_conv3d_k4s2_pack_bf16(const float *W, int32_t Cout, int32_t Cin, int32_t w_cin, int32_t c_off,
                                        void *fwd, void *dgrad, mfStream_t stream) {
  return mf_conv3d_bf16_pack(W, Cout, Cin, w_cin, c_off, 4, fwd, dgrad, nullptr, stream);
}
extern "C" int mf_conv3d_k4s2_bf16_fwd(const void *x, const void *wt, const float *bias, void *out, int32_t B,
                                       int32_t Cin, int32_t Cout, int32_t D, int32_t relu, int32_t out_f32,
                                       mfStream_t stream) {
  return mf_conv3d_bf16_fwd(x, wt, bias, out, B, Cin, Cout, D, 4, 2, 1, 1, relu, out_f32, Cout, stream);
}
extern "C" int64_t mf_conv3d_k4s2_bf16_wgrad_workspace_bytes(int32_t Cin, int32_t Cout, int32_t split) {
  return mf_conv3d_bf16_wgrad_workspace_bytes(Cin, Cout, 4, split);
}
extern "C" int32_t mf_conv3d_k4s2_bf16_wgrad_default_split(int32_t B, int32_t Cin, int32_t Cout, int32_t D) {
  return mf_conv3d_bf16_wgrad_default_split(B, Cin, Cout, D / 2, 4);
}
extern "C" int mf_conv3d_k4s2_bf16_wgrad(const void *dy, const void *x, float *dW, void *ws, int32_t B, int32_t Cin,
                                         int32_t Cout, int32_t D, int32_t w_cin, int32_t c_off, int32_t split,
                                         mfStream_t stream) {
  return mf_conv3d_bf16_wgrad(dy, x, dW, ws, B, Cin, Cout, D, 4, 2, 1, 1, w_cin, c_off, split, stream);
}

/* 2-D convolutions of the inference backbone as split-bf16 GEMMs.  An fp32 value x is carried as
 * hi = bf16(x) and lo = bf16(x - hi); a product x w is taken as hi hi + lo w_hi + hi w_lo (three exact bf16 products,
 * fp32 accumulation): relative error per product <= ~3 * 2^-18, the dropped lo lo term included.
 *   xs   bf16 [B][D][D][2 Cin]  (channels-last map: the Cin hi channels, then the Cin lo channels)
 *   wp   bf16 [Cout][ks^2][3 Cin] from mf_conv2d_split_pack
 *   out  row m = (b, oy, ox) of the Do x Do output map, Do = (D + 2 pad - dil (ks - 1) - 1) / stride + 1 a power of two:
 *        v = act(conv + bias + res[m])  (act 0 none, 1 ReLU, 2 PReLU with the single slope *slope: read on the device)
 *        out32[m * ldo32 + n] = v  and / or  outs[m * ldos + n] = hi(v), outs[m * ldos + los + n] = lo(v)
 *   ws   mf_conv2d_split_workspace_bytes(...) bytes of fp32 split-K slabs (0: none needed, ws may be null) */
extern "C" int mf_conv2d_split_pack(const float *W, int32_t Cout, int32_t Cin, int32_t ks, void *wp, mfStream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (Cout <= 0 || Cin <= 0) return 0;
  if ((ks != 1 && ks != 3) || ((uintptr_t)wp & 15)) return bad("conv2d_split_pack: kernel 1 or 3, aligned output");
  const int64_t n = (int64_t)Cout * ks * ks * 3 * Cin;
  hipLaunchKernelGGL(k_conv2_pack_split, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, W, Cout, Cin, Cin, 0,
                     ks * ks, (uint16_t *)wp);
  return mf::check_launch("mf_conv2d_split_pack");
}

extern "C" int64_t mf_conv2d_split_workspace_bytes(int32_t B, int32_t Cin, int32_t Cout, int32_t D, int32_t ks,
                                                   int32_t stride, int32_t pad, int32_t dil) {
  Geom g;
  if (B <= 0 || conv2_geom(B, Cin, Cout, D, ks, stride, pad, dil, &g)) return 0;
  return nt_workspace_bytes(kConv2Fwd, (int64_t)B * g.Do * g.Do, Cout, g.taps * 3 * Cin);
}

extern "C" int mf_conv2d_split_fwd(const void *xs, const void *wp, const float *bias, const float *res, int32_t ldr,
                                   const float *slope, int32_t act, float *out32, int32_t ldo32, void *outs, int32_t ldos,
                                   int32_t los, void *ws, int64_t ws_bytes, int32_t B, int32_t Cin, int32_t Cout,
                                   int32_t D, int32_t ks, int32_t stride, int32_t pad, int32_t dil, mfStream_t stream_) {
  if (B <= 0) return 0;
  Geom g;
  if (int e = conv2_geom(B, Cin, Cout, D, ks, stride, pad, dil, &g)) return e;
  if (act < 0 || act > 2 || (act == 2 && !slope)) return bad("conv2d_split_fwd: act 0 / 1 / 2 (PReLU needs its slope)");
  if (int e = split_out_check("conv2d_split_fwd: an output; output / residual pitches >= Cout, multiples of 8; lo plane inside the row; 16-byte aligned",
                              bias, out32, ldo32, outs, ldos, los, Cout, res, ldr))
    return e;
  if (((uintptr_t)xs | (uintptr_t)wp | (uintptr_t)ws) & 15) return bad("conv2d_split_fwd: 16-byte aligned operands");
  const int64_t M = (int64_t)B * g.Do * g.Do;
  const int K = g.taps * 3 * Cin;
  NtArgs a = nt_operands(xs, 0, 0, wp, K, 0, bias, 0, M, Cout, K, 1);
  nt_conv_geom(a, B, D, g, 3 * Cin, Cout, ks, stride, pad, dil);
  return launch_nt_split<kConv2Fwd>(a, 2 * Cin, act, out32, ldo32, outs, ldos, los, ws, ws_bytes, stream_,
                                    "mf_conv2d_split_fwd", res, ldr, slope);
}

/* The volumetric part's fp32 layers as split-bf16 GEMMs (the precision contract is 8.1's): conv4 /
 * conv3's dense channels (Convolution3D k4 s2 p1 on a channels-last grid) and the per-point 1x1 convolutions.
 *   xs   bf16 [B][D^3][2 Cin]  (a voxel's Cin hi channels, then its Cin lo channels)
 *   wp   bf16 [Cout][64][3 Cin] from mf_conv3d_k4s2_split_pack (input channels c_off .. c_off + Cin - 1 of W)
 *   out  row m = (b, output voxel): v = act(conv + bias) (relu: 0 / 1), written as out32[m * ldo32 + n] and / or
 *        outs[m * ldos + n] = hi(v), outs[m * ldos + los + n] = lo(v)
 *   ws   mf_conv3d_k4s2_split_workspace_bytes(...) bytes of fp32 split-K slabs (0: none needed, ws may be null);
 *        the slabs are added in slab order by the finish pass: the same bits from run to run */
extern "C" int mf_conv3d_k4s2_split_pack(const float *W, int32_t Cout, int32_t Cin, int32_t w_cin, int32_t c_off,
                                         void *wp, mfStream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (Cout <= 0 || Cin <= 0) return 0;
  if (c_off < 0 || c_off + Cin > w_cin || ((uintptr_t)wp & 15)) return bad("conv3d_k4s2_split_pack: channel range, aligned output");
  const int64_t n = (int64_t)Cout * 64 * 3 * Cin;
  hipLaunchKernelGGL(k_conv2_pack_split, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, W, Cout, Cin, w_cin,
                     c_off, 64, (uint16_t *)wp);
  return mf::check_launch("mf_conv3d_k4s2_split_pack");
}

extern "C" int64_t mf_conv3d_k4s2_split_workspace_bytes(int32_t B, int32_t Cin, int32_t Cout, int32_t D) {
  Geom g;
  if (B <= 0 || conv_geom(B, 2 * Cin, Cout, D, 4, 2, 1, 1, &g)) return 0;
  return nt_workspace_bytes(kConvFwdS, (int64_t)B * g.Do * g.Do * g.Do, Cout, 64 * 3 * Cin);
}

extern "C" int mf_conv3d_k4s2_split_fwd(const void *xs, const void *wp, const float *bias, int32_t relu, float *out32,
                                        int32_t ldo32, void *outs, int32_t ldos, int32_t los, void *ws, int64_t ws_bytes,
                                        int32_t B, int32_t Cin, int32_t Cout, int32_t D, mfStream_t stream_) {
  if (B <= 0) return 0;
  Geom g;
  if (int e = conv_geom(B, 2 * Cin, Cout, D, 4, 2, 1, 1, &g)) return e;
  if (Cin % 8 || (int64_t)Cout * 64 * 3 * Cin >= kMaxBf16Elems) return bad("conv3d_k4s2_split_fwd: Cin % 8 == 0, weights < 2^30 elements");
  if (int e = split_out_check("conv3d_k4s2_split_fwd: an output; pitches >= Cout, multiples of 8; lo plane inside the row; 16-byte aligned",
                              bias, out32, ldo32, outs, ldos, los, Cout))
    return e;
  if (((uintptr_t)xs | (uintptr_t)wp | (uintptr_t)ws) & 15) return bad("conv3d_k4s2_split_fwd: 16-byte aligned operands");
  const int64_t M = (int64_t)B * g.Do * g.Do * g.Do;
  const int K = 64 * 3 * Cin;
  NtArgs a = nt_operands(xs, 0, 0, wp, K, 0, bias, 0, M, Cout, K, 1);
  nt_conv_geom(a, B, D, g, 3 * Cin, Cout, 4, 2, 1, 1);
  return launch_nt_split<kConvFwdS>(a, 2 * Cin, relu ? 1 : 0, out32, ldo32, outs, ldos, los, ws, ws_bytes, stream_,
                                    "mf_conv3d_k4s2_split_fwd");
}

/* out = act(A W^T + bias) on split operands:
 *   As   bf16 [M][lda]: columns 0 .. Kp - 1 hi, Kp .. 2 Kp - 1 lo of the fp32 row (lda >= 2 Kp)
 *   wp   bf16 [Np][3 Kp] from mf_linear_split_pack (Np >= N); outputs and ws as mf_conv3d_k4s2_split_fwd
 *        (mf_linear_split_workspace_bytes(M, N, Kp)) */
extern "C" int mf_linear_split_pack(const float *W, int64_t w_gs, int32_t ldw, int32_t N, int32_t K, int32_t Np,
                                    int32_t Kp, int32_t groups, void *wp, mfStream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (N <= 0 || K <= 0 || groups <= 0) return 0;
  if (Np < N || Kp < K || Kp % 8 || ldw < K || ((uintptr_t)wp & 15))
    return bad("linear_split_pack: Np >= N, Kp >= K, Kp % 8 == 0, ldw >= K, aligned output");
  const int64_t n = (int64_t)groups * Np * 3 * Kp;
  hipLaunchKernelGGL(k_rows_pack_split, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, W, w_gs, ldw, N, K, Np,
                     Kp, groups, (uint16_t *)wp);
  return mf::check_launch("mf_linear_split_pack");
}

extern "C" int64_t mf_linear_split_workspace_bytes(int64_t M, int32_t N, int32_t Kp) {
  if (M <= 0 || N <= 0 || Kp <= 0 || N % 8) return 0;
  return nt_workspace_bytes(kRowsS, M, N, 3 * Kp);
}

extern "C" int mf_linear_split_fwd(const void *As, int32_t lda, const void *wp, const float *bias, int32_t relu,
                                   float *out32, int32_t ldo32, void *outs, int32_t ldos, int32_t los, void *ws,
                                   int64_t ws_bytes, int32_t M, int32_t N, int32_t Kp, mfStream_t stream_) {
  if (M <= 0 || N <= 0) return 0;
  if (Kp <= 0 || Kp % 8 || lda % 8 || lda < 2 * Kp || (((uintptr_t)As | (uintptr_t)wp | (uintptr_t)ws) & 15))
    return bad("linear_split_fwd: Kp, lda % 8 == 0, lda >= 2 Kp, 16-byte aligned operands");
  if ((int64_t)M * lda >= kMaxBf16Elems || (int64_t)N * 3 * Kp >= kMaxBf16Elems)
    return bad("linear_split_fwd: an operand spans >= 2^31 bytes");
  if (int e = split_out_check("linear_split_fwd: an output; N % 8 == 0; pitches >= N, multiples of 8; lo plane inside the row; 16-byte aligned",
                              bias, out32, ldo32, outs, ldos, los, N))
    return e;
  const NtArgs a = nt_operands(As, lda, 0, wp, 3 * Kp, 0, bias, 0, M, N, 3 * Kp, 1);
  return launch_nt_split<kRowsS>(a, 2 * Kp, relu ? 1 : 0, out32, ldo32, outs, ldos, los, ws, ws_bytes, stream_,
                                 "mf_linear_split_fwd");
}
