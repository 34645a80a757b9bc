// Training-time augmentation of the network's per-object inputs -- gfx950.
//
// Reference: RGBDPoseEstimationDatasetReIndexedBase._augment_rgbd
//   morefusion/datasets/rgbd_pose_estimation/reindexed.py:38-153
// a host loop per example over imgaug / cv2: _augment_mask (one-sided cut of the valid mask, a random choice of
// blobs, re-centring), _augment_rgb (contrast, HSV jitter, Gaussian blur, down-and-up resize), _augment_pcd
// (5 % drop-out, N(0, 3 mm) noise).  Here all n examples of a call go through seven launches on one stream.
//
// Randomness.  Per-example scalars are drawn on the host and arrive as params[n][kAugParams] (float64):
//   0 cut case 0..3        1 cut uniform u in [0, 1)   2 blob-count uniform u in [0, 1)   3 contrast alpha
//   4 H multiplier         5 S multiplier              6 V multiplier                     7 blur sigma
//   8 resize scale         9 example key (an integer below 2^32)                          10, 11 reserved
// Per-pixel / per-component words are Philox4x32-10 with key (seed & 0xffffffff, example key) and counter
// (pixel, stream, 0, 0): stream 0 word 0 = a component's word (pixel = its canonical id), stream 1 word 0 = the
// pixel's drop-out word, streams 2 and 3 = the words behind the pixel's three normal deviates.
// tests/augment_ref.py restates every stage in NumPy, word for word.
#include <math.h>

#include "mf_common.h"
#include "mf_centerize.h"

namespace {

constexpr int kAugParams = 12;
constexpr int kMaskThreads = 1024;
constexpr int kStats = 12;  // per example: final box y1 x1 y2 x2, components m, drawn K, largest id, kept pixels,
                            // cut box y1 x1 y2 x2

struct Philox4 { uint32_t x, y, z, w; };

__device__ __forceinline__ Philox4 philox4x32_10(uint32_t k0, uint32_t k1, uint32_t c0, uint32_t c1) {
  uint32_t c2 = 0u, c3 = 0u;
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1;
    const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return Philox4{c0, c1, c2, c3};
}

// a value another wave of the workgroup wrote or added to: read at the L2, where the atomics live
__device__ __forceinline__ uint32_t ld_l2(uint32_t *p) { return atomicAdd(p, 0u); }

// min into one 16-bit label: LDS has no 16-bit atomics, so a compare-and-swap on the word that holds it
__device__ __forceinline__ void lds_min_u16(uint16_t *lab, int idx, uint32_t v) {
  uint32_t *w = reinterpret_cast<uint32_t *>(lab) + (idx >> 1);
  const int sh = (idx & 1) * 16;
  uint32_t old = *w;
  for (;;) {
    if (((old >> sh) & 0xffffu) <= v) return;
    const uint32_t nw = (old & ~(0xffffu << sh)) | (v << sh);
    const uint32_t got = atomicCAS(w, old, nw);
    if (got == old) return;
    old = got;
  }
}

struct MaskShared {
  int y1, x1, y2, x2;  // running box (min, min, max + 1, max + 1)
  int count, changed, nroots, pad;
  unsigned long long best;  // (size << 32) | (0xffffffff - id): max = largest component, lowest id on a tie
  unsigned long long prefix;
  int krem, pad2;
};

template <class T>
__device__ __forceinline__ bool valid3(const T *p) { return p[0] == p[0] && p[1] == p[1] && p[2] == p[2]; }

// One workgroup per example.  Dynamic LDS: S*S 16-bit labels | S*S mask bits | 256 histogram bins | MaskShared.
// Global workspace per example: S*S component sizes (later keep flags) | S*S component words.
template <class T>
__global__ __launch_bounds__(kMaskThreads) void k_aug_mask(
    const T *__restrict__ pcd, const double *__restrict__ params, int S, uint32_t seed, uint32_t *__restrict__ ws,
    uint8_t *__restrict__ kept, int32_t *__restrict__ stats, int32_t *__restrict__ labels_out,
    int32_t *__restrict__ sizes_out) {
  MF_DYN_LDS(unsigned char, lds);
  const int npix = S * S, nwords = npix / 32;
  uint16_t *lab = reinterpret_cast<uint16_t *>(lds);
  uint32_t *bits = reinterpret_cast<uint32_t *>(lds + 2 * (size_t)npix);
  uint32_t *hist = bits + nwords;
  MaskShared *sh = reinterpret_cast<MaskShared *>(hist + 256);
  const int e = blockIdx.x, t = threadIdx.x, nt = blockDim.x;
  const T *src = pcd + (int64_t)e * npix * 3;
  const double *prm = params + (int64_t)e * kAugParams;
  uint32_t *cnt = ws + (int64_t)e * 2 * npix, *word = cnt + npix;
  uint8_t *kept_e = kept + (int64_t)e * npix;
  int32_t *st = stats + (int64_t)e * kStats;
  auto in_mask = [&](int p) { return (bits[p >> 5] >> (p & 31)) & 1u; };
  auto reset_box = [&]() {
    if (t == 0) { sh->y1 = S; sh->x1 = S; sh->y2 = 0; sh->x2 = 0; sh->count = 0; }
  };
  // box and pixel count of the mask bits (every thread owns whole 32-pixel words)
  auto measure = [&]() {
    int y1 = S, x1 = S, y2 = 0, x2 = 0, c = 0;
    for (int w = t; w < nwords; w += nt) {
      const uint32_t b = bits[w];
      if (!b) continue;
      for (int k = 0; k < 32; ++k)
        if ((b >> k) & 1u) {
          const int p = w * 32 + k, y = p / S, x = p % S;
          y1 = min(y1, y); x1 = min(x1, x); y2 = max(y2, y + 1); x2 = max(x2, x + 1);
          ++c;
        }
    }
    if (c) {
      atomicMin(&sh->y1, y1); atomicMin(&sh->x1, x1); atomicMax(&sh->y2, y2); atomicMax(&sh->x2, x2);
      atomicAdd(&sh->count, c);
    }
  };
  auto finish_empty = [&](int cy1, int cx1, int cy2, int cx2) {  // pure padding: no kept pixel
    for (int p = t; p < npix; p += nt) {
      kept_e[p] = 0;
      if (labels_out) labels_out[(int64_t)e * npix + p] = -1;
      if (sizes_out) sizes_out[(int64_t)e * npix + p] = 0;
    }
    if (t == 0) {
      for (int k = 0; k < 8; ++k) st[k] = 0;
      st[6] = -1;
      st[8] = cy1; st[9] = cx1; st[10] = cy2; st[11] = cx2;
    }
  };

  // ---- valid mask = no NaN in pcd, its box (masks_to_bboxes)
  reset_box();
  for (int w = t; w < nwords; w += nt) {
    uint32_t b = 0u;
    for (int k = 0; k < 32; ++k)
      if (valid3(src + 3 * (int64_t)(w * 32 + k))) b |= 1u << k;
    bits[w] = b;
  }
  __syncthreads();
  measure();
  __syncthreads();
  if (sh->count == 0) { finish_empty(0, 0, 0, 0); return; }
  // ---- one side of the box replaced (reindexed.py:84-99: measured from the image border), half-to-even
  int by1 = sh->y1, bx1 = sh->x1, by2 = sh->y2, bx2 = sh->x2;
  {
    const int cut_case = (int)prm[0];
    const double u = prm[1];
    const double dy = ((double)(by2 - by1) * 0.25) * u, dx = ((double)(bx2 - bx1) * 0.25) * u;
    if (cut_case == 0) by1 = (int)rint(dy);
    else if (cut_case == 1) by2 = (int)rint((double)S - dy);
    else if (cut_case == 2) bx1 = (int)rint(dx);
    else bx2 = (int)rint((double)S - dx);
  }
  __syncthreads();  // (everyone has read the box)
  reset_box();
  for (int w = t; w < nwords; w += nt) {
    uint32_t b = bits[w];
    if (!b) continue;
    for (int k = 0; k < 32; ++k) {
      const int p = w * 32 + k, y = p / S, x = p % S;
      if (y < by1 || y >= by2 || x < bx1 || x >= bx2) b &= ~(1u << k);
    }
    bits[w] = b;
  }
  __syncthreads();
  measure();
  __syncthreads();
  if (sh->count == 0) { finish_empty(by1, bx1, by2, bx2); return; }

  // ---- 8-connected components by label equivalence: a label is a parent pointer, a root points at itself; a pixel
  // that sees a smaller label next to it hangs its root below that label (min: the order of the updates does not
  // matter), then every pixel is pointed at its root.  At the fixed point a component's label is its first pixel.
  for (int p = t; p < npix; p += nt) lab[p] = (uint16_t)p;
  for (;;) {
    __syncthreads();
    if (t == 0) sh->changed = 0;
    __syncthreads();
    for (int p = t; p < npix; p += nt) {
      if (!in_mask(p)) continue;
      const int y = p / S, x = p % S;
      const uint32_t l = lab[p];
      uint32_t m = l;
      for (int dy = -1; dy <= 1; ++dy)
        for (int dx = -1; dx <= 1; ++dx) {
          const int yy = y + dy, xx = x + dx;
          if ((dy | dx) == 0 || yy < 0 || yy >= S || xx < 0 || xx >= S) continue;
          const int q = yy * S + xx;
          if (in_mask(q)) m = min(m, (uint32_t)lab[q]);
        }
      if (m < l) {
        lds_min_u16(lab, (int)l, m);
        sh->changed = 1;
      }
    }
    __syncthreads();
    for (int p = t; p < npix; p += nt) {
      if (!in_mask(p)) continue;
      uint32_t r = lab[p];
      while (lab[r] != r) r = lab[r];
      lab[p] = (uint16_t)r;
    }
    __syncthreads();
    if (!sh->changed) break;
  }
  if (labels_out)
    for (int p = t; p < npix; p += nt) labels_out[(int64_t)e * npix + p] = in_mask(p) ? (int32_t)lab[p] : -1;

  // ---- component sizes: one add per run of equal labels in each thread's contiguous stretch of pixels
  for (int p = t; p < npix; p += nt) cnt[p] = 0u;
  if (t == 0) { sh->nroots = 0; sh->best = 0ull; }
  __syncthreads();
  {
    const int per = (npix + nt - 1) / nt, p0 = t * per, p1 = min(p0 + per, npix);
    int run = 0;
    uint32_t cur = 0u;
    for (int p = p0; p < p1; ++p) {
      if (!in_mask(p)) continue;
      const uint32_t l = lab[p];
      if (run && l != cur) { atomicAdd(&cnt[cur], (uint32_t)run); run = 0; }
      cur = l;
      ++run;
    }
    if (run) atomicAdd(&cnt[cur], (uint32_t)run);
  }
  __syncthreads();
  const uint32_t k0 = seed, k1 = (uint32_t)prm[9];
  for (int p = t; p < npix; p += nt) {
    if (sizes_out) sizes_out[(int64_t)e * npix + p] = in_mask(p) ? (int32_t)ld_l2(&cnt[lab[p]]) : 0;
    if (!in_mask(p) || lab[p] != p) continue;
    atomicAdd(&sh->nroots, 1);
    atomicMax(&sh->best, ((unsigned long long)ld_l2(&cnt[p]) << 32) | (unsigned long long)(0xffffffffu - (uint32_t)p));
    word[p] = philox4x32_10(k0, k1, (uint32_t)p, 0u).x;
  }
  __syncthreads();
  // ---- the K = floor(u m) components with the smallest (word, id): radix select of the K-th smallest 48-bit key
  const int m_comp = sh->nroots;
  const int largest = (int)(0xffffffffu - (uint32_t)(sh->best & 0xffffffffull));
  const int K = min((int)floor(prm[2] * (double)m_comp), m_comp);
  unsigned long long thresh = 0ull;
  if (K > 0) {
    if (t == 0) { sh->prefix = 0ull; sh->krem = K; }
    for (int pass = 0; pass < 6; ++pass) {
      const int shift = 40 - 8 * pass;
      __syncthreads();
      if (t < 256) hist[t] = 0u;
      __syncthreads();
      const unsigned long long prefix = sh->prefix;
      for (int p = t; p < npix; p += nt) {
        if (!in_mask(p) || lab[p] != p) continue;
        const unsigned long long key = ((unsigned long long)ld_l2(&word[p]) << 16) | (unsigned long long)p;
        if (pass == 0 || (key >> (shift + 8)) == prefix) atomicAdd(&hist[(int)((key >> shift) & 255ull)], 1u);
      }
      __syncthreads();
      if (t == 0) {
        int cum = 0, b = 0;
        for (; b < 255; ++b) {
          if (cum + (int)hist[b] >= sh->krem) break;
          cum += (int)hist[b];
        }
        sh->prefix = (prefix << 8) | (unsigned long long)b;
        sh->krem -= cum;
      }
    }
    __syncthreads();
    thresh = sh->prefix;
  }
  // ---- keep flags per component (in place of its size), then the kept mask and its box
  for (int p = t; p < npix; p += nt) {
    if (!in_mask(p) || lab[p] != p) continue;
    const unsigned long long key = ((unsigned long long)ld_l2(&word[p]) << 16) | (unsigned long long)p;
    atomicExch(&cnt[p], (p == largest || (K > 0 && key <= thresh)) ? 1u : 0u);
  }
  __syncthreads();
  reset_box();
  for (int w = t; w < nwords; w += nt) {
    uint32_t b = bits[w];
    uint32_t last = 0xffffffffu, flag = 0u;  // (neighbours mostly share a component: one read per run)
    for (int k = 0; k < 32; ++k) {
      if (!((b >> k) & 1u)) continue;
      const uint32_t l = lab[w * 32 + k];
      if (l != last) { last = l; flag = ld_l2(&cnt[l]); }
      if (!flag) b &= ~(1u << k);
    }
    bits[w] = b;
    for (int k = 0; k < 32; ++k) kept_e[w * 32 + k] = (uint8_t)((b >> k) & 1u);
  }
  __syncthreads();
  measure();
  __syncthreads();
  if (t == 0) {
    st[0] = sh->y1; st[1] = sh->x1; st[2] = sh->y2; st[3] = sh->x2;
    st[4] = m_comp; st[5] = K; st[6] = largest; st[7] = sh->count;
    st[8] = by1; st[9] = bx1; st[10] = by2; st[11] = bx2;
  }
}

// Crop to the kept mask's box and centre back to S x S (imgviz.centerize: rgb 8-bit bilinear, points nearest);
// outside the kept mask rgb reads as 0 and points as NaN.  One thread per output pixel.
template <class T>
__global__ __launch_bounds__(256) void k_aug_center(
    const uint8_t *__restrict__ rgb, const T *__restrict__ pcd, const uint8_t *__restrict__ kept,
    const int32_t *__restrict__ stats, int S, uint8_t *__restrict__ rgb_out, T *__restrict__ pcd_out,
    uint8_t *__restrict__ keep) {
  const int i = blockIdx.y;
  const int o = blockIdx.x * blockDim.x + threadIdx.x;
  if (o >= S * S) return;
  const int32_t *st = stats + (int64_t)i * kStats;
  const int y1 = st[0], x1 = st[1], sh = st[2] - y1, sw = st[3] - x1;
  const bool ok = st[7] > 0;
  if (o == 0) keep[i] = ok ? 1 : 0;
  const int64_t base = (int64_t)i * S * S;
  uint8_t *ro = rgb_out + (base + o) * 3;
  T *po = pcd_out + (base + o) * 3;
  const T nanv = (T)__builtin_nan("");
  ro[0] = 0; ro[1] = 0; ro[2] = 0;
  po[0] = nanv; po[1] = nanv; po[2] = nanv;
  if (!ok) return;
  const mf::Centerize g = mf::centerize_geometry(sh, sw, S);
  int dy, dx;
  if (!mf::centerize_inside(g, o / S, o % S, dy, dx)) return;
  auto masked = [&](int yy, int xx) { return kept[base + (int64_t)(y1 + yy) * S + (x1 + xx)] != 0; };
  int sy, sx;
  mf::centerize_nearest(g, dy, dx, sh, sw, sy, sx);
  if (masked(sy, sx)) {
    const T *q = pcd + (base + (int64_t)(y1 + sy) * S + (x1 + sx)) * 3;
    po[0] = q[0]; po[1] = q[1]; po[2] = q[2];
  }
  auto pix = [&](int yy, int xx, int c) -> int {
    return masked(yy, xx) ? (int)rgb[(base + (int64_t)(y1 + yy) * S + (x1 + xx)) * 3 + c] : 0;
  };
  mf::centerize_linear_u8(g, dy, dx, sh, sw, pix, ro);
}

// ---- colour stage ----------------------------------------------------------------------------------------------
// imgaug LinearContrast on uint8 (a look-up table: centre 127, float32, clipped, truncated), cv2 RGB -> HSV for
// 8-bit (H in [0, 180), the 12-bit reciprocal tables), imgaug Multiply on uint8 (float32, clipped, truncated) on
// S, V and H, cv2 HSV -> RGB for 8-bit (float32 sector formula, rounded).
__device__ __forceinline__ int mul_u8(int v, float f) {
  const float x = fminf(fmaxf((float)v * f, 0.0f), 255.0f);
  return (int)x;
}

__global__ __launch_bounds__(256) void k_aug_colour(const uint8_t *__restrict__ rgb, const double *__restrict__ params,
                                                    int S, uint8_t *__restrict__ out) {
  const int i = blockIdx.y;
  const int o = blockIdx.x * blockDim.x + threadIdx.x;
  if (o >= S * S) return;
  const double *prm = params + (int64_t)i * kAugParams;
  const float alpha = (float)prm[3], mh = (float)prm[4], ms = (float)prm[5], mv = (float)prm[6];
  const uint8_t *pi = rgb + ((int64_t)i * S * S + o) * 3;
  int c[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float x = 127.0f + alpha * ((float)pi[k] - 127.0f);
    c[k] = (int)fminf(fmaxf(x, 0.0f), 255.0f);
  }
  const int r = c[0], g = c[1], b = c[2];
  const int v = max(r, max(g, b)), vmin = min(r, min(g, b)), diff = v - vmin;
  const int sdiv = v ? (int)rint(1044480.0 / (double)v) : 0;             // (255 << 12) / v
  const int hdiv = diff ? (int)rint(737280.0 / (6.0 * (double)diff)) : 0;  // (180 << 12) / (6 diff)
  int s = (diff * sdiv + 2048) >> 12;
  int h = (v == r) ? (g - b) : (v == g) ? (b - r + 2 * diff) : (r - g + 4 * diff);
  h = (h * hdiv + 2048) >> 12;
  if (h < 0) h += 180;
  s = mul_u8(s, ms);
  const int v2 = mul_u8(v, mv);
  h = mul_u8(h, mh);
  // HSV -> RGB
  const float fs = (float)s * (1.0f / 255.0f), fv = (float)v2 * (1.0f / 255.0f);
  float fr, fg, fb;
  if (s == 0) {
    fr = fg = fb = fv;
  } else {
    float fh = (float)h * (6.0f / 180.0f);
    while (fh >= 6.0f) fh -= 6.0f;
    int sector = (int)floorf(fh);
    fh -= (float)sector;
    if ((unsigned)sector >= 6u) { sector = 0; fh = 0.0f; }
    float tab[4];
    tab[0] = fv;
    tab[1] = fv * (1.0f - fs);
    tab[2] = fv * (1.0f - fs * fh);
    tab[3] = fv * (1.0f - fs * (1.0f - fh));
    const int ib = sector == 0 ? 1 : sector == 1 ? 1 : sector == 2 ? 3 : sector == 3 ? 0 : sector == 4 ? 0 : 2;
    const int ig = sector == 0 ? 3 : sector == 1 ? 0 : sector == 2 ? 0 : sector == 3 ? 2 : sector == 4 ? 1 : 1;
    const int ir = sector == 0 ? 0 : sector == 1 ? 2 : sector == 2 ? 1 : sector == 3 ? 1 : sector == 4 ? 3 : 0;
    fb = tab[ib]; fg = tab[ig]; fr = tab[ir];
  }
  uint8_t *po = out + ((int64_t)i * S * S + o) * 3;
  po[0] = (uint8_t)min(max((int)rintf(fr * 255.0f), 0), 255);
  po[1] = (uint8_t)min(max((int)rintf(fg * 255.0f), 0), 255);
  po[2] = (uint8_t)min(max((int)rintf(fb * 255.0f), 0), 255);
}

// 5 x 5 Gaussian, separable in exact integers: 8-bit fixed-point weights that sum to 256 (the centre takes the
// rounding remainder), rows then columns without an intermediate rounding, (sum + 2^15) >> 16; reflect-101
// borders; sigma < 1e-3 copies.  The 25 taps of a pixel are gathered from the image (L1 / L2 resident: 192 KB per
// example); the sums are the ones the two 1-D passes would give.
__device__ __forceinline__ int reflect101(int p, int n) {
  if (n == 1) return 0;
  while (p < 0 || p >= n) p = p < 0 ? -p : 2 * (n - 1) - p;
  return p;
}

__global__ __launch_bounds__(256) void k_aug_blur(const uint8_t *__restrict__ src, const double *__restrict__ params,
                                                  int S, uint8_t *__restrict__ out) {
  const int i = blockIdx.y;
  const int o = blockIdx.x * blockDim.x + threadIdx.x;
  if (o >= S * S) return;
  const double sigma = params[(int64_t)i * kAugParams + 7];
  const uint8_t *img = src + (int64_t)i * S * S * 3;
  uint8_t *po = out + ((int64_t)i * S * S + o) * 3;
  if (sigma < 1e-3) {
    po[0] = img[3 * o]; po[1] = img[3 * o + 1]; po[2] = img[3 * o + 2];
    return;
  }
  int q[5];
  {
    const double e1 = exp(-1.0 / (2.0 * sigma * sigma)), e2 = exp(-4.0 / (2.0 * sigma * sigma));
    const double sum = 1.0 + 2.0 * e1 + 2.0 * e2;
    const int q1 = (int)rint(e1 / sum * 256.0), q2 = (int)rint(e2 / sum * 256.0);
    q[0] = q2; q[1] = q1; q[2] = 256 - 2 * q1 - 2 * q2; q[3] = q1; q[4] = q2;
  }
  const int y = o / S, x = o % S;
  int xs[5], acc[3] = {0, 0, 0};
#pragma unroll
  for (int k = 0; k < 5; ++k) xs[k] = reflect101(x + k - 2, S);
#pragma unroll
  for (int j = 0; j < 5; ++j) {
    const uint8_t *row = img + (int64_t)reflect101(y + j - 2, S) * S * 3;
    int hsum[3] = {0, 0, 0};
#pragma unroll
    for (int k = 0; k < 5; ++k)
#pragma unroll
      for (int c = 0; c < 3; ++c) hsum[c] += q[k] * (int)row[3 * xs[k] + c];
#pragma unroll
    for (int c = 0; c < 3; ++c) acc[c] += q[j] * hsum[c];
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) po[c] = (uint8_t)((acc[c] + 32768) >> 16);
}

// cv::resize INTER_CUBIC for 8-bit: f = (float)((d + 0.5) scale - 0.5), s = floor(f), the four a = -0.75 weights
// in float32 -> short(rint(w * 2048)), taps s-1 .. s+2 clamped to the image (replicated border), rows in exact
// integers, (sum + 2^21) >> 22 saturated.
__device__ __forceinline__ void cubic_tap(int d, double scale, int &s, int w[4]) {
  float f = (float)(((double)d + 0.5) * scale - 0.5);
  s = (int)floorf(f);
  f -= (float)s;
  const float A = -0.75f;
  float c[4];
  c[0] = ((A * (f + 1.0f) - 5.0f * A) * (f + 1.0f) + 8.0f * A) * (f + 1.0f) - 4.0f * A;
  c[1] = ((A + 2.0f) * f - (A + 3.0f)) * f * f + 1.0f;
  c[2] = ((A + 2.0f) * (1.0f - f) - (A + 3.0f)) * (1.0f - f) * (1.0f - f) + 1.0f;
  c[3] = 1.0f - c[0] - c[1] - c[2];
#pragma unroll
  for (int k = 0; k < 4; ++k) w[k] = (int)(short)rintf(c[k] * 2048.0f);
}

__device__ __forceinline__ int aug_resized(double scale, int S) {  // imgaug Resize: round(S scale), at least 1
  return min(max((int)rint((double)S * scale), 1), S);
}

// down = 1: S x S -> R x R (R = round(S scale)); down = 0: R x R -> S x S.  Both images have row pitch = their
// own width inside an S*S*3 slot per example; R == S copies.
__global__ __launch_bounds__(256) void k_aug_resize(const uint8_t *__restrict__ src, const double *__restrict__ params,
                                                    int S, int down, uint8_t *__restrict__ out) {
  const int i = blockIdx.y;
  const int o = blockIdx.x * blockDim.x + threadIdx.x;
  const int R = aug_resized(params[(int64_t)i * kAugParams + 8], S);
  const int ssz = down ? S : R, dsz = down ? R : S;
  if (o >= dsz * dsz) return;
  const uint8_t *img = src + (int64_t)i * S * S * 3;
  uint8_t *po = out + ((int64_t)i * S * S + o) * 3;
  if (R == S) {
    po[0] = img[3 * o]; po[1] = img[3 * o + 1]; po[2] = img[3 * o + 2];
    return;
  }
  const double scale = 1.0 / ((double)dsz / (double)ssz);
  const int y = o / dsz, x = o % dsz;
  int sx, sy, wx[4], wy[4], xs[4];
  cubic_tap(x, scale, sx, wx);
  cubic_tap(y, scale, sy, wy);
#pragma unroll
  for (int k = 0; k < 4; ++k) xs[k] = min(max(sx - 1 + k, 0), ssz - 1);
  int acc[3] = {0, 0, 0};
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const uint8_t *row = img + (int64_t)min(max(sy - 1 + j, 0), ssz - 1) * ssz * 3;
    int hsum[3] = {0, 0, 0};
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
      for (int c = 0; c < 3; ++c) hsum[c] += wx[k] * (int)row[3 * xs[k] + c];
#pragma unroll
    for (int c = 0; c < 3; ++c) acc[c] += wy[j] * hsum[c];
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) po[c] = (uint8_t)min(max((acc[c] + (1 << 21)) >> 22, 0), 255);
}

// ---- point stage: drop-out below 0.05 * 2^32, then + 0.003 z with z standard normal (Box-Muller in float64 on
// 53-bit uniforms from the generator words); NaN stays NaN
__device__ __forceinline__ double u53(uint32_t a, uint32_t b) { return (double)(a >> 5) * 67108864.0 + (double)(b >> 6); }

template <class T>
__global__ __launch_bounds__(256) void k_aug_pcd(const T *__restrict__ pcd, const double *__restrict__ params, int S,
                                                 uint32_t seed, T *__restrict__ out) {
  const int i = blockIdx.y;
  const int o = blockIdx.x * blockDim.x + threadIdx.x;
  if (o >= S * S) return;
  const uint32_t k1 = (uint32_t)params[(int64_t)i * kAugParams + 9];
  const T *pi = pcd + ((int64_t)i * S * S + o) * 3;
  T *po = out + ((int64_t)i * S * S + o) * 3;
  const T nanv = (T)__builtin_nan("");
  const bool all_nan = pi[0] != pi[0] && pi[1] != pi[1] && pi[2] != pi[2];
  if (all_nan || philox4x32_10(seed, k1, (uint32_t)o, 1u).x < 214748365u) {  // ceil(0.05 * 2^32)
    po[0] = nanv; po[1] = nanv; po[2] = nanv;
    return;
  }
  const Philox4 a = philox4x32_10(seed, k1, (uint32_t)o, 2u), b = philox4x32_10(seed, k1, (uint32_t)o, 3u);
  const double two_pi = 6.283185307179586, inv53 = 1.0 / 9007199254740992.0;
  const double ra = sqrt(-2.0 * log((u53(a.x, a.y) + 1.0) * inv53)), ta = two_pi * (u53(a.z, a.w) * inv53);
  const double rb = sqrt(-2.0 * log((u53(b.x, b.y) + 1.0) * inv53)), tb = two_pi * (u53(b.z, b.w) * inv53);
  const double z[3] = {ra * cos(ta), ra * sin(ta), rb * cos(tb)};
#pragma unroll
  for (int c = 0; c < 3; ++c) po[c] = (T)((double)pi[c] + 0.003 * z[c]);
}

int bad_args(const char *what, int n, int S) {
  if (n < 0 || S < 8 || S > 256 || S % 8) {
    mf::set_last_error(hipErrorInvalidValue, what);
    return -(int)hipErrorInvalidValue;
  }
  return 0;
}

size_t mask_lds_bytes(int S) { return 2 * (size_t)S * S + (size_t)S * S / 8 + 256 * 4 + sizeof(MaskShared); }

}  // namespace

extern "C" int64_t mf_augment_workspace_bytes(int32_t n, int32_t S) {
  if (n < 0 || S < 8 || S > 256 || S % 8) return -1;
  // mask stage: component sizes + words (2 x uint32 per pixel); colour stage: two uint8 images
  return (int64_t)n * S * S * 8 + 2 * (((int64_t)n * S * S * 3 + 15) & ~(int64_t)15);
}

extern "C" int mf_augment_mask(const uint8_t *rgb, const void *pcd, int32_t pcd_is_f64, const double *params,
                               int32_t n, int32_t S, int64_t seed, uint8_t *rgb_out, void *pcd_out,
                               uint8_t *kept_mask, int32_t *stats, uint8_t *keep, int32_t *labels, int32_t *sizes,
                               void *workspace, mfStream_t stream) {
  if (int e = bad_args("mf_augment_mask: n >= 0, S a multiple of 8 in 8..256", n, S)) return e;
  if (n == 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  const size_t lds = mask_lds_bytes(S);
  const dim3 grid((S * S + 255) / 256, n);
  uint32_t *ws = static_cast<uint32_t *>(workspace);
  if (pcd_is_f64) {
    if (int e = mf::allow_big_lds((const void *)k_aug_mask<double>, (int)lds)) return e;
    hipLaunchKernelGGL(k_aug_mask<double>, dim3(n), dim3(kMaskThreads), lds, s, static_cast<const double *>(pcd),
                       params, S, (uint32_t)seed, ws, kept_mask, stats, labels, sizes);
    hipLaunchKernelGGL(k_aug_center<double>, grid, dim3(256), 0, s, rgb, static_cast<const double *>(pcd), kept_mask,
                       stats, S, rgb_out, static_cast<double *>(pcd_out), keep);
  } else {
    if (int e = mf::allow_big_lds((const void *)k_aug_mask<float>, (int)lds)) return e;
    hipLaunchKernelGGL(k_aug_mask<float>, dim3(n), dim3(kMaskThreads), lds, s, static_cast<const float *>(pcd),
                       params, S, (uint32_t)seed, ws, kept_mask, stats, labels, sizes);
    hipLaunchKernelGGL(k_aug_center<float>, grid, dim3(256), 0, s, rgb, static_cast<const float *>(pcd), kept_mask,
                       stats, S, rgb_out, static_cast<float *>(pcd_out), keep);
  }
  return mf::check_launch("mf_augment_mask");
}

extern "C" int mf_augment_rgb(const uint8_t *rgb, const double *params, int32_t n, int32_t S, uint8_t *rgb_out,
                              void *workspace, mfStream_t stream) {
  if (int e = bad_args("mf_augment_rgb: n >= 0, S a multiple of 8 in 8..256", n, S)) return e;
  if (n == 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  const int64_t img = ((int64_t)n * S * S * 3 + 15) & ~(int64_t)15;
  uint8_t *a = static_cast<uint8_t *>(workspace) + (int64_t)n * S * S * 8, *b = a + img;
  const dim3 grid((S * S + 255) / 256, n);
  hipLaunchKernelGGL(k_aug_colour, grid, dim3(256), 0, s, rgb, params, S, a);
  hipLaunchKernelGGL(k_aug_blur, grid, dim3(256), 0, s, a, params, S, b);
  hipLaunchKernelGGL(k_aug_resize, grid, dim3(256), 0, s, b, params, S, 1, a);
  hipLaunchKernelGGL(k_aug_resize, grid, dim3(256), 0, s, a, params, S, 0, rgb_out);
  return mf::check_launch("mf_augment_rgb");
}

extern "C" int mf_augment_pcd(const void *pcd, int32_t pcd_is_f64, const double *params, int32_t n, int32_t S,
                              int64_t seed, void *pcd_out, mfStream_t stream) {
  if (int e = bad_args("mf_augment_pcd: n >= 0, S a multiple of 8 in 8..256", n, S)) return e;
  if (n == 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((S * S + 255) / 256, n);
  if (pcd_is_f64)
    hipLaunchKernelGGL(k_aug_pcd<double>, grid, dim3(256), 0, s, static_cast<const double *>(pcd), params, S,
                       (uint32_t)seed, static_cast<double *>(pcd_out));
  else
    hipLaunchKernelGGL(k_aug_pcd<float>, grid, dim3(256), 0, s, static_cast<const float *>(pcd), params, S,
                       (uint32_t)seed, static_cast<float *>(pcd_out));
  return mf::check_launch("mf_augment_pcd");
}
