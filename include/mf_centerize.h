// imgviz.centerize on the device: the geometry and the two cv::resize sampling rules that csrc/preprocess.hip
// (k_pre_crops) and csrc/augment.hip (k_aug_center) share -- one thread per destination pixel of an S x S image
// that holds an sh x sw source crop, aspect-preserving, centred, padded.
// Device code, not part of the C ABI: it lives beside mfhip.h because this directory is on the include path of
// every build of the kernel sources (the product's, the host emulator's, a single source file compiled on its own).
#pragma once
#include <math.h>
#include <stdint.h>

namespace mf {

// cv::resize INTER_LINEAR source index + fixed-point weights for one destination index
// (modules/imgproc/src/resize.cpp, resizeGeneric_ set-up): f = (float)((d+0.5)*scale-0.5),
// s = floor(f), f -= s; clamped at both borders; weights = short(rint(w * 2048)).
__device__ __forceinline__ void linear_tap(int d, double scale, int ssize, int &s0, int &s1,
                                           int &w0, int &w1, const bool zero_frac_at_border) {
  float f = (float)(((double)d + 0.5) * scale - 0.5);
  int s = (int)floorf(f);
  f -= (float)s;
  if (zero_frac_at_border) {  // the x direction resets the fraction, y only clamps the rows
    if (s < 0) { f = 0.0f; s = 0; }
    if (s >= ssize - 1) { f = 0.0f; s = ssize - 1; }
  }
  w0 = (int)(short)rintf((1.0f - f) * 2048.0f);
  w1 = (int)(short)rintf(f * 2048.0f);
  s0 = min(max(s, 0), ssize - 1);
  s1 = min(max(s + 1, 0), ssize - 1);
}

// imgviz.centerize: scale = min(S/sh, S/sw); resized size = round(size*scale) (half-even), centred padding
struct Centerize {
  int dh, dw, ph, pw;
  bool identity;
};
__device__ __forceinline__ Centerize centerize_geometry(int sh, int sw, int S) {
  Centerize g;
  g.dh = S; g.dw = S; g.ph = 0; g.pw = 0;
  g.identity = (sh == S && sw == S);
  if (!g.identity) {
    const double scale_h = 1.0 * S / sh, scale_w = 1.0 * S / sw;
    const double scale = scale_h < scale_w ? scale_h : scale_w;
    g.dh = (int)rint(sh * scale);
    g.dw = (int)rint(sw * scale);
    if (g.dh < S) g.ph = (S - g.dh) / 2;
    if (g.dw < S) g.pw = (S - g.dw) / 2;
  }
  return g;
}
// destination pixel (oy, ox) -> position (dy, dx) inside the resized crop; false: padding
__device__ __forceinline__ bool centerize_inside(const Centerize &g, int oy, int ox, int &dy, int &dx) {
  dy = oy - g.ph;
  dx = ox - g.pw;
  return !(dy < 0 || dy >= g.dh || dx < 0 || dx >= g.dw || g.dh <= 0 || g.dw <= 0);
}
// cv::resize INTER_NEAREST: s = min(floor(d * (1/(dsize/ssize))), ssize-1)
__device__ __forceinline__ void centerize_nearest(const Centerize &g, int dy, int dx, int sh, int sw, int &sy, int &sx) {
  sy = dy;
  sx = dx;
  if (!g.identity) {
    const double ify = 1.0 / ((double)g.dh / sh), ifx = 1.0 / ((double)g.dw / sw);
    sy = min((int)floor(dy * ify), sh - 1);
    sx = min((int)floor(dx * ifx), sw - 1);
  }
}
// cv::resize INTER_LINEAR for 8-bit (2x2 box for an exact 2:1); pix(y, x, c) is the source crop's channel value
template <class Pix>
__device__ __forceinline__ void centerize_linear_u8(const Centerize &g, int dy, int dx, int sh, int sw, Pix pix,
                                                    uint8_t *ro) {
  if (g.identity) {
#pragma unroll
    for (int c = 0; c < 3; ++c) ro[c] = (uint8_t)pix(dy, dx, c);
    return;
  }
  const double scale_x = 1.0 / ((double)g.dw / sw), scale_y = 1.0 / ((double)g.dh / sh);
  const bool area2 = fabs(scale_x - 2.0) < 2.220446049250313e-16 &&
                     fabs(scale_y - 2.0) < 2.220446049250313e-16;
  if (area2) {
#pragma unroll
    for (int c = 0; c < 3; ++c)
      ro[c] = (uint8_t)((pix(2 * dy, 2 * dx, c) + pix(2 * dy, 2 * dx + 1, c) +
                         pix(2 * dy + 1, 2 * dx, c) + pix(2 * dy + 1, 2 * dx + 1, c) + 2) >> 2);
    return;
  }
  int xa, xb, a0, a1, ya, yb, b0, b1;
  linear_tap(dx, scale_x, sw, xa, xb, a0, a1, true);
  linear_tap(dy, scale_y, sh, ya, yb, b0, b1, false);
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const int r0 = pix(ya, xa, c) * a0 + pix(ya, xb, c) * a1;  // horizontal pass, row ya
    const int r1 = pix(yb, xa, c) * a0 + pix(yb, xb, c) * a1;  // row yb
    const int v = (((b0 * (r0 >> 4)) >> 16) + ((b1 * (r1 >> 4)) >> 16) + 2) >> 2;
    ro[c] = (uint8_t)min(max(v, 0), 255);
  }
}

}  // namespace mf
