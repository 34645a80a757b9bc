// One scan into the dense log-odds boxes (mfOccTree), shared by occmap.hip and occserver.hip: the scan bits of a
// cell, octomap's computeRayKeys DDA, and the per-wave key bounds.
#pragma once
#include <float.h>
#include <limits.h>
#include <math.h>
#include <stdint.h>

#include "mf_common.h"
#include "occmap_keys.h"

namespace {

__device__ __forceinline__ int find_slot(const int32_t *slots, int n_slots, int32_t label) {
  for (int s = 0; s < n_slots; ++s)
    if (slots[3 * s] == label) return s;
  return -1;
}

__device__ __forceinline__ bool load_point(const float *pts, int64_t i, float &x, float &y, float &z) {
  x = pts[3 * i];
  y = pts[3 * i + 1];
  z = pts[3 * i + 2];
  return !(isnan(x) || isnan(y) || isnan(z));
}

// MF_OCC_READ_FIRST=0: a plain atomic OR per visit (the A/B of DESIGN.md "Occupancy mapping")
#ifndef MF_OCC_READ_FIRST
#define MF_OCC_READ_FIRST 1
#endif
__device__ __forceinline__ void set_bit(uint32_t *w, uint32_t m) {
#if MF_OCC_READ_FIRST
  if (!(*w & m)) atomicOr(w, m);  // read first: a set bit needs no atomic (bits only go 0 -> 1 here)
#else
  atomicOr(w, m);
#endif
}

__device__ __forceinline__ void mark(const mfOccTree &t, int kx, int ky, int kz, int word, uint32_t m, int32_t *overflow) {
  const int64_t c = cell_of(t, kx, ky, kz);
  if (c < 0) {
    if (overflow) atomicAdd(overflow, 1);
    return;
  }
  set_bit(t.bits + 2 * c + word, m);
}

// OcTreeBaseImpl::computeRayKeys from o to p in a tree of resolution res = 1 / rf: visit(kx, ky, kz) for the origin's
// key and every key the ray passes before the end point's.  Nothing is visited if a key is out of range or both
// points share a cell.
template <class Visit>
__device__ __forceinline__ void ray_keys(const float (&o)[3], const float (&p)[3], double res, double rf, Visit visit) {
  int ke[3], ko[3];
  if (coord_key(o[0], rf, ko[0]) && coord_key(o[1], rf, ko[1]) && coord_key(o[2], rf, ko[2]) &&
      coord_key(p[0], rf, ke[0]) && coord_key(p[1], rf, ke[1]) && coord_key(p[2], rf, ke[2]) &&
      !(ko[0] == ke[0] && ko[1] == ke[1] && ko[2] == ke[2])) {
    visit(ko[0], ko[1], ko[2]);
    // point3d arithmetic in float: direction = end - origin, norm() = sqrt(double(float x*x + y*y + z*z))
    float d[3] = {p[0] - o[0], p[1] - o[1], p[2] - o[2]};
    const float nsq = d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
    const float length = (float)sqrt((double)nsq);
    for (int a = 0; a < 3; ++a) d[a] = d[a] / length;
    int step[3], cur[3] = {ko[0], ko[1], ko[2]};
    double tmax[3], tdelta[3];
    for (int a = 0; a < 3; ++a) {
      step[a] = d[a] > 0.0f ? 1 : (d[a] < 0.0f ? -1 : 0);
      if (step[a] != 0) {
        double border = ((double)(cur[a] - kKeyMax) + 0.5) * res;  // keyToCoord
        border += (double)(float)((double)step[a] * res * 0.5);
        tmax[a] = (border - (double)o[a]) / (double)d[a];
        tdelta[a] = res / (double)fabsf(d[a]);
      } else {
        tmax[a] = DBL_MAX;
        tdelta[a] = DBL_MAX;
      }
    }
    // every axis moves monotonically towards the end key and passes it by at most one cell
    const int limit = abs(ke[0] - ko[0]) + abs(ke[1] - ko[1]) + abs(ke[2] - ko[2]) + 8;
    for (int it = 0; it < limit; ++it) {
      const int a = tmax[0] < tmax[1] ? (tmax[0] < tmax[2] ? 0 : 2) : (tmax[1] < tmax[2] ? 1 : 2);
      cur[a] += step[a];
      tmax[a] += tdelta[a];
      if (cur[0] == ke[0] && cur[1] == ke[1] && cur[2] == ke[2]) break;
      const double dist = fmin(fmin(tmax[0], tmax[1]), tmax[2]);
      if (dist > (double)length) break;  // overshot the end through rounding
      visit(cur[0], cur[1], cur[2]);
    }
  }
}

// Key bounds of a wave: lane's key k belongs to tree `tree` (-1: none).  One pass per tree present in the wave, its
// leader folds the wave's min / max into s_b [n_trees, 6] (LDS, int atomics).  Every lane of the wave must call.
__device__ __forceinline__ void wave_key_bounds(int tree, const int (&k)[3], int32_t *s_b) {
  const int lane = threadIdx.x & 63;
  unsigned long long pending = __ballot(tree >= 0);
  while (pending) {
    const int leader = __ffsll(pending) - 1;
    const int t = __shfl(tree, leader);
    const bool mine = tree == t && tree >= 0;
    pending &= ~__ballot(mine);
    int v[6];
    for (int a = 0; a < 3; ++a) {
      v[a] = mine ? k[a] : INT_MAX;
      v[3 + a] = mine ? k[a] : INT_MIN;
    }
    for (int off = 32; off > 0; off >>= 1)
      for (int a = 0; a < 3; ++a) {
        v[a] = min(v[a], __shfl_xor(v[a], off));
        v[3 + a] = max(v[3 + a], __shfl_xor(v[3 + a], off));
      }
    if (lane == leader) {
      for (int a = 0; a < 3; ++a) {
        atomicMin(&s_b[6 * t + a], v[a]);
        atomicMax(&s_b[6 * t + 3 + a], v[3 + a]);
      }
    }
  }
}

}  // namespace
