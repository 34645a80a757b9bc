// OctoMap key arithmetic over the dense log-odds boxes (mfOccTree), shared by occmap.hip and occtrack.hip.
#pragma once
#include <math.h>
#include <stdint.h>

#include "mf_common.h"

namespace {

constexpr int kKeyMax = 32768;  // octomap's tree_max_val (16-bit keys, depth 16)

// OcTreeBaseImpl::coordToKeyChecked: false outside the 16-bit key range
__device__ __forceinline__ bool coord_key(float c, double rf, int &key) {
  const double s = floor((double)c * rf);
  if (!(s >= -(double)kKeyMax && s < (double)kKeyMax)) return false;  // also NaN
  key = (int)s + kKeyMax;
  return true;
}

__device__ __forceinline__ int64_t cell_of(const mfOccTree &t, int kx, int ky, int kz) {
  const int x = kx - t.lo[0], y = ky - t.lo[1], z = kz - t.lo[2];
  if (x < 0 || y < 0 || z < 0 || x >= t.dim[0] || y >= t.dim[1] || z >= t.dim[2]) return -1;
  return ((int64_t)x * t.dim[1] + y) * t.dim[2] + z;
}

}  // namespace
