// Host-side argument checks of the TSDF family and the grid mesher (csrc/tsdf.hip, tsdflabel.hip, tsdfrender.hip,
// tsdfmesh.hip, gridmesh.hip): what a volume and a camera must satisfy is written once.
#pragma once
#include <stdint.h>

#include "mf_common.h"

namespace {

// refuse a call: the text is what mf_last_error_string reports
inline int bad(const char *what) {
  mf::set_last_error(hipErrorInvalidValue, what);
  return -(int)hipErrorInvalidValue;
}

// "nx, ny, nz >= 2 with fewer than 2^31 voxels"
inline bool bad_volume(int32_t nx, int32_t ny, int32_t nz) {
  return nx < 2 || ny < 2 || nz < 2 || (int64_t)nx * ny * nz >= ((int64_t)1 << 31);
}

// "1 <= H, W <= MF_RENDER_MAX_SIDE, fx, fy > 0"
inline bool bad_camera(int32_t H, int32_t W, double fx, double fy) {
  return H < 1 || W < 1 || H > MF_RENDER_MAX_SIDE || W > MF_RENDER_MAX_SIDE || !(fx > 0.0) || !(fy > 0.0);
}

inline int64_t align16(int64_t n) { return (n + 15) & ~(int64_t)15; }

inline bool misaligned(const void *p) { return ((uintptr_t)p & 15u) != 0; }

}  // namespace
