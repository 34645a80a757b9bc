// Host side of the TSDF family and the grid mesher (csrc/tsdf.hip, tsdflabel.hip, tsdfcolor.hip, tsdfrender.hip,
// tsdfmesh.hip, gridmesh.hip): what a volume and a camera must satisfy, how the C ABI's scalars become tsdf_voxel.h's
// value types, and the two launch shapes, each written once.
#pragma once
#include <stdint.h>

#include "mf_common.h"
#include "tsdf_voxel.h"

namespace {

constexpr int kThreads = 256;  // lanes of a workgroup of a lane-per-element kernel
constexpr int kTile = 16;      // a lane-per-pixel kernel runs kTile x kTile pixels per workgroup

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

// (a call that names no origin and no pitch leaves them 0: its kernels read the lattice alone)
inline mf_tsdf::Grid grid_of(int32_t nx, int32_t ny, int32_t nz, double ox = 0.0, double oy = 0.0, double oz = 0.0,
                             double pitch = 0.0) {
  return {{nx, ny, nz}, {ox, oy, oz}, pitch};
}

inline mf_tsdf::Camera camera_of(int32_t H, int32_t W, double fx, double fy, double cx, double cy) {
  return {H, W, fx, fy, cx, cy};
}

// a lane per element of n
inline dim3 lanes(int64_t n) { return dim3((unsigned)((n + kThreads - 1) / kThreads)); }

// a lane per pixel of an H x W image
inline dim3 tiles(int H, int W) { return dim3((unsigned)((W + kTile - 1) / kTile), (unsigned)((H + kTile - 1) / kTile)); }

inline int64_t align16(int64_t n) { return (n + 15) & ~(int64_t)15; }

inline bool misaligned(const void *p) { return ((uintptr_t)p & 15u) != 0; }

}  // namespace
