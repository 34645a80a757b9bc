// The workgroup prefix sum of the two meshers (csrc/gridmesh.hip, csrc/tsdfmesh.hip): integer sums over the lanes of
// a wave with __shfl_up, then over the waves through LDS that the caller owns.
#pragma once
#include "mf_common.h"

namespace {

template <class T>
__device__ __forceinline__ T wave_incl_scan(T v) {
  const int lane = threadIdx.x & 63;
  for (int d = 1; d < 64; d <<= 1) {
    const T u = __shfl_up(v, d);
    if (lane >= d) v += u;
  }
  return v;
}

// exclusive prefix of v over the workgroup's NW waves and the total; every thread calls it, s_w is NW words of LDS
template <int NW, class T>
__device__ __forceinline__ T block_excl_scan(T v, T *s_w, T &total) {
  const T inc = wave_incl_scan(v);
  const int w = threadIdx.x >> 6;
  __syncthreads();  // the previous call's s_w has been read
  if ((threadIdx.x & 63) == 63) s_w[w] = inc;
  __syncthreads();
  T base = 0;
  total = 0;
  for (int i = 0; i < NW; ++i) {
    if (i < w) base += s_w[i];
    total += s_w[i];
  }
  return base + inc - v;
}

}  // namespace
