// The six-tetrahedra (Kuhn) triangulation of a lattice cell, shared by the two meshers: csrc/gridmesh.hip (occupancy
// grids, vertices at edge midpoints) and csrc/tsdfmesh.hip (the TSDF volume, vertices interpolated along their
// edges).  One text, so the two agree on which faces a cell has, in which order, and how they wind.
//
// Corner codes are dx * 4 + dy * 2 + dz.  A lattice point owns the seven edges towards +(1,0,0) (0,1,0) (0,0,1)
// (1,1,0) (1,0,1) (0,1,1) (1,1,1), directions 0 .. 6.  Tetrahedron t of a cell walks the axes xyz, xzy, yxz, yzx, zxy,
// zyx: corners c0 = cell, c1 = c0 + e_a, c2 = c1 + e_b, c3 = cell + (1,1,1).  With the mask m (bit i: corner i inside)
// and e(i,j) the vertex on the edge between corners i and j:
//   one corner i alone on its side:  (e(i,j0), e(i,j1), e(i,j2)), j ascending;
//   corners a < b inside, c < d outside:  (e(a,c), e(a,d), e(b,d)) then (e(a,c), e(b,d), e(b,c));
// the last two vertices of a triangle are exchanged where that makes it counter-clockwise seen from outside (kFlip
// for an even walk, inverted for an odd one).  A cell's faces are numbered in (tetrahedron, triangle) order.
#pragma once
#include "mf_common.h"

namespace {

__device__ const unsigned char kCorner[6][4] = {{0, 4, 6, 7}, {0, 4, 5, 7}, {0, 2, 6, 7},
                                                {0, 2, 3, 7}, {0, 1, 5, 7}, {0, 1, 3, 7}};
__device__ const unsigned char kOdd[6] = {0, 1, 1, 0, 0, 1};             // parity of the walk
__device__ const signed char kDirOfCode[8] = {-1, 2, 1, 5, 0, 4, 3, 6};  // edge direction of a corner-code difference
constexpr unsigned kFlip = 0x4D24u;  // masks 2, 5, 8, 10, 11, 14 of an even walk

// the corner code that edge direction d leads to (the inverse of kDirOfCode)
__device__ __forceinline__ int code_of_dir(int d) {
  return d == 0 ? 4 : d == 1 ? 2 : d == 2 ? 1 : d == 3 ? 6 : d == 4 ? 5 : d == 5 ? 3 : 7;
}

// the mask of tetrahedron t from the cell's 8 corner bits (bit = corner code)
__device__ __forceinline__ unsigned tet_mask(unsigned corners, int t) {
  unsigned m = 0;
  for (int i = 0; i < 4; ++i) m |= ((corners >> kCorner[t][i]) & 1u) << i;
  return m;
}

__device__ __forceinline__ int faces_of_mask(unsigned m) {
  const int pc = __popc(m);
  return pc == 2 ? 2 : (pc & 1);
}

__device__ __forceinline__ int cell_faces(unsigned corners) {
  if (corners == 0u || corners == 255u) return 0;
  int n = 0;
  for (int t = 0; t < 6; ++t) n += faces_of_mask(tet_mask(corners, t));
  return n;
}

// Store the faces of one cell as rows at, at + 1, ... of `faces`; a row outside [first, end) is counted, not stored.
// vertex_of(lo, d) -> the index of the vertex on the edge that the lattice point at corner code lo owns in direction d.
template <class VertexOf>
__device__ __forceinline__ void emit_cell_faces(unsigned corners, int64_t at, int64_t first, int64_t end,
                                                int32_t *__restrict__ faces, VertexOf vertex_of) {
  if (corners == 0u || corners == 255u) return;
  for (int t = 0; t < 6; ++t) {
    const unsigned m = tet_mask(corners, t);
    const int pc = __popc(m);
    if (pc == 0 || pc == 4) continue;
    // e(ci, cj): the vertex on the edge between corners ci, cj of this tetrahedron
    auto edge = [&](int ci, int cj) {
      const int lo = kCorner[t][ci < cj ? ci : cj], hi = kCorner[t][ci < cj ? cj : ci];
      return vertex_of(lo, (int)kDirOfCode[hi - lo]);  // the walk only adds axes: hi - lo is the code of the difference
    };
    const bool flip = (((kFlip >> m) & 1u) != 0u) != (kOdd[t] != 0);
    int tri[2][3];
    if (pc == 2) {
      int in[2], out[2], ni = 0, no = 0;
      for (int c = 0; c < 4; ++c) {
        if ((m >> c) & 1u) in[ni++] = c;
        else out[no++] = c;
      }
      const int ac = edge(in[0], out[0]), ad = edge(in[0], out[1]), bd = edge(in[1], out[1]), bc = edge(in[1], out[0]);
      tri[0][0] = ac, tri[0][1] = ad, tri[0][2] = bd;
      tri[1][0] = ac, tri[1][1] = bd, tri[1][2] = bc;
    } else {
      const unsigned lone = pc == 1 ? m : (~m & 15u);
      const int k = __ffs((int)lone) - 1;
      int n = 0;
      for (int c = 0; c < 4; ++c)
        if (c != k) tri[0][n++] = edge(k, c);
    }
    for (int q = 0; q < (pc == 2 ? 2 : 1); ++q) {
      if (at >= first && at < end) {
        faces[3 * at] = tri[q][0];
        faces[3 * at + 1] = tri[q][flip ? 2 : 1];
        faces[3 * at + 2] = tri[q][flip ? 1 : 2];
      }
      ++at;
    }
  }
}

}  // namespace
