// Mesh signed distance and solid voxelization (geometry/mesh_sdf.py, datasets/ycb_video.py) -- gfx950, float64.
//
// Reference: morefusion/datasets/ycb_video/models.py get_sdf / get_solid_voxel_grid (trimesh's
// nearest.signed_distance over binvox's solid grid).  Neither is linked: DESIGN.md "CAD model preparation" has the
// contract, tests/meshsdf_ref.py the NumPy mirror this file is pinned to bit for bit.
//
// A batch is M triangle meshes (packed float64 [V, 3] vertices, int32 [F, 3] faces local to the mesh, int64 [M + 1]
// offsets of each) and, per mesh, a segment of queries: explicit float64 points or the centres of a D^3 grid.
//   k_meshsdf_prepare  one lane per face: a, b, c, ab = b - a, ac = c - a and the face kind (below) -> 16 doubles.
//   k_meshsdf_query    one lane per query, 256 per workgroup, every workgroup inside one mesh's segment; the mesh's
//                      faces go through LDS in tiles of 256 records and every lane visits every face.
// Per query and face (the operation order is the mirror's, line for line):
//   distance  Ericson's closest point on a triangle (Real-Time Collision Detection 5.1.5), d2 = |p - q|^2 summed
//             x, y, z.  A face whose cross product ab x ac is exactly zero is a segment: the longest of its edges
//             ab, bc, ca (first on a tie), t = clamp(((p - s) . e) / (e . e), 0, 1) (t = 0 when e = 0).
//   arg-min   best = d2 if d2 < best (strict): in face order, so the lowest face index wins a tie.
//   winding   Omega_f = 2 atan2(det, den) (Van Oosterom-Strackee) with ap = p - a, bp, cp:
//             det = -(ap . (bp x cp)), den = |ap| |bp| |cp| + (ap . bp) |cp| + (ap . cp) |bp| + (bp . cp) |ap|;
//             segment faces contribute nothing.  S = sum of Omega_f IN FACE-INDEX ORDER (sequential; this order is
//             part of the contract), w = S / (4 pi).
// Results: dist = sqrt(best) (+inf and face -1 for a mesh without faces), inside = w >= 0.5 || dist <= 1e-8
// (trimesh's tol.merge), sdf = inside ? +dist : -dist (positive inside, as get_sdf).  Grid queries: centre
// c = origin + (i + 0.5) h per axis, (i, j, k) lexicographic; occupied = w >= 0.5 || dist <= h / 2.
// A face with an index outside its mesh is skipped (kind 2).  No atomics and no cross-lane reduction: every result is
// bitwise reproducible.  atan2 is the one library transcendental (OCML here, libm in the mirror: w may differ by an
// ulp, which moves no decision unless |w - 0.5| is that small).
#include <float.h>
#include <limits.h>
#include <math.h>

#include "mf_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kTile = 256;                           // face records per LDS tile (256 x 128 B = 32 KiB)
constexpr int kRec = 16;                             // doubles per face record
constexpr double kFourPi = 12.566370614359172;       // 4 * pi rounded to double (== 4.0 * M_PI)
constexpr double kOnSurface = 1e-8;                  // trimesh tol.merge: counted as inside
#ifndef MF_MESHSDF_ABLATE
#define MF_MESHSDF_ABLATE 0  // 0 = the product; 1 / 2 = timing variants (k_meshsdf_query below)
#endif

// record: [0..2] a, [3..5] b, [6..8] c, [9..11] ab, [12..14] ac, [15] kind (0 triangle, 1 segment, 2 skipped).
// A segment keeps a, b, c and stores its start in [9..11] and its direction in [12..14].
__global__ void __launch_bounds__(kThreads) k_meshsdf_prepare(const double *__restrict__ vert,
                                                                const int64_t *__restrict__ v_off,
                                                                const int32_t *__restrict__ faces,
                                                                const int64_t *__restrict__ f_off, int32_t n_meshes,
                                                                double *__restrict__ rec) {
  const int64_t g = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  const int64_t total = f_off[n_meshes];
  if (g >= total) return;
  int lo = 0, hi = n_meshes - 1;  // the mesh m with f_off[m] <= g < f_off[m + 1]
  while (lo < hi) {
    const int mid = (lo + hi + 1) / 2;
    if (f_off[mid] <= g) lo = mid; else hi = mid - 1;
  }
  const int64_t v0 = v_off[lo], nv = v_off[lo + 1] - v0;
  double *r = rec + g * kRec;
  double p[3][3];
  for (int k = 0; k < 3; ++k) {
    const int32_t i = faces[3 * g + k];
    if (i < 0 || (int64_t)i >= nv) {
      for (int q = 0; q < kRec; ++q) r[q] = 0.0;
      r[15] = 2.0;
      return;
    }
    for (int a = 0; a < 3; ++a) p[k][a] = vert[3 * (v0 + i) + a];
  }
  double ab[3], ac[3];
  for (int a = 0; a < 3; ++a) {
    ab[a] = p[1][a] - p[0][a];
    ac[a] = p[2][a] - p[0][a];
  }
  const double nx = ab[1] * ac[2] - ab[2] * ac[1];
  const double ny = ab[2] * ac[0] - ab[0] * ac[2];
  const double nz = ab[0] * ac[1] - ab[1] * ac[0];
  double kind = 0.0;
  if (nx == 0.0 && ny == 0.0 && nz == 0.0) {  // collinear: the longest edge ab, bc, ca
    kind = 1.0;
    double best = -1.0;
    for (int e = 0; e < 3; ++e) {
      const double *s = p[e], *t = p[(e + 1) % 3];
      const double dx = t[0] - s[0], dy = t[1] - s[1], dz = t[2] - s[2];
      const double l2 = dx * dx + dy * dy + dz * dz;
      if (l2 > best) {
        best = l2;
        ab[0] = s[0]; ab[1] = s[1]; ab[2] = s[2];
        ac[0] = dx; ac[1] = dy; ac[2] = dz;
      }
    }
  }
  for (int k = 0; k < 3; ++k)
    for (int a = 0; a < 3; ++a) r[3 * k + a] = p[k][a];
  for (int a = 0; a < 3; ++a) {
    r[9 + a] = ab[a];
    r[12 + a] = ac[a];
  }
  r[15] = kind;
}

__device__ __forceinline__ double dot3(double ax, double ay, double az, double bx, double by, double bz) {
  return ax * bx + ay * by + az * bz;
}

// squared distance from p to the face, Ericson 5.1.5 (ap = p - a etc. are the caller's)
__device__ __forceinline__ double tri_d2(const double *f, double px, double py, double pz, double apx, double apy,
                                         double apz, double bpx, double bpy, double bpz, double cpx, double cpy,
                                         double cpz) {
  const double abx = f[9], aby = f[10], abz = f[11], acx = f[12], acy = f[13], acz = f[14];
  double qx, qy, qz;
  const double d1 = dot3(abx, aby, abz, apx, apy, apz);
  const double d2 = dot3(acx, acy, acz, apx, apy, apz);
  const double d3 = dot3(abx, aby, abz, bpx, bpy, bpz);
  const double d4 = dot3(acx, acy, acz, bpx, bpy, bpz);
  const double d5 = dot3(abx, aby, abz, cpx, cpy, cpz);
  const double d6 = dot3(acx, acy, acz, cpx, cpy, cpz);
  const double vc = d1 * d4 - d3 * d2;
  const double vb = d5 * d2 - d1 * d6;
  const double va = d3 * d6 - d5 * d4;
  if (d1 <= 0.0 && d2 <= 0.0) {  // vertex a
    qx = f[0]; qy = f[1]; qz = f[2];
  } else if (d3 >= 0.0 && d4 <= d3) {  // vertex b
    qx = f[3]; qy = f[4]; qz = f[5];
  } else if (vc <= 0.0 && d1 >= 0.0 && d3 <= 0.0) {  // edge ab
    const double v = d1 / (d1 - d3);
    qx = f[0] + v * abx; qy = f[1] + v * aby; qz = f[2] + v * abz;
  } else if (d6 >= 0.0 && d5 <= d6) {  // vertex c
    qx = f[6]; qy = f[7]; qz = f[8];
  } else if (vb <= 0.0 && d2 >= 0.0 && d6 <= 0.0) {  // edge ac
    const double w = d2 / (d2 - d6);
    qx = f[0] + w * acx; qy = f[1] + w * acy; qz = f[2] + w * acz;
  } else if (va <= 0.0 && (d4 - d3) >= 0.0 && (d5 - d6) >= 0.0) {  // edge bc
    const double w = (d4 - d3) / ((d4 - d3) + (d5 - d6));
    qx = f[3] + w * (f[6] - f[3]); qy = f[4] + w * (f[7] - f[4]); qz = f[5] + w * (f[8] - f[5]);
  } else {  // interior
    const double denom = 1.0 / (va + vb + vc);
    const double v = vb * denom, w = vc * denom;
    qx = f[0] + abx * v + acx * w; qy = f[1] + aby * v + acy * w; qz = f[2] + abz * v + acz * w;
  }
  const double dx = px - qx, dy = py - qy, dz = pz - qz;
  return dx * dx + dy * dy + dz * dz;
}

// squared distance from p to the segment s + t e, t in [0, 1]
__device__ __forceinline__ double seg_d2(const double *f, double px, double py, double pz) {
  const double sx = f[9], sy = f[10], sz = f[11], ex = f[12], ey = f[13], ez = f[14];
  const double ee = ex * ex + ey * ey + ez * ez;
  double t = 0.0;
  if (ee > 0.0) {
    t = ((px - sx) * ex + (py - sy) * ey + (pz - sz) * ez) / ee;
    t = t < 0.0 ? 0.0 : (t > 1.0 ? 1.0 : t);
  }
  const double dx = px - (sx + t * ex), dy = py - (sy + t * ey), dz = pz - (sz + t * ez);
  return dx * dx + dy * dy + dz * dz;
}

__global__ void __launch_bounds__(kThreads) k_meshsdf_query(mfMeshSdfBatch P) {
  __shared__ double s_rec[kTile * kRec];
  const int t = threadIdx.x;
  const int32_t blk = (int32_t)blockIdx.x;
  int lo = 0, hi = P.n_meshes - 1;  // the mesh whose block range holds this workgroup
  while (lo < hi) {
    const int mid = (lo + hi + 1) / 2;
    if (P.blk_off[mid] <= blk) lo = mid; else hi = mid - 1;
  }
  const int m = lo;
  const int64_t q0 = P.q_off[m], nq = P.q_off[m + 1] - q0;
  const int64_t j = (int64_t)(blk - P.blk_off[m]) * kThreads + t;
  const bool valid = j < nq;
  const int64_t q = q0 + j;
  double px = 0.0, py = 0.0, pz = 0.0, tol = kOnSurface;
  if (valid) {
    if (P.points) {
      px = P.points[3 * q];
      py = P.points[3 * q + 1];
      pz = P.points[3 * q + 2];
    } else {
      const int64_t D = P.grid_dim;
      const double h = P.grid_h[m];
      const int64_t ix = j / (D * D), iy = (j / D) % D, iz = j % D;
      px = P.grid_origin[3 * m] + ((double)ix + 0.5) * h;
      py = P.grid_origin[3 * m + 1] + ((double)iy + 0.5) * h;
      pz = P.grid_origin[3 * m + 2] + ((double)iz + 0.5) * h;
      tol = 0.5 * h;
    }
  }
  const int64_t f0 = P.f_off[m], nf = P.f_off[m + 1] - f0;
  double best = INFINITY, S = 0.0;
  int32_t best_f = -1;
  for (int64_t base = 0; base < nf; base += kTile) {
    const int64_t n = nf - base < kTile ? nf - base : kTile;
    __syncthreads();  // the previous tile is consumed
    for (int k = t; k < n * kRec; k += kThreads) s_rec[k] = P.face_rec[(f0 + base) * kRec + k];
    __syncthreads();
    if (valid) {
      for (int i = 0; i < (int)n; ++i) {
        const double *f = s_rec + i * kRec;
        const double kind = f[15];
        if (kind == 2.0) continue;
        double d2;
        if (kind == 0.0) {
#if MF_MESHSDF_ABLATE == 2  // timing A/B only: the distance alone
          d2 = tri_d2(f, px, py, pz, px - f[0], py - f[1], pz - f[2], px - f[3], py - f[4], pz - f[5], px - f[6],
                      py - f[7], pz - f[8]);
#else
          const double apx = px - f[0], apy = py - f[1], apz = pz - f[2];
          const double bpx = px - f[3], bpy = py - f[4], bpz = pz - f[5];
          const double cpx = px - f[6], cpy = py - f[7], cpz = pz - f[8];
          d2 = tri_d2(f, px, py, pz, apx, apy, apz, bpx, bpy, bpz, cpx, cpy, cpz);
          const double la = sqrt(apx * apx + apy * apy + apz * apz);
          const double lb = sqrt(bpx * bpx + bpy * bpy + bpz * bpz);
          const double lc = sqrt(cpx * cpx + cpy * cpy + cpz * cpz);
          const double det = -(apx * (bpy * cpz - bpz * cpy) + apy * (bpz * cpx - bpx * cpz) +
                               apz * (bpx * cpy - bpy * cpx));
          const double den = la * lb * lc + dot3(apx, apy, apz, bpx, bpy, bpz) * lc +
                             dot3(apx, apy, apz, cpx, cpy, cpz) * lb + dot3(bpx, bpy, bpz, cpx, cpy, cpz) * la;
#if MF_MESHSDF_ABLATE == 1  // timing A/B only (tools/build_variant.sh): the winding term without its atan2
          S += det * den;
#else
          S += 2.0 * atan2(det, den);
#endif
#endif
        } else {
          d2 = seg_d2(f, px, py, pz);
        }
        if (d2 < best) {
          best = d2;
          best_f = (int32_t)(base + i);
        }
      }
    }
  }
  if (!valid) return;
  const double d = sqrt(best);
  const double w = S / kFourPi;
  const bool inside = w >= 0.5 || d <= kOnSurface;
  if (P.dist) P.dist[q] = d;
  if (P.face) P.face[q] = best_f;
  if (P.winding) P.winding[q] = w;
  if (P.sdf) P.sdf[q] = inside ? d : -d;
  if (P.occupancy) P.occupancy[q] = (uint8_t)(w >= 0.5 || d <= tol);
}

int bad(const char *what) {
  mf::set_last_error(hipErrorInvalidValue, what);
  return -(int)hipErrorInvalidValue;
}

}  // namespace

extern "C" int64_t mf_meshsdf_workspace_bytes(int64_t total_faces) {
  if (total_faces < 0 || total_faces > MF_MESHSDF_MAX_FACES) return -1;
  return (int64_t)sizeof(double) * kRec * total_faces;
}

extern "C" int mf_meshsdf_prepare(const mfMeshSdfBatch *batch, int64_t total_faces, mfStream_t stream) {
  if (!batch) return bad("mf_meshsdf_prepare: no batch");
  const mfMeshSdfBatch &P = *batch;
  if (P.n_meshes < 1 || P.n_meshes > MF_MESHSDF_MAX_MESHES) return bad("mf_meshsdf_prepare: 1..65535 meshes");
  if (mf_meshsdf_workspace_bytes(total_faces) < 0) return bad("mf_meshsdf_prepare: faces past MF_MESHSDF_MAX_FACES");
  if (total_faces == 0) return 0;
  const int64_t blocks = (total_faces + kThreads - 1) / kThreads;
  hipLaunchKernelGGL(k_meshsdf_prepare, dim3((unsigned)blocks), dim3(kThreads), 0, (hipStream_t)stream, P.vertices,
                     P.v_off, P.faces, P.f_off, P.n_meshes, P.face_rec);
  return mf::check_launch("mf_meshsdf_prepare");
}

extern "C" int mf_meshsdf_query(const mfMeshSdfBatch *batch, mfStream_t stream) {
  if (!batch) return bad("mf_meshsdf_query: no batch");
  const mfMeshSdfBatch &P = *batch;
  if (P.n_meshes < 1 || P.n_meshes > MF_MESHSDF_MAX_MESHES) return bad("mf_meshsdf_query: 1..65535 meshes");
  if (P.n_blocks < 0) return bad("mf_meshsdf_query: negative n_blocks");
  if (!P.points && (!P.grid_origin || !P.grid_h || P.grid_dim < 1 || P.grid_dim > MF_MESHSDF_MAX_GRID_DIM))
    return bad("mf_meshsdf_query: grid queries need grid_origin, grid_h and 1 <= grid_dim <= 1024");
  if (P.n_blocks == 0) return 0;
  hipLaunchKernelGGL(k_meshsdf_query, dim3(P.n_blocks), dim3(kThreads), 0, (hipStream_t)stream, P);
  return mf::check_launch("mf_meshsdf_query");
}
