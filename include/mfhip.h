/*
 * mfhip.h -- C ABI of libmfhip.so: MI355X (gfx950) kernels for MoreFusion's
 * volumetric pose hot path (voxelize -> trilinear sample -> TDF / pseudo-occupancy
 * -> ICC / ICP refinement -> KNN).
 *
 * The reference has NO binary FFI for this path: its CUDA code is source text
 * handed to cupy.ElementwiseKernel / cupy.RawKernel at run time.
 * Each entry point below therefore replaces one such JIT-kernel call site (cited
 * as file:line under /root/reference/) and is what a maintainer's ctypes stub
 * binds instead.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless marked host; buffers are borrowed,
 *     never freed or reallocated here; outputs and workspaces are caller-allocated;
 *   - all calls are asynchronous on `stream` (a hipStream_t passed as void*), never
 *     synchronise, never allocate device memory (mf_icc_* keep a small host-side
 *     hipGraph cache);
 *   - return 0 on success, a negative hipError_t otherwise (mf_last_error_string());
 *   - float = IEEE binary32, arithmetic un-fused (no FMA contraction) so that voxel
 *     indices and arg-min decisions are bit-identical to the CPU oracle;
 *   - voxel index = round-half-away((p - origin) / pitch)  (CUDA round());
 *   - layouts: points [n,3] row-major; voxel grids [B,C,X,Y,Z] (z fastest).
 */
#ifndef MFHIP_H_
#define MFHIP_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void *mfStream_t; /* hipStream_t */

int mf_version(void);
const char *mf_last_error_string(void);

/* ---- A1/A2 average_voxelization_3d -------------------------------------
 * replaces ElementwiseKernel "average_voxelization_3d_fwd" + the nonzero/divide
 * epilogue   morefusion/functions/geometry/average_voxelization_3d.py:42-118
 * and "voxelize_bwd"                                              :146-220.
 * matrix [B,C,X,Y,Z] and counts [B,X,Y,Z] are written completely (no pre-zero).
 * head [B*X*Y*Z] int32 and link [n] int32 are scratch.  nan_flag (1 int32, may
 * be NULL) is set to 1 if any point coordinate is NaN (reference raises
 * ValueError("points include nan"); the host wrapper does after reading it).
 * Sums are taken in increasing point index (== the reference's CPU loop order),
 * so results are run-to-run deterministic and bit-equal to forward_cpu. */
int mf_average_voxelization_3d_fwd(const float *values, const float *points,
                                   const int32_t *batch_indices, int64_t n, int C,
                                   int B, int X, int Y, int Z, float ox, float oy,
                                   float oz, float pitch, float *matrix,
                                   int32_t *counts, int32_t *head, int32_t *link,
                                   int32_t *nan_flag, mfStream_t stream);
int mf_average_voxelization_3d_bwd(const float *gmatrix, const float *points,
                                   const int32_t *batch_indices,
                                   const int32_t *counts, int64_t n, int C, int B,
                                   int X, int Y, int Z, float ox, float oy, float oz,
                                   float pitch, float *gvalues, mfStream_t stream);

/* ---- A3 max_voxelization_3d ---------------------------------------------
 * replaces "max_voxelization_3d_fwd" + gather, "max_voxelization_3d_bwd"
 *   morefusion/functions/geometry/max_voxelization_3d.py:58-138, :140-185.
 * Winner = max intensity, lowest point index among ties (the CPU rule :33-38;
 * the CUDA CAS/Max/Exch sequence is racy).  indices [B,X,Y,Z] (-1 = empty),
 * matrix [B,C,X,Y,Z] both written completely; key [B*X*Y*Z] uint64 scratch. */
int mf_max_voxelization_3d_fwd(const float *values, const float *points,
                               const int32_t *batch_indices, const float *intensities,
                               int64_t n, int C, int B, int X, int Y, int Z, float ox,
                               float oy, float oz, float pitch, float *matrix,
                               int32_t *indices, uint64_t *key, int32_t *nan_flag,
                               mfStream_t stream);
/* gvalues [n,C] must be zeroed by the caller. */
int mf_max_voxelization_3d_bwd(const float *gmatrix, const int32_t *indices, int64_t n,
                               int C, int B, int X, int Y, int Z, float *gvalues,
                               mfStream_t stream);

/* ---- A4 interpolate_voxel_grid ------------------------------------------
 * replaces "interpolate_voxel_grid_fwd" / "_bwd"
 *   morefusion/functions/geometry/interpolate_voxel_grid.py:159-214, :216-268.
 * points are in voxel-index units; low corner = (int)coord (trunc toward zero).
 * values: [n,C] if channels_first == 0, else [C,n] (coalesced layout the pose
 * network consumes); every row is written (zeros for rows whose batch index is outside
 * [0, B)).  gvox [B,C,X,Y,Z] is written completely by _bwd.
 * batch_start (may be NULL): B+1 row offsets, rows of item b = [batch_start[b],
 * batch_start[b+1]) -- what a caller with batch-sorted points knows for free (the pose network:
 * b * P).  With it a workgroup touches only its item's rows; without it every workgroup
 * filters all n batch_indices. */
int mf_interpolate_voxel_grid_fwd(const float *vox, const float *points,
                                  const int32_t *batch_indices, const int32_t *batch_start,
                                  int64_t n, int B, int C, int X, int Y, int Z, float *values,
                                  int channels_first, mfStream_t stream);
int mf_interpolate_voxel_grid_bwd(const float *gvalues, const float *points,
                                  const int32_t *batch_indices, const int32_t *batch_start,
                                  int64_t n, int B, int C, int X, int Y, int Z, float *gvox,
                                  int channels_first, mfStream_t stream);

/* ---- A5 occupancy_grid_3d -------------------------------------------------
 * replaces the dense [X,Y,Z,P] composite
 *   morefusion/functions/geometry/occupancy_grid_3d.py:31-85
 * with one fused min-over-points kernel.  grid [X,Y,Z]; dmin [X,Y,Z] (saved for
 * backward).  _bwd: gradient to EVERY point at the minimum distance (chainer
 * F.min rule); gpoints [P,3] must be zeroed by the caller. */
int mf_occupancy_grid_3d_fwd(const float *points, int64_t P, float pitch, float ox,
                             float oy, float oz, int X, int Y, int Z, float threshold,
                             float *grid, float *dmin, mfStream_t stream);
int mf_occupancy_grid_3d_bwd(const float *ggrid, const float *points, int64_t P,
                             float pitch, float ox, float oy, float oz, int X, int Y,
                             int Z, float threshold, const float *dmin, float *gpoints,
                             mfStream_t stream);

/* ---- A6/A7 truncated_distance_function, pseudo_occupancy_voxelization ----
 * replaces "truncated_distance_function_fwd" / "_bwd"
 *   morefusion/functions/geometry/truncated_distance_function.py:21-103, :105-166
 * tdf [X,Y,Z]; flat [X,Y,Z] int32 = p*K+k of the arg-min candidate (-1 none;
 * exact arg-min, lowest flat index among equal distances -- the reference's
 * atomicMin/atomicExch pair is racy).  K = ksize^3, ksize = ceil(trunc/pitch)
 * made odd (:36-38).  _bwd: gpoints [P,3] must be zeroed by the caller. */
int mf_truncated_distance_function_fwd(const float *points, int64_t P, float pitch,
                                       float ox, float oy, float oz, int X, int Y, int Z,
                                       float truncation, float *tdf, int32_t *flat,
                                       mfStream_t stream);
int mf_truncated_distance_function_bwd(const float *gtdf, const float *points,
                                       const int32_t *flat, int64_t P, float pitch,
                                       float ox, float oy, float oz, int X, int Y, int Z,
                                       float truncation, float *gpoints,
                                       mfStream_t stream);
/* pseudo_occupancy_voxelization epilogue (:181-213) on the TDF result:
 * grids [3,X,Y,Z] = uniform, surface, inside; wmax: 1 float scratch (zeroed here). */
int mf_pseudo_occupancy_weights(const float *tdf, const int32_t *flat, const float *sdf,
                                int X, int Y, int Z, int K, float truncation,
                                float sdf_offset, float *grids, float *wsurf, float *win,
                                float *wmax, mfStream_t stream);

/* ---- A11 geometry.nn ------------------------------------------------------
 * replaces RawKernel cuComputeDistanceGlobal + cupy.argmin
 *   morefusion/geometry/knn/nn.py:18-49, knn/cuComputeDistanceGlobal.cu:20-86
 * without materialising the R x Q matrix.  dim = 3.  out [Q] int64; optional
 * out_dist [Q] float (squared distance to the match; may be NULL). */
int mf_nn(const float *ref, int64_t R, const float *query, int64_t Q, int64_t *out,
          float *out_dist, mfStream_t stream);

/* ---- A10 IterativeClosestPointLink ----------------------------------------
 *   morefusion/contrib/iterative_closest_point_link.py:26-44
 * source [S,3] model frame, target [T,3]; Rt [12] = row-major R(3x3) then t.
 * out [16]: loss, n_matched, pad, pad, gRt[12] (d loss / d R, d loss / d t).
 * out must be zeroed by the caller. */
int mf_icp_loss_grad(const float *source, int64_t S, const float *target, int64_t T,
                     const float *Rt, float thresh, float *out, mfStream_t stream);

/* The ICP driver's whole loop on the device
 *   examples/ycb_video/pose_refinement/check_iterative_closest_point_link.py:40-70
 * (one link per instance, loss = sum of the links' losses, chainer Adam with the translations'
 * alpha scaled): n_iter x {k_icp over every link, quaternion chain rule + Adam step}, 2 launches
 * per iteration, no host synchronisation and no autograd round trip.
 *   source [sum S_l,3], src_off [L+1]; target [sum T_l,3], tgt_off [L+1]; max_T >= max_l T_l;
 *   q [L,4], t [L,3], adam_m / adam_v [L,7] updated in place; losses [n_iter,L] may be NULL;
 *   ws: 28 * L floats. */
int mf_icp_refine(const float *source, const int32_t *src_off, const float *target,
                  const int32_t *tgt_off, int32_t L, int32_t max_T, float thresh, float *q, float *t,
                  float *adam_m, float *adam_v, int32_t n_iter, int32_t step0, float alpha_q,
                  float alpha_t, float *losses, float *ws, mfStream_t stream);

/* ---- A9 IterativeCollisionCheckLink (fused) --------------------------------
 *   morefusion/contrib/iterative_collision_check_link.py:31-99 (forward),
 *   truncated_distance_function.py:105-166 (backward), driver loop
 *   examples/ycb_video/pose_refinement/check_iterative_collision_check_link.py:44-79
 *
 * A batch holds S independent scenes with O objects in total.  Device arrays:
 *   pts4      [Ptot] float4  model-frame point (x,y,z) + its sdf value (w)
 *   obj_off   [O+1]  int32   point range of object o
 *   scene_off [S+1]  int32   object range of scene s
 *   obj_scene [O]    int32
 *   pitch [O], origin [O,3], grid_target [O,D,D,D], grid_ne [O,D,D,D]
 *   q [O,4] (wxyz), t [O,3]          -- parameters (updated in place by refine)
 *   adam_m, adam_v [O,7]             -- chainer-Adam moments (q then t)
 * ws: workspace of mf_icc_workspace_bytes() bytes.
 */
typedef struct {
  const void *pts4;
  const int32_t *obj_off;
  const int32_t *scene_off;
  const int32_t *obj_scene;
  const float *pitch;
  const float *origin;
  const float *grid_target;
  const float *grid_ne;
  int32_t n_objects; /* O */
  int32_t n_scenes;  /* S */
  int32_t n_points;  /* Ptot */
  int32_t dim;       /* D (32) */
  int32_t max_scene_objects; /* max objects in one scene (<= 128 with grid_ne_binary, else <= 64) */
  float voxel_threshold;
  float sdf_offset;
  int32_t grid_ne_binary; /* != 0: the caller guarantees that every grid_ne value is exactly 0 or 1
                             (what the reference's callers pass: bool grids cast to float32) ->
                             single-pass iteration (TDF tiles and weights/sums in one kernel, two
                             launches per iteration); 0: any values, two-kernel path */
  int32_t flags;          /* reserved, must be 0 (round 5: bit 0 selected the experimental one-launch iteration
                             k_icc_iter -- same bits, measured slower, removed in round 6) */
} mfIccBatch;

/* Bytes of workspace for this batch (negative: invalid descriptor).  Holds the winners of every
 * grid, partial sums, and the per-iteration x-plane bins of voxel-frame point records:
 * (dim + 2h) * max_scene_objects * n_points * 16 B of address space, of which one iteration
 * touches only the points that fall inside a grid. */
int64_t mf_icc_workspace_bytes(const mfIccBatch *batch);

/* Once per batch (and again whenever its point / grid_target arrays change): model-frame
 * bounding spheres, scene tables, sum(grid_target) per scene, the (target grid, source object,
 * point chunk) table and the bin offsets into the workspace. */
int mf_icc_prepare(const mfIccBatch *batch, void *ws, mfStream_t stream);

/* One forward+backward: loss [S], gq [O,4], gt [O,3]; q,t not modified.
 * Requires mf_icc_prepare on the same (batch, ws). */
int mf_icc_loss_grad(const mfIccBatch *batch, const float *q, const float *t,
                     float *loss, float *gq, float *gt, void *ws, mfStream_t stream);

/* n_iter x {forward, backward, chainer-Adam step} entirely on device (one
 * hipGraph launch; no host sync).  losses [n_iter,S] and traj [n_iter,O,7]
 * (pose BEFORE each step) may be NULL.  step0 = number of Adam steps already
 * taken (bias correction). */
int mf_icc_refine(const mfIccBatch *batch, float *q, float *t, float *adam_m,
                  float *adam_v, int32_t n_iter, int32_t step0, float alpha_q,
                  float alpha_t, float *losses, float *traj, void *ws,
                  mfStream_t stream);

/* Bytes of the caller-provided loss-observer buffer of mf_icc_refine_converge: two copies of one record per scene
 * (negative: n_scenes <= 0, or window outside 1 .. 16).  8-byte aligned; its contents need no initialisation. */
int64_t mf_icc_observer_bytes(int32_t n_scenes, int32_t window);

/* mf_icc_refine until each scene's loss has converged, decided on the device: at most max_iter iterations in one
 * hipGraph launch, no host sync, same conventions as mf_icc_refine.  Every scene carries the LossObserver of the
 * reference's ROS node (ros/src/morefusion_ros/nodes/collision_based_pose_refinement.py:18-45; its constants:
 * max_delta_threshold 0.009, window 10, n_passed_threshold 3, max_iter 30), fed after the optimiser step of
 * iteration i (0-based; that step IS applied) with loss_i = losses[i, s]:
 *   i >= 1: delta = |double(loss_{i-1}) - double(loss_i)| enters a window of the `window` most recent deltas;
 *   window not empty: every delta in it < max_delta_threshold (in double) -> n_passed += 1, otherwise n_passed = 0;
 *   n_passed >= n_passed_threshold -> the scene is converged and FROZEN: from the next iteration on none of its
 *   objects takes a step, while the other scenes of the batch go on.
 * Departure from the node, on purpose: while the window holds a non-finite delta the step does not pass (n_passed
 * = 0).  Python's max() over a list holding a NaN depends on the order of the list; this rule does not.
 * Outputs: n_steps [S] = steps applied to each scene (max_iter if it never converged); q, t, adam_m, adam_v of
 * every object = bit for bit what mf_icc_refine with n_iter = n_steps[s] leaves for its scene; rows < n_steps[s] of
 * losses [max_iter,S] / traj [max_iter,O,7] (either may be NULL) as mf_icc_refine writes them, rows >= n_steps[s]
 * of that scene's columns NOT written (pre-fill them).  step0 as in mf_icc_refine; every call starts with fresh
 * observers.  observer: mf_icc_observer_bytes(n_scenes, window) bytes.  Negative return, nothing launched: max_iter
 * < 1, window outside 1 .. 16, observer or n_steps NULL. */
int mf_icc_refine_converge(const mfIccBatch *batch, float *q, float *t, float *adam_m, float *adam_v,
                           int32_t max_iter, int32_t step0, float alpha_q, float alpha_t,
                           double max_delta_threshold, int32_t window, int32_t n_passed_threshold,
                           float *losses, float *traj, int32_t *n_steps, void *observer,
                           void *ws, mfStream_t stream);

/* Launches per iteration mf_icc_refine will use for this batch: 2 = k_icc_bin + k_icc_fused ({0,1} no-entry grids:
 * the default), 3 = k_icc_bin + k_icc_tile + k_icc_accum (any no-entry grid values).  Negative: invalid descriptor. */
int mf_icc_iteration_launches(const mfIccBatch *batch);

/* The launch plan of a batch, as the launchers above will use it (host arithmetic over the descriptor and the
 * MF_ICC_GENERAL / MF_ICC_BIN_CAP environment; launches nothing, touches no device memory, the descriptor's pointers
 * may be NULL).  Fills the first n of these slots and returns how many are defined (15):
 *    0 single_pass             1 launches per iteration       2 kernel behind k_icc_bin: 0 k_icc_tile + k_icc_accum,
 *    3 workspace bytes         4 n_tab (k_icc_bin's grid)       1 k_icc_fused, 2 k_icc_fused_big
 *    5 nbins                   6 hmax                         7 dynamic LDS bytes of the fused kernel (0 on the
 *    8 LDS bytes of k_icc_tile 9 LDS bytes of k_icc_accum       two-kernel path)
 *   10 NB (k_icc_accum's blocks per object)                  11 xcd_order
 *   12 bin_cap_force          13 uniform_ns                  14 rec_n (records of the bins)
 * Negative: invalid descriptor, out == NULL or n <= 0. */
int mf_icc_plan(const mfIccBatch *batch, int64_t *out, int32_t n);

/* Measurement hook so that bench.py can time ONE kernel of an ICC iteration with HIP events:
 * stage 0 = (optional pose refresh from q, t if non-NULL) + empty the bins + k_icc_bin (pose ->
 * world points -> x-plane bins of voxel-frame records); stage 1 = k_icc_tile alone (bins ->
 * per-grid (min distance, arg-min) winners); stage 2 = k_icc_fused alone (bins -> winners ->
 * weights / sums / moments; needs grid_ne_binary).  Stages 1, 2 are repeatable: they do not
 * consume the bins (their sums simply keep adding up). */
int mf_icc_launch_stage(const mfIccBatch *batch, const float *q, const float *t, void *ws,
                        int32_t stage, mfStream_t stream);

/* Tuning aid (a `make ICC_DEBUG=1` build only): with MF_ICC_DEBUG=32 in the environment k_icc_bin / k_icc_tile /
 * k_icc_accum / k_icc_fused record wall_clock64() phase stamps per workgroup; this copies the first n 64-bit words
 * of that table to host memory (synchronous).  Not used by the product path. */
int mf_icc_debug_stamps(unsigned long long *host_out, int n);

/* ---- A13 conv3 of the pose network on sparse voxelized features -----------------
 * replaces the dense cuDNN Convolution3D(Cs+16 -> Cout, k=4, s=2, pad=1) at
 *   morefusion/contrib/singleview_3d/models/model.py:73,128
 * for the Cs voxelized channels, whose input is <= 3 % occupied (counts > 0): 8 parity
 * classes x one fp32-MFMA GEMM [n x Cs].[Cs x 8*Cout] + an output-stationary reduce.
 *   x      [B,Cs,D,D,D]  dense voxelized features (zeros where counts == 0)
 *   counts [B,D,D,D]     from mf_average_voxelization_3d_fwd
 *   Wp     packed weights from mf_sparse_conv3d_pack_weights (8*Cs*8*Cout floats)
 *   dense  [B,Cout,D/2..] optional addend (the dense occupancy-channel part), bias [Cout]
 *   out    [B,Cout,D/2,D/2,D/2] written completely; relu != 0 applies max(.,0)
 *   max_rows >= number of occupied voxels (e.g. the number of points); ws from
 *   mf_sparse_conv3d_workspace_bytes (n_points = 0 for this entry).  Deterministic (fixed tap order, no atomics). */
int64_t mf_sparse_conv3d_workspace_bytes(int32_t B, int32_t Cs, int32_t Cout, int32_t D,
                                         int32_t max_rows, int64_t n_points);
/* W [Cout, w_cin, 4,4,4]; packs input channels [c_off, c_off+Cs). */
int mf_sparse_conv3d_pack_weights(const float *W, int32_t Cout, int32_t Cs, int32_t w_cin,
                                  int32_t c_off, float *Wp, mfStream_t stream);
int mf_sparse_conv3d_k4s2_fwd(const float *x, const int32_t *counts, const float *Wp,
                              const float *dense, const float *bias, float *out, void *ws,
                              int32_t B, int32_t Cs, int32_t Cout, int32_t D, int32_t max_rows,
                              int32_t relu, mfStream_t stream);

/* ---- A12 functions.average_distance (ADD / ADD-S pose loss), batched ----------------
 * replaces the transform_points x2 + geometry.nn + gather + sub/square/sum/sqrt/mean composite
 *   morefusion/functions/loss/average_distance.py:64-85
 * and the per-object Python loop around it, contrib/singleview_3d/models/model.py:406-434.
 *   points [B,M,3] model points, T_true [B,4,4], T_pred [B,P,4,4] row-major, symmetric [B]
 *   uint8 (NULL = none): 0 -> ADD, else ADD-S (nearest true point, lowest index among equal
 *   squared distances).  out [B,P] = mean_m || true'_m - pred_m ||.
 *   nn_idx [B,P,M] int32 (may be NULL): arg-min indices of the ADD-S rows, written by _fwd and
 *   read by _bwd (NULL: _bwd searches again).
 * _bwd: gT_pred [B,P,4,4] = d(sum gout * out) / d T_pred (rows 0..2; row 3 = 0).  The true
 * pose and the model points receive no gradient (they are data in the reference's callers).
 * A point whose residual is exactly zero adds nothing to the gradient.  A predicted pose with a
 * non-finite entry gives out = NaN; no candidate of its ADD-S search compares below +inf, so its
 * nn_idx row holds 0 wherever the query is NaN (the first-minimum rule over NaN distances), and
 * its gT_pred rows are zeros (a NaN distance is not > 0).  B <= 0 or P <= 0: nothing to do,
 * returns 0; M <= 0: -hipErrorInvalidValue (-1) before any launch. */
int mf_average_distance_fwd(const float *points, const float *T_true, const float *T_pred,
                            const uint8_t *symmetric, int32_t B, int32_t M, int32_t P,
                            float *out, int32_t *nn_idx, mfStream_t stream);
int mf_average_distance_bwd(const float *points, const float *T_true, const float *T_pred,
                            const uint8_t *symmetric, const float *gout, int32_t B, int32_t M,
                            int32_t P, const int32_t *nn_idx, float *gT_pred, mfStream_t stream);

/* The same convolution fed by the POINTS (inference): average_voxelization_3d's per-voxel chains
 * write the compact rows the GEMM consumes -- the dense [B,Cs,D,D,D] tensor of
 *   morefusion/contrib/singleview_3d/models/model.py:114-128 (151 MB at B = 8) is never
 * materialised.  values [n,Cs], points [n,3] voxel-frame (origin o, pitch), batch_indices [n];
 * same means (increasing point index), same output bits as voxelize + mf_sparse_conv3d_k4s2_fwd.
 * ws from mf_sparse_conv3d_workspace_bytes(..., n_points = n). */
int mf_sparse_conv3d_k4s2_points_fwd(const float *values, const float *points,
                                     const int32_t *batch_indices, int64_t n, float ox, float oy,
                                     float oz, float pitch, const float *Wp, const float *dense,
                                     const float *bias, float *out, void *ws, int32_t B,
                                     int32_t Cs, int32_t Cout, int32_t D, int32_t max_rows,
                                     int32_t relu, mfStream_t stream);

/* ---- A13 conv4 (and the dense occupancy channels of conv3): Convolution3D k=4 s=2 pad=1 ----
 * replaces the cuDNN convolutions at
 *   morefusion/contrib/singleview_3d/models/model.py:74,139  (conv4: 256 -> 512 on 16^3, + ReLU)
 *   morefusion/contrib/singleview_3d/models/model.py:73,128  (conv3's 16 dense occupancy channels)
 * with an fp32-MFMA (v_mfma_f32_32x32x2_f32, exact fp32) implicit GEMM over CHANNELS-LAST tensors:
 *   x    [B, D,D,D, Cin]          Cin a power of two >= 4
 *   wt   [Cout, 64, Cin]          from mf_conv3d_k4s2_pack_weights (tap = (kx*4 + ky)*4 + kz)
 *   bias [Cout] or NULL, add [B, (D/2)^3, Cout] or NULL (added before the activation)
 *   out  [B, D/2,D/2,D/2, Cout]   Cout % 128 == 0; relu != 0 applies max(., 0)
 *   split: K (taps) is cut into `split` slabs (mf_conv3d_k4s2_default_split picks >= 512 workgroups),
 *   partial sums go to ws (mf_conv3d_k4s2_workspace_bytes) and are added in slab order: deterministic. */
int mf_conv3d_k4s2_pack_weights(const float *W, int32_t Cout, int32_t Cin, int32_t w_cin, int32_t c_off,
                                float *wt, mfStream_t stream);
int32_t mf_conv3d_k4s2_default_split(int32_t B, int32_t Cin, int32_t Cout, int32_t D);
int64_t mf_conv3d_k4s2_workspace_bytes(int32_t B, int32_t Cout, int32_t D, int32_t split);
int mf_conv3d_k4s2_fwd(const float *x, const float *wt, const float *bias, const float *add, float *out,
                       void *ws, int32_t B, int32_t Cin, int32_t Cout, int32_t D, int32_t split,
                       int32_t relu, mfStream_t stream);
/* [B, C, V] -> [B, V, C] (channels-first grid -> channels-last) */
int mf_to_channels_last(const float *src, float *dst, int32_t B, int32_t C, int64_t V, mfStream_t stream);

/* Channels-last forms of the inference path between conv3 and the heads (same results as the
 * channels-first entries above, other memory layout):
 *   mf_sparse_conv3d_k4s2_points_cl_fwd: as mf_sparse_conv3d_k4s2_points_fwd, but values rows have pitch
 *     ldv floats (a column block of a wider matrix), dense / out are [B, (D/2)^3, Cout]; Cout % 256 == 0.
 *   mf_interpolate_voxel_grid_cl_fwd (replaces K5, interpolate_voxel_grid.py:170-212, for vox
 *     [B, X*Y*Z, C]): out[p*ldo + c], rows of pitch ldo floats; rows with a batch index outside [0,B) = 0.
 *   mf_occupancy_convs_fwd (replaces the cuDNN Convolution3D pair model.py:69-72,120-124: 1 -> 8 k3 pad 1,
 *     8 -> 16 k3 dilation 2 pad 2, ReLU after each): grid [B,D,D,D] -> h2 [B, D^3, 16]; h1 [B, D^3, 8] scratch;
 *     w1 [27,1,8], w2 [27,8,16] = W.permute(2,3,4,1,0) of the Chainer/torch weight. */
int mf_sparse_conv3d_k4s2_points_cl_fwd(const float *values, int64_t ldv, const float *points,
                                        const int32_t *batch_indices, int64_t n, float ox, float oy,
                                        float oz, float pitch, const float *Wp, const float *dense,
                                        const float *bias, float *out, void *ws, int32_t B, int32_t Cs,
                                        int32_t Cout, int32_t D, int32_t max_rows, int32_t relu,
                                        mfStream_t stream);
int mf_interpolate_voxel_grid_cl_fwd(const float *vox, const float *points, const int32_t *batch_indices,
                                     int64_t n, int B, int C, int X, int Y, int Z, float *out, int64_t ldo,
                                     mfStream_t stream);
/* The same two with split-bf16 outputs (operands of mf_conv3d_k4s2_split_fwd / mf_linear_split_fwd): the sparse conv3
 * also writes out_split bf16 [B, (D/2)^3, 2 Cout] = the split of its fp32 output; the sampler writes hi at
 * outs[p*ldos + c] and lo at outs[p*ldos + los + c] of bf16 rows INSTEAD of the fp32 samples. */
int mf_sparse_conv3d_k4s2_points_cl_split_fwd(const float *values, int64_t ldv, const float *points,
                                              const int32_t *batch_indices, int64_t n, float ox, float oy, float oz,
                                              float pitch, const float *Wp, const float *dense, const float *bias,
                                              float *out, void *out_split, void *ws, int32_t B, int32_t Cs,
                                              int32_t Cout, int32_t D, int32_t max_rows, int32_t relu,
                                              mfStream_t stream);
int mf_interpolate_voxel_grid_cl_split_fwd(const float *vox, const float *points, const int32_t *batch_indices,
                                           int64_t n, int B, int C, int X, int Y, int Z, void *outs, int64_t ldos,
                                           int64_t los, mfStream_t stream);
int mf_occupancy_convs_fwd(const float *grid, const float *w1, const float *b1, const float *w2,
                           const float *b2, float *h1, float *h2, int32_t B, int32_t D, mfStream_t stream);
/* The same with h2's split-bf16 form written by the second convolution's own launch: h2s bf16 [B, D^3, 2 x 16] (a
 * voxel's 16 hi channels, then its 16 lo channels: the split of the fp32 value h2 gets), the operand of
 * mf_conv3d_k4s2_split_fwd on conv3's occupancy channels.  h2 may be null (only the split form is written). */
int mf_occupancy_convs_split_fwd(const float *grid, const float *w1, const float *b1, const float *w2,
                                 const float *b2, float *h1, float *h2, void *h2s, int32_t B, int32_t D,
                                 mfStream_t stream);

/* ---- per-point 1x1 convolutions (heads, point MLP) as row-major fp32-MFMA GEMMs ---------------
 * replaces the cuDNN Convolution1D(k = 1) chains at
 *   morefusion/contrib/singleview_3d/models/model.py:76-91,245-262 (three heads: 984-640-256-128-n_fg*c)
 * on points-major activations:  out[m][n] = act( sum_k A[m][k] * W[n][k] + bias[n] ),  m < M, n < N.
 *   A [M, lda], W [Npad, ldw] (Convolution1D's W[:, :, 0], zero rows up to Npad % 128 == 0), out [M, ldo];
 *   `groups` independent problems per launch at the given element strides (heads side by side, each
 *   reading / writing its own column block); K % 4 == 0 (no multiple of 32 needed); relu != 0: max(., 0). */
int mf_linear_fwd(const float *A, int64_t a_group_stride, int32_t lda, const float *W, int64_t w_group_stride,
                  int32_t ldw, const float *bias, int64_t b_group_stride, float *out, int64_t o_group_stride,
                  int32_t ldo, int32_t M, int32_t N, int32_t Npad, int32_t K, int32_t groups, int32_t relu,
                  mfStream_t stream);

/* ---- bf16 training / inference path of the 3-D CNN and the 1x1 convolution chains (round 4) --------------------
 * replaces cuDNN's forward, backward-data and backward-filter of
 *   morefusion/contrib/singleview_3d/models/model.py:73-74,125-139 (conv3, conv4: Convolution3D(.., 4, 2, pad = 1))
 *   morefusion/contrib/singleview_3d/models/model.py:59-66,76-91,101-111,239-258 (Convolution1D chains)
 * as trained by examples/ycb_video/singleview_3d/train.py:342-369 (BASELINE config 5: bf16, data-parallel).
 * All activations / gradients are bf16 (the framework's bfloat16 bit pattern, passed as void *), accumulation is
 * fp32 on v_mfma_f32_32x32x16_bf16, parameters and their gradients stay fp32 (csrc/gemm_bf16.hip).
 *
 * mf_cast_rows_bf16     fp32 [rows, src_ld] -> bf16 [rows, dst_ld] (columns >= cols zero; dst_ld % 8 == 0)
 * mf_relu_mask_bf16     dz = (y > 0) ? dy : 0 over n elements (n % 8 == 0); dy bf16, or dy32 fp32 (exactly one)
 * mf_linear_bf16        out = act(A W^T + bias): A [M, lda], W [N, ldw] bf16 (rows k-contiguous), bias fp32 [N],
 *                       out [M, ldo] bf16 or fp32 (out_f32), `accumulate`: out += (fp32 only); `groups` problems
 *                       per launch at the given element strides.  The data gradient of a layer is the same call
 *                       with the transposed weight: dA = dY W  ->  mf_linear_bf16(dY, W^T [K, N]).
 * mf_linear_wgrad_bf16  dW [N, ldc] fp32 = sum_m dY[m][n] A[m][k]; split > 1: row ranges into ws
 *                       (split * groups * N * ldc floats), summed in range order.
 * mf_conv3d_k4s2_pack_bf16   W fp32 [Cout, w_cin, 4, 4, 4] (channels c_off .. c_off + Cin) -> fwd bf16
 *                       [Cout, 64, Cin] and / or dgrad bf16 [8 parity classes, Cin, 8 slots, Cout] (either may be null)
 * mf_conv3d_k4s2_bf16_fwd    out [B, (D/2)^3, Cout] = act(conv(x [B, D^3, Cin]) + bias)      (channels-last)
 * mf_conv3d_k4s2_bf16_dgrad  dx [B, D^3, Cin] (+)= conv^T(dy [B, (D/2)^3, Cout]); bf16, or fp32 (+ accumulate)
 * mf_conv3d_k4s2_bf16_wgrad  dW fp32 in the framework layout (channels c_off ..) = sum_voxels dy (x) im2col(x);
 *                       ws: mf_conv3d_k4s2_bf16_wgrad_workspace_bytes(Cin, Cout, split)
 * D is a power of two, Cin % 8 == 0, Cout % 8 == 0.  Asynchronous, never allocate or synchronise.
 *
 * The same engines with a general geometry -- kernel ks in {3, 4}, stride in {1, 2}, pad, dilation; output size
 * Do = (D + 2 pad - dil (ks - 1) - 1) / stride + 1 a power of two -- run the occupancy branch
 *   morefusion/contrib/singleview_3d/models/model.py:69-72,120-124 (conv1_occ 1 -> 8 k3 p1, conv2_occ 8 -> 16 k3
 *   dilation 2 p2; a 1-channel input is fed as 8 channels, 7 of them zero):
 * mf_conv3d_bf16_pack   fwd [Cout, ks^3, Cin]; dgrad_k4s2 (ks = 4 only); flipT [Cin, ks^3, Cout] = the forward operand
 *                       of a stride-1 layer's data-gradient convolution (dx = conv(dy, flipT), pad' = dil (ks-1) - pad);
 *                       input channels at or beyond w_cin pack as zeros
 * mf_conv3d_bf16_fwd    out rows have pitch ldo >= Cout (a column block of a wider channels-last grid)
 * mf_conv3d_bf16_fwd_ws the same with a workspace of mf_conv3d_bf16_fwd_workspace_bytes(...) bytes (0: not needed): a
 *                       layer with too few 256 x 256 output tiles for the chip (conv4 at 16 objects: 64) splits its
 *                       reduction over fp32 slabs in the workspace, added in order (deterministic) with bias / ReLU
 * mf_conv3d_bf16_wgrad  as above; only the channels below w_cin are written */
int mf_cast_rows_bf16(const float *src, int64_t src_ld, void *dst, int64_t dst_ld, int64_t rows, int32_t cols,
                      mfStream_t stream);
int mf_relu_mask_bf16(const void *y, const void *dy, const float *dy32, void *dz, int64_t n, mfStream_t stream);
int mf_linear_bf16(const void *A, int64_t a_group_stride, int32_t lda, const void *W, int64_t w_group_stride,
                   int32_t ldw, const float *bias, int64_t b_group_stride, void *out, int64_t o_group_stride,
                   int32_t ldo, int32_t M, int32_t N, int32_t K, int32_t groups, int32_t relu, int32_t out_f32,
                   int32_t accumulate, mfStream_t stream);
int mf_linear_wgrad_bf16(const void *dY, int64_t y_group_stride, int32_t ldy, const void *A, int64_t a_group_stride,
                         int32_t lda, float *dW, int64_t w_group_stride, int32_t ldc, void *ws, int32_t M, int32_t N,
                         int32_t K, int32_t groups, int32_t split, mfStream_t stream);
int mf_conv3d_k4s2_pack_bf16(const float *W, int32_t Cout, int32_t Cin, int32_t w_cin, int32_t c_off, void *fwd,
                             void *dgrad, mfStream_t stream);
int mf_conv3d_k4s2_bf16_fwd(const void *x, const void *wt, const float *bias, void *out, int32_t B, int32_t Cin,
                            int32_t Cout, int32_t D, int32_t relu, int32_t out_f32, mfStream_t stream);
int mf_conv3d_k4s2_bf16_dgrad(const void *dy, const void *wd, void *dx, int32_t B, int32_t Cin, int32_t Cout,
                              int32_t D, int32_t out_f32, int32_t accumulate, mfStream_t stream);
int64_t mf_conv3d_k4s2_bf16_wgrad_workspace_bytes(int32_t Cin, int32_t Cout, int32_t split);
int32_t mf_conv3d_k4s2_bf16_wgrad_default_split(int32_t B, int32_t Cin, int32_t Cout, int32_t D);
int mf_conv3d_k4s2_bf16_wgrad(const void *dy, const void *x, float *dW, void *ws, int32_t B, int32_t Cin,
                              int32_t Cout, int32_t D, int32_t w_cin, int32_t c_off, int32_t split,
                              mfStream_t stream);

int mf_conv3d_bf16_pack(const float *W, int32_t Cout, int32_t Cin, int32_t w_cin, int32_t c_off, int32_t ks, void *fwd,
                        void *dgrad_k4s2, void *flipT, mfStream_t stream);
int mf_conv3d_bf16_fwd(const void *x, const void *wt, const float *bias, void *out, int32_t B, int32_t Cin,
                       int32_t Cout, int32_t D, int32_t ks, int32_t stride, int32_t pad, int32_t dil, int32_t relu,
                       int32_t out_f32, int32_t ldo, mfStream_t stream);
int64_t mf_conv3d_bf16_fwd_workspace_bytes(int32_t B, int32_t Cin, int32_t Cout, int32_t D, int32_t ks, int32_t stride,
                                           int32_t pad, int32_t dil);
int mf_conv3d_bf16_fwd_ws(const void *x, const void *wt, const float *bias, void *out, void *ws, int64_t ws_bytes,
                          int32_t B, int32_t Cin, int32_t Cout, int32_t D, int32_t ks, int32_t stride, int32_t pad,
                          int32_t dil, int32_t relu, int32_t out_f32, int32_t ldo, mfStream_t stream);
/* 2-D convolutions of the inference backbone (models/backbone2d.py) as split-bf16 GEMMs on the NT engine: an fp32 value
 * is carried as hi = bf16(x), lo = bf16(x - hi) and a product as hi w_hi + lo w_hi + hi w_lo, accumulated in fp32
 * (relative error per product <= ~3 * 2^-18).  Kernel 1 or 3, stride 1 or 2, dilation 1 .. 4, any pad, output side
 * Do a power of two; Cin, Cout % 8 == 0.
 * mf_conv2d_split_pack   W fp32 [Cout][Cin][ks][ks] -> wp bf16 [Cout][ks^2][3 Cin] = [w_hi | w_hi | w_lo] per tap
 * mf_conv2d_split_fwd    xs bf16 [B][D][D][2 Cin] (hi channels, then lo channels); row m = (b, oy, ox):
 *                        v = act(conv + bias + res[m * ldr ..])  act 0 none, 1 ReLU, 2 PReLU with the slope *slope
 *                        out32[m * ldo32 + n] = v and / or outs[m * ldos + n] = hi(v), outs[m * ldos + los + n] = lo(v)
 *                        (null outputs / bias / res are skipped; pitches multiples of 8, operands 16-byte aligned);
 *                        ws: mf_conv2d_split_workspace_bytes(...) bytes of split-K slabs (0: none needed) */
int mf_conv2d_split_pack(const float *W, int32_t Cout, int32_t Cin, int32_t ks, void *wp, mfStream_t stream);
int64_t mf_conv2d_split_workspace_bytes(int32_t B, int32_t Cin, int32_t Cout, int32_t D, int32_t ks, int32_t stride,
                                        int32_t pad, int32_t dil);
int mf_conv2d_split_fwd(const void *xs, const void *wp, const float *bias, const float *res, int32_t ldr,
                        const float *slope, int32_t act, float *out32, int32_t ldo32, void *outs, int32_t ldos,
                        int32_t los, void *ws, int64_t ws_bytes, int32_t B, int32_t Cin, int32_t Cout, int32_t D,
                        int32_t ks, int32_t stride, int32_t pad, int32_t dil, mfStream_t stream);
/* The volumetric part's fp32 layers on the same scheme (fp32 inference; the fp32-MFMA entries mf_conv3d_k4s2_fwd /
 * mf_linear_fwd are unchanged and serve small batches).  Outputs as mf_conv2d_split_fwd: v = act(.. + bias), relu 0 / 1,
 * out32[m * ldo32 + n] = v and / or outs[m * ldos + n] = hi(v), outs[m * ldos + los + n] = lo(v).  ws: the matching
 * *_workspace_bytes(...) bytes of split-K slabs (0: none needed); slabs are added in slab order (bit-reproducible).
 * mf_conv3d_k4s2_split_pack  W fp32 [Cout][w_cin][4][4][4], channels c_off .. c_off + Cin - 1 -> wp bf16 [Cout][64][3 Cin]
 * mf_conv3d_k4s2_split_fwd   Convolution3D k4 s2 p1: xs bf16 [B][D^3][2 Cin] (hi channels, then lo channels), row m =
 *                            (b, output voxel), D / 2 a power of two
 * mf_linear_split_pack       W fp32 [G][N][K] (row pitch ldw, group stride w_gs) -> wp bf16 [G][Np][3 Kp], zero padded
 * mf_linear_split_fwd        As bf16 [M][lda]: columns 0 .. Kp - 1 hi, Kp .. 2 Kp - 1 lo; wp [Np >= N][3 Kp]; N % 8 == 0 */
int mf_conv3d_k4s2_split_pack(const float *W, int32_t Cout, int32_t Cin, int32_t w_cin, int32_t c_off, void *wp,
                              mfStream_t stream);
int64_t mf_conv3d_k4s2_split_workspace_bytes(int32_t B, int32_t Cin, int32_t Cout, int32_t D);
int mf_conv3d_k4s2_split_fwd(const void *xs, const void *wp, const float *bias, int32_t relu, float *out32,
                             int32_t ldo32, void *outs, int32_t ldos, int32_t los, void *ws, int64_t ws_bytes, int32_t B,
                             int32_t Cin, int32_t Cout, int32_t D, mfStream_t stream);
int mf_linear_split_pack(const float *W, int64_t w_gs, int32_t ldw, int32_t N, int32_t K, int32_t Np, int32_t Kp,
                         int32_t groups, void *wp, mfStream_t stream);
int64_t mf_linear_split_workspace_bytes(int64_t M, int32_t N, int32_t Kp);
int mf_linear_split_fwd(const void *As, int32_t lda, const void *wp, const float *bias, int32_t relu, float *out32,
                        int32_t ldo32, void *outs, int32_t ldos, int32_t los, void *ws, int64_t ws_bytes, int32_t M,
                        int32_t N, int32_t Kp, mfStream_t stream);
/* 3 x 3 x 3, stride 1, pad = dilation convolutions between NARROW layers (read channels 8 or 16, written channels <= 16)
 * on channels-last bf16 grids -- the occupancy branch conv1_occ / conv2_occ (model.py:69-72,120-124) and conv2_occ's
 * data gradient (pack with transpose = 1): voxels are the MFMA's columns, operands straight from global memory.
 * wp: mf_conv3d_k3_narrow_bf16_pack_elems(CI) bf16, CI = channels of the tensor the convolution reads. */
int64_t mf_conv3d_k3_narrow_bf16_pack_elems(int32_t CI);
int mf_conv3d_k3_narrow_bf16_pack(const float *W, int32_t Cout, int32_t Cin, int32_t w_cin, int32_t c_off,
                                  int32_t transpose, void *wp, mfStream_t stream);
int mf_conv3d_k3_narrow_bf16(const void *x, const void *wp, const float *bias, void *out, int32_t B, int32_t CI,
                             int32_t CO, int32_t D, int32_t dil, int32_t relu, mfStream_t stream);
int64_t mf_conv3d_bf16_wgrad_workspace_bytes(int32_t Cin, int32_t Cout, int32_t ks, int32_t split);
int32_t mf_wgrad_split(int64_t tiles, int64_t ktiles, int64_t slab_bytes);
/* slabs mf_linear_wgrad_bf16 should be given for dW [N][K] over M rows (answers for the tile form that will run) */
int32_t mf_linear_wgrad_bf16_default_split(int64_t M, int32_t N, int32_t K, int32_t groups);
int32_t mf_conv3d_bf16_wgrad_default_split(int32_t B, int32_t Cin, int32_t Cout, int32_t Do, int32_t ks);
int mf_conv3d_bf16_wgrad(const void *dy, const void *x, float *dW, void *ws, int32_t B, int32_t Cin, int32_t Cout,
                         int32_t D, int32_t ks, int32_t stride, int32_t pad, int32_t dil, int32_t w_cin, int32_t c_off,
                         int32_t split, mfStream_t stream);

/* ---- conv3 of the bf16 training path on OCCUPIED VOXELS only (round 5; csrc/sparseconv_bf16.hip) -----------------
 * replaces the dense forward / backward-data / backward-filter of `L.Convolution3D(None, 256, 4, 2, pad=1)` over the
 * voxelized point features (contrib/singleview_3d/models/model.py:73,114-128; train.py:342-369): average_voxelization_3d
 * leaves <= 1000 of an object's 32768 voxels occupied in 144 of the 160 input channels.  Compact CLASS-MAJOR rows
 * (8 parity classes of the k4 / s2 / p1 geometry, each padded to a multiple of 128 rows):
 *   mf_sparse_conv3_bf16_index      points [n,3] (voxel frame: origin 0, pitch 1), batch_indices -> chains, row map,
 *                                   row -> voxel map, class row ranges, class of every 64-row block (all in ws)
 *   mf_sparse_conv3_bf16_tables     device addresses of those tables (see csrc/sparseconv_bf16.hip)
 *   mf_average_voxelization_rows_bf16_fwd / _bwd   voxel means into / gradients out of the compact rows A [rows, lda]
 *   mf_sparse_conv3_bf16_pack       W fp32 [Cout, w_cin, 4,4,4] channels c_off.. -> Wp bf16 [8][8 Cout][Cs] (forward /
 *                                   weight-gradient operand) and Wq bf16 [8][Cs][8 Cout] (data-gradient operand, or NULL)
 *   mf_linear_bf16_tiles            C = A Wp[class(row)]^T, the class of every 64-row block from the device table
 *   mf_sparse_conv3_bf16_reduce     out [B, (D/2)^3, Cout] bf16 = relu?(dense fp32 (or NULL) + bias + the <= 64
 *                                   (voxel, tap) contributions of every output voxel, in tap order)
 *   mf_sparse_conv3_bf16_gather_dy  dYg [rows, 8 Cout] = dz at the 8 output voxels each row feeds (zeros outside)
 *   mf_linear_wgrad_bf16_ranges     dWp[class] = dYg^T A over the class's row range (device table)
 *   mf_sparse_conv3_bf16_unpack_dw  dWp fp32 [8][8 Cout][Cs] -> dW fp32 [Cout, w_cin, 4,4,4] channels c_off..
 * rows = mf_sparse_conv3_bf16_max_rows(n) = n + 8 * 127 rounded up to 128.  Asynchronous, never allocate. */
int64_t mf_sparse_conv3_bf16_max_rows(int64_t n_points);
int64_t mf_sparse_conv3_bf16_workspace_bytes(int64_t n_points, int32_t B, int32_t D);
int mf_sparse_conv3_bf16_tables(void *ws, int64_t n_points, int32_t B, int32_t D, int64_t *out7);
int mf_sparse_conv3_bf16_index(const float *points, const int32_t *batch_indices, int64_t n, int32_t B, int32_t D,
                               void *ws, mfStream_t stream);
int mf_sparse_conv3_bf16_pack(const float *W, int32_t Cout, int32_t Cs, int32_t w_cin, int32_t c_off, void *Wp, void *Wq,
                              mfStream_t stream);
int mf_sparse_conv3_bf16_unpack_dw(const float *dWp, int32_t Cout, int32_t Cs, int32_t w_cin, int32_t c_off, float *dW,
                                   mfStream_t stream);
int mf_sparse_conv3_bf16_reduce(const void *C, const float *dense, const float *bias, void *ws, int64_t n_points,
                                int32_t B, int32_t D, int32_t Cout, int32_t relu, void *out, mfStream_t stream);
int mf_sparse_conv3_bf16_gather_dy(const void *dz, void *ws, int64_t n_points, int32_t B, int32_t D, int32_t Cout,
                                   void *dYg, mfStream_t stream);
int mf_linear_bf16_tiles(const void *A, int32_t lda, const void *W, int64_t w_group_stride, int32_t ldw,
                         const int32_t *tile_group, void *out, int32_t ldo, int32_t M, int32_t N, int32_t K,
                         int32_t out_f32, mfStream_t stream);
int mf_linear_wgrad_bf16_ranges(const void *dY, int32_t ldy, const void *A, int32_t lda, float *dW,
                                int64_t w_group_stride, int32_t ldc, const int32_t *m_range, int32_t groups, int32_t N,
                                int32_t K, mfStream_t stream);
/* Narrow-input data gradient of Convolution3D(.., 4, 2, pad=1) "columns first" (the 16 occupancy channels of conv3):
 * W2 bf16 [64 Cin][Cout]; T [B (D/2)^3][64 Cin] = dz W2^T through mf_linear_bf16; dx [B, D^3, Cin] = col2im gather. */
int mf_conv3d_k4s2_bf16_pack_cols(const float *W, int32_t Cout, int32_t Cin, int32_t w_cin, int32_t c_off, void *W2,
                                  mfStream_t stream);
int mf_conv3d_k4s2_bf16_col2im(const void *T, int32_t B, int32_t D, int32_t Cin, void *dx, mfStream_t stream);
int mf_average_voxelization_rows_bf16_fwd(const void *values, int64_t ldv, const float *points,
                                          const int32_t *batch_indices, int64_t n, int32_t C, int32_t B, int32_t D,
                                          const int32_t *counts, const int32_t *head, const int32_t *link,
                                          const int32_t *rowmap, void *A, int64_t lda, mfStream_t stream);
int mf_average_voxelization_rows_bf16_bwd(const void *dA, int64_t lda, const float *points,
                                          const int32_t *batch_indices, const int32_t *counts, const int32_t *rowmap,
                                          int64_t n, int32_t C, int32_t B, int32_t D, void *gvalues, int64_t ldg,
                                          mfStream_t stream);

/* Channels-last bf16 voxelization and trilinear sampling of the bf16 training path (K1/K2 and K5/K6 of SURVEY 2.1 --
 * functions/geometry/average_voxelization_3d.py:8-113, interpolate_voxel_grid.py:61-215 -- on the layout the bf16
 * convolutions consume; origin 0, pitch 1, cubic grids, as contrib/singleview_3d/models/model.py:113,131,141 call them):
 *   mf_average_voxelization_cl_bf16_fwd  values bf16 [n, ldv] -> x bf16 [B, D^3, ldx] columns [0, C): voxel means
 *     (fp32 sum in increasing point index), zeros elsewhere; counts / head [B*D^3], link [n]: int32 scratch
 *   mf_average_voxelization_cl_bf16_bwd  gvalues[p] = gx[b, voxel(p)] / count
 *   mf_interpolate_voxel_grid_cl_bf16_fwd / _bwd   vox bf16 [B, X*Y*Z, C] <-> rows bf16 [n, ld]; the backward gathers
 *     per voxel range (fp32 sums in LDS) and writes every element of gvox [B, X*Y*Z, C] once, as bf16 (out_bf16 = 1)
 *     or fp32; batch_start = B + 1 row offsets of points sorted by item, or NULL (any order, slower) */
int mf_average_voxelization_cl_bf16_fwd(const void *values, int64_t ldv, const float *points,
                                        const int32_t *batch_indices, int64_t n, int32_t C, int32_t B, int32_t D,
                                        void *x, int64_t ldx, int32_t *counts, int32_t *head, int32_t *link,
                                        mfStream_t stream);
int mf_average_voxelization_cl_bf16_bwd(const void *gx, int64_t ldx, const float *points, const int32_t *batch_indices,
                                        const int32_t *counts, int64_t n, int32_t C, int32_t B, int32_t D,
                                        void *gvalues, int64_t ldg, mfStream_t stream);
int mf_interpolate_voxel_grid_cl_bf16_fwd(const void *vox, const float *points, const int32_t *batch_indices,
                                          int64_t n, int B, int C, int X, int Y, int Z, void *out, int64_t ldo,
                                          mfStream_t stream);
int mf_interpolate_voxel_grid_cl_bf16_bwd(const void *gout, int64_t ldg, const float *points,
                                          const int32_t *batch_indices, const int32_t *batch_start, int64_t n, int B,
                                          int C, int X, int Y, int Z, void *gvox, int32_t out_bf16, mfStream_t stream);

/* Element-wise pieces of the 2-D backbone's decoder (morefusion/models/dense_fusion/pspnet.py:10-35,40-73:
 * F.resize_images bilinear align_corners, L.PReLU with one slope), forward and backward, channels-last tensors
 * [B, H, W, C], float32 (bf16 = 0) or bfloat16 (bf16 = 1), C % 8 == 0:
 *   mf_upsample_bilinear_cl_fwd  y [B, Ho, Wo, C] from x [B, H, W, C]
 *   mf_upsample_bilinear_cl_bwd  gx from gy: a gather in increasing (oy, ox) -- deterministic, no atomics
 *   mf_prelu_fwd / mf_prelu_bwd  y = x > 0 ? x : a x;  dx and dslope[0] = sum_{x <= 0} dy x (ws: mf_prelu_bwd_workspace_floats) */
int mf_upsample_bilinear_cl_fwd(const void *x, void *y, int32_t B, int32_t H, int32_t W, int32_t Ho, int32_t Wo,
                                int32_t C, int32_t bf16, mfStream_t stream);
/* the split-bf16 operand of mf_conv2d_split_fwd (hi at channel c, lo at channel los + c of rows of pitch ldy):
 *   mf_upsample_bilinear_cl_split_fwd  the resize of fp32 x [B, H, W, C] (channels-last), taken in fp32, then split
 *   mf_split_bf16                      fp32 x [B, C, H, W] at element strides (sb, sc, sh, sw), split */
int mf_upsample_bilinear_cl_split_fwd(const float *x, void *y, int32_t B, int32_t H, int32_t W, int32_t Ho, int32_t Wo,
                                      int32_t C, int32_t ldy, int32_t los, mfStream_t stream);
int mf_split_bf16(const float *x, int64_t sb, int64_t sc, int64_t sh, int64_t sw, int32_t B, int32_t C, int32_t H,
                  int32_t W, void *y, int32_t ldy, int32_t los, mfStream_t stream);
/* PSPUpsample (x2 resize -> 3 x 3 convolution) with the convolution taken first: z fp32 [B, H, W, 9 C]
 * holds the nine per-tap 1 x 1 convolutions of the low-resolution map (column t C + c, t = ky 3 + kx); output pixel p of
 * the [B, 2H, 2W] map is v = act(bias + sum over the taps whose position p + (ky - 1, kx - 1) lies inside the map of
 * bilinear(z_t) there), in increasing t, fp32.  v goes to y32[m * ld32 + c] and / or, split, to ys[m * lds + c] (hi) and
 * ys[m * lds + los + c] (lo); either may be null.  act: 0 none, 1 ReLU, 2 PReLU with *slope (device pointer). */
int mf_upsample2x_tapsum_fwd(const float *z, const float *bias, const float *slope, int32_t act, float *y32,
                             int32_t ld32, void *ys, int32_t lds, int32_t los, int32_t B, int32_t H, int32_t W, int32_t C,
                             mfStream_t stream);
/* ResNet18's stem tail in fp32 inference: max_pool2d(3, 2, 1), padding -inf, of fp32 x [B, C, H, W] at
 * element strides -> the pooled map channels-last in fp32, y32 [B, Ho, Wo, C], and / or in split form, ys [B, Ho, Wo, 2C]
 * (hi at channel c, lo at C + c); Ho = (H - 1) / 2 + 1.  C % 8 == 0, outputs 16-byte aligned, either may be null. */
int mf_maxpool3s2_split_fwd(const float *x, int64_t sb, int64_t sc, int64_t sh, int64_t sw, int32_t B, int32_t C,
                            int32_t H, int32_t W, float *y32, void *ys, mfStream_t stream);
int mf_upsample_bilinear_cl_bwd(const void *gy, void *gx, int32_t B, int32_t H, int32_t W, int32_t Ho, int32_t Wo,
                                int32_t C, int32_t bf16, mfStream_t stream);
/* ... and for channels-first tensors [B*C, H, W] (one lane per element) */
int mf_upsample_bilinear_cf_fwd(const void *x, void *y, int64_t BC, int32_t H, int32_t W, int32_t Ho, int32_t Wo,
                                int32_t bf16, mfStream_t stream);
int mf_upsample_bilinear_cf_bwd(const void *gy, void *gx, int64_t BC, int32_t H, int32_t W, int32_t Ho, int32_t Wo,
                                int32_t bf16, mfStream_t stream);
int mf_prelu_fwd(const void *x, const float *slope, void *y, int64_t n, int32_t bf16, mfStream_t stream);
/* ResNet18Extractor's input normalisation (models/resnet.py:33-36): (rgb / 255 - mean) / std on a [B, H, W, 3] image,
 * uint8 (u8 = 1) or float32 -> float32 [B, H, W, 3]; mean3 / std3 are HOST arrays of three floats. */
int mf_rgb_normalize(const void *rgb, int32_t u8, const float *mean3, const float *std3, float *out, int64_t npix,
                     mfStream_t stream);
/* BatchNorm with inference statistics (+ residual add) (+ ReLU) in one launch (models/resnet.py:44: ResNet18Extractor's
 * BatchNorm never updates): y = relu?((x - mean) * (weight / sqrt(var + eps)) + bias (+ identity)) over a dense
 * [B, C, H, W] tensor, NCHW (8 | H W) or channels-last (8 | C); fp32 / bf16 activations, fp32 parameters. */
int mf_bn_act_fwd(const void *x, const void *identity, const float *mean, const float *var, const float *weight,
                  const float *bias, float eps, void *y, int64_t n, int32_t C, int64_t HW, int32_t channels_last,
                  int32_t relu, int32_t bf16, mfStream_t stream);
/* Which kernel the most recent mf_upsample_bilinear_cl_bwd / mf_bn_act_fwd launch of this process took (a host-side
 * integer, 0 before the first launch; a refused call leaves it alone):
 *   resize backward  1 direct gather (k_up_bwd)   2 LDS tile (k_up_bwd_tile_bf16)   3 small input map (k_up_bwd_small)
 *   BatchNorm        16 generic (k_bn_act, either layout)   32 + ppt per channel group (k_bn_act_cl, ppt = 1 / 2 / 4) */
int mf_backbone2d_last_path(void);
int64_t mf_prelu_bwd_workspace_floats(int64_t n);
int mf_prelu_bwd(const void *x, const void *dy, const float *slope, void *dx, float *dslope, float *ws, int64_t n,
                 int32_t bf16, mfStream_t stream);

/* Point-wise prologue / epilogue of the volumetric part (inference), one launch each instead of ~25 torch launches:
 *   mf_point_prep: camera-frame points [B,3,P] + image features [B,Cv,P] -> voxel-frame points [n,3]
 *     ((p - origin) / pitch, model.py:236), to_center [n,4] = (center - p | 0) (:101), feature rows [n,Cv],
 *     batch indices [n];  n = B*P, Cv % 4 == 0.
 *   mf_pose_epilogue: heads' output rows [n, ldo] (rot at column 0, trans at np4, conf at 2*np4; class c at
 *     4c / 3c / c) -> rot [n,4] = q / (|q| + 1e-5) (chainer F.normalize), trans [n,3] = (p*pitch + origin) +
 *     t*pitch (:264-266), conf [n] = sigmoid (:262) of each object's class (class_id int64 [B], 1-based; an id
 *     outside 1 .. n_fg gives NaN outputs, never a read outside the row). */
/* Tile height (64 / 128 / 256 rows) the bf16 NT engine used for its most recent launch in this process (the
 * 256 x 256 form -- eight waves of 128 x 64 -- takes problems with >= 224 such tiles; MF_NT_BIG = 0 / 2 in the
 * environment forces never / wherever possible). */
int mf_gemm_bf16_last_tile(void);

/* The launch plans of the bf16 GEMM engines, answered by the very functions the launchers use (csrc/gemm_bf16.hip:
 * nt_plan / tn_plan): host arithmetic over the problem and the MF_NT_BIG / MF_NT_SPLITK / MF_TN_PP / MF_NT_HALF_MAX
 * knobs (read from the environment at every call), no device call.  Both return 0, or a negative code for a malformed
 * question.
 *   mf_gemm_bf16_nt_plan: C [M][N] per group over K.  ``mode`` 0 rows (mf_linear_bf16), 1 conv forward, 2 the k4 / s2
 *     data gradient, 3 / 4 / 5 the split-bf16 2-D conv / 3-D conv / rows; ``table``: the rows come with a group table
 *     (mf_linear_bf16_tiles); ``dgrad_rows``: (D/2)^3 of the data gradient, 0 otherwise; ``may_split``: the entry point
 *     can split K (mf_conv3d_bf16_fwd_ws and the *_split_fwd) and ``have_ws``: it was given a workspace.
 *     -> *tile = 64 / 128 / 256 rows, *S = splits of K (the *_workspace_bytes functions answer S * M * N * 4, 0 at S = 1).
 *   mf_gemm_bf16_tn_plan: a weight gradient [Ni][Nj] at row pitch ldc, reduced over ``rows`` rows, ``groups`` side by
 *     side; ``ranges``: mf_linear_wgrad_bf16_ranges; ``conv``: mf_conv3d_bf16_wgrad; ``split``: the caller's, <= 0 =
 *     the default.  -> *form = 128 (the 128 x 128 tile) / 256 (the ping-pong form), *default_split = what
 *     mf_*_wgrad_default_split answer, *finish = the pass that adds the slabs: 0 none, 1 k_wgrad_finish,
 *     2 k_wgrad_finish_deep, 3 k_wgrad_finish_conv. */
int mf_gemm_bf16_nt_plan(int32_t mode, int64_t M, int32_t N, int32_t K, int32_t groups, int32_t table,
                         int64_t dgrad_rows, int32_t may_split, int32_t have_ws, int32_t *tile, int32_t *S);
int mf_gemm_bf16_tn_plan(int32_t Ni, int32_t Nj, int32_t ldc, int64_t rows, int32_t groups, int32_t ranges,
                         int32_t conv, int32_t split, int32_t *form, int32_t *default_split, int32_t *finish);

/* PSPNet's sampled tail under bf16 training (pspnet.py:18-22,50-56 at model.py:222's pixels): the 3 x 3 windows of
 * the virtually x2 up-sampled map as GEMM rows [B * P, 576] bf16 (column c * 9 + ky * 3 + kx) from the channels-last
 * bf16 map u2 [B, H, W, 64], pix [B * P] flat indices into [2H, 2W]; and the backward: grows -> gu2 [B, H, W, 64] bf16
 * through the fp32 workspace acc [B, H, W, 64] (zeroed by the call; fp32 atomics). */
int mf_psp_tail_rows_bf16_fwd(const void *u2, const int64_t *pix, int32_t B, int32_t P, int32_t H, int32_t W, void *rows,
                              mfStream_t stream);
int mf_psp_tail_rows_bf16_bwd(const void *grows, const int64_t *pix, int32_t B, int32_t P, int32_t H, int32_t W,
                              float *acc, void *gu2, mfStream_t stream);

/* The confidence terms of the pose loss and their reduction (contrib/singleview_3d/models/model.py:417-434):
 * loss[0] = mean over objects of the mean over confident points (conf > 0) of add * conf - lambda * log(conf);
 * cnt [B] is kept for the backward (dadd, dconf [B, P] from the scalar gradient gloss[0]).  An object without a
 * confident point has cnt = 0 and the value 0 / 0 = NaN, which makes loss[0] NaN; its dadd / dconf rows are zeros (as
 * is every entry with conf <= 0) and the other objects' gradients stay finite.  _fwd with B outside 1 .. 8192 or
 * P < 1 returns -hipErrorInvalidValue (-1) before any launch and writes nothing; _bwd with B < 1 or P < 1 returns 0. */
int mf_confidence_loss_fwd(const float *add, const float *conf, int32_t B, int32_t P, float lambda, float *loss,
                           int32_t *cnt, mfStream_t stream);
int mf_confidence_loss_bwd(const float *add, const float *conf, const int32_t *cnt, const float *gloss, int32_t B,
                           int32_t P, float lambda, float *dadd, float *dconf, mfStream_t stream);

/* Pose epilogue of the TRAINING path (model.py:262-273: class selection, F.normalize, translation, sigmoid) on the
 * three heads' fp32 outputs orot [n, 4 n_fg], otrn [n, 3 n_fg], ocnf [n, n_fg]; the backward writes the three gradient
 * row blocks completely.  One launch each (torch: ~27 / ~47 incl. three index_put sorts).  rot = x / (|x| + 1e-5)
 * (an all-zero quaternion row gives zeros forward and g / 1e-5 backward).  An object whose class_id is outside
 * 1 .. n_fg has no head: its rot / trans / conf are NaN and its gradient rows are zeros, whatever the cotangents. */
int mf_pose_epilogue_train_fwd(const float *orot, const float *otrn, const float *ocnf, const int64_t *class_id,
                               const float *pts, const float *origin, const float *pitch, int32_t B, int32_t P,
                               int32_t n_fg, float *rot, float *trans, float *conf, mfStream_t stream);
int mf_pose_epilogue_train_bwd(const float *orot, const float *ocnf, const int64_t *class_id, const float *pitch,
                               const float *grot, const float *gtrans, const float *gconf, int32_t B, int32_t P,
                               int32_t n_fg, float *drot, float *dtrn, float *dcnf, mfStream_t stream);
/* transformation_matrix of a batch of poses and its backward (functions/geometry/transformation_matrix.py:5-18 =
 * quaternion_matrix.py:36-78 + compose_transform.py:5-48): T [n,4,4] row-major from q [n,4] (wxyz, any norm), t [n,3];
 * gq [n,4], gt [n,3] from gT [n,4,4].  One launch each (the torch composite: ~25 / ~60). */
int mf_transformation_matrix_fwd(const float *q, const float *t, int64_t n, float *T, mfStream_t stream);
int mf_transformation_matrix_bwd(const float *q, const float *gT, int64_t n, float *gq, float *gt, mfStream_t stream);
int mf_point_prep(const float *points_cam, const float *values, const float *origin, const float *pitch,
                  int32_t B, int32_t P, int32_t Cv, float center, float *pts, float *tc4, float *x_rows,
                  int32_t *batch_indices, mfStream_t stream);
int mf_pose_epilogue(const float *heads_out, int64_t ldo, int32_t np4, const int64_t *class_id,
                     const float *pts, const float *origin, const float *pitch, int32_t B, int32_t P, int32_t n_fg,
                     float *rot, float *trans, float *conf, mfStream_t stream);

/* ---- point-cloud baseline network (contrib/singleview_pcd, csrc/pcdnet.hip; DESIGN.md "Point-cloud baseline network")
 * Inference of examples/ycb_video/singleview_pcd/contrib/models/model.py:69-155,299-330 on rows m = b * P + p.  The GEMM
 * layers run on mf_linear_split_fwd / mf_linear_fwd, the pose epilogue on mf_pose_epilogue (pts = p - center, origin =
 * center, pitch = 1: ((p - c) + c) + t); these are the point-wise kernels in between.  None allocates or synchronises;
 * each returns a negative code without launching for B <= 0, P <= 0, B * P > INT32_MAX or a misaligned pitch.
 *   mf_pcdnet_workspace_offsets  byte offsets of the MF_PCDNET_WS_BUFFERS activation buffers in one workspace (256-byte
 *       aligned; offsets[MF_PCDNET_WS_BUFFERS] = the total), in the order pts fp32 [M][3], f1 bf16 [M][256], xs bf16
 *       [M][768], h3 bf16 [M][1024], h4 fp32 [M][1024], pooled fp32 [B][1024], gbias fp32 [B][1920], y fp32 [M][1920],
 *       h1 bf16 [M][3840], h2 bf16 [M][1536], h3h bf16 [M][768], o fp32 [M][3 np4] with np4 = 4 n_fg rounded up to 8;
 *       returns the number of buffers, or -1 (also for n_fg outside 1 .. MF_PCDNET_MAX_FG)
 *   mf_pcdnet_workspace_bytes    that total, or -1
 *   mf_pcdnet_stem   x_rows fp32 [M][32] (the PSPNet tail's rows), pcd fp32 [B][HW][3], pix int64 [M] flat pixel of each
 *       row, center fp32 [B][3] or null -> pts fp32 [M][3] = p - center (p without a center), feat1 = relu(conv1_rgb |
 *       conv1_pcd) in split form: f1 rows of pitch ld1 (rgb hi at 0, lo at 64, pcd hi at 128, lo at 192) and xs rows of
 *       pitch ldx (channel c hi at c, lo at losx + c; c < 64 rgb, 64 .. 127 pcd).  w_rgb [64][32], w_pcd [64][3].
 *   mf_pcdnet_pool   pooled [B][C] = mean over the P rows of each object of h fp32 (row pitch ldh), C % 64 == 0, in a
 *       fixed order (no atomics)
 *   mf_pcdnet_bias_relu_split  out[m][2 G g + j] = hi, out[m][2 G g + G + j] = lo of relu(y[m][G g + j] +
 *       gbias[m / P][G g + j]); y fp32 row pitch ldy, gbias [B][N], out bf16 row pitch ldo >= 2 N; G % 8 == 0, G | N */
#define MF_PCDNET_WS_BUFFERS 12
#define MF_PCDNET_MAX_FG 256
int32_t mf_pcdnet_workspace_offsets(int32_t B, int32_t P, int32_t n_fg, int64_t *offsets);
int64_t mf_pcdnet_workspace_bytes(int32_t B, int32_t P, int32_t n_fg);
int mf_pcdnet_stem(const float *x_rows, const float *pcd, const int64_t *pix, const float *center, const float *w_rgb,
                   const float *b_rgb, const float *w_pcd, const float *b_pcd, int32_t B, int32_t P, int32_t HW,
                   float *pts, void *f1, int32_t ld1, void *xs, int32_t ldx, int32_t losx, mfStream_t stream);
int mf_pcdnet_pool(const float *h, int64_t ldh, int32_t B, int32_t P, int32_t C, float *pooled, mfStream_t stream);
int mf_pcdnet_bias_relu_split(const float *y, int64_t ldy, const float *gbias, int32_t B, int32_t P, int32_t N, int32_t G,
                              void *out, int64_t ldo, mfStream_t stream);

/* The last PSPNet level (up3: bilinear x2 + Convolution2D 3x3 64->64 + PReLU; conv1 1x1 64->32; log-softmax,
 *   morefusion/models/dense_fusion/pspnet.py:10-35,57-73) evaluated ONLY at the sampled pixels the pose network
 *   reads (contrib/singleview_3d/models/model.py:222), one launch:
 *   u2 [B,64,H,W] with element strides (sb, sc, sy, sx) (NCHW or channels-last), pix [B*P] int64 flat indices into
 *   the [2H,2W] full-resolution map, w3t [9,64,64] = W3.permute(2,3,1,0), w1t [64,32] = W1[:, :, 0, 0].T,
 *   prelu_slope: device pointer to the single PReLU parameter -> out [B*P, 32] (rows). */
int mf_psp_tail_fwd(const float *u2, int64_t sb, int64_t sc, int64_t sy, int64_t sx, const int64_t *pix,
                    const float *w3t, const float *b3, const float *prelu_slope, const float *w1t,
                    const float *b1, int32_t B, int32_t P, int32_t H, int32_t W, float *out, mfStream_t stream);

/* small fused helpers of the same path */
/* pack [Ptot,3] points + [Ptot] sdf into float4 */
int mf_pack_points_sdf(const float *points, const float *sdf, int64_t n, void *pts4,
                       mfStream_t stream);

/* ---- pre-processing in front of the network ------------------
 * replaces the per-instance host loop (NumPy + imgviz/cv2) at
 *   ros/src/morefusion_ros/nodes/singleview_3d_pose_estimation.py:116-176
 *   morefusion/datasets/rgbd_pose_estimation/base.py:112-137
 * incl. geometry/pointcloud_from_depth.py:4-26 and geometry/masks_to_bboxes.py:4-38.
 *   label [H,W] int32 instance image, depth [H,W] float32 metres (NaN = invalid),
 *   rgb [H,W,3] uint8, instance_ids [n] (n <= 256).
 * mf_instance_stats: stats [n,6] = {y1, x1, y2, x2 (end-exclusive box of label == id),
 *   mask pixels, mask pixels with valid depth}; a mask without pixels leaves
 *   {INT_MAX, INT_MAX, 0, 0, 0, 0}.
 * mf_instance_crops: per instance the masked crop centerized to S x S:
 *   rgb_out [n,S,S,3] uint8 (0 outside the mask / padding; 8-bit bilinear resize),
 *   pcd_out [n,S,S,3] float32 camera-frame points (NaN outside the mask / padding / invalid
 *   depth; nearest-neighbour resize; back-projection in float64), keep [n] uint8 = mask is
 *   non-empty and has >= min_valid valid points (the reference skips the others; here
 *   their outputs are all padding).  Both calls are asynchronous and never synchronise. */
int mf_instance_stats(const int32_t *label, const float *depth, int H, int W,
                      const int32_t *instance_ids, int n_inst, int32_t *stats,
                      mfStream_t stream);
int mf_instance_crops(const uint8_t *rgb, const float *depth, const int32_t *label, int H,
                      int W, double fx, double fy, double cx, double cy,
                      const int32_t *instance_ids, const int32_t *stats, int n_inst, int S,
                      int min_valid, uint8_t *rgb_out, float *pcd_out, uint8_t *keep,
                      mfStream_t stream);

/* valid-pixel list in front of Model.predict's point selection: replaces, per object,
 *   contrib/singleview_3d/models/model.py:195-196 `iy, ix = xp.where(mask[i])` and :206
 *   `n_point = int(mask[i].sum())` with mask = ~isnan(pcd).any(channel).
 * pcd [B,HW,3] float32 -> order [B,HW] int32: the row-major
 * pixel indices h*W+w of the pixels without a NaN coordinate, in increasing order (entries beyond
 * counts[b] are left untouched), counts [B] int32.  The reference's NumPy-RNG subsample
 * (`keep`, :207-219) then indexes this list.  Asynchronous, never synchronises. */
int mf_valid_pixel_order(const float *pcd, int32_t B, int32_t HW, int32_t *order, int32_t *counts,
                         mfStream_t stream);

/* ---- occupancy mapping (contrib/multi_instance_octree_mapping.py, csrc/occmap.hip) ---------
 * The reference's per-instance OctoMap (contrib.MultiInstanceOctreeMapping) as one dense float32
 * log-odds volume per instance over a box of octree keys (key = floor(double(c) / pitch) + 32768
 * per axis, c rounded to float32 first); NaN = never touched (unknown).  cell (kx, ky, kz) is
 * element ((kx - lo[0]) * dim[1] + ky - lo[1]) * dim[2] + kz - lo[2] of `logodds`; `bits`
 * [2 * cells] uint32 holds the per-scan free / occupied bits (or the hit counts of an update)
 * between a ray-cast and the apply pass and is all-zero otherwise.
 * `slots` [n_slots, 3] int32 = {label value, tree index, scan index (0..31)}: a point whose label
 * matches a slot's value is one measurement of that tree's scan.  `trees` is a DEVICE array of
 * mfOccTree; `pts` [n, 3] float32 (NaN rows are skipped), one sensor origin per launch.
 * Every call is asynchronous, allocates nothing and never synchronises. */
typedef struct {
  float *logodds;
  uint32_t *bits;
  int32_t lo[3];
  int32_t dim[3];
  double resolution;
  double res_factor; /* 1.0 / resolution */
} mfOccTree;
/* dst (HOST pointer to the descriptor) := src where the boxes overlap, NaN elsewhere; dst bits := 0.
 * src may be NULL (a fresh box); src and dst must not alias. */
int mf_occmap_regrid(const mfOccTree *src, const mfOccTree *dst, mfStream_t stream);
/* bounds [n_trees, 6] int32 := per tree {min key x,y,z, max key x,y,z} over its measured points
 * ({INT_MAX x3, INT_MIN x3} for a tree without points); n_trees <= 256. */
int mf_occmap_bounds(const float *pts, const int32_t *label, int64_t n, const int32_t *slots,
                     int32_t n_slots, const mfOccTree *trees, int32_t n_trees, int32_t *bounds,
                     mfStream_t stream);
/* octomap's insertPointCloud ray-cast: per point the DDA keys origin -> point set bit `scan` in
 * the free word, the end key in the occupied word.  Keys outside a tree's box are dropped and
 * counted in *overflow (may be NULL; the caller sizes the boxes so that this stays 0). */
int mf_occmap_raycast(const float *pts, const int32_t *label, int64_t n, const int32_t *slots,
                      int32_t n_slots, const mfOccTree *trees, float origin_x, float origin_y,
                      float origin_z, int32_t *overflow, mfStream_t stream);
/* update(): one hit per point of tree `tree` (no merging of duplicates): integer counts in the
 * free word.  Keys outside the box are counted in *overflow (may be NULL). */
int mf_occmap_count_hits(const float *pts, int64_t n, const mfOccTree *trees, int32_t tree,
                         int32_t *overflow, mfStream_t stream);
/* One lane per cell of every tree: mode 0 applies the scans in order (occupied bit -> hit, else
 * free bit -> miss), mode 1 applies the hit counts; float32 adds with octomap's clamping, then
 * the bits are cleared.  max_cells = the largest tree's cell count. */
int mf_occmap_apply(const mfOccTree *trees, int32_t n_trees, int64_t max_cells, int32_t mode,
                    mfStream_t stream);
/* get_target_grids for B grids of D0 x D1 x D2 voxels: voxel centre origin[b] + i * pitch[b]
 * (float64, then float32), trees visited in index order, occupancy 1 - 1 / (1 + exp(l)) in float64;
 * grid_target / grid_nontarget / grid_empty [B, D0, D1, D2] float32 (last writer wins).
 * target_tree [B] int32 (-1: none).  net_target / net_nte [B, D0, D1, D2] uint8 (both NULL or
 * both set): grids_for_network(train=False) of the three grids. */
int mf_occmap_extract(const mfOccTree *trees, int32_t n_trees, const int32_t *target_tree,
                      const double *pitch, const double *origin, int32_t B, int32_t D0, int32_t D1,
                      int32_t D2, float *grid_target, float *grid_nontarget, float *grid_empty,
                      uint8_t *net_target, uint8_t *net_nte, mfStream_t stream);

/* ---- instance tracking across frames (contrib/instance_tracking.py, csrc/occtrack.hip) -------
 * The per-frame loop of the reference's map server: render the instance maps (mfOccTree boxes)
 * into the current camera, match the detector's ids against the rendering, clean both label
 * images and merge them (DESIGN.md "Instance tracking").  Label images are [H, W] int32: >= 0 an
 * instance id, -1 background, -2 uncertain.  `ref_ids` / `det_ids`: the ids the host knows may
 * occur in the rendered / detected image, each ASCENDING and without repeats (<= 1024).
 * Every call is asynchronous, allocates nothing and never synchronises; all results are bitwise
 * independent of the order in which lanes run. */
/* Host-only: bytes of `workspace` (16-byte aligned) shared by render, clean and merge; < 0: bad size. */
int64_t mf_occtrack_workspace_bytes(int32_t H, int32_t W, int32_t n_ref);
/* Host-only: int32 elements of `stats` for mf_occtrack_overlap / mf_occtrack_assign: inter
 * [n_ref, n_det], per reference id {area, edge, non-edge}, per detection {area, edge, non-edge},
 * per detection {min row, min col, max row, max col} ({INT_MAX x2, INT_MIN x2} when absent). */
int64_t mf_occtrack_stats_elems(int32_t n_ref, int32_t n_det);
/* out [n, 3] := T [4, 4] (row-major float32, DEVICE) applied to pts [n, 3] in float32:
 * ((T0 x + T1 y) + T2 z) + T3 per row, no contraction; NaN rows stay NaN. */
int mf_occtrack_transform(const float *pts, const float *T, int64_t n, float *out, mfStream_t stream);
/* castRay of every stride-2 pixel into every listed tree: pts [H * W, 3] in the map frame (NaN
 * rows: the ray through the pixel at z = 1, from K [3, 3] and sensor->map T [4, 4], both DEVICE
 * float32); slots [n_slots, 2] int32 = {tree index, instance id}.  The nearest hit wins, an exact
 * tie goes to the earlier slot.  label_rendered [H, W] (-2: no hit; the winner of pixel (j, i)
 * covers rows j-1..j, columns i-1..i); depth_rendered [H, W] float32: the winner's distance at
 * the stride-2 pixels, NaN elsewhere. */
int mf_occtrack_render(const float *pts, const float *K, const float *T, float origin_x, float origin_y,
                       float origin_z, const mfOccTree *trees, const int32_t *slots, int32_t n_slots,
                       int32_t H, int32_t W, void *workspace, int32_t *label_rendered,
                       float *depth_rendered, mfStream_t stream);
/* One pass over both images -> stats (layout above).  The edge band is the complement of the
 * rectangle (int(0.1 W), int(0.1 H)) .. (int(0.9 W), int(0.9 H)), corners included. */
int mf_occtrack_overlap(const int32_t *label_rendered, const int32_t *label_detected, int32_t H, int32_t W,
                        const int32_t *ref_ids, int32_t n_ref, const int32_t *det_ids, int32_t n_det,
                        int32_t *stats, mfStream_t stream);
/* remap [n_det + 1] := the tracked id of every detection (-2: suspicious; a new id from *counter
 * where IoU < iou_threshold and coverage < coverage_threshold), remap[n_det] := the updated
 * counter, also stored to *counter (the float32 quotients are compared in double, as the
 * reference compares them with its double literals).  suspicious_ref [n_ref] := edge > non-edge; suspicious_det
 * [n_det] := 1 (edge rule) | 2 (size rule: area < min_mask^2, box area < min_bbox^2 or a box
 * side < min_side). */
int mf_occtrack_assign(const int32_t *stats, const int32_t *ref_ids, int32_t n_ref, int32_t n_det, int32_t H,
                       int32_t W, int32_t min_mask, int32_t min_bbox, int32_t min_side, double iou_threshold,
                       double coverage_threshold, int32_t *counter, int32_t *remap, int32_t *suspicious_ref,
                       int32_t *suspicious_det, mfStream_t stream);
/* label_tracked := remap applied to label_detected (negative pixels in the edge band and
 * suspicious ids -> -2); label_reference := label_rendered with suspicious reference ids -> -2. */
int mf_occtrack_relabel(const int32_t *label_rendered, const int32_t *label_detected, int32_t H, int32_t W,
                        const int32_t *ref_ids, int32_t n_ref, const int32_t *det_ids, int32_t n_det,
                        const int32_t *remap, const int32_t *suspicious_ref, int32_t *label_tracked,
                        int32_t *label_reference, mfStream_t stream);
/* label_out := label with every 8-connected component (of equal values >= 0) below min_area
 * pixels set to -2, then every pixel whose (2 band + 1)^2 window holds two different values or
 * leaves the image set to -2.  label_out must not alias label. */
int mf_occtrack_clean(const int32_t *label, int32_t H, int32_t W, int32_t min_area, int32_t band,
                      void *workspace, int32_t *label_out, mfStream_t stream);
/* label_merged := -2, then for each id >= 0 of label_reference in ascending order the mask of
 * that id in label_tracked if it occurs there, else its mask in label_reference. */
int mf_occtrack_merge(const int32_t *label_reference, const int32_t *label_tracked, int32_t H, int32_t W,
                      const int32_t *ref_ids, int32_t n_ref, void *workspace, int32_t *label_merged,
                      mfStream_t stream);

/* ---- map server: insert and grid publication (contrib/octomap_server.py, csrc/occserver.hip) --
 * OctomapServer::insertScan / publishGrids of the reference's ROS node over the mfOccTree boxes
 * (DESIGN.md "Map server").  Only the stride-2 pixels (even row and even column) of the [H, W]
 * frame with a non-NaN point take part.  `slots` [n_slots, 3] int32 = {label value, tree index,
 * unused}: the tree that takes a label's end points (the background's label -1 included);
 * `bg_tree`: the tree that takes the frame's one free set.  Labels: >= 0 an instance id, -1
 * background, -2 uncertain (its rays still free the background).  Every call is asynchronous,
 * allocates nothing and never synchronises; no float atomics, all results are bitwise independent
 * of the order in which lanes run. */
/* bounds [n_trees, 6] int32 := per tree {min key x,y,z, max key x,y,z}: bg_tree over every valid
 * point whatever its label, any other tree over the points of its own label ({INT_MAX x3,
 * INT_MIN x3} without points); 1 <= n_trees <= 256. */
int mf_occserver_bounds(const float *pts, const int32_t *label, int32_t H, int32_t W, const int32_t *slots,
                        int32_t n_slots, const mfOccTree *trees, int32_t bg_tree, int32_t n_trees,
                        int32_t *bounds, mfStream_t stream);
/* table [n_slots + 1, 10] float64: per slot, over its label's valid stride-2 points without the
 * one of the smallest pixel index, {count, centroid x,y,z, min x,y,z, max x,y,z} (all zero when
 * count == 0).  Min / max are exact float32 values.  The centroid is float32(sum / count) of
 * float64 sums taken in one fixed order: lane t of 1024 adds its stride-2 pixels t, t + 1024, ...
 * in ascending order, then lanes fold pairwise (t += t + off, off = 512 .. 1).  Row n_slots,
 * column 0: the smallest label >= 0 of the whole image that has no slot, or -1. */
int mf_occserver_stats(const float *pts, const int32_t *label, int32_t H, int32_t W, const int32_t *slots,
                       int32_t n_slots, double *table, mfStream_t stream);
/* Per valid stride-2 pixel: the computeRayKeys DDA origin -> point sets bit 0 of the free word in
 * bg_tree; a label != -2 with a slot sets bit 0 of the occupied word at the end key of its tree;
 * a label != -1 sets the free bit of bg_tree at the end key.  Keys outside a box are dropped and
 * counted in *overflow (may be NULL). */
int mf_occserver_raycast(const float *pts, const int32_t *label, int32_t H, int32_t W, const int32_t *slots,
                         int32_t n_slots, const mfOccTree *trees, int32_t bg_tree, float origin_x,
                         float origin_y, float origin_z, int32_t *overflow, mfStream_t stream);
/* One lane per cell of every tree: occupied bit -> l + hit, else free bit -> l + miss (float32,
 * unknown cells start at 0), clamped to [lo_min, lo_max]; then the bits are cleared. */
int mf_occserver_apply(const mfOccTree *trees, int32_t n_trees, int64_t max_cells, float hit, float miss,
                       float lo_min, float lo_max, mfStream_t stream);
/* publishGrids for B grids of D^3 voxels in the SENSOR frame.  Per grid: centre = T_map_to_sensor
 * applied to center_map[b] (float32, ((T0 x + T1 y) + T2 z) + T3, no contraction); origin[b] :=
 * double(centre) - (D / 2.0 - 0.5) * double(pitch[b]); voxel centre = float32(origin + double(
 * pitch[b] * float(i))) per axis, moved to the map frame by T_sensor_to_map (same convention) and
 * searched as a float32 point.  flags & 1: map z < 0 -> noentry = float32(prob_max) and nothing
 * else.  Own tree (target_tree[b]) known with occupancy > 0.5 -> grid_target = float32(occupancy);
 * otherwise every other tree of `order` [n_trees] (tree indices in ascending instance id) that is
 * known: bg_tree with flags & 2 and occupancy < 0.5 -> noentry = float32(1 - occupancy), else
 * occupancy >= prob_max (in double) -> noentry = float32(occupancy); the last writer wins.
 * grid_nontarget_empty (uint8) := noentry != 0.  Both T are row-major [4, 4] float32, DEVICE. */
int mf_occserver_publish(const mfOccTree *trees, int32_t n_trees, const int32_t *order, int32_t bg_tree,
                         const int32_t *target_tree, const float *pitch, const float *center_map,
                         const float *T_map_to_sensor, const float *T_sensor_to_map, double prob_max,
                         int32_t flags, int32_t B, int32_t D, double *origin, float *grid_target,
                         float *grid_noentry, uint8_t *grid_nontarget_empty, mfStream_t stream);

/* ---- point-to-point ICP registration (contrib/icp_registration.py, csrc/icpreg.hip) ---------
 * open3d's voxel_down_sample + registration_icp(PointToPoint, no scaling), restated in float64
 * (DESIGN.md "ICP registration").  Point sets are packed double [n, 3] rows with int64 [n_sets + 1]
 * row offsets; rows with a NaN coordinate are dropped.  Every call is asynchronous, allocates
 * nothing and never synchronises. */
#define MF_ICPREG_MAX_CELLS (1 << 24) /* voxel-box cells (and grid cells) of one prepare call */
/* Host-only: bytes of `workspace` for mf_icpreg_prepare; < 0 past MF_ICPREG_MAX_CELLS. */
int64_t mf_icpreg_workspace_bytes(int64_t total_cells, int64_t total_grid, int64_t n_points);
/* Per set: vmin [n_sets, 3] = min of the valid rows - voxel_size / 2; ext [n_sets, 4] int32 =
 * {nx, ny, nz, n_valid}, nx = floor((max - vmin) / voxel_size) + 1 (-1: too large; all 0 for a set
 * without valid rows).  The caller reads ext back to size the boxes. */
int mf_icpreg_bounds(const double *pts, const int64_t *off, int32_t n_sets, double voxel_size,
                     double *vmin, int32_t *ext, mfStream_t stream);
/* voxel_down_sample of every set: out (packed like pts) rows off[b] .. off[b] + out_cnt[b] are the
 * voxel means (input-order float64 sums / count) in (i, j, k) lexicographic voxel order.
 * box_off [n_sets + 1] int64 = prefix of nx * ny * nz (total_cells).  A set b with grid_off[b + 1] >
 * grid_off[b] is also binned into a uniform grid of cell `cell`, dims grid_dim[b] (int32 [n_sets, 3]),
 * origin grid_origin[b] := vmin[b] - cell: grid_start[grid_off[b] ..] holds G + 1 starts into
 * grid_idx (rows relative to the set, at its rows off[b] ..), each cell's rows ascending. */
int mf_icpreg_prepare(const double *pts, const int64_t *off, int32_t n_sets, double voxel_size,
                      const double *vmin, const int32_t *ext, const int64_t *box_off,
                      int64_t total_cells, const int64_t *grid_off, const int32_t *grid_dim,
                      int64_t total_grid, double cell, int64_t n_points, void *workspace,
                      double *out, int32_t *out_cnt, double *grid_origin, int32_t *grid_start,
                      int32_t *grid_idx, mfStream_t stream);
/* One ICP problem per object (all DEVICE pointers).  Object b: source rows src_off[b] ..
 * + src_cnt[b] of src, target rows tgt_off[b] .. + tgt_cnt[b] of tgt with its grid at
 * grid_start + grid_off[b], grid_dim[b], grid_origin[b] (objects may share a target).
 * transform_init [B, 16] cad -> cam (row-major); active [B] uint8 (NULL: all).  cur [src rows, 3]
 * and corr [src rows] are workspace.  Outputs: transform [B, 16] (cad -> cam), transformation
 * [B, 16] (depth -> cad), fitness, inlier_rmse [B], n_iter [B]; optional history (all three or
 * none) [B, max_iter + 1, 16] / [B, max_iter + 1]: entry 0 = transform_init and the result there,
 * entry k = after update k, entries past n_iter repeat the last.  mode 0 = register (stop when
 * |d fitness| and |d rmse| < 1e-6), mode 1 = register_iterative (max_iter one-update steps). */
typedef struct {
  const double *src;
  const int64_t *src_off;
  const int32_t *src_cnt;
  const double *tgt;
  const int64_t *tgt_off;
  const int32_t *tgt_cnt;
  const int64_t *grid_off;
  const int32_t *grid_dim;
  const double *grid_origin;
  const int32_t *grid_start;
  const int32_t *grid_idx;
  const double *transform_init;
  const uint8_t *active;
  double *cur;
  int32_t *corr;
  double *transform;
  double *transformation;
  double *fitness;
  double *inlier_rmse;
  int32_t *n_iter;
  double *hist_transform;
  double *hist_fitness;
  double *hist_rmse;
  double max_corr_dist;
  double cell;
  int32_t n_objects;
  int32_t max_iter;
  int32_t mode;
  int32_t reserved;
} mfIcpRegBatch;
int mf_icpreg_run(const mfIcpRegBatch *batch, mfStream_t stream);

/* ---- mesh signed distance / solid voxelization (geometry/mesh_sdf.py, csrc/meshsdf.hip) -------
 * M triangle meshes and one segment of queries per mesh, float64 throughout (DESIGN.md "CAD model
 * preparation").  Per query: unsigned distance to the nearest face (Ericson's closest point), the
 * arg-min face (lowest index on a tie), the generalized winding number w (Van Oosterom-Strackee solid
 * angles summed in face-index order / 4 pi) and sdf = +d inside, -d outside, inside := w >= 0.5 or
 * d <= 1e-8.  Every call is asynchronous, allocates nothing and never synchronises. */
#define MF_MESHSDF_MAX_MESHES 65535
#define MF_MESHSDF_MAX_FACES (1LL << 26)
#define MF_MESHSDF_MAX_GRID_DIM 1024
typedef struct {
  const double *vertices;     /* packed [V, 3] */
  const int64_t *v_off;       /* [M + 1] vertex row offsets */
  const int32_t *faces;       /* packed [F, 3], indices local to the mesh (outside it: the face is skipped) */
  const int64_t *f_off;       /* [M + 1] face row offsets */
  double *face_rec;           /* workspace [F, 16]: written by mf_meshsdf_prepare, read by mf_meshsdf_query */
  const double *points;       /* packed [Q, 3] queries; NULL: grid queries (below) */
  const int64_t *q_off;       /* [M + 1] query offsets (grid queries: m * grid_dim^3) */
  const int32_t *blk_off;     /* [M + 1] workgroup offsets: blk_off[m + 1] - blk_off[m] = ceil(queries of m / 256) */
  const double *grid_origin;  /* [M, 3] grid queries: centre (i, j, k) = origin + (idx + 0.5) * grid_h[m] */
  const double *grid_h;       /* [M] cell size */
  double *dist;               /* [Q] outputs, each optional (NULL) */
  int32_t *face;
  double *winding;
  double *sdf;
  uint8_t *occupancy;         /* points: inside; grid: w >= 0.5 or d <= grid_h[m] / 2 */
  int32_t n_meshes;
  int32_t n_blocks;           /* blk_off[M] */
  int32_t grid_dim;           /* grid queries: cells per axis */
  int32_t reserved;
} mfMeshSdfBatch;
/* Host-only: bytes of face_rec for total_faces faces; < 0 past MF_MESHSDF_MAX_FACES. */
int64_t mf_meshsdf_workspace_bytes(int64_t total_faces);
/* Per-face records (vertices, edges, kind) of every mesh into face_rec; reads vertices, v_off, faces,
 * f_off (total_faces = f_off[M]). */
int mf_meshsdf_prepare(const mfMeshSdfBatch *batch, int64_t total_faces, mfStream_t stream);
/* One lane per query over every face of its mesh; face_rec as prepared. */
int mf_meshsdf_query(const mfMeshSdfBatch *batch, mfStream_t stream);

/* ---- depth / instance rasteriser and full grids (geometry/render.py, csrc/render.hip) ----------
 * One launch renders N items: item n = mesh item_mesh[n] at the float64 pose item_T[n] (cad -> camera,
 * row-major 4 x 4) into image item_target[n] with the instance id item_id[n].  Items of one target
 * occlude each other.  The arithmetic is DESIGN.md "Mesh rendering": float64 projection
 * u = fx x / z + cx, pixel (row i, col j) sampled at (u, v) = (j, i), float64 edge functions in a canonical
 * endpoint order with a top-left rule, both sides drawn, a face with a vertex at z <= near dropped whole,
 * depth = the face's plane along the pixel's ray rounded once to float32, winner = the minimum of
 * (depth bits, item, face) by a 64-bit atomic minimum: the result does not depend on the execution order.
 * Every call is asynchronous, allocates nothing and never synchronises. */
#define MF_RENDER_MAX_ITEMS 65535
#define MF_RENDER_MAX_FACES (1LL << 26) /* face records (faces summed over the items) per launch */
#define MF_RENDER_MAX_PIXELS (1LL << 28) /* n_targets * height * width */
#define MF_RENDER_MAX_SIDE 4096          /* height, width */
typedef struct {
  const double *vertices;      /* packed [V, 3] */
  const int64_t *v_off;        /* [M + 1] vertex row offsets */
  const int32_t *faces;        /* packed [F, 3], indices local to the mesh (outside it: the face is dropped) */
  const int64_t *f_off;        /* [M + 1] face row offsets */
  const int32_t *item_mesh;    /* [N] */
  const double *item_T;        /* [N, 16] */
  const int32_t *item_target;  /* [N] in [0, n_targets) */
  const int32_t *item_id;      /* [N] value written to `instance` */
  const int64_t *item_rec_off; /* [N + 1] record offsets: item n owns records item_rec_off[n] + (face of its mesh) */
  void *workspace;             /* mf_render_workspace_bytes, 16-byte aligned */
  float *depth;                /* [n_targets, height, width], NaN where nothing was hit */
  int32_t *instance;           /* [n_targets, height, width], -1 where nothing was hit */
  int32_t *face;               /* [n_targets, height, width] face of the winning item's mesh, -1 where nothing */
  int32_t *count;              /* [N] pixels each item won */
  double fx;
  double fy;
  double cx;
  double cy;
  double near;
  int32_t n_meshes;
  int32_t n_items;
  int32_t n_targets;
  int32_t height;
  int32_t width;
  int32_t reserved;
} mfRenderBatch;
/* Host-only: bytes of the workspace (z-buffer, face records, large-face list); < 0 past a cap above. */
int64_t mf_render_workspace_bytes(int64_t total_records, int64_t n_targets, int64_t height, int64_t width);
/* Clears the z-buffer and writes one record per (item, face): clipped bounding box, edges, plane; faces whose
 * box exceeds the small-face threshold are listed for the large pass.  total_records = item_rec_off[N]. */
int mf_render_setup(const mfRenderBatch *batch, int64_t total_records, mfStream_t stream);
/* Both raster passes: a lane per small face, a workgroup per (large face, 32 x 32 tile). */
int mf_render_raster(const mfRenderBatch *batch, int64_t total_records, mfStream_t stream);
/* z-buffer -> depth, instance, face and the per-item pixel counts. */
int mf_render_resolve(const mfRenderBatch *batch, int64_t total_records, mfStream_t stream);
/* grid_target_full / grid_nontarget_full of N examples in one launch (datasets/rgbd_pose_estimation/base.py
 * _get_grid_full): the points of example i (points[p_off[i] .. p_off[i + 1]), float64 [*, 3]) at T[i] into the
 * dim^3 grid of every example e: idx = rint((T_i p - origin_e) / pitch_e) kept inside [0, dim)^3;
 * target_full[e] = 1 from i = e, nontarget_full[e] = max over i != e of (position of i among the others) + 1.
 * Both outputs int32 [N, dim, dim, dim], cleared here; total_points = p_off[N]. */
int mf_full_grids(const double *points, const int64_t *p_off, const double *T, const double *pitch,
                  const double *origin, int32_t n_examples, int64_t total_points, int32_t dim,
                  int32_t *target_full, int32_t *nontarget_full, mfStream_t stream);

/* ---- picking order: occlusion counts, normals, grasp poses (contrib/picking_order.py, csrc/pickorder.hip) ----
 * What ros/src/morefusion_ros/nodes/select_picking_order.py measures on N + 1 renders, on the renderer's own
 * outputs: `instance` / `depth` [N + 1, height, width] with target 0 the composite of the N items and target 1 + n
 * item n alone, item_id[n] the value item n writes (distinct, >= 0).  DESIGN.md "Picking order".  Every call is
 * asynchronous, allocates nothing and never synchronises. */
#define MF_PICK_MAX_OBJECTS 64 /* items of one call: N + 1 targets of 4096 x 4096 still fit MF_RENDER_MAX_PIXELS */
/* whole[n]: pixels of item n alone.  occluded_by[i, j] ([N, N]): pixels that are i's alone and j's in the composite
 * (the diagonal: i's visible pixels; a row sums to whole[i]).  bbox[n] = (min_row, min_col, max_row + 1,
 * max_col + 1) of item n alone, zeros for no pixels.  All int32, cleared here. */
int mf_pick_occlusion(const int32_t *instance, const int32_t *item_id, int32_t n_items, int32_t height,
                      int32_t width, int32_t *whole, int32_t *occluded_by, int32_t *bbox, mfStream_t stream);
/* geometry/estimate_pointcloud_normals.py _estimate_pointcloud_normals_organized for n_images images of float64
 * points [n_images, height, width, 3], each inside its rectangle rect[t] = (y1, x1, y2, x2) (clipped to the image):
 * the neighbours at offset 2 outside the RECTANGLE are NaN, as the reference pads a crop.  normals (same shape) is
 * written completely, NaN outside the rectangle. */
int mf_pick_normals(const double *points, const int32_t *rect, int32_t n_images, int32_t height, int32_t width,
                    double *normals, mfStream_t stream);
/* get_grasp_pose per item, one workgroup each: the box is cut into cells of S x S pixels, S = max(1, isqrt((h w) /
 * 30)) (the seeding grid of the reference's SLIC, which is not run); cell[n] = the cell with mask pixels whose
 * centroid is nearest the mean of the centroids (first on a tie, -1: no pixels); translation[n] = mean of the
 * back-projected points (pointcloud_from_depth) over its mask pixels, normal[n] = mean of its normals (rectangle =
 * bbox[n]) that are not NaN, NaN if none.  float64 sums in the fixed order of csrc/pickorder.hip's header. */
int mf_pick_grasp(const float *depth, const int32_t *instance, const int32_t *item_id, const int32_t *bbox,
                  int32_t n_items, int32_t height, int32_t width, double fx, double fy, double cx, double cy,
                  int32_t *cell, double *translation, double *normal, mfStream_t stream);

/* ---- pose metric: batched ADD / ADD-S in float64 (metrics/average_distance_device.py, csrc/posemetric.hip) ----
 * metrics.average_distance (morefusion/metrics/average_distance.py) for n_items items in one call.  Item i is the
 * cloud item_cloud[i] (its points: points[cloud_off[c] .. cloud_off[c + 1]), float64 [*, 3], all clouds concatenated;
 * cloud_off int32 [n_clouds + 1]) under T1[i] and T2[i] (float64 [n_items, 4, 4], row-major):
 *   add[i] = mean_j |T1 p_j - T2 p_j|,   add_s[i] = mean_j min_k |T1 p_j - T2 p_k|   (exact brute force),
 * without the translations if `translate` is 0.  Items may share clouds; max_points is the longest cloud's length
 * (a host value: it sizes the grid and the workspace).  The arithmetic and the order of every sum are fixed (the
 * header of csrc/posemetric.hip, DESIGN.md "Pose metric"): a result depends on its own item alone.  An item whose
 * cloud index is out of range, or whose cloud is empty or longer than max_points, gets NaN and touches nothing.
 * Asynchronous on `stream`; allocates nothing and never synchronises.  < 0: n_items outside 0 .. 65535,
 * n_clouds < 1 or max_points < 1. */
/* Host-only: bytes of the workspace (the per-point distances of every item); < 0: bad sizes. */
int64_t mf_average_distance_f64_workspace_bytes(int32_t n_items, int32_t max_points);
int mf_average_distance_f64(const double *points, const int32_t *cloud_off, const int32_t *item_cloud,
                            const double *T1, const double *T2, int32_t n_clouds, int32_t n_items,
                            int32_t max_points, int32_t translate, double *add, double *add_s, void *workspace,
                            mfStream_t stream);

/* ---- training-time augmentation (datasets/augmentation.py, csrc/augment.hip) -----------------------
 * RGBDPoseEstimationDatasetReIndexedBase._augment_rgbd for n examples of S x S pixels (S a multiple of 8 in
 * 8..256) per call.  rgb uint8 [n, S, S, 3]; pcd float32 or float64 [n, S, S, 3] (pcd_is_f64), NaN invalid;
 * params float64 [n, 12], drawn on the host: cut case, cut uniform, blob-count uniform, contrast alpha, H, S, V
 * multipliers, blur sigma, resize scale, example key, 2 reserved.  Per-pixel / per-component words come from
 * Philox4x32-10 keyed by (seed & 0xffffffff, example key), counter (pixel, stream, 0, 0).  Outputs and workspace
 * are the caller's; nothing is allocated or synchronised.  DESIGN.md "Augmentation". */
/* Host-only: bytes of the workspace (16-byte aligned) of mf_augment_mask / mf_augment_rgb; < 0: bad size. */
int64_t mf_augment_workspace_bytes(int32_t n, int32_t S);
/* _augment_mask: valid mask -> one-sided cut -> 8-connected components (one workgroup per example, labels in
 * LDS) -> largest + the K = floor(u m) components with the smallest words -> crop to the kept mask's box and
 * imgviz.centerize back to S x S.  kept_mask uint8 [n, S, S] (before re-centring); stats int32 [n, 12]: final
 * box y1 x1 y2 x2, components m, drawn K, largest component's id, kept pixels, cut box y1 x1 y2 x2;
 * keep uint8 [n]: 0 = the mask was empty at some step and the outputs are pure padding.  labels / sizes
 * (int32 [n, S, S], may be NULL): every pixel's component id (its first pixel in raster order, -1 outside the cut
 * mask) and that component's pixel count. */
int mf_augment_mask(const uint8_t *rgb, const void *pcd, int32_t pcd_is_f64, const double *params,
                    int32_t n, int32_t S, int64_t seed, uint8_t *rgb_out, void *pcd_out,
                    uint8_t *kept_mask, int32_t *stats, uint8_t *keep, int32_t *labels, int32_t *sizes,
                    void *workspace, mfStream_t stream);
/* _augment_rgb: linear contrast, HSV multipliers, 5 x 5 Gaussian blur, bicubic resize down and back. */
int mf_augment_rgb(const uint8_t *rgb, const double *params, int32_t n, int32_t S, uint8_t *rgb_out,
                   void *workspace, mfStream_t stream);
/* _augment_pcd: 5 % pixel drop-out, then + 0.003 z per coordinate (z standard normal, float64). */
int mf_augment_pcd(const void *pcd, int32_t pcd_is_f64, const double *params, int32_t n, int32_t S,
                   int64_t seed, void *pcd_out, mfStream_t stream);

/* ---- OccupancyRegistration for a batch of objects (contrib/occupancy_registration.py, csrc/occreg.hip) -------
 * morefusion/contrib/occupancy_registration.py for B objects in one launch: one workgroup per object runs every
 * iteration {soft occupancy grid of the transformed points, penalty - reward, backward, chainer-Adam step} with no
 * host involvement (DESIGN.md "Occupancy registration"; tests/occreg_ref.py is the NumPy mirror, bit for bit).
 * Object b: points rows pts_off[b] .. pts_off[b + 1] of `points` (float32 [Ptot, 3]); grid dims[b] = (X, Y, Z) of
 * pitch[b] at origin[b]; threshold[b] in voxels; its targets grid_occ / grid_unocc are the X Y Z floats at
 * grid_off[b] (grid_off[b + 1] - grid_off[b] = X Y Z; unocc = max(grid[1], grid[2]) for 3-channel targets);
 * active [B] uint8 (NULL: all): an inactive object's pose passes through, its losses are 0.
 * All of these are DEVICE arrays.  A launcher cannot read them without synchronising, so the small per-object arrays
 * travel a second time as HOST arrays (host_*, the same values): the refusals below are decided on those, and the
 * kernel checks the device copies again (an object whose device descriptor is invalid passes through with a NaN
 * loss and touches nothing).
 * Limits: 1 .. MF_OCCREG_MAX_OBJECTS objects; n_points_total and every object's X Y Z (<= max_voxels) and the
 * batch's voxel total within int32; every dimension >= 1; 0 < threshold <= MF_OCCREG_MAX_THRESHOLD (finite);
 * pitch finite and > 0: anything else returns -hipErrorInvalidValue with mf_last_error_string set.  Points must be
 * finite.  A grid of at most MF_OCCREG_LDS_VOXELS voxels keeps its distance field in LDS, a larger one in the
 * workspace; the first MF_OCCREG_POINT_TILE points of an object keep their grid coordinates in LDS, later ones
 * are transformed again from global memory.  Every call is asynchronous on `stream`, allocates nothing and never
 * synchronises; results are bitwise reproducible (no float atomics). */
#define MF_OCCREG_MAX_OBJECTS 65535
#define MF_OCCREG_POINT_TILE 1024
#define MF_OCCREG_LDS_VOXELS 32768
#define MF_OCCREG_MAX_THRESHOLD 64.0f
#define MF_OCCREG_STEPS_PER_LAUNCH 128 /* mf_occreg_refine: one launch per this many iterations */
typedef struct {
  const float *points;
  const int32_t *pts_off;
  const float *pitch;
  const float *origin;
  const int32_t *dims;
  const float *threshold;
  const float *grid_occ;
  const float *grid_unocc;
  const int32_t *grid_off;
  const uint8_t *active;
  const int32_t *host_pts_off;
  const float *host_pitch;
  const int32_t *host_dims;
  const float *host_threshold;
  int32_t n_objects;
  int32_t n_points_total;
  int32_t max_voxels;
  int32_t reserved;
} mfOccRegBatch;
/* Host-only: bytes of `workspace` (0 when max_voxels <= MF_OCCREG_LDS_VOXELS: it may then be NULL); < 0 for
 * n_objects outside 1 .. MF_OCCREG_MAX_OBJECTS, n_points_total < 0, max_voxels < 1 or either beyond int32. */
int64_t mf_occreg_workspace_bytes(int64_t n_objects, int64_t n_points_total, int64_t max_voxels);
/* One forward and backward at the poses q [B, 4] (wxyz), t [B, 3] (untouched): loss [B] = sum(unocc m) / sum(m) -
 * sum(occ m) / sum(occ) (NaN when no voxel is within threshold of a point, as in the reference; the gradient is
 * then 0), gq [B, 4], gt [B, 3]. */
int mf_occreg_loss_grad(const mfOccRegBatch *batch, const float *q, const float *t, float *loss, float *gq,
                        float *gt, void *workspace, mfStream_t stream);
/* n_iter x {loss, gradient, chainer-Adam step} on q, t, adam_m, adam_v [B, 7] in place; step0 = Adam steps already
 * taken (bias correction: alpha * sqrt(1 - b2^s) / (1 - b1^s) in double on the host, cast once).  losses
 * [n_iter, B] (NULL: not kept): losses[k] at the pose before step k + 1; traj [n_iter + 1, B, 7] (NULL: not kept):
 * entry 0 the initial pose, entry k the pose (q then t) after step k. */
int mf_occreg_refine(const mfOccRegBatch *batch, float *q, float *t, float *adam_m, float *adam_v, int32_t n_iter,
                     int32_t step0, float alpha_q, float alpha_t, float *losses, float *traj, void *workspace,
                     mfStream_t stream);

/* ---- occupancy grids -> welded, smoothed triangle meshes (geometry/grid_mesh.py, csrc/gridmesh.hip) ----------
 * grid_msg_to_mesh of the reference (ros/src/morefusion_ros/nodes/voxel_grids_to_mesh_markers.py:80-97) for a
 * batch: the 0.5-level surface of each grid's occupancy (a cell is occupied iff its value is > 0) over the
 * six-tetrahedra subdivision of the lattice padded by one empty layer, welded, then trimesh's Humphrey filter
 * (DESIGN.md "Grid meshes"; tests/gridmesh_ref.py is the NumPy mirror, bit for bit).  Grid b: the X Y Z floats at
 * grid_off[b] of `grids`, dims[b] = (X, Y, Z) each in 1 .. MF_GRIDMESH_MAX_DIM (a grid with other dims is empty);
 * vertex = origin[b] + pitch[b] ((pa + pb) / 2 - 1) in float64 for the lattice edge pa-pb.  Vertex and face order
 * are fixed by the input alone (header of csrc/gridmesh.hip).  All arrays are DEVICE arrays; every call is
 * asynchronous on `stream`, allocates nothing and never synchronises.  Refusals return < 0. */
#define MF_GRIDMESH_MAX_DIM 32
#define MF_GRIDMESH_MAX_GRIDS 4096
#define MF_GRIDMESH_MAX_NEIGHBOURS 12 /* faces (= neighbours) at a vertex of such a surface, at most */
#define MF_GRIDMESH_MAX_ROWS 1073741824 /* vertices, and faces, of a batch */
/* Host-only: bytes (16-byte aligned parts) of the workspace of mf_gridmesh_count / _emit for n_grids grids plus the
 * one of mf_gridmesh_smooth for n_vertices vertices; < 0 past the caps above. */
int64_t mf_gridmesh_workspace_bytes(int64_t n_grids, int64_t n_vertices);
/* Count: offsets int64 [2, n_grids + 1] = the vertices (row 0) and faces (row 1) before each grid, the totals last.
 * The caller reads it back to size the buffers of mf_gridmesh_emit; `workspace` keeps the per-layer offsets. */
int mf_gridmesh_count(const float *grids, const int64_t *grid_off, const int32_t *dims, int32_t n_grids,
                      void *workspace, int64_t *offsets, mfStream_t stream);
/* Emit: vertices float64 [n_vertices, 3], faces int32 [n_faces, 3] (indices local to their mesh), packed in grid
 * order; n_vertices / n_faces are the totals of `offsets` (rows past them are not written). */
int mf_gridmesh_emit(const float *grids, const int64_t *grid_off, const int32_t *dims, const double *pitch,
                     const double *origin, int32_t n_grids, const void *workspace, const int64_t *offsets,
                     int64_t n_vertices, int64_t n_faces, double *vertices, int32_t *faces, mfStream_t stream);
/* Neighbour rows of packed meshes (offsets as above): vertex a's row neighbours[12 a ..] = the heads b of the
 * directed half-edges a -> b of its faces, as packed vertex indices in ascending order, -1 behind them;
 * degree [n_vertices] = their number (a count above 12 marks a vertex that the filter leaves in place). */
int mf_gridmesh_adjacency(const int32_t *faces, const int64_t *offsets, int32_t n_grids, int64_t n_vertices,
                          int64_t n_faces, int32_t *neighbours, int32_t *degree, mfStream_t stream);
/* trimesh.smoothing.filter_humphrey with the equal-weight Laplacian L (mean over a row, summed in ascending
 * neighbour index), `iterations` times in place: q = v; v = L q; b = v - (alpha v0 + (1 - alpha) q);
 * v = v - (beta b + (1 - beta) L b), v0 the vertices at entry.  workspace: the smooth part of
 * mf_gridmesh_workspace_bytes(0, n_vertices). */
int mf_gridmesh_smooth(double *vertices, const int32_t *neighbours, const int32_t *degree, int64_t n_vertices,
                       double alpha, double beta, int32_t iterations, void *workspace, mfStream_t stream);
/* The label test of the reference's render service (nodes/render_voxel_grids.py:66-99): label = instance where
 * something was drawn (instance != -1) and -2 elsewhere, -2 too where depth_rendered > depth_sensor + 0.01
 * (float32; false for a NaN reading).  Images [height, width]. */
int mf_gridmesh_label(const float *depth_rendered, const int32_t *instance, const float *depth_sensor,
                      int32_t height, int32_t width, int32_t *label, mfStream_t stream);

/* ---- the map server's grids in the map frame (contrib/octomap_server.py, csrc/occserver.hip) --------------
 * OctomapServer::getGridsInWorldFrame (OctomapServer.cpp:456-508): grid b = the D^3 samples around center_map[b] of
 * tree target_tree[b]: origin[b] = double(center) - (D / 2 - 0.5) double(pitch[b]) (float64 [B, 3], written),
 * sample = origin + double(pitch * float(index)) searched as a float64 coordinate; grid = float32(occupancy) where
 * the node exists and its occupancy is > 0.5, else 0. */
int mf_occserver_map_grids(const mfOccTree *trees, int32_t n_trees, const int32_t *target_tree, const float *pitch,
                           const float *center_map, int32_t B, int32_t D, double *origin, float *grid,
                           mfStream_t stream);

/* ---- camera tracking: dense point-to-plane depth alignment (contrib/camera_tracking.py, csrc/camtrack.hip) ----
 * The tracking step of KinectFusion: projective data association and point-to-plane Gauss-Newton over a depth
 * pyramid, B independent alignments per call, float64 throughout (DESIGN.md "Camera tracking"; tests/camtrack_ref.py
 * is the NumPy mirror, bit for bit).  All arrays are DEVICE arrays unless said otherwise; every call is asynchronous
 * on `stream`, allocates nothing and never synchronises.  Refusals return < 0.
 *
 * Level l of a pyramid has H_l = height >> l rows and W_l = width >> l columns (an odd size drops its last row or
 * column) and the intrinsics fx_(l+1) = fx_l / 2, fy_(l+1) = fy_l / 2, cx_(l+1) = (cx_l - 0.5) / 2, cy_(l+1) =
 * (cy_l - 0.5) / 2.  A PYRAMID is one buffer of mf_camtrack_workspace_bytes(.., MF_CAMTRACK_PYRAMID) bytes: for
 * l = 0 .. levels - 1 in turn the parts depth_l float32 [B, H_l, W_l], vertex_l float64 [B, H_l, W_l, 3], normal_l
 * float64 [B, H_l, W_l, 3], then rect int32 [levels, B, 4] = (0, 0, H_l, W_l); every part starts at the next
 * multiple of 16 bytes.
 *   depth_0 = the input.  A sample is valid iff it is > 0 (NaN is not).  depth_(l+1)(y, x): of the samples (2y, 2x),
 *   (2y, 2x + 1), (2y + 1, 2x), (2y + 1, 2x + 1) of depth_l, in this order, those that are valid and have
 *   double(d) - double(d_min) <= block_band (d_min the smallest valid one) are summed in float64 in this order,
 *   divided by their number and rounded to float32; NaN if none is valid.
 *   vertex_l(r, c) = ((z (c - cx_l)) / fx_l, (z (r - cy_l)) / fy_l, z) with z = double(depth), NaN x 3 if invalid.
 *   normal_l = mf_pick_normals of vertex_l with the rectangle (0, 0, H_l, W_l) (that entry point is called). */
#define MF_CAMTRACK_MAX_LEVELS 8
#define MF_CAMTRACK_MAX_BATCH 1024
#define MF_CAMTRACK_MAX_PIXELS (1LL << 26) /* B * height * width */
#define MF_CAMTRACK_MAX_ITERATIONS 4096    /* summed over the levels */
#define MF_CAMTRACK_PYRAMID 0
#define MF_CAMTRACK_ALIGN 1
#define MF_CAMTRACK_GROUP_PIXELS 1024 /* pixels of one workgroup of the residual launch: 256 lanes x 4 */
#define MF_CAMTRACK_PARTIAL 32        /* doubles of one workgroup's partial (29 used) */
#define MF_CAMTRACK_TRACKING 0
#define MF_CAMTRACK_LOST_PAIRS 1 /* fewer than min_pairs pairs */
#define MF_CAMTRACK_LOST_PIVOT 2 /* a Cholesky pivot was not > 0 */
/* Host-only: bytes of a pyramid (which = MF_CAMTRACK_PYRAMID) or of mf_camtrack_align's workspace (which =
 * MF_CAMTRACK_ALIGN) for B images of height x width and `levels` levels; < 0 unless 1 <= B <= MF_CAMTRACK_MAX_BATCH,
 * height, width <= MF_RENDER_MAX_SIDE, B height width <= MF_CAMTRACK_MAX_PIXELS, 1 <= levels <=
 * MF_CAMTRACK_MAX_LEVELS and the coarsest level is at least 8 x 8. */
int64_t mf_camtrack_workspace_bytes(int32_t B, int32_t height, int32_t width, int32_t levels, int32_t which);
/* depth float32 [B, height, width] -> pyramid (every part written).  fx, fy != 0, block_band >= 0. */
int mf_camtrack_prepare(const float *depth, int32_t B, int32_t height, int32_t width, int32_t levels, double fx,
                        double fy, double cx, double cy, double block_band, void *pyramid, mfStream_t stream);
/* Align the pyramid `current` to the pyramid `reference` (both of B, height, width, levels and fx .. cy).
 * T_ref_to_map, T_init float64 [B, 4, 4] row-major (rigid; T_init = the first guess of T_cur_to_map); `iterations`
 * is a HOST array int32 [levels], the Gauss-Newton iterations at the coarsest level first, each >= 0, n_iters their
 * sum.  Outputs: pose float64 [B, 7] = unit quaternion (w, x, y, z) then translation, T_cur_to_map float64 [B, 4, 4]
 * = the matrix of `pose`, status int32 [B] (MF_CAMTRACK_TRACKING / _LOST_*), stats float64 [B, n_iters, 3] = (pairs,
 * sum r^2, |increment|) of each iteration (zeros: the alignment was lost before it).
 *
 * Start (one launch): q = the quaternion of T_init's rotation (Shepperd's four branches, normalised), t its
 * translation; the rigid inverse of T_ref_to_map.  Then per iteration TWO launches:
 *   residuals -- a workgroup of 256 lanes per MF_CAMTRACK_GROUP_PIXELS pixels and alignment; lane t takes the
 *   pixels p = 1024 g + 256 s + t, s = 0 .. 3 in turn (p row-major over the level).  A pixel with a valid vertex v
 *   and normal n: v_g = R v + t, n_g = R n, p_r = T_ref^-1 v_g; rejected if p_r.z is not > 0; (col, row) =
 *   floor((fx p_r.x) / p_r.z + cx + 0.5), floor((fy p_r.y) / p_r.z + cy + 0.5), rejected outside the image or where
 *   the reference vertex or normal there has a NaN; v_ref_g = R_ref v_ref + t_ref, n_ref_g = R_ref n_ref, d =
 *   v_ref_g - v_g; rejected if |d| > distance_threshold or n_g . n_ref_g < cos_angle_threshold.  r = n_ref_g . d,
 *   J = (n_ref_g, v_g x n_ref_g).  Every 3-term sum is ((a + b) + c) (+ t).  A lane adds its pairs' 28 terms --
 *   J_i J_j for i <= j row by row (21), J_i r (6), r r -- in the order s = 0 .. 3; the 64 lanes of a wave fold by
 *   x[l] += x[l + h] for h = 32, 16, .. 1; the 4 waves add as ((w0 + w1) + w2) + w3; the pair count is an integer.
 *   One partial of MF_CAMTRACK_PARTIAL doubles per workgroup (term 28 = the count).
 *   solve -- a workgroup per alignment: sub-sum j = 0 .. 7 adds the partials g = j, j + 8, .. in turn, the total is
 *   ((((((s0 + s1) + s2) + s3) + s4) + s5) + s6) + s7.  pairs < min_pairs -> lost.  Cholesky A = L L^T row by row
 *   (each inner product subtracted term by term in increasing index; a pivot not > 0 -> lost), forward and back
 *   substitution likewise: xi = (xi_t, xi_r).  dq = (1, xi_r / 2) normalised, t = R(dq) t + xi_t, q = dq q
 *   normalised (Hamilton product, terms added left to right).  |increment| = sqrt of the squares of xi summed left to
 *   right.
 * A lost alignment gets its status, its pose back to the initial one and is left untouched by every later launch;
 * the others go on.  Only + - x / sqrt and floor are used.  workspace: MF_CAMTRACK_ALIGN bytes. */
int mf_camtrack_align(const void *current, const void *reference, int32_t B, int32_t height, int32_t width,
                      int32_t levels, double fx, double fy, double cx, double cy, const double *T_ref_to_map,
                      const double *T_init, const int32_t *iterations, double distance_threshold,
                      double cos_angle_threshold, int32_t min_pairs, double *pose, double *T_cur_to_map,
                      int32_t *status, double *stats, void *workspace, mfStream_t stream);

/* ---- TSDF fusion: integrate depth frames into a volume, ray-cast it (contrib/tsdf_volume.py, csrc/tsdf.hip) ----
 * The mapping half of KinectFusion: the model that frame-to-model tracking aligns to (DESIGN.md "TSDF fusion";
 * tests/tsdf_ref.py is the NumPy mirror, bit for bit, written from this text).  All arrays are DEVICE arrays; every
 * call is asynchronous on `stream`, allocates nothing and never synchronises.
 *
 * VOLUME: float32 [nz][ny][nx][2], x fastest, the pair (tsdf, weight) of voxel (i, j, k) at float index
 * 2 ((k ny + j) nx + i).  The centre of voxel (i, j, k) is c_a = origin_a + pitch * double(index_a) in the MAP frame
 * (origin_a, pitch float64; a = x, y, z with index i, j, k).  A fresh volume is (1, 0) everywhere; the caller fills it.
 * POSE: T_sensor_to_map float64 [16] row-major ON THE DEVICE (R_ab = T[4 a + b], t_a = T[4 a + 3]); only these 12
 * words are read.  Pinhole fx, fy, cx, cy; images [H][W] row-major.
 * ARITHMETIC: float64, + - * / and floor only, nothing contracted, every expression associated as written here;
 * float32 inputs are widened first, results are rounded to float32 at the store.  Every test is written so that a
 * NaN fails it.
 * Refused with -hipErrorInvalidValue (the function's name in mf_last_error_string) unless: nx, ny, nz >= 2 and
 * nx ny nz < 2^31; pitch > 0; truncation > 0; max_weight >= 1; 1 <= H, W <= MF_RENDER_MAX_SIDE; fx, fy > 0;
 * step > 0; 0 <= min_depth < max_depth; 1 <= max_steps <= MF_TSDF_MAX_STEPS; the arrays non-null (skip_flag and
 * code_out may be null). */
#define MF_TSDF_MAX_STEPS 65536
#define MF_TSDF_RAY_HIT 0      /* depth_out = the zero crossing */
#define MF_TSDF_RAY_LEFT 1     /* the samples ran past the far end of the box: no crossing */
#define MF_TSDF_RAY_BACKFACE 2 /* the first sample with tsdf <= 0 had no valid positive sample right before it */
#define MF_TSDF_RAY_MISS 3     /* the ray does not meet the box within [min_depth, max_depth] */
#define MF_TSDF_RAY_CAP 4      /* max_steps samples taken without an end */
/* Fuse one depth image into the volume.  One lane per voxel (256-lane workgroups over the flat voxel index).  If
 * skip_flag is non-null and *skip_flag != 0 (an int32 on the device, e.g. the status of mf_camtrack_align) no lane
 * does anything.  Per voxel, with c its centre:
 *   e_a = c_a - t_a;  p_a = (R_0a e_0 + R_1a e_1) + R_2a e_2   (p = R^T (c - t), the camera frame; x, y, z = p)
 *   required: z > 0
 *   u = fx * (x / z) + cx,  v = fy * (y / z) + cy,  col = floor(u + 0.5),  row = floor(v + 0.5)
 *   required: col >= 0, col <= W - 1, row >= 0, row <= H - 1 (compared as float64)
 *   D = double(depth[row][col]);  required: D > 0
 *   sdf = D - z;  required: sdf >= -truncation
 *   f = sdf / truncation;  if f > 1 then f = 1
 *   with (F_old, W_old) the voxel's pair: tsdf = float32((F_old * W_old + f) / (W_old + 1)),
 *   w = W_old + 1, if w > max_weight then w = max_weight, weight = float32(w).
 * A voxel that fails a requirement is not written. */
int mf_tsdf_integrate(float *volume, int32_t nx, int32_t ny, int32_t nz, double origin_x, double origin_y,
                      double origin_z, double pitch, double truncation, double max_weight, const float *depth,
                      int32_t H, int32_t W, double fx, double fy, double cx, double cy,
                      const double *T_sensor_to_map, const int32_t *skip_flag, mfStream_t stream);
/* Ray-cast the volume into a depth image.  One lane per pixel (16 x 16 pixel workgroups); depth_out float32 [H][W]
 * and code_out uint8 [H][W] (may be null) are written for EVERY pixel: depth_out = 0 unless the ray ends in a hit.
 * Pixel (row, col):
 *   q = ((col - cx) / fx, (row - cy) / fy);  d_a = (R_a0 q_0 + R_a1 q_1) + R_a2;  o_a = t_a
 *   (the camera-frame ray is (q_0, q_1, 1): the ray parameter is the camera-frame depth)
 *   lo_a = origin_a,  hi_a = origin_a + pitch * double(n_a - 1);  enter = min_depth,  exit = max_depth
 *   for a = x, y, z in turn:
 *     if d_a < 0 or d_a > 0:  t1 = (lo_a - o_a) / d_a,  t2 = (hi_a - o_a) / d_a,
 *                             (tn, tf) = (t1, t2) if t1 < t2 else (t2, t1),
 *                             enter = enter if tn <= enter else tn,  exit = exit if tf >= exit else tf
 *     else unless d_a == 0 and o_a >= lo_a and o_a <= hi_a: MISS
 *   unless enter <= exit: MISS
 *   for k = 0, 1, ..:
 *     s = enter + double(k) * step;  unless s <= exit: LEFT;  then if k >= max_steps: CAP
 *     g_a = ((o_a + s * d_a) - origin_a) / pitch,  b_a = floor(g_a),  r_a = g_a - b_a
 *     the sample is VALID iff b_a >= 0 and b_a <= n_a - 2 for all a (compared as float64) and the weights of the
 *     eight voxels (b_x + {0, 1}, b_y + {0, 1}, b_z + {0, 1}) are all > 0.  Its value, from their tsdf V_xyz:
 *       along x:  V_yz = V_0yz + r_x * (V_1yz - V_0yz);  along y:  V_z = V_0z + r_y * (V_1z - V_0z);
 *       F = V_0 + r_z * (V_1 - V_0)
 *     invalid: previous = none.  valid and F <= 0: if previous is a value P > 0 then HIT with
 *       depth_out = float32((enter + double(k - 1) * step) + step * (P / (P - F)))
 *     else BACKFACE.  valid otherwise: previous = F. */
int mf_tsdf_raycast(const float *volume, int32_t nx, int32_t ny, int32_t nz, double origin_x, double origin_y,
                    double origin_z, double pitch, double step, double min_depth, double max_depth,
                    int32_t max_steps, int32_t H, int32_t W, double fx, double fy, double cx, double cy,
                    const double *T_sensor_to_map, float *depth_out, uint8_t *code_out, mfStream_t stream);

/* ---- TSDF mesh: the fused surface as a welded triangle mesh with normals (contrib/tsdf_volume.py, csrc/tsdfmesh.hip) ----
 * TsdfVolume.extract_mesh (DESIGN.md "TSDF mesh"; tests/tsdfmesh_ref.py is the NumPy mirror, bit for bit, written
 * from this text).  All arrays are DEVICE arrays (totals too); every call is asynchronous on `stream`, allocates
 * nothing and never synchronises.  VOLUME, origin and pitch are those of "TSDF fusion": lattice point (i, j, k) sits at
 * p_a = origin_a + pitch * double(index_a) and has the pair (F, W) = (tsdf, weight).
 *
 * INSIDE: a point is inside iff F <= 0 (-0.0 is inside, a NaN is not).  OBSERVED: a point is observed iff
 * double(W) >= min_weight (min_weight > 0); cell (i, j, k), 0 <= i <= nx - 2, 0 <= j <= ny - 2, 0 <= k <= nz - 2, with
 * the corners (i + dx, j + dy, k + dz), is observed iff its eight corners are.  Only observed cells have faces.
 *
 * TRIANGULATION: the six-tetrahedra subdivision written at the head of csrc/gridmesh.hip, "occupied" read as inside.
 * Corner codes are dx * 4 + dy * 2 + dz.  Tetrahedron t = 0 .. 5 walks the axes xyz, xzy, yxz, yzx, zxy, zyx: its
 * corners are c0 = the cell, c1 = c0 + e_a, c2 = c1 + e_b, c3 = the cell + (1, 1, 1).  With e(i, j) the vertex on the
 * edge between corners i and j of the tetrahedron:
 *   one corner i alone on its side:          (e(i, j0), e(i, j1), e(i, j2)), j ascending;
 *   corners a < b inside, c < d outside:     (e(a, c), e(a, d), e(b, d)) then (e(a, c), e(b, d), e(b, c));
 * the last two vertices of a triangle are exchanged where that makes it counter-clockwise seen from the outside.
 * Degenerate triangles (a tsdf of exactly 0 at a corner) are kept.
 *
 * VERTICES: point (i, j, k) owns the edges towards + (1,0,0) (0,1,0) (0,0,1) (1,1,0) (1,0,1) (0,1,1) (1,1,1),
 * directions 0 .. 6.  An owned edge whose other end is a lattice point carries a vertex iff its ends differ in
 * inside / outside and at least one observed cell contains it; the cells that contain the edge are (i, j, k) - s with
 * s in {0, 1} on every axis where the direction's component is 0 (s = 0 elsewhere), those that are cells.  Vertices are
 * numbered by rank in ascending (k, j, i, direction) order, faces in ascending (k, j, i, tetrahedron, triangle) order of
 * their cell; faces are int32 [n_faces][3] indices into vertices float64 [n_vertices][3].
 *
 * POSITION, float64, + - * / only, nothing contracted, associated as written; a = the owner, b = the other end:
 *   r = double(F_a) / (double(F_a) - double(F_b))
 *   v_c = p_a,c + r * (p_b,c - p_a,c)                      (p as above, c = x, y, z)
 * NORMAL (normals float64 [n_vertices][3], may be null), towards positive tsdf.  At a lattice point q, per axis c with
 * q+ and q- its neighbours along c ("usable": a lattice point that is observed), F the widened tsdf:
 *   both usable: G_c = (F(q+) - F(q-)) / 2;  only q+: G_c = F(q+) - F(q);  only q-: G_c = F(q) - F(q-);  neither: 0.
 * At the vertex:
 *   g_c = G_c(a) + r * (G_c(b) - G_c(a));   s = (g_x * g_x + g_y * g_y) + g_z * g_z
 *   n_c = g_c / sqrt(s) if s > 0, else n = (0, 0, 0)      (sqrt and / correctly rounded)
 *
 * WORKSPACE of mf_tsdfmesh_workspace_bytes(nx, ny, nz) bytes, 16-byte aligned, three parts that each start at a multiple
 * of 16: flags uint8 [nz][ny][nx] (bit 0 inside, bit 1 observed), masks uint8 [nz][ny][nx] (bit d: the owned edge of
 * direction d carries a vertex), rows int64 [nz ny + 1][2] (vertices, faces before row (k, j), row index k ny + j; the
 * last entry holds the totals).  mf_tsdfmesh_count fills all three; mf_tsdfmesh_emit reads them.
 * Refused with -hipErrorInvalidValue (the function's name in mf_last_error_string) unless: nx, ny, nz >= 2 and
 * nx ny nz < 2^31; min_weight > 0; pitch > 0; 0 <= n_vertices, n_faces < 2^31; the arrays non-null (normals may be
 * null), the volume and the workspace 16-byte aligned. */
/* Host-only: the workspace's bytes; < 0 for a bad volume. */
int64_t mf_tsdfmesh_workspace_bytes(int32_t nx, int32_t ny, int32_t nz);
/* Three launches (flags, masks and row counts, scan of the rows): totals int64 [2] = (n_vertices, n_faces). */
int mf_tsdfmesh_count(const float *volume, int32_t nx, int32_t ny, int32_t nz, double min_weight, void *workspace,
                      int64_t *totals, mfStream_t stream);
/* One launch, a workgroup per row (k, j): writes every vertex (and normal) and every face.  workspace as
 * mf_tsdfmesh_count of the same volume and min_weight left it, n_vertices and n_faces its totals (rows past them are
 * not written). */
int mf_tsdfmesh_emit(const float *volume, int32_t nx, int32_t ny, int32_t nz, double origin_x, double origin_y,
                     double origin_z, double pitch, double min_weight, const void *workspace, int64_t n_vertices,
                     int64_t n_faces, double *vertices, int32_t *faces, double *normals, mfStream_t stream);

/* ---- TSDF labels: an instance label per voxel, and the pose stages' grids from it (contrib/instance_tsdf_volume.py,
 * csrc/tsdflabel.hip) ----
 * InstanceTsdfVolume (DESIGN.md "TSDF labels"; tests/tsdflabel_ref.py is the NumPy mirror, bit for bit, written from
 * this text).  All arrays are DEVICE arrays; every call is asynchronous on `stream`, allocates nothing and never
 * synchronises.  VOLUME, origin, pitch, POSE and ARITHMETIC are those of "TSDF fusion"; integers are int32 unless said
 * otherwise, and there are no float atomics: every result is independent of the order in which lanes run.
 *
 * LABELS: int32 [nz][ny][nx][2], the pair (label, count) of voxel (i, j, k) at int index 2 ((k ny + j) nx + i): the
 * volume's voxel order, 8 bytes per voxel.  A fresh volume is (0, 0) everywhere; the caller fills it.  count >= 0, and
 * count == 0 goes with label == 0.
 * VOTES: a pixel label v votes iff v >= 1 (a tracked instance id) or v == -1 (the background); -2 ("uncertain"), 0 and
 * everything below -2 cast no vote.
 * A position is INSIDE the volume iff g_a = floor((m_a - origin_a) / pitch + 0.5) satisfies g_a >= 0 and g_a <= n_a - 1
 * on every axis (compared as float64; a NaN is outside); its voxel is (g_x, g_y, g_z).
 * A rigid transform T (float64 [16] row-major on the device, 12 words read) moves p to
 *   T p := ((T[4 a] p_x + T[4 a + 1] p_y) + T[4 a + 2] p_z) + T[4 a + 3],  a = x, y, z.
 * Refused with -hipErrorInvalidValue (the function's name in mf_last_error_string) unless: nx, ny, nz >= 2 and
 * nx ny nz < 2^31; pitch > 0; truncation > 0; max_weight >= 1; 1 <= H, W <= MF_RENDER_MAX_SIDE; fx, fy > 0;
 * max_count >= 1; min_count >= 1; min_weight > 0; 1 <= B <= MF_TSDF_MAX_INSTANCES; 1 <= D <= MF_TSDF_MAX_GRID_DIM;
 * flags in 0 .. 3; the arrays non-null (skip_flag may be null). */
#define MF_TSDF_MAX_INSTANCES 64
#define MF_TSDF_MAX_GRID_DIM 256
/* mf_tsdf_integrate of the same arguments -- the (tsdf, weight) bytes it leaves are the same -- and one vote per voxel.
 * One lane per voxel; if skip_flag is non-null and *skip_flag != 0 neither array is written.  A voxel votes iff it
 * passed every requirement of mf_tsdf_integrate (it was written), sdf <= truncation (sdf as there, before the clamp)
 * and v = label_image[row][col] (int32 [H][W], the pixel its depth came from) is a voting label.  With (l, c) its pair:
 *   c == 0:     (l, c) = (v, 1)
 *   l == v:     c = min(c + 1, max_count)
 *   otherwise:  c = c - 1, and if c == 0 then l = 0. */
int mf_tsdf_integrate_labels(float *volume, int32_t *labels, int32_t nx, int32_t ny, int32_t nz, double origin_x,
                             double origin_y, double origin_z, double pitch, double truncation, double max_weight,
                             const float *depth, int32_t H, int32_t W, double fx, double fy, double cx, double cy,
                             const double *T_sensor_to_map, const int32_t *label_image, int32_t max_count,
                             const int32_t *skip_flag, mfStream_t stream);
/* The label under every pixel of a depth image (e.g. mf_tsdf_raycast's depth_out from the same pose).  One lane per
 * pixel (16 x 16 pixel workgroups); out int32 [H][W] is written for EVERY pixel.  Pixel (row, col) with d =
 * double(depth[row][col]):  unless d > 0: 0.  q as in mf_tsdf_raycast, the camera point p = (q_0 * d, q_1 * d, d),
 * m = T_sensor_to_map p.  out = the label of m's voxel if m is inside and its count >= min_count, else 0. */
int mf_tsdf_label_image(const int32_t *labels, int32_t nx, int32_t ny, int32_t nz, double origin_x, double origin_y,
                        double origin_z, double pitch, const float *depth, int32_t H, int32_t W, double fx, double fy,
                        double cx, double cy, const double *T_sensor_to_map, int32_t min_count, int32_t *out,
                        mfStream_t stream);
/* Where every instance is.  ids int32 [B] STRICTLY ASCENDING (the caller's duty: an id out of order is not found);
 * table int64 [B][10] := per id, over the voxels (i, j, k) with double(weight) >= min_weight, tsdf <= 0, label == id
 * and count >= min_count: {their number, sum i, sum j, sum k, min i, min j, min k, max i, max j, max k}; an id without
 * a voxel gets {0, 0, 0, 0, nx, ny, nz, -1, -1, -1}.  Two launches: one sets the table, one adds to it (a lane per
 * voxel, a table per workgroup in LDS, 64-bit integer atomics into `table`). */
int mf_tsdf_instance_stats(const float *volume, const int32_t *labels, int32_t nx, int32_t ny, int32_t nz,
                           double min_weight, int32_t min_count, const int32_t *ids, int32_t B, int64_t *table,
                           mfStream_t stream);
/* B grids of D^3 voxels in the SENSOR frame, in the index order of mf_occserver_publish (grid [b][x][y][z]); one lane
 * per output voxel, every output element is written.  Per grid b, with p = grid_pitch[b] (float64 [B]), c =
 * center_map[b] (float64 [B][3], MAP frame) and id = ids[b]:
 *   centre = T_map_to_sensor c;  origin[b]_a := centre_a - (double(D) / 2.0 - 0.5) * p      (origin float64 [B][3])
 *   voxel (x, y, z):  s_a = origin[b]_a + p * double(index_a);  m = T_sensor_to_map s
 *   1. flags & 1 and m_z < ground_z:                          noentry = 1
 *   2. else m outside the volume, or not double(weight) >= min_weight of its voxel (F, weight; l, c):   nothing
 *   3. else F <= 0:  if c >= min_count:  l == id: target = 1;  else l != 0: noentry = 1
 *   4. else flags & 2 and double(F) >= empty_above:           noentry = 1
 * grid_target, grid_noentry float32 (0 or 1), grid_nontarget_empty uint8 := noentry != 0. */
int mf_tsdf_publish_grids(const float *volume, const int32_t *labels, int32_t nx, int32_t ny, int32_t nz,
                          double origin_x, double origin_y, double origin_z, double pitch, const int32_t *ids,
                          const double *grid_pitch, const double *center_map, const double *T_map_to_sensor,
                          const double *T_sensor_to_map, double min_weight, int32_t min_count, double empty_above,
                          double ground_z, int32_t flags, int32_t B, int32_t D, double *origin, float *grid_target,
                          float *grid_noentry, uint8_t *grid_nontarget_empty, mfStream_t stream);

/* ---- TSDF render: the ray-cast with empty-space skipping and the label image fused in (contrib/tsdf_volume.py,
 * contrib/instance_tsdf_volume.py, csrc/tsdfrender.hip) ----
 * TsdfVolume.render / InstanceTsdfVolume.render (DESIGN.md "TSDF render"; tests/tsdfrender_ref.py is the NumPy mirror,
 * bit for bit, written from this text).  All arrays are DEVICE arrays; every call is asynchronous on `stream`, allocates
 * nothing and never synchronises.  VOLUME, origin, pitch, POSE and ARITHMETIC are those of "TSDF fusion", LABELS and
 * INSIDE those of "TSDF labels".
 *
 * CELLS AND BLOCKS: cell b = (b_x, b_y, b_z), 0 <= b_a <= n_a - 2, is what floor(g) of a ray sample names; its corners
 * are the voxels b + {0, 1}^3.  With the block edge B (2, 4, 8 or 16), block (I, J, K) = (I_x, I_y, I_z) holds the cells
 * b_a in [B I_a, min(B I_a + B - 1, n_a - 2)]: nb_a = ceil((n_a - 1) / B) blocks per axis.  Its FOOTPRINT is the voxels
 * those cells touch, [B I_a, min(B I_a + B, n_a - 1)] per axis (up to (B + 1)^3; neighbouring blocks share a layer).
 * SUMMARY: uint8 [nb_z][nb_y][nb_x], x fastest, one code per block:
 *   FREE     every footprint voxel has weight > 0 and tsdf == 1.0f (compared as values: a NaN is not free)
 *   UNKNOWN  no footprint voxel has weight > 0 (the negation of > 0: a NaN weight counts as unknown)
 *   MIXED    anything else
 * A summary describes the volume it was made from; after an integrate it is stale and must be made again.
 * Refused with -hipErrorInvalidValue (the function's name in mf_last_error_string; mf_tsdf_summary_bytes returns a
 * negative value) unless: everything "TSDF fusion" asks of mf_tsdf_raycast's arguments; B is 2, 4, 8 or 16; summary is
 * non-null; labels and label_out are both null or both non-null, and min_count >= 1 if they are given (code_out and
 * stats_out may be null). */
#define MF_TSDF_BLOCK_MIXED 0
#define MF_TSDF_BLOCK_FREE 1
#define MF_TSDF_BLOCK_UNKNOWN 2
/* Host-only: the summary's bytes, nb_x nb_y nb_z; < 0 for a bad volume or B. */
int64_t mf_tsdf_summary_bytes(int32_t nx, int32_t ny, int32_t nz, int32_t B);
/* One launch that reads the volume once, plus the layers neighbouring blocks share, and writes the code of EVERY block
 * (no pre-fill).  A workgroup per (256 voxels along x, J, K), a lane per voxel of the x run; the reduction is a logical
 * OR of two bits per voxel through wave ballots, so no result depends on an order. */
int mf_tsdf_block_summary(const float *volume, int32_t nx, int32_t ny, int32_t nz, int32_t B, uint8_t *summary,
                          mfStream_t stream);
/* mf_tsdf_raycast of the same arguments with the samples of FREE and UNKNOWN blocks not loaded: depth_out and code_out
 * are written for EVERY pixel as that contract says, word for word -- the slab test, s = enter + double(k) * step, LEFT
 * before CAP, g, b, r, F and the hit depth.  Only how a sample's outcome is obtained differs: with b of sample k,
 *   b in range and its block FREE:     the sample is VALID with F = 1.0 (what 1 + r * (1 - 1) gives on every axis)
 *   b in range and its block UNKNOWN:  the sample is INVALID
 *   otherwise (MIXED, or b out of range): as mf_tsdf_raycast evaluates it.
 * With the summary of this volume these are the outcomes of mf_tsdf_raycast, so the bytes are equal whatever the
 * volume holds.  The kernel may go from a sample k in a FREE or UNKNOWN block straight to a later sample k' iff sample
 * k' has its b in the SAME block, enter + double(k') * step <= exit and k' < max_steps: floor(g_a) is monotone in k on
 * every axis, so every sample between lies in that block too.  After a FREE run previous = 1.0, after an UNKNOWN run
 * none.  No output depends on how far the kernel tries to go.
 * label_out int32 [H][W] (with labels, "TSDF labels"): mf_tsdf_label_image's rule applied to the float32 depth_out of
 * the pixel: d = double(depth_out), unless d > 0: 0, else p = (q_0 * d, q_1 * d, d), m = T_sensor_to_map p, the label of
 * m's voxel if m is inside and its count >= min_count, else 0.  Written for every pixel.
 * stats_out int32 [H][W][2] = (sampled, visited).  A ray's samples are the k that passed both tests (LEFT, CAP).
 * sampled: those of them that were not classified FREE or UNKNOWN (MIXED or out of range), the one that ended the ray
 * included; fixed by the inputs.  visited: the samples whose position the kernel computed at all; it depends on how the
 * kernel jumps, and sampled <= visited <= the number of samples. */
int mf_tsdf_render(const float *volume, int32_t nx, int32_t ny, int32_t nz, double origin_x, double origin_y,
                   double origin_z, double pitch, double step, double min_depth, double max_depth, int32_t max_steps,
                   int32_t H, int32_t W, double fx, double fy, double cx, double cy, const double *T_sensor_to_map,
                   const uint8_t *summary, int32_t B, const int32_t *labels, int32_t min_count, float *depth_out,
                   uint8_t *code_out, int32_t *label_out, int32_t *stats_out, mfStream_t stream);

/* ---- TSDF colour: a colour per voxel, and the colour of renders and of mesh vertices from it (contrib/tsdf_volume.py,
 * csrc/tsdfcolor.hip) ----
 * TsdfVolume(colors=True) (DESIGN.md "TSDF colour"; tests/tsdfcolor_ref.py is the NumPy mirror, bit for bit, written
 * from this text).  All arrays are DEVICE arrays; every call is asynchronous on `stream`, allocates nothing and never
 * synchronises.  The VOLUME's voxel order, origin, pitch, POSE and ARITHMETIC are those of "TSDF fusion", T p is that of
 * "TSDF labels"; the (tsdf, weight) volume itself is neither read nor written by any entry point of this section.  A
 * lane reads and writes only its own output: no atomics, no result depends on an order.
 *
 * COLOURS: float32 [nz][ny][nx][4], the quadruple (r, g, b, colour weight) of voxel (i, j, k) at float index
 * 4 ((k ny + j) nx + i): 16 bytes per voxel, the array 16-byte aligned.  A fresh tensor is all zeros; the caller fills
 * it.  A voxel is COLOURED iff its colour weight is > 0 (a NaN weight is not coloured).  r, g, b are on the uint8 scale
 * 0 .. 255.
 *
 * SAMPLE, the colour at a MAP-frame point m -> rgba uint8 [4]:
 *   g_a = (m_a - origin_a) / pitch,  b_a = floor(g_a),  r_a = g_a - b_a                    (a = x, y, z)
 *   the point is USABLE iff b_a >= 0 and b_a <= n_a - 2 on every axis (compared as float64; a NaN is not usable):
 *   mf_tsdf_raycast's rule for a sample.  A point on the last lattice plane, g_a == n_a - 1 exactly, has b_a = n_a - 1
 *   and is NOT usable, like every point beyond it; one on the first plane, g_a == 0, is.
 *   not usable: rgba = (0, 0, 0, 0).  Otherwise, over the eight corners (b_x + dx, b_y + dy, b_z + dz) in the order of
 *   their codes dx * 4 + dy * 2 + dz = 0 .. 7 (dz fastest), with wx = 1 - r_x at dx = 0 and r_x at dx = 1, wy and wz alike:
 *     w = (wx * wy) * wz;  a corner that is COLOURED adds  S = S + w,  A_c = A_c + w * double(C_c)   (c = r, g, b;
 *     S and A start at 0.0, the corners are added left to right in code order; other corners add nothing)
 *   S > 0:  rgba = (q(A_r / S), q(A_g / S), q(A_b / S), 255)
 *           q(x) = floor(x + 0.5); unless q >= 0: 0; if q > 255: 255; stored as uint8
 *   else:   rgba = (0, 0, 0, 0)       (no coloured corner, or only coloured corners of weight 0)
 * rgba images and lists are uint8 [..][4], 4-byte aligned, byte order r, g, b, a.
 * Refused with -hipErrorInvalidValue (the function's name in mf_last_error_string), on the host and before any launch,
 * unless: nx, ny, nz >= 2 and nx ny nz < 2^31; pitch > 0; truncation > 0; max_weight >= 1; 1 <= H, W <=
 * MF_RENDER_MAX_SIDE; fx, fy > 0; 1 <= N < 2^31; the arrays non-null (skip_flag may be null); colors 16-byte aligned,
 * an rgba `out` 4-byte aligned. */
/* Fuse the colour image of one depth frame into COLOURS.  One lane per voxel (256-lane workgroups over the flat voxel
 * index); if skip_flag is non-null and *skip_flag != 0 no lane does anything.  rgb is uint8 [H][W][3].  A voxel takes
 * the colour of its pixel iff it passes every requirement of mf_tsdf_integrate -- z > 0, (row, col) in range, D > 0,
 * sdf >= -truncation: they depend on the depth, the pose and the geometry alone, so these are the voxels that
 * mf_tsdf_integrate of the same arguments writes -- and sdf <= truncation (sdf = D - z, before the clamp): the band in
 * which mf_tsdf_integrate_labels votes.  With (C_r, C_g, C_b, Wc) the voxel's quadruple, widened, and (row, col) its pixel:
 *   C_c = float32((C_c * Wc + double(rgb[row][col][c])) / (Wc + 1))            (c = r, g, b)
 *   w = Wc + 1, if w > max_weight then w = max_weight, colour weight = float32(w).
 * Any other voxel is not written. */
int mf_tsdf_integrate_colors(float *colors, int32_t nx, int32_t ny, int32_t nz, double origin_x, double origin_y,
                             double origin_z, double pitch, double truncation, double max_weight, const float *depth,
                             const uint8_t *rgb, int32_t H, int32_t W, double fx, double fy, double cx, double cy,
                             const double *T_sensor_to_map, const int32_t *skip_flag, mfStream_t stream);
/* The colour under every pixel of a depth image (e.g. mf_tsdf_raycast's or mf_tsdf_render's depth_out from the same
 * pose).  One lane per pixel (16 x 16 pixel workgroups); out uint8 [H][W][4] is written for EVERY pixel.  Pixel
 * (row, col) with d = double(depth[row][col]):  unless d > 0: (0, 0, 0, 0).  q as in mf_tsdf_raycast, the camera point
 * p = (q_0 * d, q_1 * d, d), m = T_sensor_to_map p, out = SAMPLE(m). */
int mf_tsdf_color_image(const float *colors, int32_t nx, int32_t ny, int32_t nz, double origin_x, double origin_y,
                        double origin_z, double pitch, const float *depth, int32_t H, int32_t W, double fx, double fy,
                        double cx, double cy, const double *T_sensor_to_map, uint8_t *out, mfStream_t stream);
/* The colour at N map-frame points (mesh vertices, instance centres, ICP targets): points float64 [N][3],
 * out uint8 [N][4] := SAMPLE(points[n]).  One lane per point (256-lane workgroups), every row of out is written. */
int mf_tsdf_sample_colors(const float *colors, int32_t nx, int32_t ny, int32_t nz, double origin_x, double origin_y,
                          double origin_z, double pitch, const double *points, int64_t N, uint8_t *out,
                          mfStream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MFHIP_H_ */
