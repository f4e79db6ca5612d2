/*
 * gaddpg.h -- C ABI of libgaddpg.so: the MI355X (gfx950) implementation of GA-DDPG's
 * PointNet++-encoded actor-critic update step.
 *
 * Boundary rules (all entry points):
 *   - extern "C", plain device pointers + sizes, no torch / C++ types.  Every pointer is a DEVICE
 *     pointer unless named host_*.  `stream` is a hipStream_t passed as void* (NULL = default).
 *   - outputs are caller-allocated; no hidden allocation, no host synchronisation, re-entrant,
 *     ordered only by `stream` (same contract as the reference extension, which launches on
 *     at::cuda::getCurrentCUDAStream() without syncing).
 *   - return value: 0 = GAD_OK, <0 = gad_status error (no exceptions cross the ABI).  The Python
 *     binding turns a non-zero status into RuntimeError, mirroring the TORCH_CHECK -> RuntimeError
 *     behaviour of the reference extension's CHECK_* macros.
 *
 * Section A replaces the C++/CUDA extension `pointnet2_ops._ext` that reference core/networks.py:10
 * and core/utils.py:32 reach through pointnet2_ops.pointnet2_utils (upstream bindings.cpp:
 * furthest_point_sampling, gather_points[_grad], ball_query, group_points[_grad], three_nn, three_interpolate[_grad]).
 * Sections B-E are the fused update-step path that sits behind core/networks.py:65-92,182-371,
 * core/ddpg.py:119-185, core/agent.py:127-139,192-259, core/loss.py:17-31 and core/utils.py:750-774.
 */
#ifndef GADDPG_H
#define GADDPG_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    GAD_OK = 0,
    GAD_ERR_NULL = -1,      /* required pointer is NULL                                   */
    GAD_ERR_SHAPE = -2,     /* size / shape outside what the kernels support              */
    GAD_ERR_LAUNCH = -3,    /* hipGetLastError() != hipSuccess after a launch             */
    GAD_ERR_UNSUPPORTED = -4
} gad_status;

int gad_abi_version(void);                 /* bumped on any signature change or new entry point (2: gad_set_option,
                                            * gad_bn_running_update, gad_replay_gather; 3: head pitch in gad_policy_outputs /
                                            * gad_actor_loss, noise type in gad_target_noise, gad_policy_sample;
                                            * 4: max-pool fused into the pooled layer's GEMM (pool_key fields, nullable
                                            * zout, gad_pool_finalize, zmax in gad_pool_bwd_stats); the deferred-BatchNorm
                                            * fields and the slab / graph switches of version 3 are gone;
                                            * 5: gad_gemm_bwd, gad_optim_jobs, gad_last_kernel; 6: gad_gemm_dw_reduce,
                                            * GAD_DW_REDUCE_LATER; 7: trailing BatchNorm blocks of gad_gemm_fwd_args (in_*)
                                            * and gad_dz_src (bn_*, gacc_*), GAD_STAT_REPLICAS 8 -> 4;
                                            * 8: split-bf16 weight mirrors (gad_split_weights; W_split* of gad_gemm_fwd_args,
                                            * W_split_t* of gad_gemm_dx_args), option "mfma_split" as a family mask;
                                            * 9: gad_transpose_batched; 10: gad_stream_priority;
                                            * 11: step replay (section H: gad_plan_*), gad_copy_buffers,
                                            * action_bias in gad_policy_outputs;
                                            * 12: the Adam `hyper` block is GAD_ADAM_HYPER = 10 floats (1 - beta1, 1 - beta2
                                            * appended); added under 12 without a bump (no existing signature or struct
                                            * layout changed): gad_replay_gather_multi, gad_replay_relabel_goals; the
                                            * argument checks of the BatchNorm / pool entry points below (a channel count of 0
                                            * is GAD_OK without a launch, a negative one, a row pitch < C or a count < 1 is
                                            * GAD_ERR_SHAPE): calls that were valid before behave as before; gad_three_nn,
                                            * gad_three_interpolate, gad_three_interpolate_grad (additive: section A now
                                            * covers all nine operators of pointnet2_ops._ext); gad_fps_tiled and
                                            * gad_fps_tiled_workspace_bytes (additive: furthest point sampling without
                                            * the size limits of gad_furthest_point_sampling); gad_ball_query_grid and
                                            * gad_ball_query_grid_workspace_bytes, option "bq_grid" (additive: the radius
                                            * search through a uniform grid in global memory); gad_three_nn_grid and
                                            * gad_three_nn_grid_workspace_bytes, option "tnn_grid" (additive: three_nn
                                            * through the same grid); gad_backproject_depth,
                                            * gad_backproject_depth_workspace_bytes, gad_cloud_gather_affine and
                                            * gad_point_state_pack (additive: section A.2, depth frame -> point state);
                                            * gad_sa_coord_grad (additive: section C, the coordinate columns of a
                                            * set-abstraction stage's first-layer gradient); gad_fp_rows, gad_fp_rows_grad,
                                            * gad_rows_act_out and gad_rows_act_bwd_stats (additive: section C.2, the entry
                                            * and exit of a feature-propagation module on the layer GEMMs)  */
/* diagnostics: which kernel family the last gad_gemm_fwd / _dx / _dw / _bwd call routed to ("gemm_fwd(stream)",
 * "gemm_dx(wide)", "gemm_bwd(stream)", "gemm_dw" = generic tile kernel, ...); bench.py labels its per-kernel table
 * with it instead of restating the routing rules.                                                  */
const char* gad_last_kernel(void);
const char* gad_last_error(void);          /* thread-local description of the last <0   */
/* Kernel-selection switches for A/B diagnostics (defaults in brackets).  "bq_cells" [1]: the LDS cell list of gad_ball_query /
 * gad_query_and_group (0: the tile scan); "bq_grid" [1]: 0 = gad_ball_query_grid runs the scan kernel and the Python routes call
 * gad_ball_query instead of it; 2 = the Python routes send every cloud beyond 4096 points to it instead of those from 262 144
 * points, where it was measured faster (profiles/ball_query_grid.txt) -- same results whatever the value.  "fwd_stream" [1]: route the wide and
 * shallow SA1 forward layers to the streaming kernel instead of the tiled one; "dx_stream" [1]: the same for their dX; "fwd_skinny" / "dx_skinny" / "dw_skinny" [1]: route
 * the small-M (<= 1024 rows) forward / dX / dW layers to the split-K kernels; "skinny_nw" [8]: wavefronts per workgroup of
 * those kernels (8, or 4 = the small-footprint instantiation: A/B in profiles/r05_skinny_footprint.txt); "fwd_stream_wgs" [256] /
 * "fwd_stream_l1_wgs" [256] / "bwd_stream_wgs" [256]: persistent workgroups of the streaming forward (SA1 layers 2 / 3; the gathered
 * layer 1) and of the fused SA1 backward (= its partial dW blocks).  Returns GAD_ERR_SHAPE for an
 * unknown name.  Not part of the numerical contract: both settings satisfy the same parity tests.
 * "mfma_split" [0; the Python package sets GAD_SPLIT_ALL when it loads the library -- its accuracy gates are green on hardware,
 * DESIGN.md section 5 -- a plain C caller gets the f32 MFMA unless it opts in]: the arithmetic of the layer GEMMs' products.
 * Precondition of the non-zero settings: finite operands with |x| < 3.39e38.
 * 0: v_mfma_f32_32x32x2_f32 throughout.  Non-zero: a mask of kernel families that form every FP32 product from split-bf16
 * terms on v_mfma_f32_32x32x16_bf16 with f32 accumulation (GAD_SPLIT_* below; 1 = every family that has the form).  A launch
 * takes the split form only if its family's bit is set AND the call carries the weight mirror it needs (W_split /
 * W_split_t; the streaming SA1 kernels split W themselves); otherwise it runs the FP32-MFMA kernel.
 * "deterministic" [0]: 1 = every entry point either returns a result that is bit-identical whatever the launch grid, the
 * grid-rows hints, the interleaving of streams or the timing, or refuses with GAD_ERR_UNSUPPORTED (gad_gemm_fwd mode 2; a scatter
 * epilogue with more than one group or with previous-layer statistics; gad_sa_coord_grad).  The layer GEMMs take the generic 64 x 64 tile kernels
 * only (no streaming / wide / skinny / split-bf16 family; gad_gemm_bwd = gad_gemm_dw then gad_gemm_dx); grid-rows hints are
 * ignored; per-workgroup partial sums (BatchNorm statistics, dbeta / dgamma, split dW, sums of squares) are stored into slots of
 * a grid-independent index and added by one ordered reduce (slot order, f64) into replica 0 of the statistics or into the arena
 * -- replicas 1..3 receive nothing; the gathered first layer's input gradient is stored per row, then dfeat is accumulated over
 * runs of rows that share no point (found from row_pt / row_grp alone), each run in ascending row order, and daction per sample
 * (row_grp / grp_per_sample, as in the default mode) in ascending row order; gad_group_points_grad / gad_gather_points_grad
 * apply their entries in (m, s) order.  Launches that add into one accumulator must still be ordered by the caller (one
 * stream, or event edges).  The slot and row buffers are library-owned device memory per stream, allocated on first use,
 * grown on demand (a growing call synchronises its stream: do not capture a graph before one uncaptured call per shape) and
 * freed when the option is set back to 0; setting it to 1 allocates nothing.  Results differ from the default mode's by
 * summation order only.                                                                                                      */
#define GAD_SPLIT_ALL 1
#define GAD_SPLIT_FWD_STREAM 2
#define GAD_SPLIT_FWD_WIDE 4
#define GAD_SPLIT_DX_WIDE 8
#define GAD_SPLIT_DW_WIDE 16
#define GAD_SPLIT_BWD_STREAM 32
#define GAD_SPLIT_DW_STREAM 64
int gad_set_option(const char* name, int value);

/* In-kernel launch timing (diagnostics / bench.py roofline): arm `slot` -- device memory, GAD_TIMING_WAVES x {start, end}
 * uint64 pairs, starts initialised to a large value, ends to 0 -- for the NEXT gad_gemm_fwd / gad_gemm_dx / gad_gemm_dw /
 * gad_segment_pool call of this thread.  Every wavefront of that launch stores its own start / end wall-clock stamp (ticks of
 * gad_wall_clock_khz()) into its entry; max(end) - min(start) is the dispatch duration a profiler would report, without
 * tracing and regardless of what other streams do.  Wavefronts beyond GAD_TIMING_WAVES are not recorded.  NULL disarms. */
#define GAD_TIMING_WAVES 16384
int gad_timing_slot(void* slot);
/* Wavefront issue priority of the launches a stream carries (ABI 10).  prio 0..3 (0 = the hardware default; 0 also removes the
 * stream from the table, 8 entries): gad_gemm_fwd / _dx / _dw / _bwd / gad_segment_pool launches on `stream` raise their
 * wavefronts with s_setprio at their first instruction, so that where they share a SIMD with the wavefronts of launches on
 * other streams (the step's weight-gradient lanes, the next step's prefetch) the arbiter issues theirs first.  This is per
 * wavefront, inside the CU -- unlike a HIP stream priority it does not change the queue mapping.  Numerics unaffected.
 * Process-wide; call it before the steps start (not thread-safe against concurrent launches).                              */
int gad_stream_priority(void* stream, int prio);
int gad_wall_clock_khz(void);              /* rate of that clock (hipDeviceAttributeWallClockRate), 0 if unavailable    */

/* Grid-size hint: the layers of SA1 / SA2 run over de-duplicated rows whose count lives on the device (n_rows_dev); the host
 * only knows the worst case (n_rows, 20-40x larger), and a grid sized for it is mostly workgroups that exit at once (~1 ns
 * each: 3-6 us of an SA2 launch).  *rows_host (a HOST int, read at call time) = the number of live rows the caller expects
 * for the NEXT tiled gad_gemm_fwd / gad_gemm_dx launch of this thread; the grid is sized for it.  It is a hint only: the
 * kernels walk the rows in a grid-stride loop bounded by the device count, so any value gives the same result.           */
int gad_grid_rows_hint(const int32_t* rows_host, void* stream);

/* ---------------------------------------------------------------------------------------------
 * A. pointnet2_ops._ext operator parity (materialising, reference API shapes)
 * ------------------------------------------------------------------------------------------- */

/* furthest_point_sampling(xyz (B,N,3) f32, npoint) -> idx (B,M) i32.  Start index 0, points with
 * |p|^2 <= 1e-3 are never selected/updated, arg-max ties resolved as the upstream block reduction
 * does.  new_xyz (B,M,3) is optional (fused gather_operation of the xyz rows).
 * Non-finite and very large coordinates are defined, for this entry point and for gad_fps_tiled alike: the picks are upstream's,
 * where the running minimum is `d < temp ? d : temp` from 1e10f and the arg-max a strict '>'.  A NaN distance (a NaN coordinate,
 * inf - inf) never updates temp and never wins, an infinite or > 1e10 distance leaves temp at 1e10f, and a point whose |p|^2 is
 * NaN is not skipped: so a point with a NaN or infinite coordinate keeps temp = 1e10f in every round and is picked again and
 * again (only a tie at 1e10f can go to another point), and a cloud of huge coordinates (every d^2 > 1e10) is sampled by the tie
 * rule alone.
 * M == 1 writes index 0 (and point 0's row) even where point 0 is skipped as a candidate.  (tests/test_gpu_fps_forms.py)      */
int gad_furthest_point_sampling(const float* xyz, int B, int N, int M, int32_t* idx,
                                float* new_xyz /*nullable*/, void* stream);
/* Limits of the entry point above: one workgroup keeps its whole cloud and the M picks in LDS, so N <= 16384, M <= N and
 * (3N + M + 64) * 4 bytes <= 160 KiB are required (GAD_ERR_SHAPE otherwise).  engine.Geometry of the Python package (the update
 * step and feature_forward) calls it and inherits the limits; the fused set-abstraction modules (sa_function) call gad_fps_tiled
 * for a shape outside them.  Upstream's operator has none of them (npoint > N included):
 *
 * gad_fps_tiled: the same operator -- same start index, skip rule, distance evaluation order and tie rule with
 * tie_bs = pow2 <= min(N, 512), hence the same indices bit for bit -- for any 1 <= N <= 4 194 304 and any M >= 0, M > N included
 * (once every remaining distance is 0 the tie rule alone picks the index, as it does upstream; a cloud whose points are all
 * skipped gives index 0 throughout).  Larger N is GAD_ERR_SHAPE: the arg-max key holds 9 tie bits + 22 index bits.
 * A cloud is cut into `groups` contiguous slices of ceil(N / groups) points, one workgroup each (grid = groups x B);
 * 0 <= groups <= N, 0 = chosen by the library (one slice per 1024 points); the result does not depend on it.  The call enqueues
 * M + 1 launches on `stream` -- one per pick, ordered by the stream alone: no workgroup waits for another inside a launch -- and
 * returns without synchronising.  B == 0 or M == 0: GAD_OK without a launch (workspace may then be NULL).
 * Workspace contract: `workspace` is caller-allocated DEVICE memory of at least gad_fps_tiled_workspace_bytes(B, N, M, groups)
 * bytes, 8-byte aligned, uninitialised on entry, owned by the call until its launches have run on `stream` (two calls in flight
 * on different streams need two workspaces), free to reuse afterwards.  It holds the running minimum distances (B,N) f32
 * -- upstream's `temp` tensor -- and one 64-bit arg-max slot per cloud and pick; the size is >= B*N*4 + B*M*8 and grows with
 * N and M.  gad_fps_tiled_workspace_bytes applies the shape checks of gad_fps_tiled and returns a negative gad_status
 * (message through gad_last_error) where that would refuse.                                                                  */
long long gad_fps_tiled_workspace_bytes(int B, int N, int M, int groups);
int gad_fps_tiled(const float* xyz, int B, int N, int M, int groups, int32_t* idx, float* new_xyz /*nullable*/,
                  void* workspace, void* stream);

/* gather_points(points (B,C,N), idx (B,M)) -> out (B,C,M);  _grad scatters back (zero-fills).  */
int gad_gather_points(const float* points, const int32_t* idx, int B, int C, int N, int M,
                      float* out, void* stream);
int gad_gather_points_grad(const float* grad_out, const int32_t* idx, int B, int C, int N, int M,
                           float* grad_points, void* stream);

/* ball_query(new_xyz (B,M,3), xyz (B,N,3), radius, nsample) -> idx (B,M,nsample) i32: first
 * nsample indices with d2 < radius^2 in ascending order, padded with the first hit, zeros if none.
 * cnt (B,M) (optional) receives the number of distinct hits kept (<= nsample).                  */
int gad_ball_query(const float* new_xyz, const float* xyz, int B, int N, int M, float radius,
                   int nsample, int32_t* idx, int32_t* cnt /*nullable*/, void* stream);
/* Up to 4096 points gad_ball_query keeps the cloud in one workgroup's LDS (a cell list for nsample <= 128, a tile scan for
 * nsample <= 256); every other shape is the scan: one wavefront per centroid walks the cloud from global memory until nsample
 * hits are found -- all N points where the ball holds fewer.
 *
 * gad_ball_query_grid: the same operator, idx and cnt equal to gad_ball_query's bit for bit for every input -- the predicate is
 * d2 = ((dx*dx) + (dy*dy)) + (dz*dz) < radius * radius, every operation rounded in float32, and it decides every candidate --
 * through a uniform grid per cloud in global memory: any N >= 1 and nsample >= 1; it pays for its seven launches from a few
 * hundred thousand points where balls hold fewer than nsample points (profiles/ball_query_grid.txt).  Each cloud's finite
 * points give its bounding box; the grid's resolution is chosen on the device from that box (cell edge >= 1.002 x radius, at
 * most 1024 cells per axis and min(max(N / 4, 64), 65536) per cloud -- a budget the host derives from N alone); a stable counting
 * sort lists the cloud by cell, indices ascending inside a cell; a wavefront per centroid tests the 27 cells around the
 * centroid's and places the nsample smallest hit indices in ascending order.  A centroid outside the box is clamped to a border
 * cell; a point or centroid with a non-finite coordinate is never a hit (such a centroid: zeros, cnt 0); flat clouds and clouds
 * of equal points are legal.  A centroid with more than 512 hits among its candidates is redone by the scan inside the same
 * launch.  radius <= 0, NaN or >= 1e18 (and option "bq_grid" = 0): the call runs gad_ball_query's scan kernel.
 * The call enqueues seven launches on `stream` (bounds, grid set-up, per-slice stable ranks, slice prefix, cell prefix, scatter,
 * query) ordered by the stream alone -- no workgroup waits for another inside a launch, no host synchronisation, no allocation.
 * The sorted cloud does not depend on scheduling: the only atomics are integer adds into counters owned by one wavefront.
 * Workspace contract as for gad_fps_tiled: caller-allocated DEVICE memory of at least
 * gad_ball_query_grid_workspace_bytes(B, N, M, nsample) bytes, 8-byte aligned, uninitialised on entry, owned by the call until
 * its launches have run on `stream`, free to reuse afterwards (also for another shape it is large enough for).  The size grows
 * with N only (about 24 bytes per point plus the cell tables, at most 16 MiB per cloud).  B * M == 0: GAD_OK without a launch
 * (workspace may then be NULL).  GAD_ERR_NULL / GAD_ERR_SHAPE: null pointers, a negative size, N < 1, nsample < 1, a misaligned
 * workspace, 3 * N or B * N beyond 2^31, B * M beyond 2^26 or B beyond 65535; gad_ball_query_grid_workspace_bytes applies the
 * same shape checks and returns the negative gad_status.  Measured against the scan: profiles/ball_query_grid.txt.           */
long long gad_ball_query_grid_workspace_bytes(int B, int N, int M, int nsample);
int gad_ball_query_grid(const float* new_xyz, const float* xyz, int B, int N, int M, float radius, int nsample, int32_t* idx,
                        int32_t* cnt /*nullable*/, void* workspace, void* stream);

/* group_points(points (B,C,N), idx (B,M,S)) -> out (B,C,M,S);  _grad: atomic scatter-add into
 * grad_points (B,C,N), which the call zero-fills first (upstream torch::zeros + atomicAdd).      */
int gad_group_points(const float* points, const int32_t* idx, int B, int C, int N, int M, int S,
                     float* out, void* stream);
int gad_group_points_grad(const float* grad_out, const int32_t* idx, int B, int C, int N, int M,
                          int S, float* grad_points, void* stream);

/* three_nn(unknown (B,n,3), known (B,m,3)) -> dist2 (B,n,3) f32, idx (B,n,3) i32: for every query point the three known points
 * of its sample that are smallest under the order (d, index), listed in ascending order, with
 *   d = ((ux-x)*(ux-x) + (uy-y)*(uy-y)) + (uz-z)*(uz-z)
 * in float32, every operation individually rounded (no FMA contraction): what upstream's three_nn_kernel computes with its
 * sequential strict-< insertion -- ties go to the lower index; a d that is NaN (or +inf) is never selected.  With m < 3 the
 * unfilled slots hold idx = 0 and dist2 = +inf (upstream's 1e40 double stored as a float).  The outputs are SQUARED distances:
 * the square root is taken by the caller (pointnet2_utils.three_nn), as upstream does.  No limit on n or m beyond int32.
 * B * n == 0: GAD_OK without a launch; otherwise m < 1 is GAD_ERR_SHAPE, as is any negative size.                            */
int gad_three_nn(const float* unknown, const float* known, int B, int n, int m, float* dist2, int32_t* idx, void* stream);
/* gad_three_nn costs n * m distance evaluations per cloud (every query lane walks all m known points through LDS tiles).
 *
 * gad_three_nn_grid: the same operator, dist2 and idx equal to gad_three_nn's bit for bit for every input -- the three known points
 * smallest under the total order (d, index), ascending, d evaluated as above for every candidate; a d that is NaN or +inf is never
 * taken, unfilled slots hold (+inf, 0), distances are squared -- through a uniform grid per cloud over the KNOWN points in global
 * memory: any n >= 0 and m >= 1.  Each cloud's finite known points give its bounding box; the cell edge is chosen on the device
 * from that box and a budget of min(max(m / 4, 64), 65536) cells (at most 1024 per axis) that the host derives from m alone: an axis
 * of zero extent gets one cell, a box whose extent overflows ends in one cell; gad_ball_query_grid's stable counting sort lists
 * the known points by cell.  A wavefront per query tests the 3 x 3 x 3 cells around the query's cell (a query outside the box is
 * clamped to a border cell), then the shells of cells around that block, and stops at the first ring after which every
 * unexamined point is provably farther than the current third-best d, strictly (a point at equal d and lower index would win):
 * the bound is the distance to the nearest face of the examined block that is not a border of the grid -- combined, for a query
 * outside the box, with its distance to the box along the other axes -- less the rounding of the cell function and of d
 * (derived in csrc/interpolate.hip), so the test may search one ring too many, never one too few; the search
 * also ends when the block covers the grid (fewer than three finite points, m < 3).  A query with a non-finite coordinate
 * returns (+inf, 0) x 3 without a search.  A query unresolved after 3 rings (far outside the box, in a large void) is redone
 * by an exhaustive walk of its cloud in the same launch: exact, only slower.
 * stats (nullable, (B,2) i32): [b][0] = queries of cloud b answered from the grid (those with a non-finite coordinate included),
 * [b][1] = queries redone exhaustively; [b][0] + [b][1] = n.  The call writes them -- the caller does not clear them -- with
 * integer adds, at most one per counter and wavefront, and only when the pointer is given.
 * The call enqueues seven launches on `stream` (bounds, grid set-up, per-slice stable ranks, slice prefix, cell prefix, scatter,
 * query) ordered by the stream alone -- no workgroup waits for another inside a launch, no host synchronisation, no allocation;
 * every loop is bounded by the grid's dimensions or by m.  There is no float atomic: the outputs do not depend on scheduling and
 * option "deterministic" changes nothing here.  Workspace contract as for gad_fps_tiled: caller-allocated DEVICE memory of at
 * least gad_three_nn_grid_workspace_bytes(B, n, m) bytes, 8-byte aligned, uninitialised on entry, owned by the call until its
 * launches have run on `stream`, free to reuse afterwards (also for another shape it is large enough for).  It holds, per cloud,
 * the bounding-box partials, the grid header, cell (m) i32, rank (m) i32, the per-slice cell counts, the cell starts and the
 * sorted (x, y, z, index) (m) x 16 bytes: the size depends on B and m only, is >= B * m * 24 and grows with m.
 * B * n == 0: GAD_OK without a launch (workspace may then be NULL).  Otherwise GAD_ERR_NULL / GAD_ERR_SHAPE: null pointers, m < 1,
 * a negative size, 3 * m, B * m or B * n beyond 2^31, B beyond 65535, a misaligned workspace;
 * gad_three_nn_grid_workspace_bytes applies the same shape checks and returns the negative gad_status.
 * Option "tnn_grid" [1]: 0 = the entry point runs gad_three_nn's kernel (stats then read [0, n]) and pointnet2_utils.three_nn
 * calls gad_three_nn; 1 = the Python route follows the measured rule (profiles/three_nn_grid.txt); 2 = it sends every shape with
 * m > 1024 (one LDS tile of gad_three_nn) to the grid.  Same results whatever the value.                                      */
long long gad_three_nn_grid_workspace_bytes(int B, int n, int m);
int gad_three_nn_grid(const float* unknown, const float* known, int B, int n, int m, float* dist2, int32_t* idx,
                      int32_t* stats /*nullable, (B,2)*/, void* workspace, void* stream);

/* three_interpolate(points (B,C,m), idx (B,n,3), weight (B,n,3)) -> out (B,C,n):
 *   out[b,c,i] = (w0 * f[idx0] + w1 * f[idx1]) + w2 * f[idx2],   f = points[b,c,:]
 * float32, every operation individually rounded, in that order.  Indices are NOT range-checked (as in gad_group_points): the
 * caller passes 0 <= idx < m.  C == 0 or n == 0: GAD_OK without a launch.
 * _grad: grad_points[b,c,idx[b,i,k]] += grad_out[b,c,i] * weight[b,i,k] over all (i, k).  The call writes EVERY element of
 * grad_points (B,C,m) -- the caller does not clear it.  The adds are f32 atomics in no fixed order (upstream torch::zeros +
 * atomicAdd): in LDS, one workgroup per chunk of rows, for m <= 8192; behind a clearing pass on the stream, in global memory,
 * beyond.  Option "deterministic": every destination is written by one thread that applies its entries in ascending
 * i * 3 + k order, each product rounded before it is added -- bit-equal to a sequential float32 accumulation from 0 in that order,
 * whatever the scheduling, for any m.  Both: m < 1 with B * C * n > 0 is GAD_ERR_SHAPE, as is any negative size.            */
int gad_three_interpolate(const float* points, const int32_t* idx, const float* weight, int B, int C, int m, int n,
                          float* out, void* stream);
int gad_three_interpolate_grad(const float* grad_out, const int32_t* idx, const float* weight, int B, int C, int n, int m,
                               float* grad_points, void* stream);

/* QueryAndGroup in one pass (ball_query + group xyz + recentre + group features + concat):
 * out (B,3+C,M,S) exactly as pointnet2_utils.QueryAndGroup(use_xyz=True) returns it; idx as above.
 * This is the HBM-bound "config 4a" kernel of BASELINE.md.                                       */
int gad_query_and_group(const float* new_xyz, const float* xyz, const float* features /*(B,C,N)*/,
                        int B, int C, int N, int M, float radius, int nsample, int32_t* idx,
                        float* out, void* stream);

/* ---- A.2 observation: depth frame -> point state (reference core/utils.py:308-314, 454-491 and env/panda_scene.py:442-450,
 * 698-714, 1178-1206, host numpy there).  Not operators of pointnet2_ops._ext: they stand in this section because they produce the
 * clouds its operators consume.  An affine `A` is 12 floats, the rows of the 3 x 4 matrix [M | t]: A[4k .. 4k+2] = M[k][0..2],
 * A[4k+3] = t_k (pose[:3, :4] of a 4 x 4 pose, flattened).
 *
 * gad_backproject_depth: depth (B,H,W) row-major, float32 metres (depth_u16 = 0; depth_div is ignored) or uint16 (depth_u16 = 1):
 * d = (float)u / depth_div, one IEEE division (numpy's astype(float32) / 5000).  mask (B,H,W) uint8, nullable (nothing masked).
 * A (B,12).  Pixel p = y * W + x of image b is KEPT iff d != 0 and mask == 0 -- a NaN depth compares unequal to 0 and is kept,
 * as by the reference's test (utils.py:460).  Its point is
 *   r_k = (M[k][0] * x + M[k][1] * y) + M[k][2],    P_k = d * r_k + t_k        (k = 0, 1, 2; x, y as float32, exact)
 * in float32, every operation individually rounded, in that order (no FMA contraction).
 * Outputs: xyz (B, H*W, 3): the kept points of image b, compacted to the front of its block in ascending pixel order -- the order
 * of numpy's boolean mask X[:, mask] -- rows past the count are left untouched; count (B) i32; pix (B, H*W) i32, nullable: the
 * source pixel p of every kept point, rows past the count untouched.  The compaction is stable and does not depend on scheduling:
 * no atomic places a point.  The call enqueues three launches on `stream` (per-tile counts, one workgroup per image scanning its
 * tile counts and writing count[b], scatter) ordered by the stream alone -- no workgroup waits for another inside a launch, no host
 * synchronisation, no allocation.  The inputs must not change between the launches.  Nothing in the images is range-checked:
 * any bit pattern is a legal depth (infinities and NaNs are kept and propagate), any non-zero mask byte masks.
 * Limits: 1 <= H, W <= 4096; B >= 0; B * H * W within 2^31 and B * ceil(H*W / 1024) within 2^23; a uint16 depth needs a finite
 * depth_div > 0; depth aligned to its element size (GAD_ERR_SHAPE otherwise, GAD_ERR_NULL for a null depth / A / xyz / count /
 * workspace).  B == 0: GAD_OK without a launch (every pointer may then be NULL).
 * Workspace contract as for gad_fps_tiled: caller-allocated DEVICE memory of at least gad_backproject_depth_workspace_bytes(B, H, W)
 * bytes (one i32 per tile of 1024 pixels), 8-byte aligned, uninitialised on entry, owned by the call until its launches have run on
 * `stream`, free to reuse afterwards; gad_backproject_depth_workspace_bytes applies the shape checks above and returns the negative
 * gad_status where the call would refuse.                                                                                        */
long long gad_backproject_depth_workspace_bytes(int B, int H, int W);
int gad_backproject_depth(const void* depth, int depth_u16, float depth_div, const uint8_t* mask /*nullable*/, const float* A,
                          int B, int H, int W, float* xyz, int32_t* count, int32_t* pix /*nullable*/, void* workspace,
                          void* stream);
/* gad_cloud_gather_affine: dst[b][j] = M_b . src[b][sel[b][j]] + t_b for j < n (se3_transform_pc of a subsample):
 *   dst_k = ((M[k][0] * x + M[k][1] * y) + M[k][2] * z) + t_k
 * in float32, every operation individually rounded, in that order.  src and dst are point-major (., 3); cloud b starts
 * src_stride / dst_stride FLOATS after cloud b - 1, so a view into a larger buffer is valid for either.  sel (B,n) i32, nullable
 * (identity: sel[b][j] = j); A (B,12), nullable (the points are copied bit for bit).  Indices are NOT range-checked (as in
 * gad_group_points): the caller passes rows that exist in src.  src and dst must not overlap.  B * n == 0: GAD_OK without a launch
 * (src / dst may then be NULL); a negative size or stride, or B * n beyond 2^31, is GAD_ERR_SHAPE.                               */
int gad_cloud_gather_affine(const float* src, int src_stride, const int32_t* sel /*nullable*/, const float* A /*nullable*/, int B,
                            int n, float* dst, int dst_stride, void* stream);
/* gad_point_state_pack: the inverse of gad_prep_points.  state (B, 4, n_lead + n) channel-major f32 (rows x, y, z, flag):
 * columns [0, n_lead) hold the lead points -- lead (n_lead,3) point-major, shared by every sample, copied bit for bit -- with flag
 * lead_flag; column n_lead + j holds M_b . src[b][sel[b][j]] + t_b, src / src_stride / sel / A and the arithmetic as in
 * gad_cloud_gather_affine, with flag 0.  Every element of state is written; stores are contiguous along the point axis.  n == 0
 * writes the lead columns only (src may then be NULL); lead may be NULL when n_lead == 0 (GAD_ERR_NULL otherwise).
 * B * (n_lead + n) == 0: GAD_OK without a launch; a negative size or stride, or B * (n_lead + n) beyond 2^31, is GAD_ERR_SHAPE. */
int gad_point_state_pack(const float* src, int src_stride, const int32_t* sel /*nullable*/, const float* A /*nullable*/,
                         const float* lead /*nullable*/, int n_lead, float lead_flag, int B, int n, float* state, void* stream);

/* ---------------------------------------------------------------------------------------------
 * B. geometry for the fused set-abstraction path (de-duplicated neighbourhood rows)
 * ------------------------------------------------------------------------------------------- */

/* point_state (B,C4,NP) channel-major f32 (rows x,y,z,flag; reference replay layout) ->
 * xyz (B,N,3) and point-major features feat (B*N,4) = [x,y,z,flag], N = NP - skip.              */
int gad_prep_points(const float* point_state, int B, int C4, int NP, int skip, float* xyz,
                    float* feat, void* stream);

/* Compact ball-query output into unique (group, point) rows.  Group g = b*M+m keeps its
 * max(cnt,1) distinct hits; the first hit carries weight nsample-cnt+1 (the padded duplicates).
 * grp_off (G+1) exclusive offsets, row_pt global point index b*Nsrc+j, row_grp = g, row_w weight,
 * n_rows device scalar = grp_off[G].  Deterministic order (g ascending, slot ascending).         */
int gad_rows_from_ball_query(const int32_t* idx, const int32_t* cnt, int G, int M, int Nsrc,
                             int nsample, int32_t* grp_off, int32_t* row_pt, int32_t* row_grp,
                             float* row_w, int32_t* n_rows, void* stream);
/* GroupAll: rows = all points, group = sample (pts_per_group points each), weight 1.            */
int gad_rows_group_all(int G, int pts_per_group, int32_t* grp_off, int32_t* row_pt,
                       int32_t* row_grp, float* row_w, int32_t* n_rows, void* stream);

/* ---------------------------------------------------------------------------------------------
 * C. layer kernels (FP32 MFMA GEMMs with fused producers / epilogues)
 *
 * Weights use the PACKED layout: W (n_out, Kp) row-major, Kp = K rounded up to 8, an optional bias
 * stored as column `ones_col`, zero padding after it.  Activations are row-major (rows, channels).
 * ------------------------------------------------------------------------------------------- */

#define GAD_MAX_GROUPS 3
/* BatchNorm statistic accumulators are replicated: a block adds into replica blockIdx.x % GAD_STAT_REPLICAS (bounds
 * same-address atomic contention); gad_bn_finalize / gad_bn_bwd_coef and the consumers' prologues sum the replicas.
 * 4 since ABI 7 (8 before: every consumer workgroup now reads them; 4 measured +0.5 %, 2 measured -0.2 %).       */
#ifndef GAD_STAT_REPLICAS
#define GAD_STAT_REPLICAS 4
#endif

typedef struct {
    /* rows */
    const int32_t* n_rows_dev; /* device scalar with the live row count, or NULL -> n_rows       */
    int32_t n_rows;            /* static row count (upper bound when n_rows_dev is given)        */
    const float* row_w;        /* (rows) multiplicity weights, NULL -> 1                         */
    /* input mode: 0 = ACT (act(scale*z+shift) of a previous layer's raw output), 1 = GATHER,
     * 2 = ACT recomputed from the gathered first layer (pre_W below)                              */
    int32_t mode;
    const float* zin;          /* ACT: (rows, zin_pitch)                                         */
    int32_t zin_pitch;
    int32_t c_in;              /* ACT: channels read from zin;  GATHER: 3 + feat_c + act_c       */
    const float* scale;        /* ACT: per-channel affine (NULL -> identity)                     */
    const float* shift;
    int32_t relu;              /* ACT: apply max(.,0) after the affine                           */
    const float* extra;        /* ACT: optional extra input column (rows) placed at index c_in   */
    int32_t ones_col;          /* column holding 1.0 (bias), or -1                               */
    /* GATHER: row r = [feat[pt] (feat_c, multiple of 4), src_xyz[pt]-ctr_xyz[grp] (3),
     *                  action[grp/grp_per_sample] (act_c)]  -- PACKED column order (features first so
     *                  they are 16-byte aligned); the host's master->packed map permutes the
     *                  reference's [xyz, features] conv-weight columns accordingly                  */
    const float* src_xyz;      /* (points,3)                                                     */
    const float* ctr_xyz;      /* (groups,3) or NULL (GroupAll: no recentring)                   */
    const float* feat;         /* (points, feat_c) point-major                                   */
    int32_t feat_c;
    const float* action;       /* (samples, act_c) or NULL                                       */
    int32_t act_c;
    int32_t grp_per_sample;
    const int32_t* row_pt;
    const int32_t* row_grp;
    /* groups (blockIdx.z): independent GEMMs sharing the row set (e.g. the three critic trunks) */
    int32_t n_groups;
    int32_t zin_off[GAD_MAX_GROUPS]; /* channel offset into zin (ACT)                            */
    int32_t w_off[GAD_MAX_GROUPS];   /* element offset into W                                    */
    int32_t out_off[GAD_MAX_GROUPS]; /* channel offset into zout / stats                         */
    int32_t n_out[GAD_MAX_GROUPS];
    const float* W;
    int32_t Kp;
    /* outputs */
    float* zout;               /* (rows, zout_pitch) raw pre-activation output (bias included); nullable when the max-pool
                                * is fused (pool_key): a pass that is never back-propagated keeps only the pooled maxima */
    int32_t zout_pitch;
    double* stat_sum;          /* per output channel sum_r w*z and sum_r w*z^2 (f64 atomics),    */
    double* stat_sq;           /*   NULL -> no statistics                                        */
    int32_t stat_stride;       /* elements between the GAD_STAT_REPLICAS replicas of the sums     */
    /* segment max-pool fused into the epilogue (the pooled layer of a set-abstraction stage): per (group, channel) the
     * packed maximum of sgn(gamma) * z over the group's rows, finished by gad_pool_finalize (which also resets the keys).
     * One group, n_out a multiple of 64, rows a multiple of 4.  pool_key == NULL: not used.                            */
    uint64_t* pool_key;        /* (groups, n_out) keys, all 0 before the launch                   */
    const int32_t* pool_row_grp; /* (rows) group index of every row (contiguous runs: CSR order)  */
    const float* pool_gamma;   /* (n_out) BatchNorm weight of THIS layer                          */
    /* train-mode BatchNorm finalisation of the INPUT layer folded into this launch (round 4; in_stat_sum == NULL: not used --
     * scale / shift are read as given).  The launch forms scale / shift of its c_in input channels from that layer's f64
     * statistics (the arithmetic of gad_bn_finalize) in every workgroup's prologue; its FIRST workgroup also publishes them to
     * `scale` / `shift` (written although declared const above), in_mean / in_istd, and applies the running-statistics update.
     * A route that has no such prologue runs gad_bn_finalize on `stream` first: results do not depend on the route.         */
    const double* in_stat_sum; /* (GAD_STAT_REPLICAS, in_stat_stride) sums of the input layer, its first channel */
    const double* in_stat_sq;
    int32_t in_stat_stride;
    double in_count;           /* rows behind the statistics (padded duplicates included)         */
    const float* in_gamma;
    const float* in_beta;
    float in_eps;
    float in_momentum;
    float* in_running_mean;    /* nullable                                                        */
    float* in_running_var;
    float* in_mean;            /* published for the backward pass; nullable                       */
    float* in_istd;
    /* mode 2 (round 4): the 64-channel ACT input is NOT read from zin but recomputed, per 32-row slab, from the gathered rows
     * of the stage's first layer (src_xyz / ctr_xyz / feat / action / row_pt / row_grp as in mode 1) and that layer's packed
     * weights -- the same products in the same order as that layer's own launch, so the values are bit-equal to what it
     * stored -- then activated with scale / shift (or the in_* block) as in mode 0.  A streaming-kernel form only: SA1's
     * rows (feat_c 4, act_c 0 / 6), Kp = c_in = n_out = 64, n_rows >= 32768; anything else is GAD_ERR_SHAPE.            */
    const float* pre_W;        /* (64, pre_Kp) packed weights of the recomputed layer                */
    int32_t pre_Kp;            /* 8 or 16                                                             */
    /* split-bf16 mirror of W (ABI 8; NULL: the launch multiplies on the FP32 MFMA whatever "mfma_split" says): three bf16
     * planes hi | mid | lo written by gad_split_weights, plane p at W_split + p * W_split_plane, row n at + n * W_split_pitch,
     * the first W_split_pitch input columns of every row.  One group only.                                              */
    const uint16_t* W_split;
    int32_t W_split_pitch;     /* bf16 elements per row (= columns mirrored: Kp, or feat_c for a gathered first layer)    */
    int32_t W_split_plane;     /* bf16 elements per plane                                                                  */
} gad_gemm_fwd_args;

int gad_gemm_fwd(const gad_gemm_fwd_args* host_args, void* stream);

/* train-mode BatchNorm finalisation: mean/var from the f64 sums over `count` rows (duplicates
 * included), scale = gamma*istd, shift = beta - mean*scale, running stats momentum update
 * (unbiased variance; count == 1: the biased one), saves mean/istd (nullable) for the backward pass.
 * All the BatchNorm entry points: C == 0 returns GAD_OK without a launch, C < 0 or count < 1 is GAD_ERR_SHAPE.   */
int gad_bn_finalize(const double* stat_sum, const double* stat_sq, int stat_stride, const float* gamma,
                    const float* beta, int C, double count, float eps, float momentum,
                    float* running_mean /*nullable*/, float* running_var /*nullable*/,
                    float* scale, float* shift, float* mean, float* istd, void* stream);
/* eval-mode: scale/shift from the running statistics */
/* momentum update of the running statistics from SAVED batch statistics (mean, istd = 1/sqrt(var_biased+eps)) of a
 * pass whose gad_bn_finalize ran with running_mean = running_var = NULL (a pass overlapped with another pass of the
 * same network on a second stream: the updates are then applied in the reference's order).  count: (C) rows behind
 * each channel's statistics.                                                                                      */
int gad_bn_running_update(const float* mean, const float* istd, const float* count, int C, float eps,
                          float momentum, float* running_mean, float* running_var, void* stream);

int gad_bn_eval_affine(const float* gamma, const float* beta, const float* running_mean,
                       const float* running_var, int C, float eps, float* scale, float* shift,
                       void* stream);

/* segment max-pool over each group's rows of act(scale*z+shift): out (G,C) point-major,
 * argmax (G,C) = global row index of the first maximum (nullable); a group without rows gives 0 and grp_off[g].  C is one of 8, 16, 32, 64, 128, 256, 512, 1024;
 * z_pitch is a multiple of 4 and >= C (anything else: GAD_ERR_SHAPE); scale and shift are both given or both NULL.   */
int gad_segment_pool(const float* z, int z_pitch, int C, const float* scale, const float* shift,
                     const int32_t* grp_off, int G, float* out, int32_t* argmax, void* stream);

/* Finish of the max-pool folded into the pooled layer's GEMM epilogue (gad_gemm_fwd_args.pool_key): finalises that
 * layer's train-mode BatchNorm from its f64 statistics (stat_sum != NULL: same arithmetic and outputs as gad_bn_finalize;
 * running_mean / running_var nullable) or takes scale / shift as given (stat_sum == NULL: eval mode), then per (group,
 * channel): zmax = the winning raw value, out = relu(scale * zmax + shift), argmax = the winner's global row where
 * out > 0, else the group's first row (grp_off[g]); the keys are reset to 0.  argmax / zmax nullable.
 * Replaces upstream's F.max_pool2d over the nsample axis (reference call site core/networks.py:66-81).              */
int gad_pool_finalize(uint64_t* key, int C, int G, const int32_t* grp_off, const double* stat_sum /*nullable*/,
                      const double* stat_sq, int stat_stride, double count, const float* gamma, const float* beta,
                      float eps, float momentum, float* running_mean, float* running_var, float* scale, float* shift,
                      float* mean /*nullable*/, float* istd /*nullable*/, float* out, int32_t* argmax, float* zmax,
                      void* stream);

/* apply act(scale*z+shift) elementwise -> out (rows,C) (used at API boundaries only); z_pitch, out_pitch >= C
 * (GAD_ERR_SHAPE otherwise: rows would overlap); scale == NULL: no affine map                      */
int gad_affine_act(const float* z, int z_pitch, int rows, int C, const float* scale,
                   const float* shift, int relu, float* out, int out_pitch, void* stream);

/* batched 2-D transpose at the operator boundary: dst[b][j][i] = src[b][i][j] for i < R, j < C; rows of src / dst are
 * src_pitch / dst_pitch floats apart, batches src_batch / dst_batch floats (upstream's (B, C, N) channel-major tensors
 * <-> the point-major rows the kernels read: replaces tensor.transpose(1, 2).contiguous() at the pointnet2_ops facade,
 * reference call sites pointnet2_modules.py forward: features (B, C, N) in, new_features (B, C', npoint) out).          */
int gad_transpose_batched(const float* src, float* dst, int B, int R, int C, int src_pitch, long long src_batch,
                          int dst_pitch, long long dst_batch, void* stream);

/* backward source of dY for a layer: dense G (rows,C) or routed from the pooled gradient        */
typedef struct {
    const float* z;            /* (rows, z_pitch) raw output of THIS layer                       */
    int32_t z_pitch;
    const float* scale;        /* this layer's forward affine (mask = scale*z+shift > 0); NULL = identity */
    const float* shift;
    int32_t relu;              /* 0: no activation after this layer (dY = G)                     */
    const float* coefP;        /* BN backward: dZ = P*dY - w*(Q + S*z); NULL -> dZ = dY          */
    const float* coefQ;
    const float* coefS;
    const float* row_w;
    int32_t gmode;             /* 0 dense G, 1 pooled (argmax routing)                           */
    const float* G;            /* dense: (rows, g_pitch)                                         */
    int32_t g_pitch;
    const int32_t* argmax;     /* pooled: (groups, C) global row index                           */
    const float* dout;         /* pooled: (groups, C)                                            */
    const int32_t* row_grp;    /* pooled: (rows)                                                 */
    int32_t c;                 /* channels of this layer (n_out)                                 */
    int32_t premasked;         /* the ReLU mask is already applied to G / dout (dX epilogue with store_masked,
                                * gad_pool_bwd_stats with mask_in_place): `relu`, scale and shift are not needed   */
    /* BatchNorm-backward coefficients formed by the consuming launch itself (round 4; bn_dbeta == NULL: coefP / Q / S are
     * read as given).  Every workgroup of a dX / dW launch forms P, Q, S of the layer's channels from the f64 sums
     * (the arithmetic of gad_bn_bwd_coef: needs `scale`) in its prologue -- no gad_bn_bwd_coef launch in front of it; the
     * launch whose block carries gacc_gamma / gacc_beta adds dgamma / dbeta to the gradient arena (first workgroup; give
     * them to exactly ONE of the launches that consume a layer).  A route without such a prologue runs gad_bn_bwd_coef on
     * `stream` first (coefP / Q / S must then point at scratch for its output).                                          */
    const double* bn_dbeta;    /* (GAD_STAT_REPLICAS, bn_stride) sums of this layer, its first channel */
    const double* bn_dgamma;
    int32_t bn_stride;
    double bn_count;
    const float* bn_mean;
    const float* bn_istd;
    double* gacc_gamma;        /* nullable */
    double* gacc_beta;
} gad_dz_src;

/* pooled-gradient statistics for the BN that feeds a segment pool: dbeta/dgamma f64 sums        */
/* mask_in_place != 0: dout[g][c] is also overwritten with its ReLU-masked value (0 where the arg-max row's
 * activation is not positive), so that the layer's dX / dW can take it as `premasked`.             */
/* zmax (nullable): (G,C) raw value of every arg-max row as saved by gad_pool_finalize -- read instead of gathering
 * z[argmax] (argmax / z may then be NULL).
 * Channels with scale == 0 (gamma == 0): every row of a group ties, so the routed row is the group's FIRST row while zmax
 * holds the value of the key's row.  With argmax and z given next to zmax, x_hat of such a channel is gathered from the
 * routed row, as the reference does.  With zmax alone there is no row to gather: x_hat comes from zmax, so dgamma of a
 * gamma == 0 channel is summed over the key's rows instead of the first rows (dbeta and the mask do not depend on it) --
 * a caller that trains gamma through zero passes argmax and z as well.
 * C: a multiple of 32 that divides 256 or is a multiple of 256.                                      */
int gad_pool_bwd_stats(float* dout, const int32_t* argmax, int G, int C, const float* z,
                       int z_pitch, const float* scale, const float* shift, const float* mean,
                       const float* istd, double* dbeta, double* dgamma, int stat_stride,
                       int mask_in_place, const float* zmax, void* stream);

/* BN backward coefficients from (dbeta,dgamma): P,Q,S above; also accumulates dgamma/dbeta into
 * the f64 gradient arena slots gacc_gamma/gacc_beta (nullable).  count >= 1 (GAD_ERR_SHAPE otherwise).   */
int gad_bn_bwd_coef(const double* dbeta, const double* dgamma, int stat_stride, const float* scale,
                    const float* mean, const float* istd, int C, double count, float* coefP,
                    float* coefQ, float* coefS, double* gacc_gamma, double* gacc_beta,
                    void* stream);

typedef struct {
    const int32_t* n_rows_dev;
    int32_t n_rows;
    gad_dz_src dz;
    int32_t n_groups;
    int32_t dz_off[GAD_MAX_GROUPS];  /* channel offset of the group inside dz (z, G, coef)       */
    int32_t w_off[GAD_MAX_GROUPS];
    int32_t n_out[GAD_MAX_GROUPS];
    int32_t gout_off[GAD_MAX_GROUPS];/* channel offset into gout                                  */
    int32_t accumulate;              /* reserved: groups adding into the same gout columns (shared input) is NOT implemented --
                                      * every group stores its own columns [gout_off, gout_off + k_valid).  Must be 0 with more
                                      * than one group (GAD_ERR_UNSUPPORTED otherwise); ignored with one group.  A layer whose
                                      * groups share their input runs as one concatenated group instead (the critic's first) */
    const float* W;
    int32_t Kp;
    int32_t k_valid;                 /* input channels to produce (columns >= k_valid are skipped)*/
    /* epilogue 0: store gout (rows, gout_pitch)                                                  */
    int32_t epilogue;
    float* gout;
    int32_t gout_pitch;
    /* epilogue 0 + statistics for the PREVIOUS layer's BN backward (nullable)                    */
    const float* zprev; int32_t zprev_pitch;
    const float* prev_scale; const float* prev_shift; const float* prev_mean; const float* prev_istd;
    double* prev_dbeta; double* prev_dgamma; int32_t stat_stride;
    int32_t store_masked;            /* with prev statistics: gout receives the ReLU-masked gradient (dY where the previous
                                      * layer's activation is positive, else 0) -> its consumer's dz is `premasked`    */
    /* epilogue 1: gather-layer scatter (packed column order): columns [0,feat_c) atomically added to
     * dfeat[row_pt], columns [feat_c+3, feat_c+3+act_c) to daction[row_grp/grp_per_sample] (f64:
     * the per-sample action gradient is a sum of many cancelling terms)                            */
    float* dfeat; int32_t feat_c; const int32_t* row_pt; const int32_t* row_grp;
    double* daction; int32_t act_c; int32_t grp_per_sample;
    /* split-bf16 mirror of W^T (ABI 8; NULL: FP32 MFMA): planes hi | mid | lo of W_split_t_plane bf16 elements, row k (input
     * channel) at + k * W_split_t_pitch, columns = the layer's n_out output channels (gad_split_weights).  One group only. */
    const uint16_t* W_split_t;
    int32_t W_split_t_pitch;
    int32_t W_split_t_plane;
} gad_gemm_dx_args;

int gad_gemm_dx(const gad_gemm_dx_args* host_args, void* stream);

typedef struct {
    gad_gemm_fwd_args in;      /* describes how the layer's INPUT rows are produced (W/zout unused) */
    gad_dz_src dz;
    int32_t dz_off[GAD_MAX_GROUPS];
    double* gacc;              /* f64 gradient arena, packed layout; group g at gacc + in.w_off[g]; ADDED to */
    int32_t row_splits;        /* rows are divided over this many blocks (0 -> auto): block s of the generic tile kernels takes
                                * the live rows [s * chunk, (s + 1) * chunk), chunk = ceil(ceil(live / row_splits) / 32) * 32
                                * (blocks past the live rows add nothing).  The deterministic mode's order is defined by this
                                * rule: the arena receives the blocks' partial sums in block order (see "deterministic")        */
    float* partial;            /* caller workspace for the per-split partial tiles (NULL -> f64 atomics) */
    int64_t partial_elems;     /* capacity of `partial` in floats                                   */
} gad_gemm_dw_args;

int gad_gemm_dw(const gad_gemm_dw_args* host_args, void* stream);

/* dX and dW of ONE layer in one call: `dx` and `dw` describe the same layer (same gradient source; dw->in = the layer
 * dx writes the gradient of).  The SA1 layers of the update step (>= 32768 rows, 64 input channels, 64 / 128 outputs,
 * BatchNorm+ReLU on both sides: reference core/networks.py:29-51 through pointnet2's SharedMLP) run as one streaming
 * pass that reads z / dY / z_prev once for both products; any other layer runs gad_gemm_dw then gad_gemm_dx on
 * `stream`.  Results are those of the two separate calls (dW: f32 partial sums per workgroup, f64 across them).
 * Round 4: the mid-size layers (SA2 / SA3: >= 2048 rows, 128 / 256 / 512 outputs, K a multiple of 64, incl. the gathered
 * first layers with their scatter epilogue) are fused as well (gemm_bwd_wide_kernel): one staged dZ tile feeds the dX and
 * the dW product.  The fused kernels leave one partial dW block per workgroup in dw->partial and a reduce launch sums
 * them into the arena: on `stream` right behind the kernel, or -- dw->row_splits == GAD_DW_REDUCE_LATER -- by the caller's
 * own gad_gemm_dw_reduce(dx, dw, other_stream) once `other_stream` waits for the kernel, which takes the reduce off the
 * dX chain (the workspace must then stay untouched until that launch has run).                                          */
#define GAD_DW_REDUCE_LATER (-2)
int gad_gemm_bwd(const gad_gemm_dx_args* dx, const gad_gemm_dw_args* dw, void* stream);
/* the deferred reduce of a gad_gemm_bwd(dx, dw) call made with GAD_DW_REDUCE_LATER (same argument blocks); a no-op for a
 * layer gad_gemm_bwd does not fuse (its dW was reduced by that call).                                                     */
int gad_gemm_dw_reduce(const gad_gemm_dx_args* dx, const gad_gemm_dw_args* dw, void* stream);

/* Coordinate gradient of a set-abstraction stage's gathered first layer (additive under ABI 12): the three packed columns
 * [col0, col0 + 3) = src_xyz[pt] - ctr_xyz[grp] that gad_gemm_dx's scatter epilogue (epilogue 1) skips between dfeat and daction.
 * Upstream reaches them through grouping_operation / gather_operation's backward (pointnet2_modules.py: grouped_xyz - new_xyz
 * enters the first 1x1 convolution, new_xyz is a gather of xyz); a caller that trains something in front of the coordinates
 * asks for them, GA-DDPG does not.
 *   dz      HOST pointer to the layer's gradient source exactly as its gad_gemm_dx call carries it: gmode 0 with a dense G
 *           (rows, g_pitch) that holds the ReLU mask already (premasked, or relu == 0), z (rows, z_pitch), coefP / Q / S given
 *           together (or all NULL: dZ = G, z is not read), row_w (NULL -> 1), c == n_out.  The bn_* block must be unset.
 *           Anything else: GAD_ERR_NULL / GAD_ERR_SHAPE / GAD_ERR_UNSUPPORTED before any launch.
 *   W       (n_out, Kp) packed f32 weights of the layer; col0 = its first coordinate column (= feat_c); Kp >= col0 + 3,
 *           1 <= n_out <= 1024.  Only columns col0 .. col0 + 2 are read.
 *   rows    n_rows static count, n_rows_dev (nullable -> n_rows) the live count on the device: rows at or beyond
 *           min(*n_rows_dev, n_rows) are never read.  row_pt (rows) global point number; row_grp (rows) group number with
 *           the rows of a group contiguous, or NULL for the GroupAll form (no recentring: no centroid terms).
 *   ctr_pt  (n_groups) global point number of every group's centroid (b * N + fps index); given exactly when row_grp is.
 *   g_new_xyz (n_groups, 3) incoming gradient of new_xyz, nullable (needs ctr_pt).
 *   dxyz    (n_points, 3) f32, ADDED to (as dfeat is): the caller clears it.  dctr (n_groups, 3) f32 scratch, required with
 *           row_grp: the caller clears it as well; on return it holds the per-group sums of t.
 * Arithmetic, f32 throughout: dZ[r][c] = P[c] * G[r][c] - w[r] * fmaf(S[c], z[r][c], Q[c]) -- the expression of gad_gemm_dx /
 * gad_gemm_dw -- then t[r][k] = sum_c dZ[r][c] * W[c * Kp + col0 + k] for k = 0..2;  dxyz[row_pt[r]][k] += t[r][k];
 * dctr[row_grp[r]][k] += t[r][k] (summed per run of equal row_grp inside a wavefront first); then a second launch, ordered
 * behind the first on `stream`: dxyz[ctr_pt[g]][k] += g_new_xyz[g][k] - dctr[g][k].  Every add is a float atomic (several
 * groups may share a centroid point; a point that is its own centroid receives both terms): the sums' order, hence their last
 * bits, vary from run to run.  A row whose point number is outside [0, n_points), a group number outside [0, n_groups) and a
 * centroid outside [0, n_points) are skipped, never written through.
 * n_rows == 0 or n_groups == 0: GAD_OK without a launch.  Option "deterministic": GAD_ERR_UNSUPPORTED (no ordered form).
 * Two launches; no workspace, no host synchronisation.                                                                   */
int gad_sa_coord_grad(const gad_dz_src* dz, const float* W, int Kp, int n_out, int col0, const int32_t* n_rows_dev,
                      int n_rows, const int32_t* row_pt, const int32_t* row_grp /*nullable*/,
                      const int32_t* ctr_pt /*nullable*/, const float* g_new_xyz /*nullable*/, int n_groups, int n_points,
                      float* dxyz, float* dctr /*nullable*/, void* stream);

/* ---- C.2 feature propagation on the layer GEMMs (additive under ABI 12) ----
 * A PointnetFPModule (upstream pointnet2_modules.py: three_interpolate -> torch.cat -> SharedMLP) is a stack of dense-row layers:
 * gad_gemm_fwd / _dx / _dw with n_rows_dev = row_w = NULL run them, the first with an identity input (mode 0, scale = NULL,
 * relu 0).  These four entry points stand where the gather and the max-pool stand for a set-abstraction stage: the row matrix
 * at the entry and its gradient, the activation at the exit and its gradient statistics.  Each takes the caller's stream,
 * allocates nothing, never synchronises the host; a zero-sized shape is GAD_OK without a launch.
 *
 * gad_fp_rows: three_interpolate written as GEMM input rows.  known_pm (B * m, k_pitch) point-major features of the known
 *   points, idx / weight (B, n, 3) of gad_three_nn and the caller's inverse-distance weights;
 *   rows[b * n + i][col_off + c] = (w0 * f[j0][c] + w1 * f[j1][c]) + w2 * f[j2][c] for c < C2, every product and sum rounded on its
 *   own: gad_three_interpolate's output, transposed, bit for bit.  Columns outside [col_off, col_off + C2) are not written.
 *   Indices are not range-checked (as for gad_three_interpolate).  16-byte accesses where C2, k_pitch, r_pitch, col_off are
 *   multiples of 4 and both base addresses 16-byte aligned, 4-byte ones otherwise.  k_pitch >= C2 and col_off + C2 <= r_pitch
 *   (GAD_ERR_SHAPE otherwise), m >= 1 unless there is nothing to write.
 * gad_fp_rows_grad: its gradient, gknown_pm[b * m + j_k][c] += w_k * drows[b * n + i][col_off + c] with float atomics into a
 *   buffer the caller cleared; an element no entry reaches stays exactly 0.  Option "deterministic": GAD_ERR_UNSUPPORTED before
 *   any launch (nothing is written) -- the caller transposes drows and takes gad_three_interpolate_grad's ordered form.        */
int gad_fp_rows(const float* known_pm, int k_pitch, const int32_t* idx, const float* weight, int B, int n, int m, int C2,
                float* rows, int r_pitch, int col_off, void* stream);
int gad_fp_rows_grad(const float* drows, int r_pitch, int col_off, const int32_t* idx, const float* weight, int B, int n, int m,
                     int C2, float* gknown_pm, int k_pitch, void* stream);
/* gad_rows_act_out: the module's output, out (B, C, n) channel-major = relu(fma(z, scale, shift)) of the last layer's raw
 *   z (B * n, z_pitch): gad_affine_act's arithmetic with the transpose folded in (an LDS tile: both sides coalesced).
 *   Any C >= 0, z_pitch >= C.
 * gad_rows_act_bwd_stats: the top of the backward.  dout (B, C, n) channel-major; G (B * n, g_pitch) row-major = dout where
 *   fma(z, scale, shift) > 0, else 0 (the layer's dX / dW take it as `premasked`); dbeta[c] += sum_r G[r][c],
 *   dgamma[c] += sum_r G[r][c] * (z[r][c] - mean[c]) * istd[c], f64 sums into the GAD_STAT_REPLICAS replicas stat_stride
 *   doubles apart (what gad_pool_bwd_stats with mask_in_place gives a pooled layer whose every row is its own group).
 *   Any C >= 0, z_pitch and g_pitch >= C, stat_stride >= C.  Option "deterministic": per-workgroup sums stored into slots of
 *   a grid that depends on (B, n, C) alone and added in slot order into replica 0 (two calls are bit-identical).              */
int gad_rows_act_out(const float* z, int z_pitch, const float* scale, const float* shift, int B, int n, int C, float* out,
                     void* stream);
int gad_rows_act_bwd_stats(const float* dout, const float* z, int z_pitch, const float* scale, const float* shift,
                           const float* mean, const float* istd, int B, int n, int C, float* G, int g_pitch, double* dbeta,
                           double* dgamma, int stat_stride, void* stream);

/* ---------------------------------------------------------------------------------------------
 * D. heads' losses (forward value + gradient wrt head outputs in one pass)
 * ------------------------------------------------------------------------------------------- */

/* Critic phase (core/ddpg.py:61-88,119-130): TD3 target y = r + (1-done)*gamma*min(q1t,q2t),
 * masked smooth-L1 on both Q heads, control-point L1 on the quaternion-normalised aux head.
 *   out9 (B,9) raw head outputs [q1, q2, aux7];  tgt_out9 (B,9) target-critic raw outputs.
 *   g_out9 (B,9) receives dLoss/d(out9).  scalars[0]=critic_loss, [1]=critic_grasp_aux_loss,
 *   [2]=#kept, [3]=#goal rows.  inv_n_* (nullable device scalars) override 1/count with a
 *   globally reduced value for data-parallel runs.                                               */
int gad_critic_loss(const float* out9, const float* tgt_out9, const float* reward,
                    const float* done, const float* perturb_flag, const float* ret,
                    const float* goal, int B, float gamma, int critic_aux, const float* inv_n,
                    float* y, float* aux_norm, float* g_out9, float* scalars, void* stream);

/* Actor phase (core/agent.py:127-139, core/ddpg.py:169-177, core/loss.py): outputs of the policy
 * head pol13 (B,13) = [mean6 raw, extra7 raw].  pi = tanh(mean)*scale + bias (core/networks.py:329-337, 359: action_bias =
 * (high + low) / 2 of the action space; ABI 11: nullable `action_bias`, NULL = symmetric bounds).  bc_loss over expert rows
 * scaled by bc_scale, goal aux over return>0 rows, and (optional) the gradient of
 * -ratio*mean(min(q1_pi,q2_pi)) wrt pi arriving as g_pi_critic (B,6) (already scaled).
 *   g_pol13 receives dLoss/d(pol13); scalars[0]=bc_loss (scaled), [1]=policy_grasp_aux_loss.     */
/* `pitch` = floats per row of the head output / gradient buffers: 6 + extra_pred_dim (13 with policy_aux, 7
 * without: reference core/agent.py:31-36); aux_norm / policy_aux need pitch >= 13.  gad_actor_loss writes every column
 * of g_pol13 for every row: columns without a loss term (6 .. pitch-1 without policy_aux or on rows with return <= 0,
 * 13 .. pitch-1 with it) receive 0, so a pitch above 13 is accepted and its extra columns are zeroed.  The chain into
 * the raw means is scale * (1 - tanh(mean)^2), taken from pol13 (not from pi, which carries the bias).            */
int gad_policy_outputs(const float* pol13, int B, int pitch, const float* action_scale, const float* action_bias /*nullable*/,
                       float* pi, float* aux_norm /*nullable*/, void* stream);
int gad_actor_loss(const float* pol13, const float* pi, const float* expert_action,
                   const float* expert_flag, const float* ret, const float* goal, int B, int pitch,
                   float bc_scale, int policy_aux, const float* action_scale,
                   const double* g_pi_critic /*nullable*/, const float* inv_n, float* g_pol13,
                   float* scalars, void* stream);
/* GaussianPolicy.forward + sample (core/networks.py:339-371) on the raw head outputs head (B,pitch) =
 * [mean 6 | extra extra_dim | log_std 6]: log_std (B,6) clamped to [-10,2]; x = mean + exp(log_std)*eps with the
 * caller's N(0,1) draw eps (B,6) (NULL -> 0); squash != 0: action = tanh(x)*scale+bias, mean_sq = tanh(mean)*scale+bias;
 * log_prob (B) = sum_c N(x; mean, std).log_prob - log(scale*(1-tanh(x)^2)+1e-6); extra (B,extra_dim) with the
 * quaternion part normalised when extra_dim == 7.  Every output is nullable.                      */
int gad_policy_sample(const float* head, int B, int pitch, int extra_dim, const float* eps /*nullable*/,
                      const float* action_scale /*nullable: 1*/, const float* action_bias /*nullable: 0*/, int squash,
                      float* mean_sq, float* log_std, float* log_prob, float* action, float* extra, void* stream);
/* -ratio * mean over rows NOT (expert & return>0) of min(q1,q2): value + dLoss/d(out9[:, :2])    */
int gad_actor_critic_loss(const float* out9, const float* expert_flag, const float* ret, int B,
                          float ratio, const float* inv_n, float* g_out9, float* scalars,
                          void* stream);
/* local mask counts of a minibatch as doubles: out4 = [#(perturb < 1), #(return > 0), #(expert >= 1), #not(expert & reward)]
 * (core/agent.py:224-229): what the masked means divide by; a data-parallel run sums them over the ranks.            */
int gad_mask_counts(const float* ret, const float* expert_flag, const float* perturb_flag, int B, double* out4,
                    void* stream);
/* TD3 target-policy smoothing (core/utils.py:568-576 + core/ddpg.py:80-82, quirk preserved):
 * normal == 0 (noise_type "uniform"): u ~ U[0,1): a = pi + clamp3(((u*3-6)*level) * [1,1,1,5,5,5])
 * normal != 0 (any other noise_type):  u ~ N(0,1): a = pi + clamp3((u*level/2) * [1,1,1,5,5,5])    */
int gad_target_noise(const float* pi, const float* u, int B, float level, int normal, float* out,
                     void* stream);

/* ---------------------------------------------------------------------------------------------
 * E. optimiser / bookkeeping over flat parameter buffers
 * ------------------------------------------------------------------------------------------- */

/* grad[i] = (float) gacc[m2p[i]] for the n master parameters (m2p[i] < 0 -> 0); accumulate != 0
 * adds to the existing grad instead (a second backward into the same .grad, as autograd does).   */
int gad_grad_from_arena(const double* gacc, const int32_t* m2p, int n, float* grad, int accumulate,
                        void* stream);
/* the same conversion + the sum of squares of the resulting gradient atomically added to *sumsq (f64; zero it first):
 * gad_grad_from_arena followed by gad_sumsq in one launch (the critic phase: clip_grad_norm_'s total norm)                 */
int gad_grad_from_arena_sumsq(const double* gacc, const int32_t* m2p, int n, float* grad, int accumulate, double* sumsq,
                              void* stream);
/* sum of squares of grad[0..n) into *out (f64, atomically accumulated; zero it first)           */
int gad_sumsq(const float* grad, int n, double* out, void* stream);
/* max |x| over segments: out[s] = max |x[seg_off[s] .. seg_off[s+1])| (0 for an empty segment; NaN if the segment holds a
 * NaN, as torch.abs(x).max() reports it)                                                        */
int gad_absmax_segments(const float* x, const int32_t* seg_off, int n_seg, float* out,
                        void* stream);
/* Adam with L2 weight decay folded into the gradient (torch.optim.Adam, amsgrad=False), over a
 * flat buffer; `hyper` is a device array of GAD_ADAM_HYPER floats {lr, beta1, beta2, eps, weight_decay, bias_c1 =
 * 1 - beta1^t, bias_c2 = sqrt(1 - beta2^t), grad_scale, 1 - beta1, 1 - beta2}, each formed in double on the host and
 * rounded once (1 - beta is NOT derived from the rounded beta on the device: 1.f - float(0.999) is 1.29e-5 off
 * float(0.001)); active[i]==0 skips an element (parameters that never receive a gradient);
 * clip_sumsq/clip_max (nullable) apply clip_grad_norm_ on the fly:
 *   g *= min(1, clip_max / (sqrt(*clip_sumsq) + 1e-6)).
 * Updated values are written to the master buffer p and mirrored into the packed compute buffer
 * packed[m2p[i]].                                                                               */
#define GAD_ADAM_HYPER 10
int gad_adam_step(float* p, const float* grad, float* exp_avg, float* exp_avg_sq,
                  const uint8_t* active, const int32_t* m2p, float* packed, int n,
                  const float* hyper, const double* clip_sumsq, float clip_max, void* stream);
/* target <- (1-tau)*target + tau*source where sel[i]==1, target <- source where sel[i]==2        */
int gad_polyak(float* target, const float* source, const uint8_t* sel, const int32_t* m2p,
               float* target_packed, int n, float tau, int hard_enable, void* stream);
/* One launch for a whole optimiser phase: each job is one flat buffer and, optionally and in this order per element:
 * .grad <- gradient arena (gad_grad_from_arena), Adam step with clip scaling and packed mirror (gad_adam_step; hyper ==
 * NULL: none), target-network update FROM THE UPDATED parameter (gad_polyak; target == NULL: none), max |p| / max |grad|
 * atomically maximised into absmax_p / absmax_grad (GAD_ABSMAX_SLOTS floats each, float bits, zeroed by the caller,
 * who takes the maximum of the slots; max |p| over every element, max |grad| over the elements with active != 0 -- the
 * reference's module_max_gradient counts a parameter without .grad as 0; a NaN element is reported as NaN, its bit pattern
 * being the largest), and counter[0..counter_n) += counter_add once per launch (BatchNorm num_batches_tracked).
 * Same arithmetic as the single-purpose entry points: bit-identical results (tests/test_gpu_optim_kernels.py).  Alignment: p, grad, exp_avg, exp_avg_sq, m2p, target, target_m2p 16 bytes;
 * active, target_sel 4 bytes (four elements per access; GAD_ERR_SHAPE otherwise).                                       */
#define GAD_MAX_OPTIM_JOBS 4
#define GAD_ABSMAX_SLOTS 8
typedef struct {
    int32_t n;
    float* p; float* grad; float* exp_avg; float* exp_avg_sq; const uint8_t* active; const int32_t* m2p; float* packed;
    const double* gacc; int32_t accumulate;
    const float* hyper; const double* clip_sumsq; float clip_max;
    float* target; const uint8_t* target_sel; const int32_t* target_m2p; float* target_packed; float tau; int32_t hard_enable;
    float* absmax_p; float* absmax_grad;
    int64_t* counter; int32_t counter_n; int32_t counter_add;
} gad_optim_job;
int gad_optim_jobs(const gad_optim_job* host_jobs, int n_jobs, void* stream);

/* packed[m2p[i]] = p[i] (refresh the compute layout after an external parameter change)          */
int gad_pack_params(const float* p, const int32_t* m2p, int n, float* packed, void* stream);

/* Split-bf16 mirrors of packed weight matrices (ABI 8; the arithmetic behind option "mfma_split": every FP32 product is
 * formed as the six leading bf16 x bf16 term products of hi + mid + lo splits -- 24 significand bits -- accumulated in f32 by
 * v_mfma_f32_32x32x16_bf16).  For each layer, from its packed f32 weights W (n_out, Kp) at packed + w_off, the first Ks
 * columns (Ks a multiple of 32):
 *   forward mirror   out + fwd_off: planes hi | mid | lo of n_out * Ks bf16, row n, column k  (reduction index k contiguous)
 *   transposed mirror out + t_off : planes hi | mid | lo of Ks * n_out bf16, row k, column n  (reduction index n contiguous)
 * (n_out, Kp and the three offsets multiples of 4: the kernel moves 8-byte groups of four bf16)
 * hi = bf16(w), mid = bf16(w - hi), lo = bf16(w - hi - mid) (round to nearest even; the residuals are exact), and every
 * value whose REDUCTION index lies in an odd block of 16 is stored NEGATED: the kernels add those blocks' products into a
 * second accumulator and subtract it, which cancels the bf16 MFMA adder's truncation bias.  Call it whenever
 * `packed` changes (after gad_pack_params / gad_adam_step / gad_optim_jobs) for networks whose launches carry W_split*. */
#define GAD_MAX_SPLIT_LAYERS 16
typedef struct {
    int32_t w_off;             /* element offset of the layer's weights in `packed`                 */
    int32_t n_out;
    int32_t Kp;                /* row pitch of the packed weights                                   */
    int32_t Ks;                /* leading columns mirrored (multiple of 32, <= Kp)                  */
    int64_t fwd_off;           /* bf16-element offsets into `out`                                   */
    int64_t t_off;
} gad_split_layer;
int gad_split_weights(const float* packed, const gad_split_layer* host_layers, int n_layers, uint16_t* out, void* stream);

/* ---------------------------------------------------------------------------------------------
 * F. replay minibatch gather (the step before the path: reference core/replay_memory.py:109-127,251-272 run as a
 *    device-side index gather over a GPU-resident float32 mirror of the buffer; the index arithmetic -- draw,
 *    successor index, episode end -- stays on the host and is the reference's).  One launch fills the update
 *    step's input buffers: out_*[b] = src[idx[b]], next cloud = point_state[nxt[b]],
 *    time[b] = timestep[end[b]] + 1 - timestep[idx[b]], time_m1 = time - 1.
 *    gad_replay_gather reads one buffer; gad_replay_gather_multi fills the same outputs from up to four buffers (the
 *    expert + online minibatch of the reference's learner), each block of output rows from its own source, and folds the
 *    hindsight-goal overwrite into the launch (goals formed on the host); gad_replay_relabel_goals forms those goals on the
 *    device instead, in a launch of its own behind either gather.
 * ------------------------------------------------------------------------------------------- */
typedef struct {
    int32_t B;
    int32_t cloud_elems;                 /* floats per transition of point_state (4 * 1030), multiple of 2 */
    const int64_t* idx; const int64_t* nxt; const int64_t* end;           /* (B) device index vectors */
    const float* point_state;            /* (cap, cloud_elems) */
    const float* action; const float* expert_action;                      /* (cap, 6) */
    const float* goal;                   /* (cap, 7) */
    const float* reward; const float* returns; const float* terminal; const float* timestep;
    const float* expert_flags; const float* perturb_flags;                /* (cap) */
    float* out_point; float* out_next_point;                              /* (B, cloud_elems) */
    float* out_action; float* out_expert_action; float* out_goal;
    float* out_reward; float* out_return; float* out_mask; float* out_time; float* out_time_m1;
    float* out_expert_flag; float* out_perturb_flag;
} gad_replay_gather_args;

int gad_replay_gather(const gad_replay_gather_args* host_args, void* stream);

/* The same gather from up to GAD_REPLAY_MAX_SRC device-resident buffers in ONE launch: the reference's learner draws
 * batch_size rows from the expert buffer and int(batch_size * online_buffer_ratio) rows from the online buffer and
 * concatenates them key by key, expert rows first (core/trainer.py:212-232).  Output row b belongs to source s with
 * row_start[s] <= b < row_start[s + 1] (row_start[0] = 0, non-decreasing, row_start[n_src] = B); idx[b], nxt[b] and end[b]
 * are indices LOCAL to that source (end indexes its timestep).  A source that owns no row is never read and may be all NULL.
 * All sources share cloud_elems.  Per-row arithmetic is gad_replay_gather's (time = timestep[end] + 1 - timestep[idx],
 * time_m1 = time - 1); with n_src = 1 and relabel = NULL the outputs are bit-identical to it.
 * relabel: NULL, or (B, 8) float32 rows [goal (7) | flag]: out_goal[b] = relabel[b, 0:7] where relabel[b, 7] > 0, else the
 * gathered goal (the hindsight goals of reference core/replay_memory.py:233-249, formed on the host).
 * Clouds move as 16-byte groups when cloud_elems % 4 == 0 and out_point, out_next_point and the point_state of every source
 * that owns a row are 16-byte aligned, as 8-byte pairs otherwise (chosen per launch on the host; same bytes either way).
 * Refused before any launch: NULL args (GAD_ERR_NULL); n_src outside 1..GAD_REPLAY_MAX_SRC, B outside 1..65535, cloud_elems
 * odd or < 2, a row_start that does not run 0 .. B without decreasing (GAD_ERR_SHAPE); a NULL index vector, a NULL output other
 * than out_next_point, a NULL pointer in a source that owns a row (GAD_ERR_NULL). */
#define GAD_REPLAY_MAX_SRC 4
typedef struct {
    const float* point_state;            /* (cap, cloud_elems) */
    const float* action; const float* expert_action;                      /* (cap, 6) */
    const float* goal;                   /* (cap, 7) */
    const float* reward; const float* returns; const float* terminal; const float* timestep;
    const float* expert_flags; const float* perturb_flags;                /* (cap) */
} gad_replay_src;
typedef struct {
    int32_t B;                           /* output rows = sum of the sources' shares */
    int32_t cloud_elems;                 /* floats per transition of point_state, multiple of 2; the same for every source */
    int32_t n_src;
    int32_t row_start[GAD_REPLAY_MAX_SRC + 1];
    gad_replay_src src[GAD_REPLAY_MAX_SRC];
    const int64_t* idx; const int64_t* nxt; const int64_t* end;           /* (B) device index vectors, source-local */
    const float* relabel;                /* (B, 8) or NULL */
    float* out_point; float* out_next_point;                              /* (B, cloud_elems); out_next_point may be NULL */
    float* out_action; float* out_expert_action; float* out_goal;
    float* out_reward; float* out_return; float* out_mask; float* out_time; float* out_time_m1;
    float* out_expert_flag; float* out_perturb_flag;
} gad_replay_mix_args;

int gad_replay_gather_multi(const gad_replay_mix_args* host_args, void* stream);

/* Hindsight goals formed on the device (reference core/replay_memory.py:233-249: the goal of an on-policy row becomes the pose
 * its own episode ended in, seen from the row's pose).  Runs on the gather's stream AFTER the gather that wrote out_goal and
 * updates it in place.  B, n_src and row_start have gad_replay_gather_multi's meaning; idx[b] and end[b] are local to the
 * source that owns row b.  A source whose state_pose is NULL does not relabel: its rows are left alone.  For row b of a
 * relabelling source with expert_flags[idx[b]] == 0.0f:
 *   A = state_pose[idx[b]], E = state_pose[end[b]]   (row-major 4 x 4; the bottom rows are taken as (0, 0, 0, 1) and not read)
 *   R = A_R^T E_R, t = A_R^T (E_t - A_t)             (= se3_inverse(A) . E)
 *   out_goal[b] = [quaternion (w, x, y, z) of R | t]
 * Every other row of out_goal is not written at all.  The quaternion is the float32 closed form: of the four candidates
 * 1 + tr, 1 + R00 - R11 - R22, 1 - R00 + R11 - R22, 1 - R00 - R11 + R22 (= 4w^2, 4x^2, 4y^2, 4z^2) the largest, m, picks the
 * branch; its component vector is divided by 2 sqrt(m), normalised to unit length and negated if w < 0.  If any component
 * comes out non-finite the identity quaternion (1, 0, 0, 0) is written ("identity when the conversion fails", reference
 * core/utils.py:299-306; the host's own answer for NaN input depends on LAPACK and is not reproduced); t is written as
 * computed.
 * Contract: rigid poses, i.e. R orthonormal to float32 rounding; the result then agrees with the host's
 * BaseMemory.onpolicy_goals to float32 rounding of the 3 x 3 products (not bit for bit: tests/test_gpu_device_relabel.py
 * states the gate).  For any other finite matrix the output is finite and of unit length but is NOT the host's Bar-Itzhack
 * best fit (a zero matrix gives (1, 0, 0, 0) here, (0, 1, 0, 0) on the host).
 * One lane per row, 64-lane workgroups; pose rows are read as 16-byte groups when every relabelling source's state_pose is
 * 16-byte aligned, as single floats otherwise (same result either way).
 * Refused before any launch: NULL args (GAD_ERR_NULL); n_src outside 1..GAD_REPLAY_MAX_SRC, B outside 1..65535, a row_start
 * that does not run 0 .. B without decreasing (GAD_ERR_SHAPE); NULL idx, end or out_goal, a source that owns rows and has
 * state_pose set but expert_flags NULL (GAD_ERR_NULL). */
typedef struct {
    const float* state_pose;             /* (cap, 16) row-major 4 x 4 poses, or NULL: this source's rows keep their goals */
    const float* expert_flags;           /* (cap) */
} gad_replay_relabel_src;
typedef struct {
    int32_t B;
    int32_t n_src;
    int32_t row_start[GAD_REPLAY_MAX_SRC + 1];
    gad_replay_relabel_src src[GAD_REPLAY_MAX_SRC];
    const int64_t* idx; const int64_t* end;                               /* (B) device index vectors, source-local */
    float* out_goal;                     /* (B, 7), updated in place */
} gad_replay_relabel_args;

int gad_replay_relabel_goals(const gad_replay_relabel_args* host_args, void* stream);

/* ---------------------------------------------------------------------------------------------
 * G. housekeeping
 * ------------------------------------------------------------------------------------------- */

/* Clears up to six device buffers in one launch (pN may be NULL; nN = bytes, multiples of 4).  Replaces the
 * tensor.zero_() calls the reference's autograd does implicitly (fresh .grad / statistics buffers every backward,
 * core/agent.py:261-280 set_mode -> zero_grad): gradient arenas, BatchNorm-backward statistics and the scatter
 * targets of one backward pass. */
int gad_zero_buffers(void* p0, long long n0, void* p1, long long n1, void* p2, long long n2, void* p3,
                     long long n3, void* p4, long long n4, void* p5, long long n5, void* stream);

/* Copies up to GAD_COPY_MAX_SEGS device buffers in one launch (bytes: multiples of 4, 4-byte aligned; a segment with a NULL
 * pointer or 0 bytes is skipped).  add != 0: the segment is float32 data and dst[i] = src[i] + add (the step's "remaining time
 * minus one" vector of the TD target, reference core/ddpg.py:100-104, is formed while the time vector is copied).  Replaces the
 * key-by-key tensor copies with which a device-resident minibatch was adopted into the step's static input buffers
 * (reference core/agent.py:211-240 prepare_data: one .cuda() per key). */
#define GAD_COPY_MAX_SEGS 16
typedef struct {
    void* dst;
    const void* src;
    long long bytes;
    float add;
    int32_t reserved_;
} gad_copy_seg;
int gad_copy_buffers(const gad_copy_seg* host_segs, int n_segs, void* stream);

/* ---------------------------------------------------------------------------------------------
 * H. step replay (ABI 11)
 *
 * The update step of reference core/ddpg.py:146-185 / core/agent.py:211-259 is ~240 launches of the entry points above on four
 * streams.  The reference's host walks its step from Python, one torch call after the other
 * (core/train_test_offline.py:117-126: sample, update_parameters, read the losses -- every iteration); a host that does the
 * same over this ABI pays one foreign call per launch.  A gad_plan is the recorded list -- launches with their argument words,
 * device copies / clears, stream forks and joins -- replayed by ONE call: gad_plan_run walks it in C and enqueues every item on
 * the stream of its lane.  Nothing is captured or re-ordered (this is not a HIP graph: measured slower on this part); the
 * launches are exactly those the item-by-item host would have made, in the same order on every stream.
 *
 *   - lanes: small integers naming the streams of a run; gad_plan_run takes the table lane -> hipStream_t.
 *   - argument words: one uint64 per argument of the entry point, the trailing `stream` excluded, with its kind
 *     (GAD_ARG_*: I32 = int / int32_t, I64 = pointers and long long, F32 = float bits in the low half, F64 = double bits).
 *     gad_plan_add_call checks count and kinds against the entry point's real signature and fails with GAD_ERR_SHAPE on a
 *     mismatch.  Pointers to host argument blocks (gad_gemm_fwd_args, gad_optim_job[], ...) are stored as pointers: the
 *     caller keeps the blocks alive and may edit them between runs.
 *   - gad_plan_patch rewrites one word of an item (a scalar that changes from step to step, the pinned block of this
 *     step's ring slot, an event handle); 0 in the event word of a record / wait-event item makes it a no-op.
 *   - gad_plan_arm_timing: gad_timing_slot for ONE launch item of the next run (consumed by it).
 *   - a plan is not thread-safe; two plans may run from two threads.  gad_plan_add_* return the item's index (>= 0).
 * ------------------------------------------------------------------------------------------- */
#define GAD_ARG_I32 0
#define GAD_ARG_I64 1
#define GAD_ARG_F32 2
#define GAD_ARG_F64 3
#define GAD_PLAN_MAX_LANES 16
typedef struct gad_plan gad_plan;
int gad_plan_create(gad_plan** out);
int gad_plan_destroy(gad_plan* plan);
int gad_plan_size(const gad_plan* plan);
int gad_plan_add_call(gad_plan* plan, const char* entry, const uint64_t* words, const uint8_t* kinds, int n_words, int lane);
/* `waiter_lane` waits for everything enqueued so far on `signal_lane` (plan-owned event: record + hipStreamWaitEvent) */
int gad_plan_add_wait(gad_plan* plan, int waiter_lane, int signal_lane);
/* caller-owned hipEvent_t (nullable, patchable word 0): record on / make wait the lane's stream */
int gad_plan_add_record(gad_plan* plan, int lane, void* event);
int gad_plan_add_wait_event(gad_plan* plan, int lane, void* event);
int gad_plan_add_memset(gad_plan* plan, void* dst, long long bytes, int lane);                 /* hipMemsetAsync(dst, 0, bytes) */
int gad_plan_add_memcpy(gad_plan* plan, void* dst, const void* src, long long bytes, int lane); /* hipMemcpyAsync, any direction;
                                                                                                 * words: dst, src, bytes     */
int gad_plan_patch(gad_plan* plan, int item, int word, uint64_t value);
int gad_plan_arm_timing(gad_plan* plan, int item, void* slot);
/* enqueue items [first, first + count) (count < 0: to the end); no host synchronisation.  On failure: the status of the item
 * that failed, gad_last_error() names it. */
int gad_plan_run(gad_plan* plan, void* const* streams, int n_streams, int first, int count);
int gad_plan_entry_count(void);               /* the entry points a plan can replay (every one above that takes a stream) */
const char* gad_plan_entry_name(int i);

#ifdef __cplusplus
}
#endif
#endif /* GADDPG_H */
