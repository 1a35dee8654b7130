/* gsplat_hip.h -- C ABI of libgsplat_hip.so: the MI355X (gfx950) rasterization hot path.
 *
 * This is the drop-in boundary.  The first group of entry points replaces, one for one, the
 * functions of the reference's `splat_cuda` extension (joeyan/gaussian_splatting
 * src/bindings.cpp:118-159); the fused per-Gaussian stage, the prefix-mode renderer, the multi-GPU
 * bookkeeping and the training-loop operations further down replace the reference's Python glue
 * around them (cited per function).  All take plain device pointers + sizes + a hipStream_t (as
 * void*); no torch types, no exceptions, no hidden allocation, no device synchronisation.  Work
 * is enqueued on `stream` and the call returns.
 *
 * Conventions
 *   dtype      GS_F32 (0) or GS_F64 (1); all floating tensors of one call share it.
 *   layouts    row-major, contiguous, exactly the reference's tensor shapes (cited per function).
 *   outputs    caller-allocated.  Backward outputs marked "accumulated" are added into
 *              (atomicAdd semantics, render_backward.cu:269-281) and must be zeroed by the caller.
 *   return     0 on success, a negative GS_E* code otherwise; gs_last_error() gives the text.
 *   tile rows  [tile_row0, tile_row1) restricts binning/rendering to those rows of 16-px tiles
 *              (multi-GPU sharding); pass 0 and n_tiles_y for the whole image.
 */
#ifndef GSPLAT_HIP_H
#define GSPLAT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GS_F32 0
#define GS_F64 1

#define GS_OK 0
#define GS_EINVAL (-1)   /* bad argument (shape, dtype, n_sh not in {1,4,9,16}, ...) */
#define GS_EHIP (-2)     /* a HIP runtime call or kernel launch failed */

#define GS_TILE 16       /* tile edge in pixels (splat_py/structs.py:4) */
#define GS_PACKED_WIDTH 12 /* scalars per packed splat record, see gs_pack_splats */
#define GS_SORT_PREFIX 1024 /* entries ordered per long tile list in prefix mode, see gs_tile_emit_sort */

const char* gs_last_error(void);
int gs_abi_version(void);

/* ---- per-Gaussian projection ------------------------------------------------------------ */
/* camera_projection_cuda (bindings.cpp:121; projection.cu:9-54).  xyz[N,3], K[3,3] -> uv[N,2] */
int gs_camera_projection(const void* xyz, const void* K, int N, void* uv, int dtype, void* stream);
/* camera_projection_backward_cuda (bindings.cpp:122; projection_backward.cu:9-90).
 * rows with z <= 0 are left untouched (Q10). */
int gs_camera_projection_backward(const void* xyz, const void* K, const void* uv_grad_out, int N,
                                  void* xyz_grad_in, int dtype, void* stream);
/* compute_sigma_world_cuda (bindings.cpp:127; projection.cu:57-152).
 * quaternion[N,4] (w,x,y,z), scale[N,3] (log) -> sigma_world[N,3,3] */
int gs_compute_sigma_world(const void* quaternion, const void* scale, int N, void* sigma_world,
                           int dtype, void* stream);
/* compute_sigma_world_backward_cuda (bindings.cpp:128; projection_backward.cu:174-382) */
int gs_compute_sigma_world_backward(const void* quaternion, const void* scale,
                                    const void* sigma_world_grad_out, int N,
                                    void* quaternion_grad_in, void* scale_grad_in, int dtype,
                                    void* stream);
/* compute_projection_jacobian_cuda (bindings.cpp:133; projection.cu:155-211). -> J[N,2,3] */
int gs_compute_projection_jacobian(const void* xyz, const void* K, int N, void* J, int dtype,
                                   void* stream);
/* compute_projection_jacobian_backward_cuda (bindings.cpp:138; projection_backward.cu:93-166) */
int gs_compute_projection_jacobian_backward(const void* xyz, const void* K,
                                            const void* jac_grad_out, int N, void* xyz_grad_in,
                                            int dtype, void* stream);
/* compute_conic_cuda (bindings.cpp:143; projection.cu:214-311).
 * sigma_world[N,3,3], J[N,2,3], camera_T_world[4,4] -> conic[N,3] = (S00, S01+S10, S11) */
int gs_compute_conic(const void* sigma_world, const void* J, const void* camera_T_world, int N,
                     void* conic, int dtype, void* stream);
/* compute_conic_backward_cuda (bindings.cpp:145; projection_backward.cu:385-550) */
int gs_compute_conic_backward(const void* sigma_world, const void* J, const void* camera_T_world,
                              const void* conic_grad_out, int N, void* sigma_world_grad_in,
                              void* J_grad_in, int dtype, void* stream);

/* ---- spherical harmonics ------------------------------------------------------------------ */
/* precompute_rgb_from_sh_cuda (bindings.cpp:148-152; precompute_sh.cu:8-58,113-250).
 * xyz[N,3], sh_coeff[N,3,n_sh] (or [N,3] when n_sh==1), matrix[4,4] whose translation column is
 * the camera centre (Q8; read on the device, no host sync) -> rgb[N,3] */
int gs_precompute_rgb_from_sh(const void* xyz, const void* sh_coeff, const void* matrix, int N,
                              int n_sh, void* rgb, int dtype, void* stream);
/* precompute_rgb_from_sh_backward_cuda (bindings.cpp:153-157; precompute_sh.cu:61-111,252-389) */
int gs_precompute_rgb_from_sh_backward(const void* xyz, const void* matrix, const void* grad_rgb,
                                       int N, int n_sh, void* grad_sh, int dtype, void* stream);

/* ---- tile binning + per-tile depth sort (fp32 only) ----------------------------------------- */
/* get_sorted_gaussian_list (bindings.cpp:147; tile_culling.cu:124-340) is split in two so that
 * the caller owns every allocation:
 *
 *   1. gs_tile_count   OBB/SAT test of every Gaussian against its candidate tiles
 *                      (tile_culling.cu:8-177), per-tile counts and their exclusive prefix:
 *                      tile_ranges[T+1] == splat_start_end_idx_by_tile_idx.  tile_ranges[T] is the
 *                      instance count S (read it back to size the outputs of step 2).
 *   2. gs_tile_emit_sort  re-runs the test, scatters (z bits, gaussian) keys into each tile's
 *                      segment and sorts every segment front-to-back in LDS
 *                      (tile_culling.cu:179-242,327-329).  Order == the reference's fp64 key
 *                      z + (max_z+1)*tile (tile_culling.cu:236-237) with ties broken by ascending
 *                      Gaussian index.
 *
 * uvs[V,2], xyz_camera_frame[V,3], conic[V,3]; n_tiles = n_tiles_x*n_tiles_y.
 * host_mirror (gs_tile_count, gs_tile_count_cut; may be NULL): a device-accessible pointer to 3 ints of PINNED HOST
 *   memory that receives, when the scan finishes, (instance count, visible count, x) with x = the length of the
 *   LONGEST tile list of the rows (gs_tile_count) / the complete instance count (gs_tile_count_cut) -- the frame's
 *   host read without a copy kernel in the stream (record an event behind the call and wait for it).  A caller that
 *   knows the longest list can tell gs_tile_emit_sort_bounded and gs_render_tiles_prefix_phased what they need
 *   not launch.
 * visible_count: NULL, or a device pointer to the number of valid rows when the inputs are
 *   capacity-V buffers whose fill level only the device knows (gs_preprocess_forward); rows
 *   beyond it are ignored and tile_ranges then has T+2 entries, [T+1] = *visible_count, so that
 *   one 8-byte read returns S and V.  Pass the same V and visible_count to both calls.
 * subset, subset_count: both NULL, or a device list of row indices and a device pointer to its
 *   length: only those rows are tested (multi-GPU band mode: the Gaussians whose candidate window
 *   reaches the rank's rows, gs_halo_plan's send_index).  The list must contain every row that has
 *   a tile in [tile_row0, tile_row1); the resulting lists are then the same as without it.
 * workspace: int32[gs_tile_workspace_ints(n_tiles)] scratch written by step 1 and read by step 2
 *   (per-workgroup tile histograms, or per-tile cursors that step 1 leaves zeroed and step 2 returns to zero;
 *   keep it untouched between the two calls; step 2 may be repeated on it -- a larger capacity);
 * keys: uint64[S] scratch.  S may be an over-estimate (a capacity): instances beyond it are not
 * written and tiles reaching beyond it are left unsorted, so a caller may launch step 2 before it
 * has read the true count and repeat it with the exact S only if the count exceeded the capacity.
 *
 * sort_prefix: 0 = every segment is sorted in full (what get_sorted_gaussian_list returns).
 *   GS_SORT_PREFIX = prefix mode for the fused renderer: the forward pass stops reading a tile's
 *   list once all its pixels are saturated (render.cu:106,162), on dense scenes after a small part
 *   of it, so for a tile with GS_SORT_PREFIX < n <= 8192 entries only the GS_SORT_PREFIX nearest are
 *   selected and ordered into sorted_gaussians[start .. start+GS_SORT_PREFIX); the rest of that
 *   segment is undefined.  Results stay exact: gs_render_tiles_prefix raises tile_flags[t] when a
 *   tile ran out of prefix with an unsaturated pixel, sorts those tiles in full from the untouched
 *   `keys` (gs_tile_sort_flagged) and renders them again -- plain enqueues, no host read. */
size_t gs_tile_workspace_ints(int n_tiles);
int gs_tile_count(const void* uvs, const void* conic, int V, const int32_t* visible_count,
                  const int32_t* subset, const int32_t* subset_count, int n_tiles_x, int n_tiles_y,
                  float mh_dist, int tile_row0, int tile_row1, int32_t* workspace,
                  int32_t* tile_ranges /*[T+1] or [T+2]*/, int32_t* host_mirror, void* stream);
int gs_tile_emit_sort(const void* uvs, const void* xyz_camera_frame, const void* conic, int V,
                      const int32_t* visible_count, const int32_t* subset,
                      const int32_t* subset_count, int n_tiles_x, int n_tiles_y, float mh_dist,
                      int tile_row0, int tile_row1, const int32_t* tile_ranges, int32_t* workspace,
                      uint64_t* keys, int64_t S, int32_t* sorted_gaussians /*[S]*/, int sort_prefix,
                      void* stream);
/* gs_tile_emit_sort with a bound on the list lengths (ABI 6): longest_list >= 0 promises that no tile of the rows has
 * more entries, and the sort launches that only serve longer lists are not enqueued (a sparse frame otherwise pays
 * ~5 us for a kernel that finds nothing to do); < 0 = no promise.  The bound may be a GUESS only if the caller checks
 * it against the count pass's result afterwards and repeats the call when it was too small. */
int gs_tile_emit_sort_bounded(const void* uvs, const void* xyz_camera_frame, const void* conic, int V,
                              const int32_t* visible_count, const int32_t* subset, const int32_t* subset_count,
                              int n_tiles_x, int n_tiles_y, float mh_dist, int tile_row0, int tile_row1,
                              const int32_t* tile_ranges, int32_t* workspace, uint64_t* keys, int64_t S,
                              int32_t* sorted_gaussians /*[S]*/, int sort_prefix, int64_t longest_list, void* stream);
/* Full sort of the tiles t in the row band with tile_flags[t] != 0 (keys as left by
 * gs_tile_emit_sort(..., GS_SORT_PREFIX, ...), same S). */
int gs_tile_sort_flagged(const int32_t* tile_ranges, const uint64_t* keys, int64_t S,
                         const int32_t* tile_flags, int n_tiles_x, int tile_row0, int tile_row1,
                         int32_t* sorted_gaussians, void* stream);

/* ---- depth-bucketed binning ("depth cut", fp32, ABI 6; no reference counterpart) ----------------------------
 * For dense frames the tile lists are several times longer than what the render consumes (workload D: ~2800
 * entries per tile, no pixel composites deeper than the 743rd).  Here the count pass walks the visible Gaussians
 * in NBK = 1024 DEPTH BUCKETS of about equal population (one workgroup per bucket), so that its per-workgroup tile
 * histograms are a cumulative depth histogram per tile and every tile knows, exactly, the last bucket b*(t) up to
 * which it holds at most GS_SORT_PREFIX entries.  Only those are emitted and sorted (a true depth prefix of the
 * complete list, completely ordered).  Exact like the prefix sort: gs_render_tiles_cut flags a truncated tile
 * that reaches the end of its list with an unsaturated pixel, emits + sorts the COMPLETE lists of the flagged tiles
 * into the caller's overflow buffers at full_ranges and renders them again; gs_render_tiles_backward_slab reads a
 * flagged tile's list from there.  No host read in between.
 *
 *   gs_preprocess_forward_cut   gs_preprocess_forward + bin_records float[N,8] (u v conic0 conic1 | conic2 z 0 0 per
 *                               visible Gaussian: what the binning reads, one 32-byte sector), and inside cut_workspace
 *                               the bucket boundaries and every visible Gaussian's bucket.  depth_hist: int32
 *                               [GS_CUT_HIST_BINS] that is ALL ZERO on entry and all zero again on exit (allocate once,
 *                               zero once, hand to every frame on the stream): the depth histogram of every
 *                               sample_stride-th visible Gaussian (sample_stride = gs_cut_sample_stride(N)) whose
 *                               quantiles are the boundaries.  uv, xyz_camera_frame and conic may be NULL here (their
 *                               values are in bin_records: uv = columns 0-1, conic = columns 2-4, z = column 5).
 *   gs_tile_count_cut           buckets, counts, cut: tile_ranges[T+3] (prefix of the KEPT counts; [T] = entries kept
 *                               S', [T+1] = V, [T+2] = all entries S), full_ranges[T+1] (prefix of the complete counts)
 *   gs_tile_emit_sort_cut       keys + sorted lists of the kept entries (capacity S as in gs_tile_emit_sort)
 * workspace: int32[gs_tile_workspace_ints(T)] as for gs_tile_count; cut_workspace: int32[gs_cut_workspace_ints(N, T)],
 * both untouched until the frame's backward has run.  Needs the LDS-histogram regime: gs_cut_supported(...) != 0. */
#define GS_CUT_BUCKETS 1024
#define GS_CUT_HIST_BINS 8192
#define GS_CUT_MAX_SAMPLES 65536
size_t gs_cut_workspace_ints(int n_gaussians, int n_tiles);
int gs_cut_sample_stride(int n_gaussians);
int gs_cut_supported(int n_tiles_x, int tile_row0, int tile_row1, int n_gaussians);
int gs_tile_count_cut(const void* bin_records, int N, const int32_t* visible_count, int n_tiles_x, int n_tiles_y,
                      float mh_dist, int tile_row0, int tile_row1, int32_t* workspace, int32_t* cut_workspace,
                      int32_t* tile_ranges /*[T+3]*/, int32_t* full_ranges /*[T+1]*/, int32_t* host_mirror, void* stream);
int gs_tile_emit_sort_cut(const void* bin_records, int N, int n_tiles_x, int n_tiles_y, float mh_dist, int tile_row0,
                          int tile_row1, const int32_t* tile_ranges, int32_t* workspace, int32_t* cut_workspace,
                          uint64_t* keys, int64_t S, int32_t* sorted_gaussians, void* stream);
/* tests / tools: device pointers into the cut workspace -- b*(t) int32[T], complete counts int32[T], bucket bounds
 * uint32[1024] (sortable depth bits, inclusive upper bound), bucket offsets int32[1025], control int32[2] (deepest
 * bucket any tile wants, flagged tiles of the frame) */
int gs_cut_debug_views(int32_t* cut_workspace, int N, int n_tiles, int32_t** bstar, int32_t** totals, uint32_t** bounds,
                       int32_t** bucket_offsets, int32_t** ctrl);

/* ---- fused per-Gaussian stage (fp32) ----------------------------------------------------------------
 * One pass replacing the PyTorch glue and per-Gaussian kernels of rasterize()
 * (splat_py/rasterize.py:29-99: utils.py:60-72 transform, projection.cu:9-19, the frustum cull
 * :33-49, the boolean-mask gathers :52-75, torch.sigmoid :60, projection.cu:57-257,
 * precompute_sh.cu:8-58 on cat(rgb, sh) :89).  Survivors are compacted in Gaussian order, so
 * the visible index equals the reference's boolean-mask index.
 *   inputs   xyz[N,3] quaternion[N,4] scale[N,3] opacity[N,1] (logits) rgb[N,3]
 *            sh[N,3,n_sh-1] (NULL when n_sh == 1), camera_T_world[4,4], K[3,3]
 *   mh_dist, band_row0, band_row1: a multi-GPU rank passes its tile-row band; rgb_render (and the
 *            colour inside packed) is then evaluated only for Gaussians whose candidate tile window
 *            reaches the band (0 elsewhere).  Pass 0 and n_tile_rows for the whole frame.
 *   workspace int32[gs_preprocess_workspace_ints(N)]
 *   outputs  camera_center[3]; visible_count[1] (= V, on the device); culling_mask uint8[N]
 *            (1 = culled); rank int32[N] (visible index or -1); and, with capacity N rows of which
 *            the first V are written: vis_idx int32, uv[.,2], xyz_camera_frame[.,3], conic[.,3],
 *            opacity_act[.,1] = sigmoid, rgb_render[.,3], packed[.,12] (see gs_pack_splats).  vis_idx and
 *            rgb_render may be NULL (not written: the renderer reads the colour from the packed record).
 * The entry of this form is gs_preprocess_forward, its depth-cut form gs_preprocess_forward_cut (above): both are declared
 * with the classic entries below and forward to gs_preprocess_forward_mode, which takes a raster mode as well. */
size_t gs_preprocess_workspace_ints(int N);

/* Backward of the above (projection_backward.cu:9-471, precompute_sh.cu:61-111 and the autograd of
 * the glue: sigmoid', the cat split, the dense scatter of rasterize.py:52-75, matmul').
 * grad_slab: the render gradients, one row of 9 floats per visible Gaussian in the order
 *   (rgb_render 3 | opacity_act 1 | uv 2 | conic 3) -- the layout gs_render_tiles_backward_slab
 *   accumulates into; the row of visible Gaussian v is grad_slab[(v - v_base) * 9].
 * Writes the dense parameter gradients, every row exactly once (zeros for culled Gaussians):
 * grad_xyz[N,3], grad_quaternion[N,4], grad_scale[N,3], grad_opacity_logit[N,1],
 * grad_rgb_param[N,3], grad_sh[N,3,n_sh-1] (NULL when n_sh == 1).
 * A slice [i0, i1) of the Gaussians (multi-GPU: the slice this rank owns) is processed by passing
 * the parameter / rank / output pointers advanced to row i0, N = i1 - i0, and a slab that holds
 * the rows of the slice's visible Gaussians with v_base = their first visible index;
 * opacity_act stays the full array (it is indexed by v).
 * gs_preprocess_backward (classic entries, below) has these arguments, gs_preprocess_backward_mode a raster mode as well. */

/* gs_preprocess_backward with the optimizer step folded in (ABI 9; single-GPU form, no reference counterpart):
 * the gradients are computed exactly as above, grad_xyz[N,3] is written as above, and for quaternion[N,4],
 * scale[N,3], opacity[N,1] (the pre-sigmoid parameter, not opacity_act), rgb[N,3] and (n_sh > 1) sh[N,3,n_sh-1]
 * NO gradient is written: the kernel applies gs_adam_step's update to the parameter and its exp_avg / exp_avg_sq
 * IN PLACE, for every one of the N Gaussians (culled ones with gradient 0: the moments decay and the parameter
 * moves, as a dense zero gradient through gs_adam_step would make them).  The result is bit-identical to
 * gs_preprocess_backward followed by gs_adam_step over the five tensors (one shared definition of the arithmetic,
 * -ffp-contract=off).  xyz is only read: its gradient is needed by the densification statistics anyway, the
 * caller steps it with gs_adam_step.
 * quaternion and scale are inputs of the gradient and outputs of the step: they are passed once.
 * Per tensor: <t>_lr and <t>_step (the 1-based step count AFTER this step, >= 1) as lr[k] / step[k] of gs_adam_step;
 * beta1, beta2, eps are shared by the five tensors.  All pointers fp32 device memory; quaternion and its moments
 * 16-byte aligned; sh and its moments may be unaligned (scalar accesses then) and are NULL / ignored when
 * n_sh == 1.  v_base and slices [i0, i1) as in gs_preprocess_backward (every per-Gaussian pointer advanced to row
 * i0).  There is no gathered (multi-GPU) form. */
int gs_preprocess_backward_adam(const void* xyz, int n_sh, const void* camera_T_world, const void* K,
                                const void* camera_center, const int32_t* rank, const void* opacity_act,
                                const void* grad_slab, int v_base, int N, void* grad_xyz,
                                void* quaternion, void* quaternion_exp_avg, void* quaternion_exp_avg_sq,
                                double quaternion_lr, int64_t quaternion_step,
                                void* scale, void* scale_exp_avg, void* scale_exp_avg_sq, double scale_lr,
                                int64_t scale_step,
                                void* opacity, void* opacity_exp_avg, void* opacity_exp_avg_sq, double opacity_lr,
                                int64_t opacity_step,
                                void* rgb, void* rgb_exp_avg, void* rgb_exp_avg_sq, double rgb_lr, int64_t rgb_step,
                                void* sh, void* sh_exp_avg, void* sh_exp_avg_sq, double sh_lr, int64_t sh_step,
                                double beta1, double beta2, double eps, void* stream);

/* The gradient of camera_T_world from the same render-gradient slab (ABI 10; the reference's pipeline gets the part of
 * it that flows through the positions from autograd, rasterize.py:29, and none through ComputeConic).  The rotation
 * block A and the translation t are twelve free numbers (no orthonormality assumed).  Per visible Gaussian, with
 * c = A p + t, G = [[g_c0, g_c1], [g_c1, g_c2]] and g_cam the camera-frame position gradient gs_preprocess_backward
 * forms:  dL/dA += 2 J^T G (J A) Sigma + g_cam p^T,  dL/dt += g_cam.  The SH view direction carries no gradient
 * (as for xyz), so the slab's colour and opacity columns are not read.
 *   inputs    xyz, quaternion, scale, camera_T_world, K, rank, grad_slab as gs_preprocess_backward takes them;
 *             workspace float[gs_pose_workspace_floats(N)].  A caller that wants the sum over the Gaussians
 *             [i0, i1) only passes xyz, quaternion, scale and rank advanced to row i0, N = i1 - i0 and, if its slab
 *             starts at another visible index than 0, that index as v_base.
 *   output    grad_camera_T_world[4,4] row-major, written (not accumulated), last row 0; all zeros for N == 0 or
 *             when no Gaussian is visible
 * Two launches, no atomics: the sums are added in an order that depends on N only, so equal inputs give equal
 * bits.  Must be enqueued BEFORE gs_preprocess_backward_adam, which overwrites the quaternion and scale it reads.
 * gs_pose_backward (classic entries, below) has these arguments, gs_pose_backward_mode opacity_act and a raster mode too. */
size_t gs_pose_workspace_floats(int N);

/* ---- antialiased opacity (fp32, ABI 14; the 2D factor of Mip-Splatting, no reference counterpart) -----------
 * The fp32 packed record dilates every projected covariance by 0.25 px^2 and leaves the opacity alone, so a splat
 * smaller than a pixel deposits several times the light it holds.  GS_RASTER_ANTIALIASED multiplies the record's
 * opacity by comp = sqrt(det Sigma_2D / det(Sigma_2D + 0.25 I)), which makes a splat's integrated weight independent of
 * the dilation, and differentiates through the factor.  Arithmetic (fp32, no contraction, IEEE divide and square root;
 * one definition, csrc/pg_math.h aa_terms_of / aa_fold_row), with conic = the per-Gaussian stage's conic output:
 *     a0 = conic0, c0 = conic2, b = conic1 * 0.5, a = a0 + 0.25, c = c0 + 0.25
 *     det_d = a c - b b   (the bits of packed[7])        det_0 = a0 c0 - b b        rho = det_0 / det_d
 *     comp = (det_0 > 0 && det_d > 0) ? sqrt(rho) : 0    (a NaN compares false: 0)
 *     opa_eff = opacity_act * comp
 *   forward   packed[3] = opa_eff, packed[2] = the cutoff radius for opa_eff (-1 when comp == 0: the row never
 *             contributes).  opacity_act (the sigmoid), uv, xyz_camera_frame, conic, rgb_render, bin_records, every other
 *             packed column, the culling mask, rank and vis_idx keep the classic call's bits; the binning never reads the
 *             opacity, so tile ranges and sorted lists do too.
 *   backward  column 3 of a slab row is g = dL/d opa_eff.  With y = opacity_act the row is folded in registers where
 *             the kernels load it (the slab in memory is not rewritten):
 *                 slab3' = g comp                        (then d sigmoid: grad_opacity_logit = slab3' (1 - y) y)
 *                 comp > 0:  g_rho = g y 0.5 / comp
 *                     slab6 += g_rho (c0 det_d - det_0 c) / (det_d det_d)
 *                     slab7 += g_rho b (det_0 - det_d)   / (det_d det_d)
 *                     slab8 += g_rho (a0 det_d - det_0 a) / (det_d det_d)
 *             comp recomputed from the parameters with the forward's functions.  The true derivative: no epsilon guards
 *             0.5 / comp, which grows without bound for a needle whose det_0 cancels; a row with comp == 0 gets no conic
 *             term and opacity gradient 0.
 * gs_preprocess_forward_mode   the arguments of gs_preprocess_forward_cut + raster_mode; bin_records, cut_workspace and
 *                              depth_hist all NULL = the form of gs_preprocess_forward.  Whole frames only with
 *                              GS_RASTER_ANTIALIASED (band_row0 = 0, band_row1 = n_tile_rows).
 * gs_preprocess_backward_mode  gs_preprocess_backward + raster_mode; slices [i0, i1) and v_base as there.
 * gs_pose_backward_mode        gs_pose_backward + opacity_act (the full [V,1] array, indexed by v: the fold needs y; may
 *                              be NULL with GS_RASTER_CLASSIC) + raster_mode.
 * raster_mode is a bit mask (ABI 19): GS_RASTER_ANTIALIASED | GS_RASTER_FISHEYE in any combination; a value with any
 * other bit set returns GS_EINVAL (message names raster_mode) and writes nothing.  With GS_RASTER_CLASSIC each entry
 * launches exactly the kernels of the entry it extends, with GS_RASTER_ANTIALIASED exactly those of ABI 14.  The band,
 * list, gathered and Adam forms of the per-Gaussian stage have neither mode.
 *
 * ---- fisheye camera (fp32, ABI 19; the equidistant model, gsplat's camera_model="fisheye"; no reference counterpart) ----
 * GS_RASTER_FISHEYE replaces the pinhole projection and its Jacobian in the per-Gaussian stage; K stays the 3x3
 * matrix (fx, fy, cx, cy; no skew, no distortion coefficients).  With (x, y, z) = xyz_camera_frame (unchanged):
 *     r2 = x x + y y      q = 1 / (r2 + z z)      r = sqrt(r2)      theta = atan2(r, z)
 *     s = theta / r                                                   (r2 == 0:  s = 1 / z)
 *     u = fx s x + cx     v = fy s y + cy
 *     a = (z q - s) / r2                                              (r2 == 0:  a = -2 / (3 z^3))
 *     J = [[fx (s + x x a),  fx x y a,        -fx x q],
 *          [fy x y a,        fy (s + y y a),  -fy y q]]
 *   forward   the cull keeps its form (z < near | z > far | u, v outside the padded image: the usable field of view stays
 *             under 180 degrees); uv, conic = J W Sigma (J W)^T, bin_records and the packed record follow the model;
 *             xyz_camera_frame, opacity_act and rgb_render keep the pinhole call's bits on a row visible in both; sort
 *             keys, depth buckets and the depth maps keep using z.
 *   backward  gJ reaches the camera-frame position through all six entries (J1 and J3 are not zero) and g_uv through
 *             g_uv^T J (when z > 0, as for the pinhole model), with  d = -(2 z q q + 3 a) / r2  (r2 == 0: 8 / (5 z^5)):
 *                 ds = (a x, a y, -q)     da = (d x, d y, 2 q q)     dq = -2 q q (x, y, z)
 *             For r2 < z z / 16 a and d are evaluated as their series in r2 / (z z) (their closed forms cancel near the
 *             axis); one definition, csrc/pg_math.h fisheye_terms_of / fisheye_J6_of / fisheye_cam_grad_of.
 * Arithmetic: fp32, no contraction, IEEE divide and square root; atan2f is the device library's. */
#define GS_RASTER_CLASSIC 0
#define GS_RASTER_ANTIALIASED 1
#define GS_RASTER_FISHEYE 2
int gs_preprocess_forward_mode(const void* xyz, const void* quaternion, const void* scale,
                               const void* opacity, const void* rgb, const void* sh, int n_sh,
                               const void* camera_T_world, const void* K, int N, int W, int H,
                               float near_thresh, float far_thresh, float cull_mask_padding,
                               float mh_dist, int band_row0, int band_row1,
                               int32_t* workspace, void* camera_center, int32_t* visible_count,
                               uint8_t* culling_mask, int32_t* rank, int32_t* vis_idx, void* uv,
                               void* xyz_camera_frame, void* conic, void* opacity_act, void* rgb_render,
                               void* packed, void* bin_records, int32_t* cut_workspace, int32_t* depth_hist,
                               int sample_stride, int raster_mode, void* stream);
int gs_preprocess_backward_mode(const void* xyz, const void* quaternion, const void* scale, int n_sh,
                                const void* camera_T_world, const void* K, const void* camera_center,
                                const int32_t* rank, const void* opacity_act, const void* grad_slab,
                                int v_base, int N, void* grad_xyz, void* grad_quaternion,
                                void* grad_scale, void* grad_opacity_logit, void* grad_rgb_param,
                                void* grad_sh, int raster_mode, void* stream);
int gs_pose_backward_mode(const void* xyz, const void* quaternion, const void* scale, const void* camera_T_world,
                          const void* K, const int32_t* rank, const void* opacity_act, const void* grad_slab, int v_base,
                          int N, void* workspace, void* grad_camera_T_world, int raster_mode, void* stream);

/* ---- 3D smoothing filter (fp32, ABI 20; the 3D half of Mip-Splatting, no reference counterpart) ----------------
 * GS_RASTER_ANTIALIASED keeps a splat smaller than a pixel from adding light when the camera moves away; the other half
 * is a per-Gaussian low-pass of the world-space covariance, sized by the finest rate at which any training camera
 * samples the Gaussian, so that a scene does not grow needles when the camera moves closer.  filter3d [N] float32 holds
 * phi >= 0, a variance in world units; it is a constant of the frame and carries no gradient.  Arithmetic (fp32, no
 * contraction, IEEE divide and square root; one definition, csrc/pg_math.h filter3d_sigma / filter3d_terms_of /
 * filter3d_bwd_of), with s_k = exp(scale_k):
 *     Sigma_eff = Sigma + phi I          (the three diagonal entries of Sigma_world gain phi: R diag(s^2 + phi) R^T)
 *     rho3  = ((s_0^2 / (s_0^2 + phi)) (s_1^2 / (s_1^2 + phi))) (s_2^2 / (s_2^2 + phi))
 *     comp3 = rho3 > 0 ? sqrt(rho3) : 0                            (a NaN compares false: 0)
 *     opa3  = opacity_act * comp3
 *   forward   everything downstream reads Sigma_eff and opa3 where it read Sigma and the sigmoid: conic, bin_records, the
 *             packed record's a, b, c, det; with GS_RASTER_ANTIALIASED comp is taken from the filtered conic and
 *             packed[3] = opa3 * comp; the cutoff radius is evaluated on the final values.  A row with comp3 == 0 gets
 *             packed[2] = -1 and never contributes.  opacity_act stays the sigmoid; uv, xyz_camera_frame, rgb_render, the
 *             culling mask, rank and vis_idx do not depend on phi.
 *   backward  with g = column 3 of the slab row (GS_RASTER_ANTIALIASED: after the fold of "antialiased opacity", which
 *             takes opa3 in the place of y) and y = opacity_act:
 *                 grad_opacity_logit = g comp3 (1 - y) y
 *                 grad_scale[k]     += g opa3 phi / (s_k^2 + phi)
 *             and the slab's conic columns reach quaternion and scale as dL/dSigma_eff = dL/dSigma, through the
 *             unfiltered scale, unchanged.  No epsilon; a comp3 == 0 row gets opacity gradient 0 and no scale term.
 *             gs_pose_backward_filtered forms the same Sigma_eff and, under the fold, the same opa3.  A filter can make
 *             a splat millions of pixels wide: with a filter the fold's three conic terms are formed beyond
 *             det_d > 1e18 as g_rho (c0 - rho c) / det_d, g_rho b (rho - 1) / det_d, g_rho (a0 - rho a) / det_d, whose
 *             products stay inside fp32's range (det_d det_d does not); below, the expressions above, bit for bit.
 *             This widens the range, it does not remove the limit: from conic ~ 1e19 px^2 on det_0 = a0 c0 - b b and
 *             det_d themselves are infinite and comp = sqrt(inf / inf) is not a number, with or without a filter.
 * With phi == 0 every expression is exact, so such a row carries the values of the call without a filter, forward and
 * backward.
 * gs_preprocess_forward_filtered / gs_preprocess_backward_filtered / gs_pose_backward_filtered: the arguments of the
 * _mode entries with filter3d in front of raster_mode.  filter3d == NULL launches exactly what the _mode entry launches;
 * the filter is selected by the pointer, not by a raster_mode bit (raster_mode stays GS_RASTER_ANTIALIASED |
 * GS_RASTER_FISHEYE, anything else GS_EINVAL as there).  Whole frames only: a tile-row band with a filter is GS_EINVAL
 * (message names filter3d).  The backward entries take slices like the _mode ones: filter3d then points at the slice's
 * first row, as xyz, quaternion, scale and rank do.
 *
 * gs_filter3d_rate: rate[g] = max(rate[g], max over the cameras k that see Gaussian g of f_k / depth), the sampling
 * rate in pixels per world unit.  camera_T_world [C,4,4], K [C,3,3] float32, sizes [C,2] int32 = (W, H) per camera.  With
 * c = camera_T_world_k xyz_g and (u, v) the model's own projection (GS_RASTER_CLASSIC: the pinhole one; GS_RASTER_FISHEYE:
 * the equidistant one above), camera k sees g when z > near_thresh and -pad_fraction W < u < W + pad_fraction W,
 * -pad_fraction H < v < H + pad_fraction H; f = max(fx, fy); depth = z (pinhole) or |c| (fisheye: the radial rate, which
 * understates the tangential one by theta / sin(theta)).  rate is read and written: a row no camera sees keeps its
 * value and calls over subsets of the cameras compose exactly (start from zeros).  One launch, one thread per Gaussian;
 * xyz is read once.  C == 0 or N == 0 returns GS_OK without a launch; a raster_mode that is neither value, a negative
 * count or a NULL pointer is GS_EINVAL and writes nothing.  The filter is phi = variance / rate^2 (Mip-Splatting:
 * variance 0.2 px^2; fused.filter3d_from_rate). */
int gs_preprocess_forward_filtered(const void* xyz, const void* quaternion, const void* scale,
                                   const void* opacity, const void* rgb, const void* sh, int n_sh,
                                   const void* camera_T_world, const void* K, int N, int W, int H,
                                   float near_thresh, float far_thresh, float cull_mask_padding,
                                   float mh_dist, int band_row0, int band_row1,
                                   int32_t* workspace, void* camera_center, int32_t* visible_count,
                                   uint8_t* culling_mask, int32_t* rank, int32_t* vis_idx, void* uv,
                                   void* xyz_camera_frame, void* conic, void* opacity_act, void* rgb_render,
                                   void* packed, void* bin_records, int32_t* cut_workspace, int32_t* depth_hist,
                                   int sample_stride, const void* filter3d, int raster_mode, void* stream);
int gs_preprocess_backward_filtered(const void* xyz, const void* quaternion, const void* scale, int n_sh,
                                    const void* camera_T_world, const void* K, const void* camera_center,
                                    const int32_t* rank, const void* opacity_act, const void* grad_slab,
                                    int v_base, int N, void* grad_xyz, void* grad_quaternion,
                                    void* grad_scale, void* grad_opacity_logit, void* grad_rgb_param,
                                    void* grad_sh, const void* filter3d, int raster_mode, void* stream);
int gs_pose_backward_filtered(const void* xyz, const void* quaternion, const void* scale, const void* camera_T_world,
                              const void* K, const int32_t* rank, const void* opacity_act, const void* grad_slab,
                              int v_base, int N, void* workspace, void* grad_camera_T_world, const void* filter3d,
                              int raster_mode, void* stream);
int gs_filter3d_rate(const void* xyz, const void* camera_T_world, const void* K, const int32_t* sizes, int C, int N,
                     float near_thresh, float pad_fraction, int raster_mode, void* rate, void* stream);

/* ---- Normals (ABI 21; no reference counterpart) -------------------------------------------------------------------
 * What the normal-consistency regulariser of 2DGS needs around gs_render_features (channels n_x, n_y, n_z, z): the
 * visible Gaussians' normals, and the normal of the rendered depth map.  fp32, no contraction, IEEE divide and square
 * root; no scratch, no atomics, no workspace.
 *
 * gs_gaussian_normals: for each visible row v < V, with i = vis_idx[v] the Gaussian's dense row:
 *     qhat = quaternion[i] / |quaternion[i]|                      (csrc/pg_math.h sigma_world_of's normalisation)
 *     R    = quat_to_rot(qhat)
 *     a    = the index of the smallest of scale[i, 0:3], the log-scales themselves; on a tie the lowest index
 *     n_c  = W R[:, a]       with W the rotation of camera_T_world (rows 0..2, columns 0..2)
 *     normals[v] = n_c . xyz_camera_frame[v] > 0 ? -n_c : n_c     (faces the camera; an exact 0 is not flipped)
 *   The normal does not depend on the projection model: there is no raster_mode.  normals [V,3] is written for the V
 *   rows and nothing behind them.  V == 0 returns GS_OK without a launch.
 * gs_gaussian_normals_backward: grad_normals [V,3] -> grad_quaternion [N,4], through W, the rotation and the
 *   normalisation, with the axis and the flip held constant (the normal is piecewise constant in scale and xyz: they
 *   get no gradient).  One thread per Gaussian of the N through rank (rank[i] = the visible row of Gaussian i, negative
 *   when culled, as gs_preprocess_backward reads it; whole frames: no v_base): every one of the N rows is WRITTEN,
 *   culled rows as zeros.  N == 0 returns GS_OK without a launch.
 *
 * gs_depth_normal: the normal of the surface a rendered depth map describes.  depth, alpha [H,W] as gs_render_zalpha
 *   writes them (sum w z, sum w), d = depth / alpha, K float32 [3,3] on the device.  Pixel (x, y) has the renderer's
 *   integer coordinate, no half-pixel offset, and back-projects to
 *       GS_RASTER_CLASSIC   P = d ((x - cx) / fx, (y - cy) / fy, 1)
 *       GS_RASTER_FISHEYE   a = ((x - cx) / fx, (y - cy) / fy), theta = |a|,  P = d (tan(theta) / theta a, 1)
 *                           tan(theta) / theta from +, *, / alone (csrc/normals.hip tan_over_theta; no library call, so
 *                           the tests' float32 restatement repeats it): up to theta = pi / 4 the quotient of the series
 *                           of sin(theta) / theta and cos(theta) -- no division by theta, 1 at the axis -- beyond it
 *                           the same series at pi / 2 - theta; within 2.6e-7 relative.  theta >= pi / 2 (in float32:
 *                           not below the float above pi / 2) is an invalid ray
 *       n = normalize((P(x, y + 1) - P(x, y - 1)) x (P(x + 1, y) - P(x - 1, y)))
 *   2DGS's depth_to_normal orientation: towards the camera, like the Gaussians' normals.  A pixel is valid iff it is
 *   not on the image's border, it and its four neighbours have alpha > min_alpha and, under the fisheye model, a valid
 *   ray, and the cross product's squared norm is > 0 (a NaN compares false).  normal [H,W,3] is written for every pixel,
 *   (0, 0, 0) where invalid.  min_alpha must be >= 0 (so that d is formed only where alpha > 0).
 * gs_depth_normal_backward: grad_normal [H,W,3] -> grad_depth, grad_alpha [H,W], both written for every pixel (not
 *   accumulated), with d d / d depth = 1 / alpha, d d / d alpha = -depth / alpha^2 and the validity decisions constants.
 *   A gather: each pixel sums, in a fixed order, the terms of the up to four valid centres whose stencil holds it;
 *   two runs are bit-equal.
 * Both: raster_mode other than the two values, a negative size, a min_alpha that is negative or not a number, or a NULL
 * pointer is GS_EINVAL and writes nothing; W == 0 or H == 0 returns GS_OK without a launch. */
int gs_gaussian_normals(const void* quaternion, const void* scale, const void* camera_T_world, const int32_t* vis_idx,
                        const void* xyz_camera_frame, int V, void* normals, void* stream);
int gs_gaussian_normals_backward(const void* quaternion, const void* scale, const void* camera_T_world,
                                 const int32_t* rank, const void* xyz_camera_frame, const void* grad_normals, int V, int N,
                                 void* grad_quaternion, void* stream);
int gs_depth_normal(const void* depth, const void* alpha, const void* K, int W, int H, float min_alpha, int raster_mode,
                    void* normal, void* stream);
int gs_depth_normal_backward(const void* depth, const void* alpha, const void* K, const void* grad_normal, int W, int H,
                             float min_alpha, int raster_mode, void* grad_depth, void* grad_alpha, void* stream);

/* ---- the classic per-Gaussian entries: one-line forwards, kept for callers outside the package ----
 *   gs_preprocess_forward      -> gs_preprocess_forward_cut with bin_records, cut_workspace, depth_hist NULL, sample_stride 0
 *   gs_preprocess_forward_cut  -> gs_preprocess_forward_mode with GS_RASTER_CLASSIC
 *   gs_preprocess_backward     -> gs_preprocess_backward_mode with GS_RASTER_CLASSIC
 *   gs_pose_backward           -> gs_pose_backward_mode with opacity_act NULL and GS_RASTER_CLASSIC
 * The _mode entries forward in the same way to the _filtered ones (ABI 20) with filter3d NULL; the package's own callers
 * (fused.py, csrc/frame_hip.cpp) call those in every mode. */
int gs_preprocess_forward(const void* xyz, const void* quaternion, const void* scale,
                          const void* opacity, const void* rgb, const void* sh, int n_sh,
                          const void* camera_T_world, const void* K, int N, int W, int H,
                          float near_thresh, float far_thresh, float cull_mask_padding,
                          float mh_dist, int band_row0, int band_row1,
                          int32_t* workspace, void* camera_center, int32_t* visible_count,
                          uint8_t* culling_mask, int32_t* rank, int32_t* vis_idx, void* uv,
                          void* xyz_camera_frame, void* conic, void* opacity_act, void* rgb_render,
                          void* packed, void* stream);
int gs_preprocess_forward_cut(const void* xyz, const void* quaternion, const void* scale,
                              const void* opacity, const void* rgb, const void* sh, int n_sh,
                              const void* camera_T_world, const void* K, int N, int W, int H,
                              float near_thresh, float far_thresh, float cull_mask_padding,
                              float mh_dist, int band_row0, int band_row1,
                              int32_t* workspace, void* camera_center, int32_t* visible_count,
                              uint8_t* culling_mask, int32_t* rank, int32_t* vis_idx, void* uv,
                              void* xyz_camera_frame, void* conic, void* opacity_act, void* rgb_render,
                              void* packed, void* bin_records, int32_t* cut_workspace, int32_t* depth_hist,
                              int sample_stride, void* stream);
int gs_preprocess_backward(const void* xyz, const void* quaternion, const void* scale, int n_sh,
                           const void* camera_T_world, const void* K, const void* camera_center,
                           const int32_t* rank, const void* opacity_act, const void* grad_slab,
                           int v_base, int N, void* grad_xyz, void* grad_quaternion,
                           void* grad_scale, void* grad_opacity_logit, void* grad_rgb_param,
                           void* grad_sh, void* stream);
int gs_pose_backward(const void* xyz, const void* quaternion, const void* scale, const void* camera_T_world,
                     const void* K, const int32_t* rank, const void* grad_slab, int v_base, int N, void* workspace,
                     void* grad_camera_T_world, void* stream);

/* ---- tile renderer ---------------------------------------------------------------------------- */
/* Packs what the render kernels read per splat into one 48-byte (fp32) record per visible Gaussian:
 *   packed[V][12] = (u, v, r2, opacity | a, b, c, det | 1/det, SH_0*col0, SH_0*col1, SH_0*col2)
 * a/b/c as render.cu:117-128 forms them (+0.25 dilation for fp32, none for fp64); r2 is a
 * conservative squared cutoff radius: a pixel farther than sqrt(r2) from (u, v) provably has
 * alpha < 1/255 and is skipped exactly as render.cu:145-148 would skip it (+inf for fp64, which
 * has no alpha threshold); col = rgb[V,3] when rgb is given with n_sh == 1, stored as the product
 * SH_0 * col that sh_to_rgb forms per pixel (spherical_harmonics.cuh:83) (else unused: the kernels
 * then gather the [3, n_sh] coefficients from `rgb` directly).
 * uvs[V,2], opacity[V,1], conic[V,3], rgb[V,3] or NULL. */
int gs_pack_splats(const void* uvs, const void* opacity, const void* conic, const void* rgb, int V,
                   void* packed, int dtype, void* stream);
/* render_tiles_cuda (bindings.cpp:119; render.cu:8-422), the reference's arguments in the reference's order:
 * uvs[V,2], opacity[V,1], rgb[V,3,n_sh], conic[V,3], view_dir_by_pixel[H,W,3] (ignored when n_sh==1),
 * tile_ranges = splat_start_end_idx_by_tile_idx int32[n_tiles+1], sorted_gaussians =
 * gaussian_idx_by_splat_idx int32[S], background_rgb[3] -> num_splats_per_pixel int32[H,W],
 * final_weight_per_pixel[H,W], image[H,W,3]; then the sizes the tensors carry in the reference.  The
 * per-splat record of the render loops is formed while the tile lists are staged (no packing pass). */
int gs_render_tiles(const void* uvs, const void* opacity, const void* rgb, const void* conic,
                    const void* view_dir_by_pixel, const int32_t* tile_ranges,
                    const int32_t* sorted_gaussians, const void* background_rgb,
                    int32_t* num_splats_per_pixel, void* final_weight_per_pixel, void* image, int W, int H,
                    int n_sh, int tile_row0, int tile_row1, int dtype, void* stream);
/* The same from packed records (gs_pack_splats, or the `packed` output of gs_preprocess_forward): one
 * 48-byte gather per list entry instead of four partial ones -- the form the fused renderer uses. */
int gs_render_tiles_packed(const void* packed, const void* rgb, const void* view_dir_by_pixel,
                           const int32_t* tile_ranges, const int32_t* sorted_gaussians,
                           const void* background_rgb, int W, int H, int n_sh, int tile_row0,
                           int tile_row1, int32_t* num_splats_per_pixel, void* final_weight_per_pixel,
                           void* image, int dtype, void* segment_state, void* stream);
/* The same kernel over lists produced with sort_prefix = GS_SORT_PREFIX (fp32, n_sh == 1).
 * Enqueues (1) a provisional render that reads at most the ordered prefix of a prefix-sorted tile
 * and writes tile_flags[t] = 1 if tile t ran out of it with an unsaturated pixel (0 otherwise),
 * (2) gs_tile_sort_flagged, (3) a second render of the flagged tiles from their full lists.
 * Afterwards every output equals what gs_render_tiles_packed gives on fully sorted lists, and the
 * segments of the flagged tiles in sorted_gaussians are fully sorted (the backward pass reads them).
 * keys, S: as passed to gs_tile_emit_sort.  tile_flags: int32[n_tiles] scratch/out.
 * tile_cost (may be NULL): int32[n_tiles] out, the time each tile of [tile_row0, tile_row1) took to render
 * (16-shader-cycle units) -- a scheduling hint for gs_render_tiles_backward_slab, no effect on any result. */
int gs_render_tiles_prefix(const void* packed, const void* rgb, const int32_t* tile_ranges,
                           int32_t* sorted_gaussians, const uint64_t* keys, int64_t S,
                           const void* background_rgb, int W, int H, int tile_row0, int tile_row1,
                           int32_t* tile_flags, int32_t* num_splats_per_pixel,
                           void* final_weight_per_pixel, void* image, int32_t* tile_cost, void* segment_state,
                           void* stream);
/* The same in two separately callable phases (ABI 6): GS_PREFIX_RENDER = step (1), GS_PREFIX_REPAIR = steps (2) + (3)
 * on the flags step (1) left, both = gs_render_tiles_prefix.  A frame none of whose lists exceeds GS_SORT_PREFIX
 * cannot raise a flag: a caller that knows (the count pass's longest list) enqueues the render alone, one that only
 * guessed enqueues the repair when the count says otherwise -- later in the stream, the same result. */
#define GS_PREFIX_RENDER 1
#define GS_PREFIX_REPAIR 2
int gs_render_tiles_prefix_phased(const void* packed, const void* rgb, const int32_t* tile_ranges,
                                  int32_t* sorted_gaussians, const uint64_t* keys, int64_t S,
                                  const void* background_rgb, int W, int H, int tile_row0, int tile_row1,
                                  int32_t* tile_flags, int32_t* num_splats_per_pixel, void* final_weight_per_pixel,
                                  void* image, int32_t* tile_cost, void* segment_state, int phases, void* stream);
/* Depth segments of the fused backward (fp32, n_sh == 1; ABI 5).  segment_state (may be NULL): a 16-byte aligned
 * device workspace of gs_render_segment_workspace_bytes(W, H, tile_row0, tile_row1) bytes (ABI 6: sized for the
 * tile rows the three calls are given -- 32 KB per tile of the band, not of the grid) that gs_render_tiles_packed /
 * gs_render_tiles_prefix fill -- per (tile, 128-entry segment of its list, pixel) the transmittance at the
 * segment's far boundary and the colour the segment contributed, per pixel where its walk ends and what the
 * backward's first step does there -- and that gs_render_tiles_backward_slab, given the same pointer, uses to
 * launch one workgroup per (tile, segment) instead of one per tile: 3-4x more, shorter work items, the same
 * gradients up to fp32 rounding (what a multi-GPU rank's band of a few hundred tiles needs to fill the chip;
 * no reference counterpart).  The contents are private to the library. */
size_t gs_render_segment_workspace_bytes(int W, int H, int tile_row0, int tile_row1);
/* render_tiles_backward_cuda (bindings.cpp:120; render_backward.cu:12-595), the reference's arguments in the
 * reference's order.  grad_rgb[V,3,n_sh], grad_opacity[V,1], grad_uv[V,2], grad_conic[V,3] are accumulated.
 * backward_mode: GS_BACKWARD_DEFAULT / _COMPAT / _EXACT (below); COMPAT is bug-compatible with
 * render_backward.cu:185. */
int gs_render_tiles_backward(const void* uvs, const void* opacity, const void* rgb, const void* conic,
                             const void* view_dir_by_pixel, const int32_t* tile_ranges,
                             const int32_t* sorted_gaussians, const void* background_rgb,
                             const int32_t* num_splats_per_pixel, const void* final_weight_per_pixel,
                             const void* grad_image, void* grad_rgb, void* grad_opacity, void* grad_uv,
                             void* grad_conic, int W, int H, int n_sh, int tile_row0, int tile_row1, int dtype,
                             int backward_mode, void* stream);
/* The same from packed records (see gs_render_tiles_packed). */
int gs_render_tiles_backward_packed(const void* packed, const void* rgb, const void* view_dir_by_pixel,
                                    const int32_t* tile_ranges, const int32_t* sorted_gaussians,
                                    const void* background_rgb, const int32_t* num_splats_per_pixel,
                                    const void* final_weight_per_pixel, const void* grad_image, int W,
                                    int H, int n_sh, int tile_row0, int tile_row1, void* grad_rgb,
                                    void* grad_opacity, void* grad_uv, void* grad_conic, int dtype,
                                    int backward_mode, void* stream);
/* The fused renderer's form of the above (fp32, n_sh == 1): the four gradients of a Gaussian are
 * accumulated into one row of grad_slab[V, 9] = (rgb 3 | opacity 1 | uv 2 | conic 3).  zero_slab_rows: 0 = the
 * slab is zero-initialised (or holds values to accumulate onto); n > 0 = the call clears its first n rows itself
 * (16-byte aligned slab), in the launch that also makes the tile order -- one prologue kernel instead of a fill
 * and a single-workgroup kernel one after the other.
 * tile_cost / tile_order: with the costs gs_render_tiles_prefix measured and an int32[n_tiles + 8] workspace, the
 * tiles' workgroups are started longest-first (shorter drain at the end of the kernel; grids below 2048 tiles keep
 * the natural order).  Both NULL: natural order.  tile_order alone: the order gs_render_backward_prologue left in
 * it (the fused frames call the prologue as its own entry so that this one is the render kernel and nothing else).
 * The gradients do not depend on the order.
 * segment_state (may be NULL): the workspace the forward filled -> (tile, depth segment) work items, see
 * gs_render_segment_workspace_bytes; tile_cost / tile_order are then not used.
 * cut_flags / full_ranges / overflow_sorted (all NULL, or all given; ABI 6): a frame rendered by gs_render_tiles_cut --
 * a tile with cut_flags[t] != 0 reads its (complete) list from overflow_sorted at full_ranges[t]. */
/* The backward's prologue as its own call (ABI 6): clears the first zero_slab_rows rows of grad_slab[., 9] (0: none)
 * and, if tile_order is given, leaves the launch order of the rows' tiles there -- longest-first from tile_cost
 * (grids of >= 2048 tiles), the natural order otherwise -- in ONE launch; hand tile_order (and tile_cost = NULL,
 * zero_slab_rows = 0) to gs_render_tiles_backward_slab. */
int gs_render_backward_prologue(void* grad_slab, int64_t zero_slab_rows, const int32_t* tile_cost, int32_t* tile_order,
                                int W, int H, int tile_row0, int tile_row1, void* stream);
int gs_render_tiles_backward_slab(const void* packed, const void* rgb, const int32_t* tile_ranges,
                                  const int32_t* sorted_gaussians, const void* background_rgb,
                                  const int32_t* num_splats_per_pixel,
                                  const void* final_weight_per_pixel, const void* grad_image, int W,
                                  int H, int tile_row0, int tile_row1, void* grad_slab, int64_t zero_slab_rows,
                                  const int32_t* tile_cost, int32_t* tile_order, const void* segment_state,
                                  const int32_t* cut_flags, const int32_t* full_ranges, const int32_t* overflow_sorted,
                                  int backward_mode, void* stream);
/* Forward render of a frame binned by gs_tile_count_cut / gs_tile_emit_sort_cut (fp32, one colour coefficient per
 * channel; ABI 6).  tile_ranges / sorted_gaussians: the kept depth prefixes (capacity S as in gs_render_tiles_prefix);
 * a truncated tile that ends with an unsaturated pixel gets tile_flags[t] = 1, the complete lists of such tiles are
 * emitted into overflow_keys / overflow_sorted (capacity overflow_capacity >= full_ranges[T], the frame's complete
 * instance count; only flagged tiles' segments are written) and they are rendered again -- plain enqueues, no host
 * read; the three repair launches exit at once while nothing is flagged.  bin_records, workspace, cut_workspace: as
 * given to gs_tile_count_cut.  host_flagged (may be NULL): one int of device-accessible pinned host memory that receives
 * the number of flagged tiles (a policy hint for later frames: a frame whose tiles mostly need their complete lists
 * is cheaper without the cut).  Results are those of gs_render_tiles_packed on the complete sorted lists, bit for bit. */
int gs_render_tiles_cut(const void* packed, const void* rgb, const int32_t* tile_ranges, const int32_t* sorted_gaussians,
                        int64_t S, const int32_t* full_ranges, const void* bin_records, int N, float mh_dist,
                        int32_t* workspace, int32_t* cut_workspace, uint64_t* overflow_keys, int32_t* overflow_sorted,
                        int64_t overflow_capacity, const void* background_rgb, int W, int H, int tile_row0, int tile_row1,
                        int32_t* tile_flags, int32_t* num_splats_per_pixel, void* final_weight_per_pixel, void* image,
                        int32_t* tile_cost, int32_t* host_flagged, void* stream);
/* Gradient mode of the render backward: the `backward_mode` argument of the three entry points above
 * (ABI 5: per call, so that a trainer switching modes cannot race a backward that the autograd engine's
 * own thread has queued).  GS_BACKWARD_DEFAULT takes the process-wide default, which gs_set_backward_mode
 * sets (initially COMPAT) and which is read once, at the call.
 *   GS_BACKWARD_COMPAT  the reference's arithmetic, including render_backward.cu:185: the transmittance is
 *                       divided back by (1 - alpha) only while the CHUNK-LOCAL splat index is below
 *                       num_splats - 1, so for pixels that composite deeper than the reference's first
 *                       shared-memory chunk (960 splats in fp32 with one colour coefficient) the weights of
 *                       the later chunks are off by a factor 1 / (1 - alpha_last)
 *   GS_BACKWARD_EXACT   the same with the GLOBAL splat index: the mathematically exact gradient of the
 *                       forward pass.  Identical to COMPAT whenever no pixel composites past the first chunk. */
#define GS_BACKWARD_DEFAULT (-1)
#define GS_BACKWARD_COMPAT 0
#define GS_BACKWARD_EXACT 1
int gs_set_backward_mode(int mode);
int gs_get_backward_mode(void);

/* render_depth_cuda (bindings.cpp:158; depth.cu:7-177), fp32 only.  depth_image[H,W] is written
 * only where the accumulated alpha passes alpha_threshold (caller pre-fills with -1). */
int gs_render_depth(const void* packed, const void* xyz_camera_frame, const int32_t* tile_ranges,
                    const int32_t* sorted_gaussians, int W, int H, float alpha_threshold,
                    void* depth_image, void* stream);

/* Differentiable depth and accumulated opacity of a rendered frame (ABI 11; no reference counterpart), fp32, for the
 * packed records of gs_pack_splats / gs_preprocess_forward.  For pixel p and the list entries
 * k < num_splats_per_pixel[p] (what the colour forward walked, in its order), with alpha_k and the contribute decision
 * formed exactly as gs_render_tiles_packed forms them (cutoff radius, alpha >= 1/255):
 *   T_k = prod_{j < k, contributing} (1 - alpha_j),  w_k = alpha_k T_k,
 *   depth[p] = sum w_k z_k  with z = xyz_camera_frame[:, 2] (camera-frame z, NOT the range gs_render_depth writes),
 *   alpha[p] = sum w_k,  transmittance[p] = T behind the last contributor (= 1 - alpha[p], stored itself because the
 *   difference loses its digits as alpha approaches 1).
 * No background term and no normalisation (callers form depth / alpha).  Nothing beyond num_splats_per_pixel is
 * read, so the lists may be prefix-sorted (gs_render_tiles_prefix orders a tile as far as any of its pixels walked).
 *   inputs    packed[V,12], xyz_camera_frame[V,3], tile_ranges, sorted_gaussians, num_splats_per_pixel[H,W] as
 *             gs_render_tiles_packed takes / writes them
 *   outputs   depth[H,W], alpha[H,W], transmittance[H,W]: written for every pixel of the tile rows
 *             [tile_row0, tile_row1), untouched elsewhere.  Empty lists (V == 0) give 0, 0, 1. */
int gs_render_zalpha(const void* packed, const void* xyz_camera_frame, const int32_t* tile_ranges,
                     const int32_t* sorted_gaussians, const int32_t* num_splats_per_pixel, int W, int H,
                     int tile_row0, int tile_row1, void* depth, void* alpha, void* transmittance, void* stream);
/* Backward of the above: the TRUE derivative of the two maps, the contribute / stop decisions held constant (no
 * walk quirk of render_backward.cu is replicated; alpha above 0.9999 enters as 0.9999, Q4).
 *   grad_depth, grad_alpha   [H,W]; either may be NULL = all zeros (both NULL: nothing is launched)
 *   transmittance            what gs_render_zalpha wrote
 *   grad_slab                [V,9] (rgb 3 | opacity 1 | uv 2 | conic 3, the layout gs_preprocess_backward reads):
 *                            columns 3..8 accumulated, columns 0..2 untouched
 *   grad_z                   float[V], accumulated: dL/dz of each visible Gaussian (gs_z_backward takes it on)
 * Both are added into (one atomic per value per (list entry, tile)); the caller zeroes them, e.g. with
 * gs_render_backward_prologue.  Rows of Gaussians no pixel uses are not touched. */
int gs_render_zalpha_backward(const void* packed, const void* xyz_camera_frame, const int32_t* tile_ranges,
                              const int32_t* sorted_gaussians, const int32_t* num_splats_per_pixel,
                              const void* transmittance, const void* grad_depth, const void* grad_alpha, int W, int H,
                              int tile_row0, int tile_row1, void* grad_slab, void* grad_z, void* stream);
/* z = camera_T_world[2,0:3] . xyz + camera_T_world[2,3] back to the positions: for every Gaussian i of the N with
 * rank[i] >= 0, grad_xyz[i,:] += grad_z[rank[i] - v_base] * camera_T_world[2,0:3] (one fused multiply-add per
 * element; culled rows untouched).  rank, v_base and slices as in gs_preprocess_backward, after which it runs on the
 * same grad_xyz[N,3].  One thread per Gaussian, no atomics.  N == 0 launches nothing. */
int gs_z_backward(const int32_t* rank, const void* grad_z, const void* camera_T_world, int v_base, int N,
                  void* grad_xyz, void* stream);

/* Depth distortion of a rendered frame (ABI 16; no reference counterpart), fp32: the regulariser of Mip-NeRF 360 /
 * 2DGS without its normalisations, together with the depth and alpha maps.  With alpha_k, the contribute decision, T_k
 * and w_k = alpha_k T_k exactly as gs_render_zalpha forms them (the same code), z = xyz_camera_frame[:, 2], and for the
 * contributors in front of entry k  A_<k = sum_{j<k} w_j,  D_<k = sum_{j<k} w_j z_j:
 *   distortion[p] = 2 sum_k w_k (z_k A_<k - D_<k) = sum_{i != j} w_i w_j (z_later - z_earlier)
 * over the entries k < num_splats_per_pixel[p] in LIST order: no |.| is taken.  On lists sorted by z (the fused
 * frame's own, sorted by the bits of this z) that is sum_{i,j} w_i w_j |z_i - z_j|.  No background term, no
 * normalisation by alpha, no depth warp: the value is in units of z, callers scale z.  Per contributing visit
 *   X = fma(w, fma(z, A, -D), X),  D = fma(w, z, D),  A += w,  T = fma(-alpha, T, T),   the store is 2 X,
 * so depth, alpha and transmittance are bit-equal to gs_render_zalpha's.
 *   outputs   distortion[H,W], depth[H,W], alpha[H,W], transmittance[H,W]: written for every pixel of the tile rows
 *             [tile_row0, tile_row1), untouched elsewhere.  Empty lists (V == 0) give 0, 0, 0, 1. */
int gs_render_distortion(const void* packed, const void* xyz_camera_frame, const int32_t* tile_ranges,
                         const int32_t* sorted_gaussians, const int32_t* num_splats_per_pixel, int W, int H,
                         int tile_row0, int tile_row1, void* distortion, void* depth, void* alpha, void* transmittance,
                         void* stream);
/* Backward of the above for all three maps at once: the TRUE derivative, decisions held constant, as
 * gs_render_zalpha_backward (no walk quirk; alpha above 0.9999 enters as 0.9999).  Back to front from transmittance
 * with the suffix sums A_>k, D_>k; the prefixes come from the forward's totals,
 *   A_<k = alpha[p] - A_>k - w_k,  D_<k = depth[p] - D_>k - w_k z_k,
 *   e_k = 2 [z_k (A_<k - A_>k) - D_<k + D_>k]   (d distortion / d w_k),
 *   c_k = fma(grad_distortion, e_k, fma(grad_depth, z_k, grad_alpha)),
 *   dL/dz_k = grad_depth w_k + grad_distortion 2 w_k (A_<k - A_>k),
 * then dL/dalpha_k = T_k c_k - S / (1 - alpha_k), S = fma(w_k, c_k, S) and alpha -> opacity, u, v, conic as
 * gs_render_zalpha_backward: with grad_distortion NULL the result is that call's.
 *   transmittance, depth, alpha                [H,W], what gs_render_distortion wrote
 *   grad_distortion, grad_depth, grad_alpha    [H,W]; any may be NULL = all zeros (all NULL: nothing is launched)
 *   grad_slab   [V,9]: columns 3..8 accumulated, columns 0..2 untouched
 *   grad_z      float[V], accumulated: dL/dz of each visible Gaussian (gs_z_backward takes it on)
 * Both are added into (one atomic per value per (list entry, tile)); the caller zeroes them.  Rows of Gaussians no
 * pixel uses are not touched.  Empty lists (V == 0) touch nothing. */
int gs_render_distortion_backward(const void* packed, const void* xyz_camera_frame, const int32_t* tile_ranges,
                                  const int32_t* sorted_gaussians, const int32_t* num_splats_per_pixel,
                                  const void* transmittance, const void* depth, const void* alpha,
                                  const void* grad_distortion, const void* grad_depth, const void* grad_alpha, int W,
                                  int H, int tile_row0, int tile_row1, void* grad_slab, void* grad_z, void* stream);

/* Median depth of a rendered frame (ABI 22; 2DGS's depth_ratio = 1, gsplat's median depth), fp32, together with the
 * depth and alpha maps.  With alpha_k, the contribute decision and T_k (the transmittance in front of entry k) exactly
 * as gs_render_zalpha forms them (the same code; T <- fma(-alpha, T, T) on contributors only), the MEDIAN ENTRY of
 * pixel p is the last contributing entry k < num_splats_per_pixel[p] with T_k > 0.5f (strict, fp32, the walk's own T):
 * the entry during which T falls to 0.5 or below, or the last contributor if it never falls that far (2DGS's rule,
 * `if (T > 0.5) median = depth`, evaluated before the blend).  The entries are taken in LIST order.
 *   median_depth[p] = xyz_camera_frame[g, 2] of the median entry's Gaussian g: not weighted, not normalised; 0 where
 *                     the pixel has no contributor
 *   median_index[p] = g, a sorted_gaussians value (an index among the frame's visible Gaussians); -1 where the pixel
 *                     has no contributor
 * One walk: it stands in place of gs_render_zalpha, and depth, alpha and transmittance are bit-equal to that call's.
 *   outputs   median_depth[H,W], median_index[H,W] (int32), depth[H,W], alpha[H,W], transmittance[H,W]: written for
 *             every pixel of the tile rows [tile_row0, tile_row1), untouched elsewhere.  Empty lists (V == 0) give
 *             0, -1, 0, 0, 1.  A NULL output is GS_EINVAL. */
int gs_render_median_depth(const void* packed, const void* xyz_camera_frame, const int32_t* tile_ranges,
                           const int32_t* sorted_gaussians, const int32_t* num_splats_per_pixel, int W, int H,
                           int tile_row0, int tile_row1, void* median_depth, int32_t* median_index, void* depth,
                           void* alpha, void* transmittance, void* stream);
/* Backward of median_depth, the choice of entry held constant: grad_z[median_index[p]] += grad_median_depth[p] for every
 * pixel p of the tile rows with median_index[p] >= 0.  Nothing goes to the slab (uv, conic, opacity), and no lists or
 * records are read; the gradients of depth and alpha take gs_render_zalpha_backward.
 *   median_index        [H,W], what gs_render_median_depth wrote: every value is -1 or a row of grad_z
 *   grad_median_depth   [H,W]; NULL = all zeros: nothing is launched
 *   grad_z              float[V], accumulated (gs_z_backward takes it on); the caller zeroes it.  Rows no pixel selects
 *                       are not touched.  One atomic per (8 x 8 pixel patch, distinct Gaussian in it). */
int gs_median_depth_backward(const int32_t* median_index, const void* grad_median_depth, int W, int H,
                             int tile_row0, int tile_row1, void* grad_z, void* stream);

/* Per-Gaussian feature vectors composited with the frame's weights (ABI 12; no reference counterpart), fp32.  With
 * alpha_k, the contribute decision, T_k and w_k = alpha_k T_k exactly as gs_render_zalpha forms them (the same code),
 * for pixel p and the list entries k < num_splats_per_pixel[p]:
 *   feature_map[p, c] = sum w_k features[g_k, c]  (c < n_channels),  alpha[p] = sum w_k,  transmittance[p] = T_end,
 * per contributing visit  F[c] = fma(w, f[c], F[c]) for every channel, A += w, T = fma(-alpha, T, T): alpha and
 * transmittance are bit-equal to gs_render_zalpha's, and one channel holding z gives its depth bit for bit.  No
 * background term and no normalisation.
 *   features    [V, n_channels], rows in the index space of sorted_gaussians (visible rows, as xyz_camera_frame)
 *   n_channels  1 .. 32, anything else is GS_EINVAL (callers with more split the channels).  The kernels are
 *               instantiated for 4, 8, 16 and 32 channels; a count in between runs the next one with the channels
 *               beyond n_channels staged as zeros, and nothing beyond column n_channels - 1 is read or written
 *   outputs     feature_map[H,W,n_channels], alpha[H,W], transmittance[H,W]: written for every pixel of the tile rows
 *               [tile_row0, tile_row1), untouched elsewhere.  Empty lists (V == 0) give 0, 0, 1. */
int gs_render_features(const void* packed, const void* features, int n_channels, const int32_t* tile_ranges,
                       const int32_t* sorted_gaussians, const int32_t* num_splats_per_pixel, int W, int H,
                       int tile_row0, int tile_row1, void* feature_map, void* alpha, void* transmittance,
                       void* stream);
/* Backward of the above: the TRUE derivative, decisions held constant, as gs_render_zalpha_backward (no walk quirk;
 * alpha above 0.9999 enters as 0.9999), with c_k = grad_alpha + sum_c grad_feature_map[c] f_k[c] formed as a fused
 * multiply-add chain from grad_alpha over the channels ascending.
 *   grad_feature_map [H,W,n_channels], grad_alpha [H,W]   either may be NULL = all zeros (both NULL: nothing is launched)
 *   grad_slab        [V,9]: columns 3..8 accumulated, columns 0..2 untouched
 *   grad_features    [V,n_channels], accumulated: dL/df[k, c] = sum_pixels w_k g[c]; NULL skips it altogether
 * Both are added into (the slab: one atomic per value per (list entry, tile); grad_features: one per value per
 * (list entry, 8 x 8 patch), from v_mfma_f32_16x16x4_f32 contractions over the patch's pixels); the caller zeroes
 * them.  Rows of Gaussians no pixel uses are not touched. */
int gs_render_features_backward(const void* packed, const void* features, int n_channels, const int32_t* tile_ranges,
                                const int32_t* sorted_gaussians, const int32_t* num_splats_per_pixel,
                                const void* transmittance, const void* grad_feature_map, const void* grad_alpha, int W,
                                int H, int tile_row0, int tile_row1, void* grad_slab, void* grad_features,
                                void* stream);

/* Per-Gaussian contribution statistics of a rendered frame (ABI 15; no reference counterpart), fp32, forward only:
 * the blending weights of the frame reduced over the PIXELS per Gaussian.  Packed records, lists and
 * num_splats_per_pixel as gs_render_zalpha takes them; nothing beyond num_splats_per_pixel is read, so the lists may
 * be prefix-sorted.  For pixel p and the entries k < num_splats_per_pixel[p], alpha_k, the contribute decision and T_k
 * are formed by the code of gs_render_zalpha, w_k = alpha_k T_k, then T = fma(-alpha, T, T): w_k has the bits of the
 * depth kernel's weight.  For every contributing visit of Gaussian g = sorted_gaussians[k], with the row
 * r = row_index ? row_index[g] : g:
 *   weight_sum[r]  += w_k            float.  Added within a tile in a fixed order (lanes, then the tile's four 8 x 8
 *                                    patches), one float atomic per (list entry, tile): a Gaussian inside one tile has
 *                                    a reproducible sum, one in several tiles a sum in the order the tiles arrive
 *   weight_max[r]   = max(., w_k)    float.  The weights are positive, so the maximum is taken as an integer atomic on
 *                                    the bits: independent of any order, bit-reproducible.  The caller starts it at 0
 *                                    (any non-negative float is a valid start; negative values are not)
 *   pixel_count[r] += 1              int32, exact: the pixels the Gaussian contributes to
 * All three are ACCUMULATED, so a caller sweeps many views into the same buffers; any of them may be NULL, which
 * skips it (all three NULL: the arguments are checked, nothing is launched, GS_OK).  Rows of Gaussians no pixel uses
 * are not touched, bit for bit.
 *   row_index  NULL or int32[V]: the caller's row of each visible Gaussian (the frame's vis_idx), so that a sweep
 *              accumulates straight into [N] arrays -- no [V] temporary, no scatter
 * GS_EINVAL with a gs_last_error() text for an empty image, bad tile rows, NULL tile_ranges / num_splats_per_pixel or
 * a packed pointer that is not 16-byte aligned.  Empty lists (V == 0) touch nothing. */
int gs_render_contributions(const void* packed, const int32_t* tile_ranges, const int32_t* sorted_gaussians,
                            const int32_t* num_splats_per_pixel, const int32_t* row_index, int W, int H,
                            int tile_row0, int tile_row1, void* weight_sum, void* weight_max,
                            int32_t* pixel_count, void* stream);
/* Measurement aid (ABI 15; scripts/contributions_cost.py): the list entries gs_render_contributions stages per step
 * from the next call on, 64 (the default, the backward walks' chunk) or 256 (the forward walks'); 0 only asks.
 * -> the value before the call.  Both instantiations compute the same statistics. */
int gs_debug_contributions_chunk(int chunk);

/* Cost-balanced bands (multi-GPU; no reference counterpart): the band images of unequal bands are all-gathered as
 * equal chunks of chunk_rows = 16 x (tallest band) + 1 pixel rows, each starting at its rank's band; the last row of
 * a chunk carries the per-tile-row costs of that band (floats; 0 outside the band).
 *   gs_band_row_costs   cost_row[r] = sum over the tiles of row r of min(list length, cap) + tile_cost per tile, for
 *                       r in [tile_row0, tile_row1), 0 elsewhere (n_tile_rows floats)
 *   gs_band_assemble    gathered float[G][chunk_rows][3 W] -> image float[H][3 W] (pixel row y from the chunk of the
 *                       band that holds tile row y / 16, band_rows = the G + 1 boundaries, HOST array) and
 *                       host_costs float[n_tile_rows] (device-accessible PINNED host memory: the summed cost rows,
 *                       what balances the next frame's bands; record an event behind the call and wait for it) */
int gs_band_row_costs(const int32_t* tile_ranges, int n_tiles_x, int n_tile_rows, int tile_row0, int tile_row1,
                      int tile_cost, int cap, void* cost_row, void* stream);
int gs_band_assemble(const void* gathered, const int32_t* band_rows, int G, int chunk_rows, int W, int H, int n_tile_rows,
                     void* image, void* host_costs, void* stream);
/* ---- multi-GPU: tile-row bands with owner-sliced gradients ------------------------------------
 * (no reference counterpart: the reference is single-GPU; BASELINE.json north_star asks for frames
 * sharded by tile rows over up to 8 GPUs.)  Rank b renders tile rows [band_rows[b], band_rows[b+1]);
 * rank r owns the Gaussians [256*owner_blocks[r], 256*owner_blocks[r+1]) and runs the per-Gaussian
 * backward for them, so the partial render gradients of the bands are exchanged sparsely: a row
 * travels only from a rank whose band the Gaussian's candidate tile window reaches to its owner.
 *
 * gs_halo_plan (after gs_preprocess_forward of the same frame; inputs are the capacity-N buffers
 * and the device-side visible_count):
 *   mask[N]        bit s = visible Gaussian v reaches the band of rank s
 *   send_index[N]  the visible indices with bit `rank`, ascending: row k of the send buffer is
 *                  grad_slab[send_index[k]]; consecutive owners' parts, plan[4 + r] rows for owner r
 *   plan[4 + 2G]   device record for the frame's host read: number of rows in send_index, V,
 *                  v_lo, v_hi (visible-index range of the Gaussians this rank owns),
 *                  send counts [G], receive counts [G]
 *   workspace      int32[gs_halo_workspace_ints(N, G)], read again by gs_halo_gather_sum
 * band_rows, owner_blocks: host arrays of G + 1 ints.  G <= GS_MAX_RANKS.
 *
 * gs_halo_gather_sum (after the all_to_all): recv holds, for sender s = 0..G-1 at row offset
 * recv_offsets[s] (host array, the exclusive prefix of the receive counts), the rows of the
 * Gaussians v in [v_lo, v_hi) with bit s, ascending; out[(v - v_lo) * 9 ..] = their sum, every
 * row of the range written once (zeros where no band reaches the Gaussian). */
#define GS_MAX_RANKS 8
size_t gs_halo_workspace_ints(int N, int G);
int gs_halo_plan(const void* uvs, const void* conic, int N, const int32_t* visible_count,
                 const int32_t* preprocess_workspace, int n_tiles_x, int n_tiles_y, float mh_dist,
                 const int32_t* band_rows, const int32_t* owner_blocks, int G, int rank,
                 uint32_t* mask, int32_t* workspace, int32_t* send_index, int32_t* plan,
                 void* stream);
int gs_halo_gather_sum(const uint32_t* mask, const int32_t* workspace, int N, int G, int rank,
                       int v_lo, int v_hi, const void* recv, const int32_t* recv_offsets,
                       void* out, void* stream);

/* ---- multi-GPU: band-compact per-Gaussian stage (ABI 5; no reference counterpart) -------------------------
 * A rank evaluates the per-Gaussian stage in full only for the Gaussians that can reach its band, into arrays
 * compacted to those rows.
 * gs_band_project: for every Gaussian the transform, projection and frustum cull of gs_preprocess_forward (same
 *   culling_mask, rank, vis_idx, uv[V,2], opacity_act[V], visible_count, camera_center, workspace), plus mask[V]:
 *   bit s = the Gaussian can reach the tile rows [band_rows[s], band_rows[s+1]) -- its candidate window
 *   (tile_culling.cu:138-156) bounded from the largest scale, a superset of the exact window that needs no
 *   covariance and is the same on every rank.  halo_workspace: int32[gs_halo_workspace_ints(N, G)].
 * gs_halo_plan_masked: gs_halo_plan's send list, split sizes and gather layout from those masks.
 * gs_preprocess_forward_list: rows l < *list_count of `list` (visible indices, ascending: the send list): Sigma, J,
 *   conic, SH colour and the packed record of Gaussian vis_idx[list[l]], written at row l of uv_l[.,2],
 *   xyz_camera_frame_l[.,3], conic_l[.,3], packed_l[.,12] (capacity rows allocated).  Bit-identical to the rows
 *   gs_preprocess_forward writes.  Binning, sort and render take the compact arrays (visible_count = list_count);
 *   the render-gradient slab [rows, 9] of the band is then the send buffer of the gradient exchange. */
int gs_band_project(const void* xyz, const void* scale, const void* opacity, const void* camera_T_world, const void* K,
                    int N, int W, int H, float near_thresh, float far_thresh, float cull_mask_padding, float mh_dist,
                    const int32_t* band_rows, int G, int32_t* workspace, void* camera_center, int32_t* visible_count,
                    uint8_t* culling_mask, int32_t* rank, int32_t* vis_idx, void* uv, void* opacity_act, uint32_t* mask,
                    int32_t* halo_workspace, void* stream);
int gs_halo_plan_masked(const uint32_t* mask, int N, const int32_t* visible_count,
                        const int32_t* preprocess_workspace, const int32_t* owner_blocks, int G, int rank,
                        int32_t* workspace, int32_t* send_index, int32_t* plan,
                        int32_t* plan_host /* NULL, or 4 + 2 G ints of device-accessible pinned host memory: a copy of
                                              plan, written by the same kernel (the host read without a copy) */,
                        void* stream);
int gs_preprocess_forward_list(const void* xyz, const void* quaternion, const void* scale, const void* rgb, const void* sh,
                               int n_sh, const void* camera_T_world, const void* K, const void* camera_center,
                               const int32_t* list, const int32_t* list_count, int capacity, const int32_t* vis_idx,
                               const void* uv, const void* opacity_act, void* uv_l, void* xyz_camera_frame_l, void* conic_l,
                               void* packed_l, void* stream);

/* ---- touch masks handed from the render forward to the render backward (ABI 8; no reference counterpart) -------
 * The fused backward walks the lists its forward walked and needs the same (64 entries x 4 patches) touch masks.  The
 * `_m` forms of the fused frame's three render entries take touch_masks: uint64[n_tiles_of_the_GRID * 16 * 4] (512 bytes
 * per tile; NULL = the forms without `_m`).  The forward (its repair pass included) stores the masks of the first 1024
 * list entries of every tile it renders: touch_masks[(tile * 16 + word) * 4 + patch]; the backward reads them instead
 * of evaluating 256 ellipse-rectangle tests per 64-entry chunk, and builds the words beyond itself.  Results are
 * bit-identical with and without.  The buffer must be the one the SAME frame's forward wrote. */
int gs_render_tiles_prefix_phased_m(const void* packed, const void* rgb, const int32_t* tile_ranges,
                                    int32_t* sorted_gaussians, const uint64_t* keys, int64_t S,
                                    const void* background_rgb, int W, int H, int tile_row0, int tile_row1,
                                    int32_t* tile_flags, int32_t* num_splats_per_pixel, void* final_weight_per_pixel,
                                    void* image, int32_t* tile_cost, void* segment_state, int phases, uint64_t* touch_masks,
                                    void* stream);
int gs_render_tiles_cut_m(const void* packed, const void* rgb, const int32_t* tile_ranges, const int32_t* sorted_gaussians,
                          int64_t S, const int32_t* full_ranges, const void* bin_records, int N, float mh_dist,
                          int32_t* workspace, int32_t* cut_workspace, uint64_t* overflow_keys, int32_t* overflow_sorted,
                          int64_t overflow_capacity, const void* background_rgb, int W, int H, int tile_row0, int tile_row1,
                          int32_t* tile_flags, int32_t* num_splats_per_pixel, void* final_weight_per_pixel, void* image,
                          int32_t* tile_cost, int32_t* host_flagged, uint64_t* touch_masks, void* stream);
int gs_render_tiles_backward_slab_m(const void* packed, const void* rgb, const int32_t* tile_ranges,
                                    const int32_t* sorted_gaussians, const void* background_rgb,
                                    const int32_t* num_splats_per_pixel, const void* final_weight_per_pixel,
                                    const void* grad_image, int W, int H, int tile_row0, int tile_row1, void* grad_slab,
                                    int64_t zero_slab_rows, const int32_t* tile_cost, int32_t* tile_order,
                                    const void* segment_state, const int32_t* cut_flags, const int32_t* full_ranges,
                                    const int32_t* overflow_sorted, int backward_mode, const uint64_t* touch_masks,
                                    void* stream);
/* The absgrad form of gs_render_tiles_backward_slab_m (ABI 18; AbsGS, gsplat's absgrad=True): the same walk in every
 * mode -- tile order, depth segments, depth-cut overflow lists, handed-over touch masks, compat and exact backward
 * modes, the prologue conventions of zero_slab_rows / tile_cost / tile_order -- and the same nine sums into
 * grad_slab[V, 9].  Next to them it accumulates, per Gaussian, the per-pixel MAGNITUDES of the terms whose signed sum is
 * the slab's uv pair: with g_u(p, k), g_v(p, k) the contribution of pixel p's visit of list entry k to grad_u, grad_v,
 *   grad_uv_abs[g, 0] += sum |g_u(p, k)|,   grad_uv_abs[g, 1] += sum |g_v(p, k)|
 * over the (pixel, entry) pairs the colour backward adds up (same contribute / stop / background decisions, alpha
 * capped at 0.9999 the same way, the reference's Q1 weight quirk in compat mode the same way), so that
 * grad_uv_abs[g, j] >= |grad_slab[g, 4 + j]| up to rounding.  Opposite-signed terms of a large Gaussian cancel in the
 * slab and add here: the densification signal that does not miss such Gaussians.
 * grad_uv_abs: float32 [V, 2], ACCUMULATED onto -- the caller clears it (zero_slab_rows covers the slab only); rows of
 * Gaussians no pixel used are not touched.  NULL returns GS_EINVAL.  fp32, one colour coefficient per channel. */
int gs_render_tiles_backward_slab_abs(const void* packed, const void* rgb, const int32_t* tile_ranges,
                                      const int32_t* sorted_gaussians, const void* background_rgb,
                                      const int32_t* num_splats_per_pixel, const void* final_weight_per_pixel,
                                      const void* grad_image, int W, int H, int tile_row0, int tile_row1, void* grad_slab,
                                      int64_t zero_slab_rows, const int32_t* tile_cost, int32_t* tile_order,
                                      const void* segment_state, const int32_t* cut_flags, const int32_t* full_ranges,
                                      const int32_t* overflow_sorted, int backward_mode, const uint64_t* touch_masks,
                                      void* grad_uv_abs, void* stream);

/* ---- multi-GPU: the fused band frontend (ABI 8; no reference counterpart) --------------------------------------
 * gs_band_frontend = gs_band_project + gs_halo_plan_masked + gs_preprocess_forward_list in four launches instead of
 * nine, with every count taken per 256-block of the GAUSSIAN index (owner slices are whole such blocks, so the
 * exchange plan is 2 G differences of scanned offsets).  Same outputs, bit for bit: culling_mask[N], rank[N]
 * (Gaussian -> visible index or -1), uv[V,2] and opacity_act[V] by visible index, camera_center; the send list
 * send_index[L] (visible indices with this rank's band bit, ascending) and, at its rows l, list_g[L] (their Gaussian
 * indices) and the band-compact arrays uv_l[L,2], xyz_camera_frame_l[L,3], conic_l[L,3], packed_l[L,12]; plan[4 + 2G]
 * = (L, V, v_lo, v_hi, send counts[G], receive counts[G]) on the device and -- plan_host != NULL -- the same ints
 * in device-accessible pinned host memory.  All row arrays need capacity N.  workspace:
 * int32[gs_band_frontend_workspace_ints(N, G)] = per-block counts and scanned offsets of the visible Gaussians and of
 * every band's Gaussians, and a 16-bit mask per Gaussian (bit 15 = visible, bit s = can reach band s); it is read
 * again by the two calls below.  band_rows, owner_blocks: host arrays of G + 1 ints.
 * gs_band_gather_sum (after the all_to_all; recv / recv_offsets as for gs_halo_gather_sum): out[(v - v_lo) * 9 ..] =
 *   the sum over the senders, ascending, of the received rows of every visible Gaussian this rank owns.
 * gs_preprocess_backward_gathered: gs_preprocess_backward for the owned slice (pointers of xyz, quaternion, scale,
 *   rank_of_gaussian and of the six gradients start at Gaussian 256 * owner_blocks[rank]; n rows) with the
 *   render-gradient row of each Gaussian summed on the spot from recv instead of read from a slab -- the same bits as
 *   gs_band_gather_sum followed by gs_preprocess_backward, one launch and one [owned, 9] round trip less. */
size_t gs_band_frontend_workspace_ints(int N, int G);
int gs_band_frontend(const void* xyz, const void* quaternion, const void* scale, const void* opacity, const void* rgb,
                     const void* sh, int n_sh, const void* camera_T_world, const void* K, int N, int W, int H,
                     float near_thresh, float far_thresh, float cull_mask_padding, float mh_dist, const int32_t* band_rows,
                     const int32_t* owner_blocks, int G, int rank, int32_t* workspace, void* camera_center,
                     uint8_t* culling_mask, int32_t* rank_out, void* uv, void* opacity_act, int32_t* send_index,
                     int32_t* list_g, void* uv_l, void* xyz_camera_frame_l, void* conic_l, void* packed_l, int32_t* plan,
                     int32_t* plan_host, void* stream);
int gs_band_gather_sum(const int32_t* workspace, int N, int G, int rank, const int32_t* owner_blocks,
                       const int32_t* rank_of_gaussian, int v_lo, const void* recv, const int32_t* recv_offsets, void* out,
                       void* stream);
int gs_preprocess_backward_gathered(const void* xyz, const void* quaternion, const void* scale, int n_sh,
                                    const void* camera_T_world, const void* K, const void* camera_center,
                                    const int32_t* rank_of_gaussian, const void* opacity_act, const int32_t* workspace,
                                    int N_total, int G, int rank, const int32_t* owner_blocks, const void* recv,
                                    const int32_t* recv_offsets, int n, void* grad_xyz, void* grad_quaternion,
                                    void* grad_scale, void* grad_opacity_logit, void* grad_rgb_param, void* grad_sh,
                                    void* stream);

/* ---- training-loop operations behind the rasterizer ------------------------------
 * gs_adam_step: torch.optim.Adam.step() as the reference uses it (splat_py/optimizer_manager.py:15-42
 * builds the optimizer with one group per parameter tensor and a learning rate each; trainer.py:376
 * steps it): defaults amsgrad=False, weight_decay=0, maximize=False.  One launch updates up to 8
 * parameter tensors in place.  params/grads/exp_avg/exp_avg_sq: host arrays of n_groups device
 * pointers (fp32, numel[k] elements each); lr[k], step[k] (the 1-based step count AFTER the
 * increment, per tensor as in torch's state["step"]); beta1, beta2, eps as the Python floats.
 * Update order == torch/optim/adam.py _single_tensor_adam on the ATen CPU kernels. */
int gs_adam_step(int n_groups, void* const* params, const void* const* grads, void* const* exp_avg,
                 void* const* exp_avg_sq, const int64_t* numel, const double* lr,
                 const int64_t* step, double beta1, double beta2, double eps, void* stream);
/* gs_adam_step restricted to the rows a frame saw (ABI 13; the `sparse_adam` / SelectiveAdam of other trainers).
 * Tensor k is [n_rows, row_width[k]] (numel[k] == n_rows * row_width[k], row_width[k] >= 1); skip_row: n_rows bytes on
 * the device, nonzero = leave the row alone (a bool culling mask as the rasterizer returns it).
 *   rows with skip_row[r] == 0   params / exp_avg / exp_avg_sq take exactly gs_adam_step's update with the same lr[k],
 *                                step[k], betas and eps: bit-identical to a dense step restricted to those rows
 *   rows with skip_row[r] != 0   every bit of params / exp_avg / exp_avg_sq is unchanged (NaN payloads and infinities
 *                                included: no arithmetic touches them); grads is not read there
 * step[k] is the global count (it advances whether or not a row was seen).  One launch for up to 8 tensors; a float4
 * chunk without a visible element is neither loaded nor stored, so the traffic follows the visible rows where they
 * are contiguous or wide (28 B per visible element plus n_rows mask bytes per tensor).  n_rows == 0 returns GS_OK
 * without a launch; skip_row may be NULL only then. */
int gs_adam_step_rows(int n_groups, void* const* params, const void* const* grads, void* const* exp_avg,
                      void* const* exp_avg_sq, const int64_t* numel, const int64_t* row_width,
                      const void* skip_row, int64_t n_rows, const double* lr, const int64_t* step, double beta1,
                      double beta2, double eps, void* stream);
/* Measurement aid (ABI 7; bench.py `roofline.hbm_copy_gbs_measured`): a float4 grid-stride stream copy of `bytes` bytes
 * (multiple of 16, as are both pointers) with `blocks` workgroups of 256 lanes, non-temporal loads and stores.
 * No reference counterpart. */
int gs_stream_copy(void* dst, const void* src, size_t bytes, int blocks, void* stream);
/* Densification statistics of trainer.py:378-385 in one pass and without the boolean-mask
 * index_put: for every Gaussian i with rank[i] >= 0 (its visible index; -1 = culled)
 *   uv_grad_accum[i] += |uv_grad[rank[i]] * (K[0,0], K[1,1])|,  grad_accum_count[i] += 1
 * (K: the device-resident fp32 3x3 intrinsics, read on the device: no host sync)
 * and for every i  xyz_grad_accum[i] += |xyz_grad[i]|  (skipped when xyz_grad is NULL).
 * uv_grad: rows of 2 floats, uv_row_stride floats apart (9 for the view of the fused path's slab). */
int gs_accumulate_grad_stats(const void* uv_grad, int uv_row_stride, const int32_t* rank,
                             const void* xyz_grad, const void* K, int N, void* uv_grad_accum,
                             void* xyz_grad_accum, int32_t* grad_accum_count, void* stream);

/* The training loss of trainer.py:363-374, value and gradient in one call:
 *   loss = (1 - ssim_frac) * l1_loss(image, target) + ssim_frac * (1 - SSIM(image, target))
 * SSIM = torchmetrics 1.2.1 StructuralSimilarityIndexMeasure(data_range=1.0) (trainer.py:24): 11x11
 * Gaussian window (sigma 1.5), k1 0.01, k2 0.03, mean over the pixels whose window lies inside the
 * image.  image, target: [H, W, 3] fp32 (the rasterizer's layout; H, W > 10).
 * loss_out: float[4] = (loss, l1, ssim, mse) -- mse is the trainer's debug l2_loss (trainer.py:366-367,
 * psnr = -10 log10(mse)).  grad_image: [H, W, 3] = d loss / d image, or NULL.
 * workspace: gs_ssim_l1_workspace_bytes(H, W) bytes (per-tile partial sums, reduced in a fixed order). */
size_t gs_ssim_l1_workspace_bytes(int H, int W);
int gs_ssim_l1_loss(const void* image, const void* target, int H, int W, float ssim_frac,
                    void* workspace, void* loss_out, void* grad_image, void* stream);

/* Adaptive density control, the data movement of splat_py/trainer.py:114-206 (delete / clone / split) and
 * of splat_py/optimizer_manager.py:78-172 (the same surgery on Adam's exp_avg / exp_avg_sq) in one pass:
 * every source row is read once and every row of the new Gaussian set is written once, for up to 8
 * parameter tensors (fp32, `width[k]` floats per row, N0 rows) together with their optimizer state
 * (src_exp_avg[k] / src_exp_avg_sq[k]: NULL when the tensor has no state yet).  The per-row decisions
 * come as destination indices (gaussian_splatting_amd/densify.py forms them from the reference's masks
 * with prefix sums; -1 = does not apply):
 *   dst_self[i]     row of Gaussian i in the new set when it survives unsplit (parameters + state copied)
 *   dst_clone[i]    row of its clone (trainer.py:123-161): parameters copied, xyz - 0.01 * xyz_grad_accum /
 *                   grad_accum_count, optimizer state zero
 *   split_self[i], split_clone[i]   rank among the n_split split rows when the Gaussian (its clone) is
 *                   split (trainer.py:163-206): `samples` new rows at sample_base + s * n_split + rank with
 *                   xyz + R(q / |q|) (random * exp(scale)), scale = log(exp(scale) / split_scale_factor),
 *                   quaternion = q / |q|, the rest copied, optimizer state zero
 * kind[k]: 0 plain, 1 xyz, 2 scale (log), 3 quaternion (w, x, y, z) -- the tensors the split transforms;
 * xyz / scale / quaternion: the SOURCE tensors again (read by the transform whatever tensor a thread moves);
 * random_samples: [n_split * samples, 3] uniform numbers in the order of trainer.py:176.
 * The destination tensors are caller-allocated with the new row count and must not alias the sources. */
int gs_densify_move(int n_tensors, const void* const* src, void* const* dst, const void* const* src_exp_avg,
                    void* const* dst_exp_avg, const void* const* src_exp_avg_sq, void* const* dst_exp_avg_sq,
                    const int32_t* width, const int32_t* kind, int N0, const int32_t* dst_self,
                    const int32_t* dst_clone, const int32_t* split_self, const int32_t* split_clone,
                    const void* xyz, const void* scale, const void* quaternion, const void* xyz_grad_accum,
                    const int32_t* grad_accum_count, const void* random_samples, int n_split, int samples,
                    int sample_base, float split_scale_factor, void* stream);

/* ---- MCMC densification (ABI 17; no reference counterpart) --------------------------------------------------------
 * The device side of "3D Gaussian Splatting as Markov Chain Monte Carlo" (gaussian_splatting_amd/densify.py:
 * MCMCController): training at a fixed budget of Gaussians, dead ones relocated onto live ones, positions perturbed by
 * covariance-shaped noise every iteration.  All tensors fp32. */
#define GS_MCMC_MAX_RATIO 51   /* a Gaussian sampled more often is corrected as one of 51 copies */
/* Relocation, IN PLACE and many-to-one: up to 8 tensors params[k] of [n_rows, width[k]] floats with their Adam moments
 * (exp_avg[k] / exp_avg_sq[k]: both NULL when the tensor has no state yet).  kind[k]: 0 plain, 2 scale (log, width 3)
 * as in gs_densify_move, 4 opacity (logit, width 1); exactly one opacity and one scale tensor, else GS_EINVAL with a
 * gs_last_error() text.  ratio[r] = 1 + the number of times row r was drawn as a source.  Two launches, one after the
 * other on `stream`, no temporary buffer, no address written by two threads:
 *   A  every row r with ratio[r] > 1, n = min(ratio[r], GS_MCMC_MAX_RATIO), x its opacity logit:
 *        o         = min(1 / (1 + exp(-x)), 1 - 2^-24)
 *        o_new     = 1 - (1 - o)^(1/n)
 *        denom     = sum_{i=1..n} sum_{k=0..i-1} C(i-1,k) (-1)^k o_new^(k+1) / sqrt(k+1)
 *        scale[c] += log(o / denom)                                          c = 0..2
 *        opacity   = logit(min(max(o_new, min_opacity), 1 - 2^-24))
 *      evaluated in double and rounded once to fp32 (fp32 loses up to four digits of the alternating sum); both
 *      moments of the row become 0 in every tensor that has them.  A row with ratio[r] <= 1 is neither read nor
 *      written: every bit of it stays, NaN payloads included.
 *   B  for every m < M, row src_rows[m] (as A left it) is copied to row dst_rows[m] in every tensor and the moments of
 *      the destination row become 0.
 * Preconditions, documented and not checked: the dst_rows are distinct, no destination row is a source, every
 * src_rows[m] has ratio > 1, all rows are in [0, n_rows).  M == 0 or n_rows == 0 returns GS_OK without a launch;
 * ratio, dst_rows and src_rows may be NULL only then. */
int gs_mcmc_relocate(int n_tensors, void* const* params, void* const* exp_avg, void* const* exp_avg_sq,
                     const int32_t* width, const int32_t* kind, int n_rows, const int32_t* ratio /*[n_rows]*/,
                     const int32_t* dst_rows /*[M]*/, const int32_t* src_rows /*[M]*/, int M,
                     float min_opacity, void* stream);
/* The position noise of every iteration, one launch, xyz[N,3] modified in place:
 *   o    = 1 / (1 + expf(-opacity))                           opacity[N,1] logits
 *   gate = 1 / (1 + expf(-gate_k * ((1 - o) - gate_x0)))      ~1 for a nearly transparent Gaussian, ~0 for a solid one
 *   S    = Sigma_world(quaternion, scale)                     as gs_compute_sigma_world: q normalised, exp(scale)
 *   e    = noise * (gate * step)                              noise[N,3]: the caller's standard normal samples
 *   xyz[r] += (S[3r] * e0 + S[3r+1] * e1) + S[3r+2] * e2      r = 0..2
 * in fp32 with the roundings as written (no contraction); expf is the library's IEEE-only exponential, so the result
 * is a function of the inputs' bits.  68 bytes per Gaussian, 56 read and 12 written.  quaternion must be 16-byte
 * aligned.  N == 0 launches nothing. */
int gs_mcmc_add_noise(void* xyz, const void* quaternion, const void* scale, const void* opacity,
                      const void* noise /*[N,3]*/, int N, float step, float gate_k, float gate_x0,
                      void* stream);

/* ---- Bilateral-grid colour correction (ABI 23; no reference counterpart) ------------------------------------------
 * Per-image appearance compensation between the rendered image and the loss ("Bilateral Guided Radiance Field
 * Processing"; gaussian_splatting_amd/bilagrid.py).  All tensors fp32.
 *   grid  [12, L, Hg, Wg]   channel 4r + j is entry (r, j) of a 3x4 affine A;  L, Hg, Wg >= 1
 *   image [H, W, 3]         the rasterizer's layout;  H, W >= 1
 * Pixel (px, py) samples the grid at gx = (px + 0.5) / W (Wg - 1), gy = (py + 0.5) / H (Hg - 1) and
 * gz = clamp(0.299 R + 0.587 G + 0.114 B, 0, 1) (L - 1), trilinearly: per axis of n nodes i0 = min(floor(g),
 * max(n - 2, 0)), i1 = min(i0 + 1, n - 1), f = g - i0, interpolated as a0 + f (a1 - a0) (x, then y, then z), and
 *   out[p, r] = A[r,0] R + A[r,1] G + A[r,2] B + A[r,3].
 * The xy cell is computed in integers, i0 = (2 px + 1)(Wg - 1) div (2 W), and f is one division of exact integers.
 * A grid whose every node is the identity affine returns the image's bits.  This is grid_sample(mode="bilinear",
 * align_corners=True, padding_mode="border") over (gx, gy, gz), followed by the affine.
 * Limits: H, W < 2^23, W Wg and H Hg < 2^30, 12 L Hg Wg < 2^31; otherwise GS_EINVAL. */
int gs_bilagrid_slice(const void* grid, const void* image, int H, int W, int L, int Hg, int Wg, void* out,
                      void* stream);
/* Its backward for grad_out [H, W, 3]; either output may be NULL and is then skipped.
 *   grad_grid[4r + j, z, y, x] = sum over the pixels of w_z w_y w_x grad_out[p, r] (R, G, B, 1)[j]
 *   grad_image[p, j]           = sum_r A[r,j] grad_out[p,r] + (0.299, 0.587, 0.114)[j] dz(p)
 *   dz(p) = (L - 1) sum_r grad_out[p,r] ((dA/dgz)[r,:3] . rgb + (dA/dgz)[r,3]), dA/dgz the z-lerp's a1 - a0 interpolated
 *           in x and y; dz = 0 where the luma is <= 0 or >= 1 and for L = 1 (the border clamp's derivative)
 * grad_grid is reduced without atomics: partial sums per chunk of the pixels of one xy cell go to `workspace`
 * (gs_bilagrid_workspace_bytes(H, W, L, Hg, Wg) bytes; required iff grad_grid is not NULL) and a second launch sums
 * them per node in index order.  Two calls on the same inputs return the same bits; every element of grad_grid is
 * written, nodes that no pixel reaches as exact zeros. */
size_t gs_bilagrid_workspace_bytes(int H, int W, int L, int Hg, int Wg);
int gs_bilagrid_slice_backward(const void* grid, const void* image, const void* grad_out, int H, int W, int L, int Hg,
                               int Wg, void* workspace, void* grad_image, void* grad_grid, void* stream);
/* Total variation of grids [n_grids, 12, L, Hg, Wg]: the sum over the three grid axes of two or more nodes of the
 * mean of (G[.. i + 1 ..] - G[.. i ..])^2 over all adjacent pairs of that axis (all grids, all channels); an axis of
 * one node contributes zero.  tv_out: float[1]; grad_grids: d tv / d grids in the grids' layout, or NULL.
 * workspace: gs_bilagrid_tv_workspace_bytes bytes of fp64 per-workgroup partial sums, reduced in a fixed order. */
size_t gs_bilagrid_tv_workspace_bytes(int64_t n_grids, int L, int Hg, int Wg);
int gs_bilagrid_tv(const void* grids, int64_t n_grids, int L, int Hg, int Wg, void* workspace, void* tv_out,
                   void* grad_grids, void* stream);

/* ---- TSDF fusion and mesh extraction (ABI 24; no reference counterpart) -------------------------------------------
 * Depth maps to a triangle mesh (gaussian_splatting_amd/mesh.py): fuse rendered depth maps into a
 * truncated signed distance volume, then triangulate a level set of it.  fp32, no contraction, IEEE divide and square
 * root; no atomics, no scratch.
 *
 * The volume has nx x ny x nz nodes; node (i, j, k) sits at origin + voxel_size (i, j, k) in world coordinates (each
 * coordinate origin_a + voxel_size * (float)index).  Arrays put x fastest: n = (k ny + j) nx + i, in 64 bits.
 *     tsdf   [nz, ny, nx]      fresh: 1        weight [nz, ny, nx]   fresh: 0        color [nz, ny, nx, 3] or NULL   fresh: 0
 * Limits: ny <= 262140, nz <= 65535 (the launch grid), else GS_EINVAL.
 *
 * gs_tsdf_integrate fuses C views of one size (W, H) in one launch: depth [C, H, W] is the camera-frame z
 * (gs_render_median_depth's, or depth / alpha), image [C, H, W, 3] or NULL, camera_T_world [C, 4, 4] and K [C, 3, 3] as
 * gs_filter3d_rate takes them.  A pixel is invalid where its depth is <= 0, not finite or > depth_max.  For the node at p
 * the views are taken in the order c = 0 .. C - 1:
 *     pc = camera_T_world_c p                       (csrc/pg_math.h to_camera); skip unless pc.z > near_thresh
 *     (u, v) = the model's own projection           (GS_RASTER_CLASSIC: fx x / z + cx; GS_RASTER_FISHEYE: the equidistant one)
 *     px = floor(u + 0.5), py = floor(v + 0.5)      the renderer's integer pixel coordinate, no half-pixel offset; skip
 *                                                   outside [0, W) x [0, H)
 *     d = depth[c, py, px]                          skip if invalid
 *     sdf = (d - pc.z) * (|pc| / pc.z)              |pc| = sqrt(x x + y y + z z): the signed distance ALONG THE RAY, so the
 *                                                   band has one metric width at every view angle; skip unless
 *                                                   sdf >= -sdf_trunc
 *     t = min(1, sdf / sdf_trunc),  W1 = W + 1,  tsdf = (tsdf W + t) / W1,  each colour channel likewise with the
 *     pixel's colour,  W = min(W1, max_weight)
 * A node that no view updates is not written: it keeps every bit.  One call with C views gives the bits of C calls with
 * one view each in the same order (the state is carried in fp32 registers).  Giving exactly one of image and color, a
 * raster_mode that is neither value, a negative count, sdf_trunc or max_weight not > 0, a parameter that is not a number
 * or a NULL pointer is GS_EINVAL and writes nothing; C == 0, an empty image or an empty volume returns GS_OK without a
 * launch.  depth_max may be infinite. */
int gs_tsdf_integrate(const void* depth, const void* image, const void* camera_T_world, const void* K, int C, int W, int H,
                      int raster_mode, float near_thresh, float sdf_trunc, float max_weight, float depth_max,
                      float origin_x, float origin_y, float origin_z, float voxel_size, int nx, int ny, int nz, void* tsdf,
                      void* weight, void* color, void* stream);
/* Marching tetrahedra on the Kuhn split of each cell, in two passes with a scan by the caller between them.
 * Cell (i, j, k), i < nx - 1, j < ny - 1, k < nz - 1, has the 8 corner nodes (i..i+1, j..j+1, k..k+1) and the linear index
 * of its low corner.  It is ACTIVE iff all 8 corners have weight >= min_weight (> 0).  A corner is INSIDE iff
 * f = tsdf - level < 0.  Tetrahedron q = 0..5 of a cell is {v0, v1, v2, v3} = {000, e_a, e_a + e_b, 111} with (a, b, c) =
 * xyz, xzy, yxz, yzx, zxy, zyx.  Every tetrahedron edge points in one of the directions e = 0..6: (1,0,0) (0,1,0) (0,0,1)
 * (1,1,0) (1,0,1) (0,1,1) (1,1,1), and is owned by its lower node.
 *   Vertices: edge (n, e) carries one iff it lies in at least one active cell and its ends differ in sign.  With a the
 *     owning node and b the other end, s = f_a / (f_a - f_b), position = origin + voxel_size ((i, j, k) + s dir_e), colour =
 *     color_a + s (color_b - color_a).  Vertices are numbered in ascending (n, e).
 *   Faces: a tetrahedron of an active cell with 1 or 3 corners inside gives one triangle through its three cut edges, one
 *     with 2 inside (p < q in tetrahedron order, r < s outside) the quad pr, ps, qs, qr as the two triangles (pr, ps, qs) and
 *     (pr, qs, qr): the quad is split along the diagonal pr - qs.  Every triangle is wound so that its normal points
 *     towards positive tsdf (free space, the cameras); which corner of a triangle comes first is not specified.  Faces are
 *     int32 triples of vertex numbers, ordered by (cell, q, triangle).  The mesh is watertight wherever active cells meet.
 * gs_tsdf_extract_count writes, per node n: edge_mask [N] uint8 (bit e: edge (n, e) carries a vertex), vert_count [N]
 *   int32 (its popcount) and face_count [N] int32 (the triangles of cell n; 0 for a node that is no cell's low corner).
 *   workspace: gs_tsdf_extract_workspace_bytes(nx, ny, nz) bytes (one activity byte per cell).
 * gs_tsdf_extract_emit takes vert_offset and face_offset [N] int32, the EXCLUSIVE prefix sums of the two counts (the caller
 *   has checked that the totals are <= 2^31 - 1), and writes vertices [Nv, 3], colors [Nv, 3] (iff color is given; exactly
 *   one of the two is GS_EINVAL) and faces [Nf, 3].  Each vertex is computed once; a vertex id is found as vert_offset[owner] +
 *   popcount(edge_mask[owner] & ((1 << e) - 1)).  No atomics: two calls on the same volume return the same bits.
 * Both: a negative size or one over the limits, min_weight not > 0, a parameter that is not a number or a NULL pointer is
 * GS_EINVAL and writes nothing; an empty volume returns GS_OK without a launch. */
size_t gs_tsdf_extract_workspace_bytes(int nx, int ny, int nz);
int gs_tsdf_extract_count(const void* tsdf, const void* weight, int nx, int ny, int nz, float level, float min_weight,
                          void* workspace, void* edge_mask, int32_t* vert_count, int32_t* face_count, void* stream);
int gs_tsdf_extract_emit(const void* tsdf, const void* color, const void* edge_mask, const int32_t* vert_offset,
                         const int32_t* face_offset, const int32_t* face_count, int nx, int ny, int nz, float level,
                         float origin_x, float origin_y, float origin_z, float voxel_size, void* vertices, void* colors,
                         int32_t* faces, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GSPLAT_HIP_H */
