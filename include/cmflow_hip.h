/*
 * cmflow_hip.h -- C ABI of libcmflow_hip.so, the MI355X (gfx950) drop-in for the native
 * layer of the CMFlow hot path.
 *
 * Conventions (all entry points):
 *   - plain pointers to DEVICE memory + sizes; no torch / ATen types cross this boundary.
 *   - `stream` is a hipStream_t passed as void* (NULL = the legacy default stream).  Work is
 *     enqueued asynchronously, nothing is synchronised, nothing is retained after return --
 *     same threading model as the reference wrappers, which enqueue on
 *     at::cuda::getCurrentCUDAStream() (lib/src/ball_query.cpp:22).
 *   - the caller allocates every buffer, outputs included (lib/pointnet2_utils.py:200-202,246-248).  Two entry points
 *     need working memory their reference signature has no argument for and take it from a library-owned scratch, one
 *     buffer per (device, stream), allocated with hipMalloc on first use, grown on demand and kept for the life of the
 *     process: cmf_ball_query (spilled hit lists when nsample > 32 and more than 768 workgroups: 32 KB per workgroup,
 *     64 MB at b = 32, m = 4096; the cell grid of clouds with 4096-8192 points: 16 * b * n + 16 KB * b bytes, used by two
 *     launches) and cmf_group_points_grad (inverse index or scatter plan: <= 4 * b * (n + 1 + npoints * nsample) bytes);
 *     cmf_query_and_group keeps the indices there when the caller passes idx == NULL.  The buffer of a (device, stream) is
 *     handed out under a lock that is held until the last launch using it has been enqueued, so calls from several host
 *     threads onto one stream are safe; a buffer that must grow is retired (kept allocated), never freed while work may
 *     be queued on it.  Nothing else is retained between calls.
 *   - return value: hipError_t as int (0 = hipSuccess).  The reference launchers print and
 *     exit(-1) on a launch failure (lib/src/ball_query_gpu.cu:62-66); this library reports the
 *     error to the caller instead.  Invalid arguments return hipErrorInvalidValue (1).
 *   - all floating point is fp32, all indices int32, tensors dense row-major ("contiguous").
 */
#ifndef CMFLOW_HIP_H
#define CMFLOW_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

/* ---- the three kernels CMFlow uses from the reference's `pointnet2_cuda` extension -------- */

/* Replaces ball_query_kernel_launcher_fast (lib/src/ball_query_gpu.cu:48-49; binding
 * lib/src/ball_query.cpp:14-25).  new_xyz (b,m,3), xyz (b,n,3) -> idx (b,m,nsample).
 * First `nsample` points with d2 < radius*radius in index order, padded with the first hit;
 * idx is left untouched for an empty ball (caller pre-zeroes it, lib/pointnet2_utils.py:246). */
int cmf_ball_query(int b, int n, int m, float radius, int nsample,
                   const float *new_xyz, const float *xyz, int *idx, void *stream);
/* The nq <= 4 ball queries of one multi-scale grouping call (utils/model_utils/radarflow_util.py:111-118; models/cmflow.py:21-22:
 * (r, nsample) = (2,4) (4,8) (8,16) (16,32)) over the same centres and cloud in ONE launch, optionally for nclouds <= 2 (centres,
 * cloud) pairs of equal geometry: idx[c * nq + q] is (B, M, nsamples[q]) and equals cmf_ball_query(radii[q], nsamples[q]) bit for
 * bit; zero_empty != 0 writes the rows of empty balls as zeros (callers that do not pre-zero idx).  n <= 1024.  radii / nsamples /
 * the pointer tables are HOST arrays. */
int cmf_ball_query_multi(int b, int n, int m, int nq, const float *radii, const int *nsamples, int nclouds,
                         const float *const *new_xyz, const float *const *xyz, int *const *idx, int zero_empty, void *stream);

/* Replaces group_points_kernel_launcher_fast (lib/src/group_points_gpu.cu:69-70).
 * points (b,c,n), idx (b,npoints,nsample) -> out (b,c,npoints,nsample). */
int cmf_group_points(int b, int c, int n, int npoints, int nsample,
                     const float *points, const int *idx, float *out, void *stream);

/* Replaces group_points_grad_kernel_launcher_fast (lib/src/group_points_gpu.cu:27-28).
 * grad_out (b,c,npoints,nsample), idx -> grad_points (b,c,n) += scatter (caller zero-fills,
 * lib/pointnet2_utils.py:218).  The reference adds with fp32 atomics (order varies run to run); here rows of <= 8192 entries
 * over <= 2048 targets (plan form) and per-centre lists of 16 / 32 / 64 slots over <= 8192 targets (pad-folded CSR gather)
 * are summed in a fixed order: bit-reproducible.  Other shapes use LDS atomics unless CMF_GROUP_GRAD_DETERMINISTIC=1. */
int cmf_group_points_grad(int b, int c, int n, int npoints, int nsample,
                          const float *grad_out, const int *idx, float *grad_points, void *stream);

/* QueryAndGroup.forward (lib/pointnet2_utils.py:269-292) as one call: ball query (cmf_ball_query semantics; an empty ball
 * groups point 0, the reference's pre-zeroed idx) + grouped xyz minus the centre (:279-280) + grouped features (:283),
 * concatenated as the reference does (:285): out (b, 3*use_xyz + c, m, nsample), relative xyz planes first.
 * new_xyz (b,m,3) centres, xyz (b,n,3), features (b,c,n) or NULL with c == 0 (then use_xyz must be set), idx (b,m,nsample)
 * optional output (what GroupingOperation.backward needs, :204).  n <= 1024 and 3*use_xyz + c <= 24: ONE launch (the
 * waves that find the neighbour lists gather them; measured faster up to that width); otherwise the query followed by one
 * gather launch that writes the relative-xyz planes and the LDS-staged feature planes.  idx == NULL: the indices live in the
 * library's per-stream scratch between the two launches. */
int cmf_query_and_group(int b, int n, int m, float radius, int nsample, int c, int use_xyz,
                        const float *new_xyz, const float *xyz, const float *features, int *idx, float *out, void *stream);

/* ---- torch-level hot loops of the reference, as kernels ------------------------------------ */

/* knn_point (utils/model_utils/radarflow_util.py:88-99 = square_distance :8-30 + topk).
 * xyz (b,n,3) database, new_xyz (b,s,3) queries -> idx (b,s,nsample) int32 in canonical order
 * (ascending distance, ties by lowest index); dist (b,s,nsample) optional (may be NULL).
 * nsample <= 32. */
int cmf_knn(int b, int n, int s, int nsample, const float *xyz, const float *new_xyz,
            int *idx, float *dist, void *stream);

/* WeightedKabsch (models/cmflow.py:128-169).  A, Bm (b,3,n) point sets, W (b,n) weights
 * (normalised by the caller, cmflow.py:105-106) -> trans (b,4,4).  aux (b,32) doubles receives
 * {U,S,V of H, cA, cB, D} for the backward pass (may be NULL).
 * Rank-deficient H (fewer than three independent weighted points, a collinear or exactly planar cloud, all weights
 * zero): the rotation is not unique there.  The solve returns a PROPER rotation (R^T R = I, det R = +1, finite) that
 * agrees with the determined subspace and completes the rest orthonormally (H = 0: R = I), t = cB - R cA as always,
 * bottom row (0,0,0,1).  Singular values below 1e-14 of the largest are stored as exact zeros in aux, so the backward
 * pass (which divides by s_i + s_j) sends no gradient through a pair of undetermined directions: every gradient stays
 * finite.  tests/test_gpu_kabsch.py pins these properties, not the particular completion. */
int cmf_weighted_kabsch(int b, int n, const float *A, const float *Bm, const float *W,
                        float *trans, double *aux, void *stream);

/* Backward of cmf_weighted_kabsch.  grad_trans (b,4,4) -> grad_A, grad_B (b,3,n), grad_W (b,n)
 * (any of the three may be NULL).  Uses the polar-factor derivative (well conditioned: divides
 * by s_i + s_j, not s_i^2 - s_j^2 as a generic SVD backward does). */
int cmf_weighted_kabsch_grad(int b, int n, const float *A, const float *Bm, const float *W,
                             const double *aux, const float *grad_trans,
                             float *grad_A, float *grad_B, float *grad_W, void *stream);

/* The ego-motion head and the rigid refinement around that solve (models/cmflow.py:96-125) as one call per direction:
 *   w = (score + eps) / sum(score + eps),  B = pc1 + flow,  trans = weighted_kabsch(pc1, B, w),  mask = score > thres,
 *   sf = mask ? (R pc1 + t - pc1) : flow
 * pc1, flow (b,3,n), score (b,n) -> W (b,n), Bm (b,3,n) [kept for the backward call], trans (b,4,4), aux (b,32) doubles,
 * sf (b,3,n), mask (b,n) bytes.  One wavefront per sample. */
int cmf_ego_refine(int b, int n, float eps, float thres, const float *pc1, const float *flow, const float *score,
                   float *W, float *Bm, float *trans, double *aux, float *sf, unsigned char *mask, void *stream);
/* Backward: g_sf (b,3,n), g_trans (b,4,4; may be NULL) -> g_flow (b,3,n), g_score (b,n; may be NULL); g_w (b,n) scratch. */
int cmf_ego_refine_grad(int b, int n, float eps, const float *pc1, const float *score, const float *W, const float *Bm,
                        const unsigned char *mask, const double *aux, const float *g_sf, const float *g_trans,
                        float *g_flow, float *g_w, float *g_score, void *stream);

/* ---- point-major grouping (the layout the fused path computes in) ------------------------------ */

/* Layout helpers of the host side (each one launch where torch takes a fill, a copy and sometimes a subtraction):
 * cmf_pad_rows: dst[r][c] = c < k ? src[r * ld_src + c] : 0 for c < ld_dst (rows padded to 16-byte multiples);
 * cmf_inputs_point_major: the model's four inputs as point-major rows -- pc1, pc2 (b,3,n) -> x1, x2 (b,n,3); ft1, ft2 (b,c,n) ->
 *   a1, a2 (b,n,cp) with zero columns c..cp-1 (models/cmflow.py:59-64 keeps them channel-major);
 * cmf_rel_xyz: out (b,m,S,4) = (xyz[b][idx[b][p][s]] - centre[b][p], 0), the neighbours' relative coordinates
 *   (utils/model_utils/radarflow_util.py:207-208). */
int cmf_pad_rows(long long rows, int k, const float *src, long long ld_src, float *dst, int ld_dst, void *stream);
int cmf_inputs_point_major(int b, int n, int c, int cp, const float *pc1, const float *pc2, const float *ft1, const float *ft2,
                           float *x1, float *x2, float *a1, float *a2, void *stream);
int cmf_rel_xyz(int b, int n, int m, int S, const float *xyz, const float *centre, const int *idx, float *out, void *stream);

/* Row gather: feat (b,n,ldf) rows of c floats, idx (b,entries) -> out (b,entries,c) with
 * out[b,e,:] = feat[b,idx[b,e],:].  Same operation as cmf_group_points on the transposed layout
 * (reference: lib/src/group_points_gpu.cu:47-66 via utils/model_utils/radarflow_util.py:52-63),
 * with coalesced 16-byte accesses instead of a 4-byte gather. */
int cmf_group_rows(int b, int n, int c, int ldf, int entries,
                   const float *feat, const int *idx, float *out, void *stream);

/* Inverse index of idx (b,entries) with values in [0,n): offsets (b,n+1), inv (b,entries) --
 * for each target point the entries that reference it, ascending.  Feeds cmf_group_rows_grad. */
int cmf_build_inverse(int b, int n, int entries, const int *idx, int *offsets, int *inv, void *stream);
/* Same, for idx of shape (b,P,S): small P / n take an O(P*S) LDS-matrix path instead of a scan. */
int cmf_build_inverse_ps(int b, int n, int P, int S, const int *idx, int *offsets, int *inv, void *stream);

/* Backward of cmf_group_rows as a deterministic segmented sum (replaces the fp32 atomics of
 * lib/src/group_points_gpu.cu:8-25): grad_feat[b,j,:] (row stride ldg) = (accumulate ? old : 0) +
 * sum_{e in inv(j)} grad_out[b,e,:], summed in ascending e. */
int cmf_group_rows_grad(int b, int n, int c, int ldg, int entries, int accumulate,
                        const float *grad_out, const int *offsets, const int *inv,
                        float *grad_feat, void *stream);

/* ---- fp32 MFMA GEMM with fused BatchNorm/activation prologue and epilogues ---------------------- *
 * Every 1x1 Conv2d of the reference (utils/model_utils/radarflow_util.py:132-139,174,246-251,
 * 299-305) is  C[M,N] = epi( pro(A)[M,K] * B[K,N] )  on point-major matrices.
 *   a_t: A is stored [K][M] (lda = row stride) instead of [M][K];  b_t: B is stored [N][K]
 *        (a conv weight (out,in)) instead of [K][N].
 *   pro_a/pro_c [K]  (a_t == 0 only): A' = relu(pro_a[k]*A + pro_c[k])   -- producer's BN+ReLU
 *   prob_a/prob_c [N] (b_t == 0 only): B' = relu(prob_a[n]*B + prob_c[n])
 *   bias [N], act: 0 none / 1 relu / 2 leaky(0.1) / 3 sigmoid
 *   stats: [ceil(M/128)][2][N] per-row-tile partial (sum, sum of squares) of the stored C
 *   bwd_mode 1: C = acc * [ea[n]*Z + ec[n] > 0], stats <- partial (sum C, sum C*(Z-emean)*einvstd)
 *   dxyz (bwd_mode 1, 2 or 3 with stats, optional): rows of (dx,dy,dz,0) per output row; stats becomes [tiles][5][N]
 *                with the three extra partials sum C*d_k -- the xyz-weight gradient of the set-conv's / cost volume's
 *                first conv comes out of the epilogue instead of a 4-column GEMM over the same rows
 *   bwd_mode 2: C = acc * (Z > 0 ? 1 : 0.1)        bwd_mode 3: C = acc * [Z > 0]     (stats: column sums of C in row 0)
 *   split_k > 1: contraction split over split_k slabs in `workspace` ([split_k][M][N] floats),
 *                summed in a fixed order by a second kernel (deterministic weight gradients)
 *   accumulate: C += result
 * Row strides (lda, ldb) must be multiples of 4 floats and A, B 16-byte aligned. */
int cmf_gemm(int M, int N, int K, int a_t, int b_t,
             const float *A, long long lda, const float *B, long long ldb, float *C, long long ldc,
             const float *pro_a, const float *pro_c, const float *prob_a, const float *prob_c,
             const float *bias, int act, float *stats,
             int bwd_mode, const float *Z, long long ldz,
             const float *ea, const float *ec, const float *emean, const float *einvstd,
             const float *dxyz, int split_k, float *workspace, int accumulate, void *stream);
int cmf_gemm_tiles_m(int M);
/* The persistent form of the tiled kernel (csrc/gemm_persist.hip: workgroups stay resident and write tile t out between the
 * MFMAs of tile t + 1) takes the data-gradient calls with a backward epilogue on interior shapes (M, N multiples of 128,
 * K a multiple of 16, K >= 192).  mode 0: never; 1: where a workgroup gets at least three tiles (default; also
 * CMF_GEMM_PERSIST=0|1|2); 2: wherever the shape allows.  grid: its workgroup count (multiple of 8), 0 = two per CU.
 * Outputs are bit-identical to the non-persistent kernel's; the column statistics are summed in a different (fixed) order.
 * Returns 0, -1 on an invalid argument.  Process-wide. */
int cmf_gemm_persist_config(int mode, int grid);
/* Diagnostics / tests: the <= 64-channel forward layers (cmf_gemm's per-wave kernels) have a full-tile body that issues all of a
 * wave's loads before its first wait; on = 1 sends full tiles through the general body as well (also CMF_THIN_GENERAL=1).  Outputs
 * and statistics of the two bodies are bit-identical.  Returns the previous setting.  Process-wide. */
int cmf_thin_general(int on);

/* Live timing of the tiled GEMM kernel for bench.py's `roofline` object.  Between _begin and _end every launch of the
 * tiled kernel with 2*M*N*K >= min_flops is bracketed by a HIP event pair on the stream it is launched on -- inside
 * the library, so launches issued by cmf_setconv_forward/_backward count like direct cmf_gemm calls.  _end synchronises
 * the device and returns the number of bracketed launches, the sum of their durations (ms) and of their FLOPs, and the
 * launch count / FLOPs of ALL cmf_gemm calls in the window (thin kernels included): the share the measurement covers.
 * Not re-entrant (one window at a time); every output pointer may be NULL. */
/* Diagnostics (tools/gemm_timeline.py): _arm makes the NEXT tiled launch record, per workgroup, {start, end of main loop,
 * end} on the 100 MHz wall clock, (xcc_id << 32 | HW_ID) and three epilogue stamps (first transposition visible, band-0 stores
 * issued, last band done); _read synchronises and copies the 8 x u64 records to host memory, returning the workgroup
 * count of that launch. */
int cmf_gemm_trace_arm(void);
long long cmf_gemm_trace_read(unsigned long long *host_out, long long max_workgroups);
typedef struct cmf_gemm_launch_record {
    int M, N, K;          /* as passed to cmf_gemm (C is M x N, contraction K) */
    int layout;           /* bit 1: a_t, bit 0: b_t, bit 2: persistent kernel */
    int split_k, kind;    /* epilogue kind: 0 raw store, 1 forward (bias/act/stats), 2 backward BN+ReLU, 3 backward (leaky) ReLU */
    int bm, bn;           /* block tile */
    float ms;             /* duration between the two events */
} cmf_gemm_launch_record;
int cmf_gemm_profile_begin(double min_flops);
/* Bracket only every n-th launch that reaches min_flops (default 1 = all; the event pairs themselves cost 0.13-0.18 ms per training step
 * when every large launch carries one); every eligible launch is still counted: cmf_gemm_profile_eligible (after cmf_gemm_profile_end). */
int cmf_gemm_profile_sampling(int every);
int cmf_gemm_profile_eligible(long long *launches, double *flops);
int cmf_gemm_profile_end(long long *launches_timed, double *ms_timed, double *flops_timed, long long *launches_all,
                         double *flops_all);
/* per-launch records of the last closed window (shape, layout, kind, duration); returns the number available */
long long cmf_gemm_profile_records(cmf_gemm_launch_record *out, long long max_records);

/* ---- BatchNorm / activation / pooling kernels around the GEMMs (point-major) ---------------------- *
 * Per-channel reductions use a partial buffer [ceil(rows/128)][2][C] (no atomics, fixed order). */

/* partial (sum, sumsq) over `count` rows -> mean, invstd (biased variance), running-stat update
 * (momentum, unbiased variance: torch BatchNorm2d train semantics, radarflow_util.py:133-139), and the
 * folded affine a = gamma*invstd, c = beta - mean*a.  tiles == 0: eval mode, fold the running stats.
 * num_batches_tracked (int64, optional) is incremented by one (nn.BatchNorm2d's counter). */
int cmf_bn_finalize(int tiles, int C, double count, const float *partial, const float *gamma,
                    const float *beta, float eps, float momentum, float *running_mean, float *running_var,
                    float *mean_out, float *invstd_out, float *a_out, float *c_out,
                    long long *num_batches_tracked, void *stream);
/* out[2][C] = sum over tiles of partial[t][2][C]; optionally acc0[C] += row 0 (dbeta), acc1[C] += row 1
 * (dgamma): the BN-backward sums land directly in the parameters' gradient buffers */
int cmf_colsum_finalize(int tiles, int C, const float *partial, float *out, float *acc0, float *acc1, void *stream);
/* out[ncols] = sum over tiles of partial[t][ncols] (fixed order); same optional accumulation of the first 2*C columns */
int cmf_colsum(int tiles, int ncols, const float *partial, float *out, int C, float *acc0, float *acc1, void *stream);

/* Set-conv / cost-volume grouping with the first 1x1 conv hoisted per point
 * (QueryAndGroup + first Conv2d, lib/pointnet2_utils.py:277-285 + radarflow_util.py:151;
 *  cost volume radarflow_util.py:207-216):
 *   z[b,p,s,:] = act( ysrc[b,idx[b,p,s],:] + (yctr ? yctr[b,p,:] : 0) + Wx (xyz_src[b,idx] - xyz_ctr[b,p]) )
 * ysrc (b,n_src,ld_src), yctr (b,P,ld_ctr) or NULL, Wx (C,3) with row stride ldw, idx (b,P,S);
 * act 0 none / 2 leaky(0.1); z (b,P,S,C); dxyz (b,P,S,4) relative coordinates (optional);
 * partial: BN statistics of z (optional); partial_x (optional, with partial): [tiles][3*C+4] extra sums
 * sum z*d_k (k=0..2, per channel) and sum d_k, used by cmf_setconv_dwx in the backward pass.
 * z == NULL (yctr == NULL, partial given): the statistics only, bit-identical to the writing form's. */
int cmf_group_affine(int b, int n_src, int P, int S, int C,
                     const float *ysrc, int ld_src, const float *yctr, int ld_ctr,
                     const float *xyz_src, const float *xyz_ctr, const float *Wx, int ldw,
                     const int *idx, int act, float *z, float *dxyz, float *partial, float *partial_x, void *stream);

/* The same first layer WITHOUT the (b,P,S,C) tensor, for inference (nothing of it is needed afterwards): cmf_group_prep writes what
 * depends on the neighbour lists only -- rows[b,p,s] = b*n_src + idx[b,p,s], dxyz (b,P,S,4) = xyz_src[idx] - xyz_ctr[p], wx3 (3,C) the
 * coordinate columns of Wx as planes -- and cmf_gemm_gather_affine is the NEXT layer's GEMM
 *   out[m,n] = sum_k relu( pro_a[k] * ( Y[rows[m],k] + wx3[0,k] dx_m + wx3[1,k] dy_m + wx3[2,k] dz_m ) + pro_c[k] ) * W[n,k]
 * with that layer formed in its A-operand path (rows gathered by the LDS-direct loads, the coordinate term + BN + ReLU applied to
 * the fragments).  Same operations in the same order as cmf_group_affine followed by cmf_gemm with the A prologue: bit-identical.
 * M, N multiples of 128, K a multiple of 16, pointers 16-byte aligned. */
int cmf_group_prep(int b, int n_src, int P, int S, int C, const float *xyz_src, const float *xyz_ctr, const float *Wx, int ldw,
                   const int *idx, int *rows, float *dxyz, float *wx3, void *stream);
int cmf_gemm_gather_affine(int M, int N, int K, const float *Y, long long ldy, const int *rows, const float *dxyz,
                           const float *wx3, const float *pro_a, const float *pro_c, const float *W, long long ldw,
                           float *C, long long ldc, float *stats /* [M/128][2][N] partial sums of the output, or NULL */, void *stream);
/* ... and the weight gradient of that next layer with the first layer formed in its B-operand staging (register-staged loop, the
 * rows' source indices requested one chunk ahead):
 *   dW[cout,cin] (+)= sum_r dZ[r,cout] * relu( prob_a[k] * ( Y[rows[r],k] + wx3[:,k] . dxyz[r] ) + prob_c[k] )
 * bit-identical to cmf_gemm(a_t = 1, b_t = 0, prob_a, prob_c) on the materialised tensor.  cout, cin multiples of 128, nrows of 16;
 * split_k > 1: deterministic slabs in `workspace` (split_k * cout * cin floats). */
/* ... and the data gradient INTO that first layer (cmf_gemm's backward kind with dxyz: mask by the first layer's BN + ReLU, BN-backward
 * and dxyz partial sums [tiles_m][5][cin]) with the first layer's pre-activations formed from the per-point rows in the epilogue:
 *   dU[m,k] = (dZ @ W)[m,k] * [ea[k] z + ec[k] > 0],   z = Y[rows[m],k] + wx3[:,k] . dxyz[m]
 * bit-identical to cmf_gemm(bwd_mode = 1, Z = the materialised tensor, dxyz) in the non-persistent kernel.  M, cin multiples of 128. */
int cmf_gemm_dx_gather(int M, int cin, int cout, const float *dZ, long long ldz, const float *W, long long ldw,
                       float *dU, long long ldu, const float *Y, long long ldy, const int *rows, const float *dxyz,
                       const float *wx3, const float *ea, const float *ec, const float *emean, const float *einvstd,
                       float *stats, void *stream);
/* ... and the same data gradient when only its sums per source point are needed (the grouping's backward pass): the rows walk the
 * slots in inverse-index order (cmf_group_perm: arows[m] the slot at position m, pts[m] its source point, dxyz2 its relative
 * coordinates) and the kernel stores no dU -- for every run of equal source points inside a 64-row range it writes the run's column
 * sums to pieces[(point + m / 64)][cin] (P + M / 64 rows), which cmf_group_rows_grad_bn_cf_pieces adds per point in range order. */
int cmf_group_perm(int b, int entries, const int *inv, const int *rows, const float *dxyz, int *perm, int *pts, float *dxyz2, void *stream);
int cmf_gemm_dx_gather_sum(int M, int cin, int cout, const float *dZ, long long ldz, const float *W, long long ldw,
                           const float *Y, long long ldy, const int *arows, const int *pts, const float *dxyz2,
                           const float *wx3, const float *ea, const float *ec, const float *emean, const float *einvstd,
                           float *pieces, float *stats, void *stream);
int cmf_gemm_dw_gather(int cout, int cin, long long nrows, const float *dZ, long long ldz, const float *Y, long long ldy,
                       const int *rows, const float *dxyz, const float *wx3, const float *prob_a, const float *prob_c,
                       float *dW, long long lddw, int split_k, float *workspace, int accumulate, void *stream);
/* cmf_gemm_dw_gather with the train-mode BatchNorm backward of its output gradient formed in the A-operand staging:
 * dZ = a * (dU - s1/nrows - zhat * s2/nrows), zhat = (Z - mean) * invstd, (s1 | s2) = sums[2][cout]; dU, Z (nrows, cout); dZ_out
 * (nrows, cout) receives dZ and must not alias dU.  Bit-identical to cmf_bn_bwd_apply followed by cmf_gemm_dw_gather. */
int cmf_gemm_dw_gather_bn_bwd(int cout, int cin, long long nrows, const float *dU, long long ldu, const float *Z, long long ldz,
                              const float *a, const float *mean, const float *invstd, const float *sums, float *dZ_out, long long ldo,
                              const float *Y, long long ldy, const int *rows, const float *dxyz, const float *wx3,
                              const float *prob_a, const float *prob_c, float *dW, long long lddw, int split_k, float *workspace,
                              int accumulate, void *stream);
/* The split count with which cmf_gemm_dw_gather takes its 256-row tiles (workspace: split * cout * cin floats); 0 = no preference. */
int cmf_gemm_dw_gather_split(int cout, int cin, long long nrows);

/* out[p,:] = max_s relu(a*z[p,s,:] + c): BN + ReLU + max over the ball (radarflow_util.py:151-155);
 * argmax (P,C) uint8 optional. */
int cmf_bn_relu_maxpool(long long P, int S, int C, const float *z, const float *a, const float *c,
                        float *out, long long ldo, unsigned char *argmax, void *stream);
int cmf_maxpool_bwd(long long P, int S, int C, const float *dout, long long ldd, const float *z,
                    const float *a, const float *c, const float *mean, const float *invstd,
                    const unsigned char *argmax, float *dU, float *partial, void *stream);

/* out = relu(a*z + c) (row strides ldz / ldo: out may be a column slice of a concat buffer) */
int cmf_affine_relu(long long M, int C, const float *z, long long ldz, const float *a, const float *c,
                    float *out, long long ldo, void *stream);
/* dU = dY * [a*z + c > 0] + partial (sum dU, sum dU*(z-mean)*invstd) */
int cmf_act_bwd_stats(long long M, int C, const float *dY, long long ldy, const float *z, long long ldz,
                      const float *a, const float *c, const float *mean, const float *invstd,
                      float *dU, float *partial, void *stream);
/* in place: dZ = a*(dU - s1/M - zhat*s2/M) with sums = {s1[C], s2[C]}; sums == NULL: dZ = a*dU (eval BN) */
int cmf_bn_bwd_apply(long long M, int C, float *dU, const float *z, long long ldz, const float *a,
                     const float *mean, const float *invstd, const float *sums, void *stream);

/* One backward layer of a NARROW [1x1 conv + BatchNorm + ReLU] stack (cout, cin <= 64, cout % 8 == 0; the reference's
 * mlp_convs / mlp2_convs of PointLocalFeature, radarflow_util.py:144-162, at its 32 / 64 channel widths) in one pass over
 * the rows -- what bn_bwd_apply + the weight-gradient cmf_gemm + the data-gradient cmf_gemm compute as three kernels
 * streaming eight [rows, C] matrices is done here streaming four:
 *   dZ    = a (dU - s1/rows - (z - mean) invstd s2/rows)          (sums = {s1[cout], s2[cout]}; NULL: dZ = a dU, eval BN)
 *   dx    = mask_in(dZ @ w),  mask_in = [a_in x + c_in > 0]       in_mode 1: x is the pre-BN output of the layer below;
 *           stats[tile][2 or 5][cin] get the per-128-row-tile sums of dx, dx (x - mean_in) invstd_in (and dx * dxyz_k when
 *           dxyz is given), as cmf_gemm's backward epilogue does.  in_mode 0: x is an activated input, dx = dZ @ w.
 *   dw (+)= dZ^T @ act_in(x),  act_in = relu(a_in x + c_in) (in_mode 1) or identity; summed over cmf_thin_bwd_slabs(rows)
 *           slabs [cout][cin] in `slabs` in fixed order (deterministic).
 * dx == NULL skips the data gradient (and stats), dw == NULL the weight gradient.  dU and z rows must be 16-byte aligned. */
int cmf_thin_bwd_supported(int cout, int cin);
int cmf_thin_bwd_slabs(long long rows, int *tiles_per_workgroup);
int cmf_thin_bwd_layer(long long rows, int cout, int cin, const float *dU, long long lddu, const float *z, long long ldz,
                       const float *a, const float *mean, const float *invstd, const float *sums,
                       const float *w, long long ldw, const float *x, long long ldx, int in_mode,
                       const float *a_in, const float *c_in, const float *mean_in, const float *invstd_in, const float *dxyz,
                       float *dx, long long lddx, float *stats, float *dw, long long lddw, int accumulate, float *slabs,
                       void *stream);

/* The same layer directly behind the max over the ball (radarflow_util.py:155-157 backward), dense: rows = P * S, row
 * (p, s) of dU is (s == argmax[p][:]) ? g[p][:] : 0 and is formed on the fly from the per-point arrays of
 * cmf_maxpool_bwd_point -- the [P*S, cout] gradient of the pooled tensor is never stored.  x is the pre-BN output of the
 * layer below (in_mode 1); whole 128-row tiles and multiples of 32 channels only. */
int cmf_maxpool_bwd_point(long long P, int S, int C, const float *dout, long long ldd, const float *z,
                          const float *a, const float *c, const float *mean, const float *invstd,
                          const unsigned char *argmax, float *g, float *partial, void *stream);
int cmf_thin_bwd_layer_pooled(long long P, int S, int cout, int cin, const float *g, const unsigned char *argmax,
                              const float *z, const float *a, const float *mean, const float *invstd, const float *sums,
                              const float *w, const float *x, const float *a_in, const float *c_in, const float *mean_in,
                              const float *invstd_in, float *dx, float *stats, float *dw, int accumulate, float *slabs,
                              void *stream);

/* The fused backward layer for a WIDE input: cout = 64, cin a multiple of 128 (<= 1024), whole 128-row tiles, input
 * through BN + ReLU (in_mode 1), both products -- the 256 -> 64 conv of a second-encoder block (radarflow_util.py:144-162),
 * whose two gradients are the worst GEMM shapes of the step (K = 64 / 64 output rows).  dU is either given
 * ([rows][64], row stride lddu) or pooled (pool_g != NULL: rows = P * pool_S, per-point arrays of cmf_maxpool_bwd_point).
 * slabs: cmf_thin_bwd_wide_slabs(rows, cin, NULL) x 64 x cin floats of workspace. */
int cmf_thin_bwd_wide_supported(int cout, int cin);
int cmf_thin_bwd_wide_slabs(long long rows, int cin, int *tiles_per_workgroup);
int cmf_thin_bwd_wide_layer(long long rows, int cin, const float *dU, long long lddu, const float *pool_g,
                            const unsigned char *pool_am, int pool_S, const float *z, long long ldz,
                            const float *a, const float *mean, const float *invstd, const float *sums,
                            const float *w, long long ldw, const float *x, long long ldx,
                            const float *a_in, const float *c_in, const float *mean_in, const float *invstd_in,
                            float *dx, long long lddx, float *stats, float *dw, long long lddw, int accumulate, float *slabs,
                            void *stream);

/* Backward of the set-conv's grouping with the BatchNorm backward of the first layer fused in
 * (radarflow_util.py:148-151 backward): dZ = a*(dU - s1/M - zhat*s2/M) is formed on the fly from dU and z,
 * summed over the inverse index into grad_feat (b,n,c) with row stride ldg, and never written.  sums = {s1[C], s2[C]} or NULL
 * (eval-mode BN: dZ = a*dU). */
int cmf_group_rows_grad_bn(int b, int n, int c, int entries, const float *dU, const float *z,
                           const float *a, const float *mean, const float *invstd, const float *sums,
                           float inv_count, const int *offsets, const int *inv, float *grad_feat, int ldg, void *stream);
/* The same result without reading z, for z produced by cmf_group_affine from per-point rows: every entry e of inv(j)
 * gathers the same source row, z[e,:] = y[j,:] + wx . (xyz_src[j] - xyz_ctr[e / S]), so
 *   sum_e (z[e,:] - mean) = cnt_j*(y[j,:] - mean) + wx . D_j,   D_j = sum_e (xyz_src[j] - xyz_ctr[e / S]),
 * and only dU is streamed.  y (b,n,c) rows with stride ldy, wx (c,3) rows with stride ldw, xyz_src (b,n,3),
 * xyz_ctr (b, entries/S, 3); entries = centres * S in (centre, slot) order. */
int cmf_group_rows_grad_bn_cf(int b, int n, int c, int entries, int S, const float *dU, const float *y, long long ldy,
                              const float *wx, long long ldw, const float *xyz_src, const float *xyz_ctr,
                              const float *a, const float *mean, const float *invstd, const float *sums,
                              float inv_count, const int *offsets, const int *inv, float *grad_feat, int ldg, void *stream);
/* ... with the sums of dU over every point's slots already formed by cmf_gemm_dx_gather_sum (`pieces`): dU is not read */
int cmf_group_rows_grad_bn_cf_pieces(int b, int n, int c, int entries, int S, const float *pieces, const float *y, long long ldy,
                                     const float *wx, long long ldw, const float *xyz_src, const float *xyz_ctr,
                                     const float *a, const float *mean, const float *invstd, const float *sums,
                                     float inv_count, const int *offsets, const int *inv, float *grad_feat, int ldg, void *stream);

/* dW_xyz of the set-conv's first conv from column sums only (no pass over the grouped tensor):
 *   dWx[c,k] = a_c*( q_k[c] - (s1_c/M)*u_k - (s2_c/M)*invstd_c*(tz_k[c] - mean_c*u_k) )
 * bwd5 = {s1,s2,q0,q1,q2}[C] (cmf_gemm dxyz partials, reduced), fwd = {tz0,tz1,tz2}[C] then {u0,u1,u2,.}
 * (cmf_group_affine extra partials, reduced); train == 0: dWx = a*q.  dwx rows have stride ld floats
 * (the xyz columns of the (out, 3+C) conv weight gradient); accumulate: += instead of =. */
int cmf_setconv_dwx(int C, float inv_count, int train, const float *bwd5, const float *fwd,
                    const float *a, const float *mean, const float *invstd, float *dwx, int ld, int accumulate,
                    void *stream);

/* ---- the rest of the reference's pointnet2_cuda extension (lib/src/pointnet2_api.cpp:10-25) ------------ *
 * Not called by CMFlow (only by the unused lib/pointnet2_modules.py); provided so the drop-in module is
 * complete.  Argument order = the reference launchers. */
/* gather_points_kernel_launcher_fast (sampling_gpu.cu:27-44): out[b,c,j] = points[b,c,idx[b,j]] */
int cmf_gather_points(int b, int c, int n, int npoints, const float *points, const int *idx, float *out, void *stream);
/* gather_points_grad_kernel_launcher_fast (sampling_gpu.cu:66-83): accumulates into grad_points */
int cmf_gather_points_grad(int b, int c, int n, int npoints, const float *grad_out, const int *idx,
                           float *grad_points, void *stream);
/* furthest_point_sampling_kernel_launcher (sampling_gpu.cu:212-250): temp (b,n) pre-filled with 1e10 */
int cmf_furthest_point_sampling(int b, int n, int m, const float *dataset, float *temp, int *idxs, void *stream);
/* knn_kernel_launcher_fast (interpolate_gpu.cu:60-78): k nearest `known` points per `unknown`, ascending,
 * first-seen wins ties, squared distances; 0 < k <= 200, the reference's range (k <= 64: a lane per query with its list in
 * registers; above: a wave per query, the list spread over its lanes).  Slots behind a cloud of m < k points read index 0,
 * distance 0. */
int cmf_knn_points(int b, int n, int m, int k, const float *unknown, const float *known,
                   float *dist2, int *idx, void *stream);
/* three_nn_kernel_launcher_fast (interpolate_gpu.cu:127-146) */
int cmf_three_nn(int b, int n, int m, const float *unknown, const float *known, float *dist2, int *idx, void *stream);
/* three_interpolate_kernel_launcher_fast (interpolate_gpu.cu:172-189) and its grad (:217-233) */
int cmf_three_interpolate(int b, int c, int m, int n, const float *points, const int *idx,
                          const float *weight, float *out, void *stream);
int cmf_three_interpolate_grad(int b, int c, int n, int m, const float *grad_out, const int *idx,
                               const float *weight, float *grad_points, void *stream);

/* ---- one set-conv block (PointLocalFeature, radarflow_util.py:121-162) per call ------------------------- *
 * Host-side sequencing of the kernels above for one (radius, nsample) scale: ball query -> gather with the
 * hoisted first conv -> (BN, ReLU, 1x1 conv) x 2 -> BN + ReLU + max over the ball -> (1x1 conv, BN, ReLU) x 3.
 * All device memory is caller provided: `saved` keeps what backward needs, `scratch` is transient; sizes come
 * from cmf_setconv_sizes.  The forward and backward calls must see the same descriptor geometry and `saved`. */
typedef struct cmf_setconv_desc {
    int B, N, S;                 /* samples, points per sample, nsample (<= 64) */
    int O1;                      /* channels of the hoisted first conv */
    int C[5];                    /* output channels of layers 2..6 */
    float radius;
    int training;                /* 1: batch statistics + running-stat update; 0: fold the running statistics */
    float eps[6], momentum[6];
    const float *xyz;            /* (B,N,3) */
    const float *y; long long ldy;      /* (B,N,O1) rows, stride ldy: feats @ W_f^T */
    const float *wx; long long ldwx;    /* (O1,3) xyz columns of the first conv weight, row stride ldwx */
    const float *w[5];           /* layers 2..6 weights (C[i], C_in) dense */
    const float *gamma[6], *beta[6];
    float *rmean[6], *rvar[6];
    long long *nbt[6];           /* num_batches_tracked counters (may be NULL) */
    float *saved, *scratch;
    float *out; long long ldo;   /* (B*N, C[4]) */
    /* backward */
    const float *dout; long long lddout;
    float *dy; long long lddy;   /* (B,N,O1) rows with stride lddy (0 = dense O1), or NULL */
    float *dwx; long long lddwx; int acc_wx;
    float *dw[5]; int acc_w[5];  /* weight gradients: written (0) or accumulated into (1) */
    float *dgamma[6], *dbeta[6]; int acc_bn[6];
    int inference;               /* 1 (with training == 0): no backward call will follow -- the forward call may skip what only the
                                    backward pass reads (the grouped first-layer tensor: cmf_gemm_gather_affine) */
    int idx_ready;               /* 1: this block's ball query has been issued already (cmf_setconv_queries wrote the indices into
                                    `saved`); the forward call does not launch its own */
} cmf_setconv_desc;
/* Arena sizes in floats (each pointer may be NULL); host arithmetic over the SHAPE fields of the descriptor (B, N, S, O1, C, ldy,
 * training) -- no pointer of it is read.  The arenas are sized by PATH: a block whose shapes take the gathering GEMMs (M = B*N*S and
 * O1, C[0] multiples of 128, ldy a multiple of 4: the second encoder) keeps M row indices + 3*O1 floats where the materialised
 * first-layer tensor would take M x O1.
 *   scratch_bwd             valid for ANY backward call on these shapes;
 *   scratch_bwd_input_grad  valid only for a backward call that sets d->dy (produces the input gradient): such a block with S >= 2
 *                           then holds (B*N + M/64) x O1 + 6 M floats where the data gradient into the first layer would take M x O1.
 *                           Never larger than scratch_bwd, equal to it for every other block.  A backward call without d->dy on an
 *                           arena of this size overruns it.
 * With the compact sizes d->y and d->w[0] must be 16-byte aligned (the forward / backward calls refuse them otherwise). */
int cmf_setconv_sizes(const cmf_setconv_desc *d, long long *saved_floats, long long *scratch_fwd, long long *scratch_bwd,
                      long long *scratch_bwd_input_grad);
/* Device memory the library holds on the current device outside caller-provided arenas: the per-(stream, slot) scratch buffers of the
 * drop-in entry points (cmf_ball_query spill lists, cmf_group_points_grad plans / inverse indices), live + retired, in bytes. */
long long cmf_mem_stats(void);
/* The ball queries of n blocks, issued ahead of their forward calls on ONE stream: blocks that share centres and cloud (the scales of
 * a MultiScaleEncoder call, radarflow_util.py:111-118) are served by one cmf_ball_query_multi launch, two clouds of equal geometry
 * (the weight-shared first encoder, models/cmflow.py:72-73) by the same launch -- 12 launches per CMFlow forward become 2.  The
 * indices land where cmf_setconv_forward keeps them (head of `saved`); the caller then sets idx_ready in the descriptors. */
int cmf_setconv_queries(int n, const cmf_setconv_desc *descs, void *stream);
int cmf_setconv_forward(const cmf_setconv_desc *d, void *stream);
int cmf_setconv_backward(const cmf_setconv_desc *d, void *stream);
/* Which kernels cmf_setconv_forward / _backward run the neighbour-slot layers of this descriptor with -- 0: the per-layer kernels,
 * 1: the register chain's inference pass (csrc/setconv_chain.hip; eval-mode BatchNorm, d->inference), 2: the chain's training passes
 * (eval-mode BatchNorm with a backward call to follow, M = B*N*S a multiple of 128).  Host arithmetic with the predicate the dispatch
 * itself uses: B, N, S, O1, C, training, inference, ldy and the alignment of d->y are read; nothing is launched.  For tests and
 * tools that must know a call exercised the kernel they mean. */
int cmf_setconv_path(const cmf_setconv_desc *d);
/* The optimizer step of the reference's loop (main.py:107: torch.optim.Adam with L2 weight decay) over a flat gradient bucket in ONE
 * launch: grad / m / v are flat arrays of `total` floats in bucket order, params[t] the address of tensor t and offsets[t] its first
 * element in the bucket (offsets[n_tensors] = total; both tables in device memory).  step >= 1 is the count INCLUDING this update.
 *   g' = g + wd p;  m += (1 - b1)(g' - m);  v = b2 v + (1 - b2) g'^2;  p -= lr / (1 - b1^step) * m / (sqrt(v) / sqrt(1 - b2^step) + eps) */
int cmf_adam_step(int n_tensors, const long long *offsets, float *const *params, long long total, const float *grad, float *m, float *v,
                  double lr, double beta1, double beta2, double eps, double weight_decay, long long step, void *stream);

/* The guarded optimizer step: the L2 norm of the flat gradient bucket on the device, clipping by it, and skipping a step whose norm is
 * not finite -- two launches behind the backward pass, no host read, bit-reproducible.
 *
 * cmf_grad_norm_parts(total): the number P of workgroups (1 <= P <= 256; 0 for total <= 0) of the sum of squares and the length of
 * `partials`.  Host arithmetic on `total` alone (not the device, its CU count or the environment), callable without a device:
 * slabs = ceil(total / 1024), P = min(256, ceil(slabs / 4)); workgroup b owns the contiguous slabs [b slabs / P, (b + 1) slabs / P).
 * cmf_grad_sumsq: partials[b] = the sum over workgroup b's elements of (double)x * (double)x, accumulated in double (the square of an
 * fp32 value is exact in double, only the additions round: relative error <= total * 2^-53), lanes, waves and LDS folded in a fixed
 * order, no atomics.  A NaN or +-Inf element makes its partial non-finite; finite fp32 values cannot overflow.  `grad` must be 16-byte
 * aligned (hipErrorInvalidValue otherwise).
 * cmf_grad_norm: cmf_grad_sumsq, then one workgroup folds the P partials in a fixed order: out[0] = sumsq, out[1] = sqrt(sumsq), doubles.
 *
 * cmf_adam_step_guarded: cmf_adam_step behind a prologue.  `partials` is what cmf_grad_sumsq left for the same `grad`; every
 * workgroup folds it with the fold cmf_grad_norm uses (the same bits) and derives, identically everywhere:
 *     normf     = (float)sqrt(sumsq)                 // double sqrt, rounded once
 *     nonfinite = !isfinite(sumsq)
 *     if (nonfinite && skip)  -> return before any store to p, m, v
 *     scale = 1.f
 *     if (!nonfinite && clip_on) { coef = max_norm_f / (normf + 1e-6f); scale = coef < 1.f ? coef : 1.f; }   // torch's clip_grad_norm_ formula, in fp32
 *     g = fmaf(wd, p, grad[e] * scale)               // then exactly cmf_adam_step's update
 * clip_on = max_grad_norm is positive and finite (<= 0 or +inf: no clipping; NaN: hipErrorInvalidValue), max_norm_f = (float)max_grad_norm.
 * `grad` is NOT modified: read after the step it holds the unclipped gradient.  A non-finite norm with skip_nonfinite = 0 means
 * "guard off": scale = 1 and the update is cmf_adam_step's, NaNs included.  With scale = 1 and no skip the result is bit-identical to
 * cmf_adam_step's.
 * step: as in cmf_adam_step the bias corrections are formed on the host, in double, from `step` -- so `step` counts CALLS, and a skipped
 * call advances it like any other (no device-side pow, and the guarded step equals the unguarded one whenever nothing is clipped or
 * skipped).
 * record: 8 doubles in device memory, updated by one lane with plain loads and stores (launches on one stream are ordered):
 *   [0] calls   [1] calls with a non-finite norm   [2] clipped calls (scale < 1)   [3] sum of normf over the finite calls
 *   [4] max of normf over the finite calls   [5] last sumsq   [6] last normf   [7] last scale */
int cmf_grad_norm_parts(long long total);
int cmf_grad_sumsq(long long total, const float *grad, double *partials, void *stream);
int cmf_grad_norm(long long total, const float *grad, double *partials, double *out, void *stream);
int cmf_adam_step_guarded(int n_tensors, const long long *offsets, float *const *params, long long total, const float *grad, float *m,
                          float *v, double lr, double beta1, double beta2, double eps, double weight_decay, long long step,
                          double max_grad_norm, int skip_nonfinite, const double *partials, double *record, void *stream);

/* Averaged weights: an exponential moving average of the parameters, kept inside the optimizer's launch.
 *
 * cmf_adam_step_ema / cmf_adam_step_guarded_ema: cmf_adam_step / cmf_adam_step_guarded (the same kernels, instantiated with the average
 * on; parameters and moments get the same bits) and, for every element, with pn the value just stored to the parameter and ev = ema[e]:
 *     ema[e] = fmaf(omd, pn - ev, ev)                // omd = (float)(1.0 - ema_decay): formed in double on the host, rounded once
 * one explicit fma, so the result does not depend on contraction.  The lerp form on purpose: its fixed point is pn itself (pn == ev gives
 * ev back bit for bit), where d * ev + (1 - d) * pn carries a relative bias of order 2^-24 / (1 - d) -- 3e-5 at d = 0.999.
 * ema: `total` floats in bucket order in device memory, 4-byte aligned like m and v; 0 < ema_decay < 1 (anything else, NaN included:
 * hipErrorInvalidValue, nothing launched).  The caller initialises ema (to the parameters: no debiasing is then needed).
 * Skip rule (guarded form): the return on a skipped step (non-finite norm and skip_nonfinite) is in front of EVERY store, the one to ema
 * included -- a skipped step leaves p, m, v and ema untouched.  Without skip a NaN reaches ema[e] wherever it reaches the parameter.
 *
 * cmf_param_exchange: every parameter element is swapped with flat[e] (params[t][e - offsets[t]] <-> flat[e]) through the same address
 * table and chunk walk as cmf_adam_step.  Pure copies: applied twice it is the identity, bit for bit.  flat: `total` floats in bucket
 * order, 4-byte aligned.  One launch; run the model on the averaged weights between two calls with flat = ema. */
int cmf_adam_step_ema(int n_tensors, const long long *offsets, float *const *params, long long total, const float *grad, float *m, float *v,
                      double lr, double beta1, double beta2, double eps, double weight_decay, long long step, float *ema, double ema_decay,
                      void *stream);
int cmf_adam_step_guarded_ema(int n_tensors, const long long *offsets, float *const *params, long long total, const float *grad, float *m,
                              float *v, double lr, double beta1, double beta2, double eps, double weight_decay, long long step,
                              double max_grad_norm, int skip_nonfinite, const double *partials, double *record, float *ema,
                              double ema_decay, void *stream);
int cmf_param_exchange(int n_tensors, const long long *offsets, float *const *params, long long total, float *flat, void *stream);

/* Float offsets, inside `saved`, of the six per-layer BatchNorm blocks (mean | invstd | a | c, 4*C_l floats each). */
int cmf_setconv_bn_offsets(const cmf_setconv_desc *d, long long *offsets6);

/* [1x1 conv (no bias) + BatchNorm + ReLU] x L on a materialised input: the stacks of the flow / motion heads
 * (utils/model_utils/radarflow_util.py:253-261,277-285: 512 -> 256 -> 128 -> 64) sequenced by the library like a set-conv
 * block -- forward GEMM with train-mode statistics, fold; backward: BN-backward sums, BN backward in place, weight
 * gradient (deterministic split-K), masked data gradient.  Issued from Python one kernel at a time these chains were host
 * bound (25 launches of 5-45 us with 15-30 us between them: the two heads' backward passes took 1.0 ms of a 22 ms step with
 * the GPU idle).  C[0] = input channels, C[l] = output channels of layer l (1..L, L <= 4, all multiples of 4).
 * saved: z_1 .. z_L and the BN blocks (mean | invstd | a | c) ; scratch: partial sums, gradient buffers, split-K slabs. */
typedef struct cmf_mlp_desc {
    long long M; int L; int C[5]; int training;
    float eps[4], momentum[4];
    const float *x; long long ldx;                       /* (M, C[0]) activated input, row stride ldx */
    const float *w[4];                                   /* (C[l], C[l-1]) dense */
    const float *gamma[4], *beta[4];
    float *rmean[4], *rvar[4]; long long *nbt[4];        /* running statistics (nbt NULL: counter not touched) */
    float *saved, *scratch;
    float *out; long long ldo;                           /* forward: relu(bn_L(z_L)), (M, C[L]) */
    const float *dout; long long lddout;                 /* backward */
    float *dx; long long lddx;                           /* (M, C[0]) or NULL */
    float *dw[4]; int acc_w[4];
    float *dgamma[4], *dbeta[4]; int acc_bn[4];
} cmf_mlp_desc;
int cmf_mlp_sizes(const cmf_mlp_desc *d, long long *saved_floats, long long *scratch_fwd, long long *scratch_bwd);
int cmf_mlp_forward(const cmf_mlp_desc *d, void *stream);
int cmf_mlp_backward(const cmf_mlp_desc *d, void *stream);

/* Deferred nn.BatchNorm2d running-statistics update.  A weight-shared encoder is called twice per step
 * (cmflow.py:72-73); to run the two calls CONCURRENTLY they are issued with rmean/rvar/nbt == NULL (batch statistics
 * only) and the momentum updates are applied afterwards, in call order, from each call's saved batch mean / invstd.
 * table (device memory): one entry per BN layer; offset = float offset of that layer's BN block inside a call's `saved`
 * arena (saved0 = first call, saved1 = second call). */
typedef struct cmf_bn_update_entry {
    float *rmean, *rvar; long long *nbt;
    int C; float momentum, eps; double count;      /* channels; bn.momentum, bn.eps; rows the statistics were taken over */
    long long offset;
} cmf_bn_update_entry;
int cmf_bn_running_update(int n_entries, const cmf_bn_update_entry *table, int n_calls, const float *saved0,
                          const float *saved1, void *stream);

/* The independent scales of a MultiScaleEncoder (radarflow_util.py:101-118) in one call (the *_multi entry points below):
 * descs[i] is issued on streams[i] from its own host thread inside the library (n <= 16).  The caller orders the streams
 * against its own (events before and after); nothing is synchronised.
 * The per-point tails (layers 4-6: three <= 64-channel layers over the B*N points) are taken out of the chains and
 * run for ALL blocks of the call as batched launches on one stream -- one launch per kernel of the tail instead of one per
 * block (at N = 256 these kernels are 128 workgroups of latency each; the eight chains of an encoder call spent 1.5 ms of
 * the 22 ms training step in them).  Forward: cmf_setconv_forward_heads_multi (up to the max over the ball, per stream),
 * join the streams, cmf_setconv_tail_forward(n, descs, stream).  Backward: cmf_setconv_tail_backward(n, descs, stream) (from
 * dout to the gradient of the pooled features + the gradients of layers 4-6), fork, cmf_setconv_backward_bodies_multi.
 * Same kernels, same order per block: results are bit-identical to cmf_setconv_forward / _backward.  CMF_TAIL_BATCH=0 (or
 * blocks whose tails differ in width / mode) runs the tails block by block. */
int cmf_setconv_forward_heads_multi(int n, const cmf_setconv_desc *descs, void *const *streams);
/* 1 when cmf_setconv_forward_heads_multi will run these blocks' slot-level bodies in lock step as batched launches on streams[0]
 * alone (narrow blocks with train-mode BatchNorm and indices ready: the first encoder) -- the caller may then pass its own stream for
 * every entry and needs no fork / join around the call; else 0. */
int cmf_setconv_forward_bodies_batched(int n, const cmf_setconv_desc *descs);
int cmf_setconv_backward_bodies_batched(int n, const cmf_setconv_desc *descs);      /* the same for cmf_setconv_backward_bodies_multi */
int cmf_setconv_tail_forward(int n, const cmf_setconv_desc *descs, void *stream);
int cmf_setconv_tail_backward(int n, const cmf_setconv_desc *descs, void *stream);
int cmf_setconv_backward_bodies_multi(int n, const cmf_setconv_desc *descs, void *const *streams);

/* Cost-volume weighting (radarflow_util.py:219-221,235-236): out[m,c] = sum_k w[m,k,c] * x[m,k,c] over rows
 * m = sample*n1 + point.  idx == NULL: x is (M,K,C) dense.  idx (M,K) int32: x is (samples*n_src, C) per-point rows
 * and the k-th operand of row m is x[sample*n_src + idx[m,k]] (the grouped tensor is never materialised).
 * The gradient call writes dw = dcost*x and dx = dcost*w, each (M,K,C) (either may be NULL).  leaky bit 0: x is a
 * stored LeakyReLU(0.1) activation and dx is multiplied by its derivative; bit 1: w is a stored ReLU activation
 * (WeightNet, radarflow_util.py:307-318) and dw is masked by w > 0 -- gradients w.r.t. the pre-activations.
 * C % 4 == 0, 16-byte aligned pointers. */
int cmf_weighted_ksum(long long M, int K, int C, int n1, int n_src, const float *w, const float *x, const int *idx,
                      float *out, void *stream);
/* dx_colsum (optional): [cmf_weighted_ksum_grad_tiles(C)][C] per-workgroup column sums of dx, to be reduced with
 * cmf_colsum -- the bias gradient of the layer that produced x; cmf_weighted_ksum_grad_tiles returns 0 when C does not
 * allow it. */
int cmf_weighted_ksum_grad_tiles(int C);
int cmf_weighted_ksum_grad(long long M, int K, int C, int n1, int n_src, int leaky, const float *dcost, const float *w,
                           const float *x, const int *idx, float *dw, float *dx, float *dx_colsum, void *stream);
/* The same weighting with WeightNet's last layer (radarflow_util.py:307-318: Conv2d(8, C, 1) + ReLU) folded in: the
 * weights are not an operand but recomputed where they are used, w[m,k,c] = relu(bl[c] + sum_j h[m,k,j] * Wl[c,j]) with
 * h (M*K, 8) the hidden activation, Wl (C, 8), bl (C) -- the (M,K,C) weight tensor and its gradient never exist.
 * C in {256, 512, 1024} (cmf_weightnet_ksum_tiles(C) > 0), M*K < 2^31, x / idx / leaky bit 0 as above.
 * The gradient call writes dx (M,K,C), dh (M*K, 8) and one partial row per workgroup,
 * part [cmf_weightnet_ksum_tiles(C)][C*8 + C + C + 8] = sums of dWl (C,8) | dbl (C) | column sums of dx (C) | column sums
 * of dh (8), to be reduced in fixed order with cmf_colsum.  leaky bit 2 (value 4): h is itself a stored ReLU activation
 * (WeightNet's second hidden layer) -- dh is then masked by h > 0, i.e. it is the gradient w.r.t. that layer's
 * pre-activation and its column sums are that layer's bias gradient.  dcost has row stride ldd floats (>= C: it may be a column block of a wider gradient). */
int cmf_weightnet_ksum_tiles(int C);
int cmf_weightnet_ksum(long long M, int K, int C, int n1, int n_src, const float *h, const float *Wl, const float *bl,
                       const float *x, const int *idx, float *out, void *stream);
int cmf_weightnet_ksum_grad(long long M, int K, int C, int n1, int n_src, int leaky, const float *dcost, long long ldd, const float *h,
                            const float *Wl, const float *bl, const float *x, const int *idx, float *dx, float *dh,
                            float *part, void *stream);

/* Global feature of Backbone (cmflow.py:76-81,89-91: torch.max over the points, expand, cat): out[b,n,0:C] = f[b,n,:],
 * out[b,n,C:2C] = max_n' f[b,n',:], point-major rows with strides ldf / ldo floats (multiples of 4, so out may be a
 * column block of a wider buffer); arg (B,C) int32 = first row attaining the maximum.  The gradient call returns
 * df[b,n,c] = dout[b,n,c] + (n == arg[b,c]) * sum_n' dout[b,n',C+c].  C % 4 == 0, 16-byte aligned pointers. */
int cmf_global_max_cat(int B, int N, int C, const float *f, long long ldf, float *out, long long ldo, int *arg, void *stream);
int cmf_global_max_cat_grad(int B, int N, int C, const float *dout, long long ldd, const int *arg, float *df, long long ldf,
                            void *stream);

/* Weight of the stacked first conv of a MultiScaleEncoder (radarflow_util.py:132-139: the feature half of every scale's
 * first 1x1 conv applied to the SAME input, here one GEMM): wf[(s*O1 + r)][c], Kp columns, from the n_w conv weights
 * w[s] = [O1][3 + cin] (xyz columns first): columns [0, cin - n_tail) = input channels n_tail.., then the first n_tail
 * input channels, then zeros up to Kp.  cmf_unstack_first_conv_grad adds the GEMM's weight gradient dwf [n_w*O1][Kp] back
 * into the conv weights' gradients g[s] (same layout as w[s]; the xyz columns are not touched).  n_w <= 8; w / g are
 * HOST arrays of device pointers. */
int cmf_stack_first_conv(int n_w, int O1, int cin, int n_tail, int Kp, const float *const *w, float *wf, void *stream);
int cmf_unstack_first_conv_grad(int n_w, int O1, int cin, int n_tail, int Kp, const float *dwf, float *const *g, void *stream);

/* ---- the training step's loss -------------------------------------------------------------
 * RadarFlowLoss of losses/radar_loss.py:260-292 for model 'cmflow' / 'cmflow_t': SoftChamfer (:17-58),
 * SpatialSmoothness (:60-97), RadialDisplacement (:99-122), EgoMotion (:162-183), MotionSeg (:185-205),
 * OpticalFlow (:207-243 with utils/util.py:31-58) and DynamicFlow (:245-258), forward AND the gradient of the
 * weighted total with respect to the three network outputs, in one call (3 launches, no host sync; the
 * reference reads 8 loss items back with .item(), :156-159,285-288).  Layouts are the reference's:
 * clouds/flows (B,3,N), per-point scalars (B,N), opt (B,N,2), transforms (B,4,4) row-major.
 * items[9] = total, Loss (self-supervised sum), smoothnessLoss, chamferLoss, veloLoss, egoLoss, maskLoss,
 * opticalLoss, superviseLoss.  Gradient outputs may be NULL (evaluation).
 * Cloud size: num_nb < N <= CMF_RADAR_LOSS_MAX_N, num_nb in {4, 8, 16} (the reference has no limit, radar_loss.py:60-97).
 * N <= 704 with num_nb == 8 (the reference's training size is 256) keeps a sample in one workgroup's LDS; everything else
 * takes the tiled form (the cloud streamed through LDS in tiles of 256 points, a sample's lists in `workspace`): same terms,
 * same per-point arithmetic, the per-sample sums folded in another fixed order.  cmf_radar_loss_tiled forces the tiled
 * form at any size (tests compare the two forms on the same input). */
#define CMF_RADAR_LOSS_MAX_N 65536
typedef struct cmf_radar_loss_desc {
    int B, N;
    const float *pc1, *pc2, *pred_f, *gt_f;                                    /* (B,3,N) */
    const float *vel1, *mseg_pre, *mseg_gt, *dyn_mask, *radar_u, *radar_v;     /* (B,N) */
    const float *opt;                                                          /* (B,N,2) */
    const float *pre_trans, *gt_trans;                                         /* (B,4,4) */
    const float *camera_inverse;                                               /* (3,3) inverse intrinsics */
    const float *t_camera_radar;                                               /* (4,4) */
    float w_self, w_em, w_ms, w_opt, w_dyn;                                    /* radar_loss.py:262: 1,1,1,0.1,1 */
    float zeta, alpha; int num_nb; float lower_bound;                          /* 0.005, 0.5, 8, 0.25 */
    int self_only;             /* 1: model 'raflow' (radar_loss.py:274-276) -- only the three self-supervised terms;
                                  the inputs of the other four may be NULL, their items are reported as 0 */
    float *items;                                                              /* [9] */
    float *d_pred_f, *d_pre_trans, *d_mseg_pre;                                /* (B,3,N), (B,4,4), (B,N) or NULL */
    float *workspace;                                                          /* cmf_radar_loss_workspace_nb floats */
    const float *t_camera_radar_batch;   /* (B,4,4) or NULL.  Non-NULL: sample i projects through row i instead of t_camera_radar
                                            (cmf_augment_batch's calib); NULL: the shared matrix.  Appended last: a caller built
                                            against the shorter struct must zero-initialise the descriptor */
} cmf_radar_loss_desc;
long long cmf_radar_loss_workspace_nb(int b, int n, int num_nb);   /* floats; num_nb as in the descriptor */
int cmf_radar_loss(const cmf_radar_loss_desc *d, void *stream);
int cmf_radar_loss_tiled(const cmf_radar_loss_desc *d, void *stream);   /* workspace: cmf_radar_loss_workspace_tiled */
long long cmf_radar_loss_workspace_tiled(int b, int n, int num_nb);

/* ---- evaluation metrics of one batch ------------------------------------------------------
 * utils/eval_util.py: eval_scene_flow :42-86, eval_motion_seg :104-118, eval_trans_RPE :89-102 (with
 * utils/odometry_util.py:61-160), which copy every tensor to the host and run numpy.  pc (B,3,N) as
 * main_util.py:175 passes it; pred, labels (B,N,3); mask, pred_m (B,N) with 1 = static; transforms (B,4,4);
 * (r_res, theta_res, phi_res) the radar resolution of dataset/vod.py:21-23.
 * metrics[14] (fp64) = rne, 50-50 rne, mov_rne, stat_rne, sas, ras, epe, accs, accr, acc, miou, sen, RTE, RAE.
 * workspace: 16 * B doubles. */
int cmf_eval_metrics(int b, int n, const float *pc, const float *pred, const float *labels, const float *mask,
                     const float *pred_m, const float *gt_trans, const float *pred_trans,
                     float r_res, float theta_res, float phi_res, double *metrics, double *workspace, void *stream);

/* Pseudo labels of the training step (main_util.py:63-67): dyn_mask = extract_dynamic_from_fg (:209-225), mseg_gt =
 * where(dyn_mask == 1, mseg_label_RRV (:253-265), dyn_mask).  pc1 (B,3,N); gt_trans (B,4,4); vel1, fg_mask (B,N)
 * (fg_mask 1 = background); interval (B); flow_label (B,N,3).  Outputs (B,N) floats, 1 = static; residual may be NULL. */
int cmf_pseudo_labels(int b, int n, const float *pc1, const float *gt_trans, const float *vel1, const float *interval,
                      const float *fg_mask, const float *flow_label, float vr_thres,
                      float *dyn_mask, float *mseg_gt, float *residual, void *stream);

/* Test-only: occupies `stream` for about `microseconds` with a one-wave kernel that polls the constant 100 MHz clock
 * (s_sleep between polls: no measurable load on the chip).  tests/test_gpu_stress.py uses it to shift the relative timing of
 * the side-stream chains at every fork point (fused_blocks.stress_*): results must not depend on it. */
int cmf_debug_spin(float microseconds, void *stream);

/* ---- ragged batches: B samples of their own point counts in one call (inference) ------------------------------------
 * The reference evaluates on the WHOLE cloud of every frame (dataset/vod.py:92-111 resamples for training only), one frame pair per
 * forward (main.py:203: batch_size = 1), N1 != N2.  Here a batch of such pairs is a padded (B, Nmax, .) tensor plus per-sample counts
 * in DEVICE memory (const int *, B entries); the counted forms below are the five places where a sample's size enters the
 * arithmetic.  Everything else of the eval-mode model is row-wise and runs on the padded rows unchanged.  Every counted form equals
 * its dense entry point called with b = 1 on the truncated sample (rows [0, count)), in the strength stated per function; counts are
 * clamped to [0, rows in memory] inside the kernels, so a wrong count cannot make them leave the padded tensors; a count of 0 (a
 * caller's error: a sample has at least one point) is not finite garbage but NaN / -inf -- the weights divide by a zero score sum, the
 * maximum of no rows is -inf.  Padded input rows must be finite; they never influence a valid output.
 *
 * cmf_ball_query_multi_counted: cmf_ball_query_multi with candidates j < n_src[c][s] and centres p < n_ctr[c][s] (tables of nclouds
 *   device pointers, host arrays).  Valid centres: bit-identical to cmf_ball_query(b = 1, n = n_src, m = n_ctr) per scale; the rows of
 *   padded centres and of empty balls are zeros.  n <= 1024 (the one-scan kernel); larger clouds are refused, not sent elsewhere.
 * cmf_setconv_queries_counted: cmf_setconv_queries over ragged samples, counts[i] the count array of block i (centres = cloud in a
 *   set-conv block; the blocks of one cloud must share one array).  Refuses N > 1024.
 * cmf_knn_counted: cmf_knn with candidates j < n_src[s]; canonical order; indices (and distances) bit-identical to
 *   cmf_knn(b = 1, n = n_src[s]) for every query row, padded query rows included (their lists are valid rows of their own sample).
 * cmf_global_max_cat_counted: maximum and arg over the rows < cnt[s], bit-identical to the dense call on the truncated sample; ALL N
 *   rows of out are written (copy | that maximum).
 * cmf_ego_refine_counted: score sum, weights, weighted centroids, covariance over the rows < cnt[s] in the dense kernel's order:
 *   trans, aux and the valid slices of W, Bm, sf, mask are bit-identical to cmf_ego_refine(b = 1, n = cnt[s]); padded slots of W, Bm,
 *   sf, mask are zeros.  stat (b,n), optional: score with the padded slots zeroed.
 * cmf_eval_metrics_counted: per sample the 14 metrics of cmf_eval_metrics(b = 1, n = cnt[s]) on its valid rows, then their mean over
 *   the samples in index order -- what main_util.py:176-192 accumulates with the test loader's batch size 1.  A sample without
 *   static points gives stat_rne = NaN (0 / 0, numpy's mean of an empty selection) and so does the mean; a sample without moving
 *   points gives mov_rne = 0 (0 / 1e-6): both exactly as cmf_eval_metrics at b = 1.  workspace: 16 * B doubles.
 *
 * Training on ragged batches (eval-mode BatchNorm): every layer is row-wise in both directions, so a padded row carries an exactly
 * zero gradient and a valid row never reads a padded one; the two places where gradients fan in over a sample have counted forms that
 * make this hold by construction, whatever the incoming gradient holds behind a sample's count:
 * cmf_ego_refine_grad_counted: cmf_ego_refine_grad with rows n apart and every sum (masked G_R / g_t, the Kabsch backward, sum g_w w,
 *   the score sum) over the rows < cnt[s] in the dense kernel's order: the valid slices of g_flow, g_w, g_score are bit-identical to
 *   cmf_ego_refine_grad(b = 1, n = cnt[s]) on the truncated sample; their padded slots are zeros.  W, Bm, mask, aux: as
 *   cmf_ego_refine_counted wrote them (aux is required).
 * cmf_global_max_cat_grad_counted: df[s,n,c] = dout[s,n,c] + (n == arg[s,c]) * sum_{n' < cnt[s]} dout[s,n',C+c] for n < cnt[s], bit-
 *   identical to cmf_global_max_cat_grad(B = 1, N = cnt[s]) on the truncated sample; the rows behind the count are zeros.  dout may
 *   be row-strided (ldd) as in the dense call. */
int cmf_ball_query_multi_counted(int b, int n, int m, int nq, const float *radii, const int *nsamples, int nclouds,
                                 const float *const *new_xyz, const float *const *xyz, int *const *idx,
                                 const int *const *n_ctr, const int *const *n_src, void *stream);
int cmf_setconv_queries_counted(int n, const cmf_setconv_desc *descs, const int *const *counts, void *stream);
int cmf_knn_counted(int b, int n, int s, int nsample, const float *xyz, const float *new_xyz, const int *n_src,
                    int *idx, float *dist, void *stream);
int cmf_global_max_cat_counted(int B, int N, int C, const float *f, long long ldf, float *out, long long ldo, int *arg,
                               const int *cnt, void *stream);
int cmf_ego_refine_counted(int b, int n, float eps, float thres, const float *pc1, const float *flow, const float *score,
                           const int *cnt, float *W, float *Bm, float *trans, double *aux, float *sf, unsigned char *mask,
                           float *stat, void *stream);
int cmf_eval_metrics_counted(int b, int n, const int *cnt, const float *pc, const float *pred, const float *labels, const float *mask,
                             const float *pred_m, const float *gt_trans, const float *pred_trans,
                             float r_res, float theta_res, float phi_res, double *metrics, double *workspace, void *stream);
int cmf_ego_refine_grad_counted(int b, int n, float eps, const float *pc1, const float *score, const int *cnt, const float *W,
                                const float *Bm, const unsigned char *mask, const double *aux, const float *g_sf,
                                const float *g_trans, float *g_flow, float *g_w, float *g_score, void *stream);
int cmf_global_max_cat_grad_counted(int B, int N, int C, const float *dout, long long ldd, const int *arg, float *df, long long ldf,
                                    const int *cnt, void *stream);

/* ---- ragged batches: the loss and the pseudo labels on whole frames ---------------------------------------------------------
 * cmf_radar_loss_counted: cmf_radar_loss on B padded samples of their own sizes.  Everything indexed by the points of cloud 1 (pc1,
 *   pred_f, gt_f, the per-point scalars, opt, d_pred_f, d_mseg_pre) has row stride N1max, pc2 has row stride N2max; n1, n2 (B ints in
 *   DEVICE memory) are the valid counts.  items (B,9): for sample i the nine items cmf_radar_loss returns with B = 1 on the truncated
 *   sample (pc1[i,:,:n1[i]], pc2[i,:,:n2[i]], ...): every mean over points divides by n1[i] (the cloud-2 side of the Chamfer term by
 *   n2[i], its density masks average over the other cloud's valid points), the smoothness factor N is n1[i], the class counts and
 *   masked means of the motion-seg / optical / dynamic terms run over the sample's valid points.  items_mean[9]: their mean over the
 *   B samples, folded in index order -- the reference's protocol at batch size 1, as cmf_eval_metrics_counted defines its metrics.
 *   This is NOT cmf_radar_loss on a batch of equal-sized samples: the dense loss (like the reference) pools the class counts and
 *   the masked sums of those three terms over the whole batch before dividing; here every sample divides by its own.
 *   The gradients are those of items_mean[0]: the B = 1 gradients of the truncated sample, multiplied by 1/B as the last operation
 *   (exactly the dense B = 1 values / B when B is a power of two); padded slots of d_pred_f and d_mseg_pre are written as 0.
 *   With n1[i] == n2[i] the items of sample i are bit-identical to the dense call of the same form (LDS / tiled) at B = 1; with
 *   n1 != n2 the cloud-2 Chamfer summands are weighted by (float)n1 / (float)n2 (exactly 1 in the equal case) before the one
 *   division by n1 -- one more rounding per summand.  Slots behind a count are read as points at infinite distance with zero
 *   weight; their content does not influence any output as long as it is finite.  Counts are clamped inside the kernels to
 *   [num_nb + 1, N1max] and [1, N2max]: a wrong count gives wrong numbers, never an access outside the tensors.
 *   Forms as cmf_radar_loss: max(N1max, N2max) <= 704 with num_nb == 8 keeps a sample in one workgroup's LDS, everything else up to
 *   CMF_RADAR_LOSS_MAX_N takes the tiled kernels; cmf_radar_loss_counted_tiled forces the tiled form.  No floating-point atomics:
 *   results are bit-reproducible and independent of the padded sizes and of the other samples in the batch.
 * cmf_pseudo_labels_counted: cmf_pseudo_labels with rows nmax apart and the one reduction over a sample it contains -- the mean
 *   residual of mseg_label_RRV (main_util.py:260); extract_dynamic_from_fg (:209-225) is per point -- over the first n1[s] points.
 *   Valid slots are bit-identical to cmf_pseudo_labels(b = 1, n = n1[s]) on the truncated sample; padded slots of dyn_mask, mseg_gt
 *   (and residual) are written as 0 -- cmf_radar_loss_counted never reads them.  n1 is clamped to [0, nmax]. */
typedef struct cmf_radar_loss_counted_desc {
    int B, N1max, N2max;
    const int *n1, *n2;                                                        /* (B) device */
    const float *pc1, *pred_f, *gt_f;                                          /* (B,3,N1max) */
    const float *pc2;                                                          /* (B,3,N2max) */
    const float *vel1, *mseg_pre, *mseg_gt, *dyn_mask, *radar_u, *radar_v;     /* (B,N1max) */
    const float *opt;                                                          /* (B,N1max,2) */
    const float *pre_trans, *gt_trans;                                         /* (B,4,4) */
    const float *camera_inverse;                                               /* (3,3) inverse intrinsics */
    const float *t_camera_radar;                                               /* (4,4) */
    float w_self, w_em, w_ms, w_opt, w_dyn;
    float zeta, alpha; int num_nb; float lower_bound;
    int self_only;                                                             /* as in cmf_radar_loss_desc */
    float *items;                                                              /* (B,9) per sample */
    float *items_mean;                                                         /* [9] */
    float *d_pred_f, *d_pre_trans, *d_mseg_pre;                                /* (B,3,N1max), (B,4,4), (B,N1max) or NULL */
    float *workspace;                                                          /* cmf_radar_loss_counted_workspace floats */
    const float *t_camera_radar_batch;                                         /* (B,4,4) or NULL, as in cmf_radar_loss_desc */
} cmf_radar_loss_counted_desc;
long long cmf_radar_loss_counted_workspace(int b, int n1max, int n2max, int num_nb);
int cmf_radar_loss_counted(const cmf_radar_loss_counted_desc *d, void *stream);
int cmf_radar_loss_counted_tiled(const cmf_radar_loss_counted_desc *d, void *stream);   /* workspace: ..._workspace_tiled */
long long cmf_radar_loss_counted_workspace_tiled(int b, int n1max, int n2max, int num_nb);
int cmf_pseudo_labels_counted(int b, int nmax, const int *n1, const float *pc1, const float *gt_trans, const float *vel1,
                              const float *interval, const float *fg_mask, const float *flow_label, float vr_thres,
                              float *dyn_mask, float *mseg_gt, float *residual, void *stream);

/* ---- a training split that lives on the device: one batch per launch ------------------------------------------------------------
 * cmf_draw_batch: the training batch of one step from packed whole frames (cmflow_amd/dataset.py DeviceSplit) -- frame choice, the
 *   reference's per-frame resampling to npoints (dataset/vod.py:95-121 sample_points) and the layout of extract_data_info
 *   (main_util.py:21-36) in one launch, one workgroup per (slot, cloud).
 *   Packed split of nframes frames: tab1 (off1[nframes], 14) per point of cloud 1 = xyz 3 | features 3 | label 3 | mask | radar_u |
 *   radar_v | opt_flow 2; tab2 (off2[nframes], 6) = xyz 3 | features 3; off1, off2 (nframes + 1) int32 row offsets; trans (nframes,16);
 *   interval (nframes).  max_points: the largest point count of any frame and cloud of the split, <= CMF_DRAW_MAX_POINTS (the sort
 *   keys of one cloud, 8 bytes a point over the next power of two, live in one workgroup's LDS: 16384 * 8 = 128 KiB of the CU's
 *   160 KiB; the next power of two would not fit); it sizes the launch's LDS.  frames (B) int32: the frame of every slot.
 *   -> pc1, pc2, ft1, ft2 (B,3,N); gt_trans (B,4,4); flow_label (B,N,3); fg_mask (B,N); interval_out (B); radar_u, radar_v (B,N);
 *   opt_flow (B,N,2); idx1, idx2 (B,N) int32: the drawn point of every output position, N = npoints <= CMF_DRAW_MAX_NPOINTS.
 *   Every float is a copy: out[..j..] = table row idx[slot][j] of the slot's frame, bit for bit.
 *   Sampling, per (slot, cloud), for a frame of n points: u32(i) = word 0 of Philox4x32-10 with counter (slot, cloud, i, 0) and the
 *   key of the call = words 0, 1 of Philox4x32-10 with counter (seed lo, seed hi, draw lo, draw hi) and key (0, 0).
 *     n <  N: idx = 0 .. n-1, then for j = 0 .. N-n-1 the point (u32(j) * n) >> 32 (independent uniform draws);
 *     n >= N: point i gets the 64-bit key (u32(i) << 32) | i; the N smallest keys in ascending order are the draw (a uniformly
 *             random N-subset in uniformly random order; the keys are distinct).
 *   A slot's outputs depend on (seed, draw, slot, frame) only.  tests/draw_ref.py restates the rule on the host.
 *   Frame ids and offsets are trusted like the counts of the ragged entry points; ids are clamped to [0, nframes-1] and a frame's
 *   count to [1, max_points] inside the kernel: a bad id gives wrong data, not an access outside the tables. */
#define CMF_DRAW_MAX_POINTS 16384
#define CMF_DRAW_MAX_NPOINTS 32768
int cmf_draw_batch(int B, int npoints, int nframes, int max_points, const float *tab1, const float *tab2, const int *off1,
                   const int *off2, const float *trans, const float *interval, const int *frames,
                   unsigned long long seed, unsigned long long draw,
                   float *pc1, float *pc2, float *ft1, float *ft2, float *gt_trans, float *flow_label, float *fg_mask,
                   float *interval_out, float *radar_u, float *radar_v, float *opt_flow, int *idx1, int *idx2, void *stream);

/* cmf_draw_batch_at: slots slot0 .. slot0 + B - 1 of a larger (global) batch -- a data-parallel rank's share, DeviceSplit.draw's
 *   slot0.  The same kernel and arguments as cmf_draw_batch (which is slot0 = 0); local slot s samples with counter
 *   (slot0 + s, cloud, i, 0) and everything else, frames[s] and every output row, is indexed by the local slot.  So row s equals, bit
 *   for bit, row slot0 + s of the one call that draws the whole global batch with the same (seed, draw) and the same frame in that
 *   slot.  slot0 >= 0 and slot0 + B <= INT_MAX, an argument error otherwise. */
int cmf_draw_batch_at(int slot0, int B, int npoints, int nframes, int max_points, const float *tab1, const float *tab2,
                      const int *off1, const int *off2, const float *trans, const float *interval, const int *frames,
                      unsigned long long seed, unsigned long long draw,
                      float *pc1, float *pc2, float *ft1, float *ft2, float *gt_trans, float *flow_label, float *fg_mask,
                      float *interval_out, float *radar_u, float *radar_v, float *opt_flow, int *idx1, int *idx2, void *stream);

/* cmf_draw_frames: B WHOLE frames of the same packed split as one ragged batch (DeviceSplit.draw_frames) -- no sampling, the
 *   padding rule of dataset.collate_ragged and the layout of extract_data_info_ragged in one launch, one workgroup per (chunk of 256
 *   positions, cloud, slot).  Tables, offsets, trans, interval and frames as cmf_draw_batch.
 *   -> pc1, ft1 (B,3,nmax1); pc2, ft2 (B,3,nmax2); gt_trans (B,4,4); flow_label (B,nmax1,3); fg_mask, radar_u, radar_v (B,nmax1);
 *   interval_out (B); opt_flow (B,nmax1,2); n1, n2 (B) int32: the point counts of the slot's frame.
 *   Every float is a copy: position j < n of a slot is table row j of its frame, position j >= n is table row 0 (the frame's first
 *   point with its label, mask, u, v and flow row) -- with nmax1, nmax2 the largest counts of the batch this is, bit for bit, what
 *   as_batch_dict_ragged(extract_data_info_ragged(collate_ragged(items))) gives for the same frames.
 *   nmax1, nmax2 <= CMF_DRAW_MAX_NPOINTS; CMF_DRAW_MAX_POINTS does not bound them (nothing is sorted, no LDS is used).  B <= 65535.
 *   Frame ids and offsets are trusted; ids are clamped to [0, nframes-1] and a frame's count to [1, nmax] inside the kernel, and
 *   n1, n2 receive the clamped count: a bad id or a too-small nmax gives wrong data, not an access outside the tables.  Offsets
 *   are expected to describe frames of at least one row (DeviceSplit.from_items refuses empty ones); should one be empty all the
 *   same, its count is 1 and the row read is clamped to the table's last row, off[nframes] - 1. */
int cmf_draw_frames(int B, int nmax1, int nmax2, int nframes, const float *tab1, const float *tab2, const int *off1,
                    const int *off2, const float *trans, const float *interval, const int *frames,
                    float *pc1, float *pc2, float *ft1, float *ft2, float *gt_trans, float *flow_label, float *fg_mask,
                    float *interval_out, float *radar_u, float *radar_v, float *opt_flow, int *n1, int *n2, void *stream);

/* cmf_augment_batch: one label-consistent transform per slot of an already drawn batch, in place (dataset.augment_batch; DESIGN.md
 *   section 19) -- a rotation about the sensor's z axis, optionally after a mirror of the y axis.  Both fix the sensor origin, so
 *   ranges, radial velocities, features, masks, intervals and pixel measurements are untouched; coordinates, flow labels, gt_trans
 *   and the radar-to-camera transform change covariantly.  A definition, not an approximation of one; tests/augment_ref.py
 *   restates it in numpy, bit for bit.  One launch, one workgroup per (chunk of 256 positions, slot); dense batches (n1 == n2) and
 *   ragged ones alike; padded positions are transformed like any other (a ragged batch's padding stays a copy of the first row).
 *   pc1 (B,3,n1), pc2 (B,3,n2), flow_label (B,n1,3), gt_trans (B,16): in place.  t_camera_radar (16): the shared calibration.
 *   -> aug (B,16): the slot's transform A as a 4 x 4; calib (B,16): the slot's radar-to-camera transform (cmf_radar_loss_desc's
 *   t_camera_radar_batch).
 *   Generator: the key of the call = words 0, 1 of Philox4x32-10 with counter (seed lo, seed hi, aug_draw lo, aug_draw hi) and key
 *   (0, 0), as in cmf_draw_batch; slot s takes the words of counter (slot0 + s, 2, 0, 0) under that key.  cmf_draw_batch's counters
 *   have 0 or 1 in that second place, so the two streams never meet, even with aug_draw == draw.  u32 = word 0 decides the angle;
 *   m = -1 when mirror != 0 and bit 31 of word 1 is set, else m = +1.
 *   Angle, float64, every operation rounded on its own (no contraction), no trigonometric function:
 *     r = u32 * 2^-32;   t = ((2 r) - 1) * tan_half_max;   q = t * t;   d = 1 + q;   c = (1 - q) / d;   s = (2 t) / d;
 *     cf = (float)c;   sf = (float)s.
 *   The angle is 2 atan(t) with t uniform in [-tan_half_max, tan_half_max): tan_half_max = tan(yaw_max / 2) (the caller's, computed
 *   once on the host) bounds it by yaw_max, but it is uniform in t and NOT exactly uniform in the angle (its density is
 *   proportional to 1 + t^2: at yaw_max = 10 degrees it varies by 0.8 %, towards 180 degrees the angles crowd at the two ends).  c * c + s * s = 1 up to float64 rounding,
 *   cf * cf + sf * sf = 1 up to float32 rounding of the two: A is orthogonal to about 2^-23, not exactly.
 *   A = [cf, -m sf, 0;  sf, m cf, 0;  0, 0, 1]  (its float32 entries; the products by m = +-1 are exact).
 *   Points of pc1, pc2 and rows of flow_label, float32, every operation rounded on its own:
 *     ym = m * y;   x' = (cf * x) - (sf * ym);   y' = (sf * x) + (cf * ym);   z' = z (not touched).
 *   Transforms, float64 from the float32 entries, every operation rounded on its own, a dot product of three terms is
 *   (a0 b0 + a1 b1) + a2 b2 with the zeros and ones of A taking part as numbers, each result rounded to float32 once at the end.
 *   With R, t the upper 3 x 3 and the translation of gt_trans, Rc, tc those of t_camera_radar, and A^-1 := A^T = diag(1, m, 1) Rz^T
 *   (the transpose of the float32 entries -- the inverse up to the rounding above):
 *     H = R A^T:  H[i][j] = (R[i][0] A[j][0] + R[i][1] A[j][1]) + R[i][2] A[j][2]        (float64, kept)
 *     gt_trans':  R'[i][j] = (A[i][0] H[0][j] + A[i][1] H[1][j]) + A[i][2] H[2][j];   t'[i] = (A[i][0] t[0] + A[i][1] t[1]) + A[i][2] t[2]
 *     calib:      Rc'[i][j] = (Rc[i][0] A[j][0] + Rc[i][1] A[j][1]) + Rc[i][2] A[j][2];   tc' = tc (copied)
 *     aug:        A in the upper 3 x 3, zero translation.
 *   The bottom rows of the three are written as exactly (0,0,0,1).
 *   Exact identity: a slot with cf == 1, sf == 0 (either sign) and m == 1 is not computed but copied -- its points, flow rows and
 *   gt_trans (all 16 entries) keep their bits (signed zeros and NaN payloads included), aug = I, and the upper three rows of calib are
 *   those of t_camera_radar bit for bit.
 *   tan_half_max == 0 with mirror == 0 makes every slot such a slot.
 *   1 <= B <= 65535, 1 <= n1, n2 <= CMF_DRAW_MAX_NPOINTS, slot0 >= 0, slot0 + B <= INT_MAX, tan_half_max finite and >= 0: an argument
 *   error otherwise, never an access outside the tensors. */
int cmf_augment_batch(int slot0, int B, int n1, int n2, unsigned long long seed, unsigned long long aug_draw,
                      double tan_half_max, int mirror, const float *t_camera_radar, float *pc1, float *pc2, float *flow_label,
                      float *gt_trans, float *aug, float *calib, void *stream);

/* ---- from raw radar scans to the packed split (cmflow_amd/prepare.py) ----------------------------------------
 * The arithmetic of the reference's offline preprocess step (preprocess/utils/get_flow_samples.py) on batches of scans and pairs.
 * Scans are packed: scans (scan_off[nscans], ncols >= 5) float32 rows x y z RCS v_r ..., scan_off (nscans + 1) int32 row offsets.
 * Calibration: t_camera_radar (16 doubles, row-major 4 x 4) and projection (12 doubles, row-major 3 x 4), one set for all scans
 * (calib_per_scan = 0) or one per scan (calib_per_scan = 1: (nscans,16), (nscans,12)).
 * The input filter on a row: p_cam = t_camera_radar [x y z 1], uvw = projection p_cam, u = rint(uvw0 / uvw2), v = rint(uvw1 / uvw2)
 * (half to even), all in float64; kept when 0 < u <= width, 0 < v <= height and zlo <= z <= zhi.  There is no depth test: a point
 * behind the camera whose projection lands in the image is kept, as in the reference.  A row whose uvw2 is zero or not finite is
 * dropped (the reference's result is undefined there).  Kept rows keep scan order.
 *
 * cmf_prepare_count: the filter on every row, one workgroup per scan, any scan length.
 *   -> keep (rows) int32: the row's position among the kept rows of its scan, or -1 for a dropped row; uv (rows,2) int32: the pixel
 *   of a kept row (0, 0 for a dropped one); count (nscans) int32: kept rows per scan. */
int cmf_prepare_count(int nscans, int ncols, const float *scans, const int *scan_off, const double *t_camera_radar,
                      const double *projection, int calib_per_scan, int width, int height, double zlo, double zhi,
                      int *keep, int *uv, int *count, void *stream);

/* cmf_prepare_scans: the inference front end -- the same filter, the kept rows of scan s written in scan order to
 *   pc (nscans,3,nmax) = x y z and ft (nscans,3,nmax) = v_r RCS RCS, CMFlow.forward_ragged's padded layout; n (nscans) int32 =
 *   min(kept, nmax) (a scan with more kept rows than nmax is truncated); slots from n on are exact zeros.  nmax <=
 *   CMF_DRAW_MAX_NPOINTS. */
int cmf_prepare_scans(int nscans, int ncols, int nmax, const float *scans, const int *scan_off, const double *t_camera_radar,
                      const double *projection, int calib_per_scan, int width, int height, double zlo, double zhi,
                      float *pc, float *ft, int *n, void *stream);

/* cmf_prepare_pairs: the tab1 / tab2 rows (cmf_draw_batch's layout) of npairs frame pairs, one workgroup per pair.
 *   keep, uv: cmf_prepare_count's results for the same scans.  pairs (npairs,2) int32: scan of frame 1, scan of frame 2.  off1, off2
 *   (npairs + 1) int32: the pair's first row in tab1 / tab2 -- the prefix sums of count[pairs[:,0]] / count[pairs[:,1]], which the
 *   host forms; a pair with more than CMF_DRAW_MAX_POINTS kept rows in a cloud is the caller's error (its points beyond that number
 *   stay background).  t_inv (npairs,16) doubles: inv(radar1_radar2), the frame-1 -> frame-2 rigid transform of static points.
 *   boxes (box_off[npairs], CMF_PREP_BOX_DOUBLES) doubles, box_off (npairs + 1) int32: the matched boxes of every pair, a record =
 *   centre 3 | rotation 9 (row-major; columns = box axes) | half extents 3 | T_b1_b2 16 (row-major) | score.  boxes must not be NULL
 *   (pass one unused record when there is none).
 *   Foreground: boxes in record order; a point is in a box when |(p - c) . axis_a| <= half_a for a = 0, 1, 2 (closed); its in-box
 *   flow is (T_b1_b2 [p 1])[:3] - p.  A box that holds at least one point and whose largest in-box flow norm is < 3 gives its points
 *   that flow (rounded to float32), confidence (float)score, and makes them foreground; a later box overwrites an earlier one.
 *   mode CMF_PREP_MODE_GT: flow_r = (t_inv [p 1])[:3] - p; a foreground point with ||label - flow_r|| > 0.05 (the float32 label, in
 *   float64) keeps its label with mask = 1 - confidence (float32); every other point gets label (float)flow_r, mask 1; u, v and
 *   optical flow are zeros.  mode CMF_PREP_MODE_PSEUDO: foreground as above without the 0.05 rule, background label 0 mask 1;
 *   u, v = the filter's pixel; optical flow = flow[pair][v - 1][u - 1][0..1] from a (height,width,2) float32 image, zeros when
 *   flow or flow[pair] is NULL (flow: npairs device pointers in device memory).
 *   -> tab1 (off1[npairs],14), tab2 (off2[npairs],6). */
#define CMF_PREP_BOX_DOUBLES 32
#define CMF_PREP_MODE_GT 0
#define CMF_PREP_MODE_PSEUDO 1
int cmf_prepare_pairs(int npairs, int ncols, const float *scans, const int *scan_off, const int *keep, const int *uv,
                      const int *pairs, const int *off1, const int *off2, const double *t_inv, const double *boxes,
                      const int *box_off, int mode, const float *const *flow, int width, int height,
                      float *tab1, float *tab2, void *stream);

/* ---- a test run's per-frame results kept on the device (cmflow_amd/results.py) ---------------------------------
 * The store of a split of F frames is packed like its cloud-1 table: off1 (F+1) int32 as in cmf_draw_batch, and per point of cloud 1
 * flow (off1[F],3), score (off1[F]) and mask8 (off1[F]) bytes; per frame trans_pred, trans_gt (F,16), done (F) bytes, metrics (F,14).
 *
 * cmf_pack_results: the outputs of one ragged batch (CMFlow.forward_ragged on a batch of cmf_draw_frames) into the store -- one
 *   launch, the inverse of cmf_draw_frames.  frames, n1 (B) int32: the frame and the cloud-1 count of every slot, as cmf_draw_frames
 *   wrote them; sf (B,3,nmax); stat_cls (B,nmax) or NULL (then score is not touched and may be NULL); mask (B,nmax) bytes;
 *   pre_trans, gt_trans (B,16).  For slot s, f = frames[s] and rows i < min(n1[s], off1[f+1] - off1[f], nmax):
 *     flow[off1[f] + i] = (sf[s,0,i], sf[s,1,i], sf[s,2,i]);  score[off1[f] + i] = stat_cls[s,i];  mask8[off1[f] + i] = mask[s,i];
 *   and trans_pred[f] = pre_trans[s], trans_gt[f] = gt_trans[s], done[f] = 1.  Every value is a copy.
 *   Guarantees: a packed row is written by exactly one thread per slot (no atomics); positions of a slot from that row count on -- the
 *   padded part of the batch -- are never READ, so they may hold anything; a frame larger than nmax (a batch drawn with a too-small
 *   nmax1) leaves its remaining rows unwritten.  The same frame in two slots of one call is allowed only in the sense that both slots
 *   write it: with identical slot contents (the same frame through the same network) the two writes store identical values and the
 *   result is defined; with different contents every row ends up with one slot's value or the other's, unspecified which.
 *   Frame ids are clamped to [0, nframes-1] as in cmf_draw_frames; offsets are trusted to be ascending, and a frame whose rows would
 *   not lie inside [0, total) (total = off1[nframes], passed on the host) has nothing written: a bad id or offset gives wrong data,
 *   not an access outside the store.  B <= 65535, nmax <= CMF_DRAW_MAX_NPOINTS.
 *
 * cmf_eval_metrics_frames: cmf_eval_metrics_counted's per-sample metrics, scattered instead of averaged.  Arguments as there, plus
 *   frames (b) int32 and table (nframes,14) doubles: row frames[s] (clamped to [0, nframes-1]) receives, for the 14 metrics in
 *   cmf_eval_metrics' order, the per-sample value cmf_eval_metrics_counted averages -- the same kernel for the 16 partial sums and the
 *   same expressions after it, so a row is, value for value (NaN for NaN), what cmf_eval_metrics_counted returns for that sample alone
 *   at b = 1, and the mean of a batch's rows in slot order is what it returns for the batch.  No mean is taken and no other row of
 *   the table is touched.  Two slots with the same frame write the same row; identical inputs give identical values.
 *   workspace: 16 * b doubles.
 *
 * cmf_pose_chain: the sensor's pose along every clip from per-frame transforms -- a definition, not an approximation of one.
 *   T (nframes,16) float32 row-major: T_k maps static points from scan-1 to scan-2 sensor coordinates of frame k.  clips (nclips,2)
 *   int32 in DEVICE memory: [first, last) frame ranges, clamped to [0, nframes].  poses (nframes,16) float64.  Per clip [a, b):
 *     P = I;  for k = a .. b-1:  P = P . inv(T_k);  poses[k] = P
 *   with inv(T) = (R^T, -R^T t), the rigid inverse of odometry_util.se3_inverse, whether or not R is exactly orthonormal.
 *   Arithmetic: float64 from the float32 entries; inv's translation is  -((R[0][r] t0 + R[1][r] t1) + R[2][r] t2);  an entry of
 *   the product is  ((P[r][0] M[0][c] + P[r][1] M[1][c]) + P[r][2] M[2][c]) + P[r][3] M[3][c]  with M = inv(T_k) and its bottom row
 *   (0,0,0,1) taking part as numbers; every multiplication and addition is rounded on its own (no contraction); the bottom row
 *   of every pose is written as exactly (0,0,0,1).  tests/results_ref.py restates this in numpy, bit for bit.
 *   One lane per clip walks its frames in order (a parallel scan would change the association).  Rows of poses outside every clip,
 *   and an empty clip, are not written: the caller pre-fills poses (results.py: NaN).  Overlapping clips are the caller's error
 *   (each writes its own chain; which one a shared row keeps is unspecified). */
int cmf_pack_results(int B, int nmax, int nframes, const int *frames, const int *n1, const int *off1, long long total,
                     const float *sf, const float *stat_cls, const unsigned char *mask, const float *pre_trans,
                     const float *gt_trans, float *flow, float *score, unsigned char *mask8, float *trans_pred,
                     float *trans_gt, unsigned char *done, void *stream);
int cmf_eval_metrics_frames(int b, int n, const int *cnt, const float *pc, const float *pred, const float *labels, const float *mask,
                            const float *pred_m, const float *gt_trans, const float *pred_trans,
                            float r_res, float theta_res, float phi_res, int nframes, const int *frames, double *table,
                            double *workspace, void *stream);
int cmf_pose_chain(int nframes, int nclips, const float *T, const int *clips, double *poses, void *stream);

/* ---- a test run's results as bird's-eye-view images (cmflow_amd/vis.py) -----------------------------------------
 * The reference's `--vis` branch (main_util.py:170-172) on the packed store above: per-point colour, then a small rasteriser.  Both
 * entries take a SELECTION of frames: frames (nsel) int64 in device memory (ids clamped to [0, nframes-1]; the same id may occur
 * twice), or NULL for frames 0 .. nsel-1.  off1 / total as in cmf_pack_results: a frame whose rows do not lie inside [0, total) is
 * treated as empty, so a bad id or offset gives a wrong picture, never an access outside the store.
 *
 * cmf_vis_point_colors (utils/vis_util.py:32-42,63 and :139-140 with utils/vis_ops.py:3-50,54-91): colors (total,3) and drawn (total)
 *   bytes, written at the store's own rows for the selected frames and nowhere else.  One wavefront per frame, lane-strided.
 *   flow (total,3) float32: the store's; tab1: the split's cloud-1 table with ld_tab floats per row (label flow at columns 6..8, mask
 *   at column 9); mask (total) bytes: the store's.  What a layer does not read may be NULL.  Layers:
 *     CMF_VIS_FLOW     the predicted flow on the Middlebury wheel: rad_max = max_i sqrt(fx_i^2 + fy_i^2) over the frame (exact in any
 *                      order), d = rad_max + 1e-5, u = fx / d, v = -(fy / d), and then flow_xy_to_colors(u, v):
 *                        rad = sqrt(u^2 + v^2);  a = atan2(-v, -u) / pi;  fk = (a + 1) / 2 * 54;  k0 = floor(fk) clamped to [0, 54];
 *                        k1 = k0 + 1, 55 -> 0;  f = fk - k0;  per channel col = (1 - f) * (w[k0] / 255) + f * (w[k1] / 255);
 *                        rad <= 1: col = 1 - rad * (1 - col), else col = col * 0.75;  value = floor(255 * col).
 *                      All in float64 from the float32 inputs, every operation rounded on its own, in this order (the reference takes
 *                      the angle in float32).  A NaN flow gives an unspecified colour for its frame, never a
 *                      read outside the 55-entry table.
 *     CMF_VIS_FLOW_GT  the same with the label flow as (fx, fy) but the PREDICTED flow's d, as vis_util.py:41-42 forms x_gt, y_gt.
 *     CMF_VIS_SEG      the predicted mask byte: 0 -> (255, 99, 71), otherwise (65, 105, 225).
 *     CMF_VIS_SEG_GT   the split's mask column: == 0 -> (255, 99, 71), == 1 -> (65, 105, 225), any other value: colour (0, 0, 0)
 *                      and drawn = 0 (the reference scatters `mask == 0` and `mask == 1` and nothing else).
 *   drawn is 1 for every point of the other three layers.
 *
 * cmf_vis_render_bev (utils/vis_util.py:65-90 and :139-165): out (nsel,height,width,3) bytes, a pure function of the inputs -- no
 *   atomics, every pixel written once by the thread that owns it.  xyz: the cloud-1 positions with ld_xyz floats per row (the
 *   split's tab1).  All arithmetic float32, + - * and compares only, nothing contracted:
 *     pixel (row r, col c) has the centre cx = c + 0.5, cy = r + 0.5; a point sits at pu = (px - x0) * inv_s, pv = (y1 - py) * inv_s
 *     (row 0 is the largest y) and covers the pixel iff (cx-pu)*(cx-pu) + (cy-pv)*(cy-pv) <= r2.  The pixel takes the colour of the
 *     HIGHEST-indexed point of the frame with drawn != 0 that covers it (matplotlib paints in order), else (80, 80, 80).  A NaN
 *     coordinate covers nothing.  guides != 0: a pixel whose centre x = x0 + cx * s, y = y1 - cy * s lies on a guide is white, over
 *     the points -- range rings r = 10 .. 50: (r-half)^2 <= x*x + y*y <= (r+half)^2, x >= 0, |y| <= 10 (r = 10) or 12.5; bearing
 *     lines at 0, +-5, +-10, +-15 degrees: |y - t*x| <= half * k, 0 <= x <= 60, (t, k) = (tan, sqrt(1 + tan^2)) from a table of float
 *     literals.  The reference's text labels are not drawn.
 *   The host passes s (metres per pixel), inv_s = 1/s, half = s/2, radius (pixels; used only to cull, must satisfy
 *   r2 <= (radius + 0.5)^2) and r2 as float32.  nsel <= 65535, width, height <= CMF_VIS_MAX_SIDE.
 *   tests/vis_ref.py restates both entries in numpy, bit for bit. */
#define CMF_VIS_FLOW 0
#define CMF_VIS_FLOW_GT 1
#define CMF_VIS_SEG 2
#define CMF_VIS_SEG_GT 3
#define CMF_VIS_MAX_SIDE 4096
int cmf_vis_point_colors(int nsel, int nframes, const long long *frames, const int *off1, long long total, int layer,
                         const float *flow, const float *tab1, int ld_tab, const unsigned char *mask,
                         unsigned char *colors, unsigned char *drawn, void *stream);
int cmf_vis_render_bev(int nsel, int nframes, const long long *frames, const int *off1, long long total, const float *xyz,
                       int ld_xyz, const unsigned char *colors, const unsigned char *drawn, int width, int height,
                       float x0, float y1, float s, float inv_s, float half, float radius, float r2, int guides,
                       unsigned char *out, void *stream);

/* ---- a test run's clouds accumulated over a window of frames (cmflow_amd/accumulate.py) -------------------------
 * cmf_accumulate: for every selected target frame j, the cloud-1 points of the last frames of j's clip brought into j's scan-1
 * sensor coordinates -- a definition, not an approximation of one.  Frames of a clip [a, b) are consecutive scan pairs: scan 2 of
 * frame k is scan 1 of frame k+1 (the contract of cmf_pose_chain), and T_k (T (nframes,16) float32, row-major) maps static points
 * from scan-1 to scan-2 coordinates of frame k.
 *   frames (nsel) int64 in device memory, ids clamped to [0, nframes-1], the same id may occur twice; NULL: frames 0 .. nsel-1.
 *   first (nsel) int32: the first frame a of the clip of every selected target, clamped to [0, j].
 *   off1 / total / tab1 / ld_tab: the split's cloud-1 table (xyz at columns 0..2, label flow 6..8, mask 9; ld_tab >= 10).
 *   gt == 0: flow (total,3) and mask (total) bytes are the store's, T its trans_pred; a point is MOVING iff its mask byte is 0.
 *   gt != 0: flow and mask are not read (may be NULL); the flow is tab1's columns 6..8, a point is MOVING iff tab1 column 9 == 0.0f,
 *            and T is the split's trans.  Every other mask value is static.
 *   window W, 1 <= W <= CMF_ACCUM_MAX_WINDOW; mode: CMF_ACCUM_KEEP, CMF_ACCUM_PROPAGATE or CMF_ACCUM_DROP.
 *   cap_off (nsel+1) int32 in device memory, ascending: target s owns output rows cap_off[s] .. cap_off[s+1]-1 (its capacity; the
 *   host passes the sum of its sources' point counts); cap_total: the rows of the outputs.
 *   Outputs: xyz (cap_total,3) float32; src (cap_total) int32, the point's row in tab1 / the store; age (cap_total) bytes;
 *   count (nsel) int32, the rows of the target that hold points.
 * For target j the ages are g = 0 .. G-1, G = min(W, j - a + 1); the source of age g is frame i = j - g (never across the clip's start).
 *   Chain, 3x4 float64 from the float32 entries, affine:  M_0 = I,  M_g = M_g-1 . T_j-g:
 *     c < 3:  M_g[r][c] = (M[r][0] T[0][c] + M[r][1] T[1][c]) + M[r][2] T[2][c]
 *             M_g[r][3] = ((M[r][0] T[0][3] + M[r][1] T[1][3]) + M[r][2] T[2][3]) + M[r][3]          (M = M_g-1, T = T_j-g)
 *   M_g takes scan-1 coordinates of frame j-g to scan-1 coordinates of frame j.  No inverse is taken anywhere: a T that is not exactly
 *   orthonormal is used as it is.
 *   A point p (float32 xyz) of source i at age g:
 *     g == 0:                          xyz = p, copied bit for bit
 *     static, or mode KEEP:            q_r = ((M_g[r][0] px + M_g[r][1] py) + M_g[r][2] pz) + M_g[r][3]
 *     moving, mode PROPAGATE, g >= 1:  with f its flow, tp_r the same expression with T_i in place of M_g, and N = M_g-1:
 *                                        d_r = ((double)p_r + (double)f_r) - tp_r
 *                                        e_r = (N[r][0] d_0 + N[r][1] d_1) + N[r][2] d_2
 *                                        q_r = q_r + (double)g * e_r
 *                                      a constant displacement per step in the ego-compensated frame; at g = 1 the flow's endpoint p + f
 *     moving, mode DROP, g >= 1:       the point is left out
 *   and xyz_r = (float)q_r.  Every multiplication and addition is rounded on its own (no contraction).
 *   Row order: oldest age first, the current frame (g = 0) last -- rendered, "the highest index wins" paints the newest scan on top;
 *   inside an age the source frame's own point order.  tests/accumulate_ref.py restates all of this in numpy, bit for bit.
 * Guarantees, as cmf_pack_results: every output row inside a target's capacity is written exactly once, by one thread (no atomics):
 *   the first count[s] rows hold points, the rows behind them xyz 0, src -1, age 255 (only DROP, or a capacity larger than the sources'
 *   point count, leaves such rows); points that do not fit into the capacity are left out; rows outside every capacity are not touched.
 *   A source frame whose rows do not lie inside [0, total), and a target whose capacity does not lie inside [0, cap_total), is treated
 *   as empty: a bad id or offset gives wrong data, never an access outside a buffer.  total, cap_total <= INT_MAX.
 *   One workgroup per target; the chain is formed once per target by one lane, in order. */
#define CMF_ACCUM_MAX_WINDOW 64
#define CMF_ACCUM_KEEP 0
#define CMF_ACCUM_PROPAGATE 1
#define CMF_ACCUM_DROP 2
int cmf_accumulate(int nsel, int nframes, const long long *frames, const int *first, const int *off1, long long total,
                   const float *tab1, int ld_tab, const float *flow, const unsigned char *mask, const float *T, int window,
                   int mode, int gt, const int *cap_off, long long cap_total, float *xyz, int *src, unsigned char *age,
                   int *count, void *stream);

/* ---- moving-object instances of a test run (cmflow_amd/instances.py) ---------------------------------------------
 * cmf_cluster_moving: density-based clustering (DBSCAN with its one order-dependent choice pinned) of the moving cloud-1 points of
 * every selected frame, each frame on its own -- a definition, not an approximation of one.
 *   frames (nsel) int64 in device memory, ids clamped to [0, nframes-1], the same id may occur twice; NULL: frames 0 .. nsel-1.
 *   off1 / total / tab1 / ld_tab: the split's cloud-1 table (xyz at columns 0..2, label flow 6..8, mask 9; ld_tab >= 10).
 *   gt == 0: flow (total,3) and mask (total) bytes are the store's, T (nframes,16) its trans_pred; a point is a CANDIDATE iff its
 *            mask byte is 0.
 *   gt != 0: flow and mask are not read (may be NULL); the flow is tab1's columns 6..8, a point is a candidate iff tab1 column 9
 *            == 0.0f, and T is the split's trans.
 *   eps2 = (double)eps * (double)eps, w2 = (double)flow_weight * (double)flow_weight, formed by the host; min_points >= 1.
 * For a frame with n points, p_i its float32 positions, f_i the flow and T the frame's transform, a point's own-motion
 * displacement is cmf_accumulate's d, expression for expression:
 *     tp_r = ((T[r][0] px + T[r][1] py) + T[r][2] pz) + T[r][3]         d_r = ((double)p_r + (double)f_r) - tp_r
 * and for two candidates i, j, with dx.. = (double)p_i - (double)p_j and ex.. = d_i - d_j:
 *     D2(i,j) = ((dx*dx + dy*dy) + dz*dz) + w2 * ((ex*ex + ey*ey) + ez*ez)
 * All float64, every operation rounded on its own (no contraction).  w2 = 0 clusters by position alone (for finite d).
 *   Neighbours: candidates i, j with D2(i,j) <= eps2; a point is its own neighbour (a NaN distance is no neighbour, not even of itself).
 *   Core:       a candidate with at least min_points neighbours, itself included.
 *   Instances:  the connected components of the core points under the neighbour relation.
 *   Border:     a candidate that is not core but has a core neighbour; it joins the instance of the core neighbour with the smallest
 *               D2, the lowest point index among equal D2 -- the one place where textbook DBSCAN depends on the visiting order.
 *   Noise:      any other candidate.
 *   Numbering:  a frame's instances are 0 .. K-1 in ascending order of their lowest-indexed core point, the instance's seed.
 *   Statistics of an instance over its members (core and border) in ascending point index: size; centroid_r = (float)(S_r /
 *               (double)size) with S_r the float64 sum of (double)p_r in that order from 0.0; disp_r likewise from d_r; lo_r, hi_r
 *               the smallest and largest float32 coordinate (from the first member, replaced only where v < lo_r, v > hi_r); seed.
 * Outputs, packed like the cloud-1 table: label (total) int32, the instance id inside the frame or -1; kind (total) bytes,
 *   CMF_INST_NONE (no candidate), _NOISE, _BORDER, _CORE; count (nframes) int32, the K of frame f at count[f].  The instance tables share
 *   the points' row space -- instance c of frame f is row off1[f] + c, K <= n always: size, seed (total) int32, seed the frame-local
 *   point index; centroid, disp, lo, hi (total,3) float32.
 * Guarantees, as cmf_accumulate: every label, kind and table row of a selected frame is written, by the one thread that owns it (no
 *   atomics, no global scratch); table rows behind K hold size 0, seed -1 and zeros; rows of unselected frames are not touched; the
 *   same id selected twice writes the same values twice.  A frame with more than CMF_INST_MAX_POINTS points has no candidates (count
 *   0, labels -1, kind 0, empty table rows); a frame whose rows do not lie inside [0, total) owns no rows and gets count 0: a bad id or
 *   offset gives wrong data, never an access outside a buffer.  total <= INT_MAX.
 *   One workgroup per selected frame, one thread per candidate, the candidates in 52 KB of LDS; every pair distance is formed once
 *   (a thread keeps its row of the neighbour relation as bits in registers); the components are the fixed point "every core point
 *   carries the lowest core index of its component", reached by rounds that read only what the round before wrote, so the result
 *   does not depend on the schedule.  tests/instances_ref.py restates all of this in numpy, bit for bit. */
#define CMF_INST_MAX_POINTS 1024
#define CMF_INST_NONE 0
#define CMF_INST_NOISE 1
#define CMF_INST_BORDER 2
#define CMF_INST_CORE 3
int cmf_cluster_moving(int nsel, int nframes, const long long *frames, const int *off1, long long total, const float *tab1,
                       int ld_tab, const float *flow, const unsigned char *mask, const float *T, int gt, double eps2, double w2,
                       int min_points, int *label, unsigned char *kind, int *count, int *size, int *seed, float *centroid,
                       float *disp, float *lo, float *hi, void *stream);

/* ---- moving-object instances tracked across a clip's frames (cmflow_amd/tracks.py) -------------------------------
 * cmf_track_instances: the instances of cmf_cluster_moving associated from frame to frame inside every clip, by a gated greedy
 * nearest-first matching against a constant-displacement prediction -- a definition, not an approximation of one.  Frames of a clip
 * are consecutive scan pairs (the contract of cmf_pose_chain and cmf_accumulate): T_f maps static points from scan-1 coordinates
 * of frame f to its scan-2 coordinates, which are the scan-1 coordinates of frame f+1.
 *   clips (nclips,2) int32 in device memory: [first, last) frame ranges, clamped to [0, nframes] (last < first: empty).
 *   off1 (nframes+1) / total: the split's cloud-1 offsets; count (nframes), label (total) int32, centroid, disp (total,3) float32:
 *   cmf_cluster_moving's outputs -- instance c of frame f is row off1[f] + c.  T (nframes,16) float32, row-major: the transforms the
 *   instances were clustered with.  gate2 = (double)gate * (double)gate, formed by the host; 0 <= max_gap <= CMF_TRACK_MAX_GAP.
 * Rows.  With base = off1[first], a clip with base outside [0, total] owns no rows.  Its frames are visited in order with top = base
 *   at the start; frame f OWNS its rows iff top <= off1[f] <= off1[f+1] <= total, and then top = off1[f+1] (so the rows of a clip's
 *   frames are disjoint and ascend).  A frame that owns no rows has K = 0; otherwise K = count[f] clamped to [0, min(n_f, 1024)].
 * Per clip the state is the list of live tracks in ascending track id, empty at the clip's first frame; a live track carries
 *   P (3 float64), its predicted position in the current frame's scan-1 coordinates, D (3 float64), its own-motion displacement per
 *   frame, and miss, hits, last_row, the frames of its first and last match.  Everything below is float64 from the float32 entries,
 *   every multiplication and addition rounded on its own (no contraction).  At frame f, with its K instances, c_j the centroid of
 *   instance j and T = T_f:
 *   1. Cost:        for a live track and an instance j, e_r = P_r - (double)c_j,r and G2 = (e0 e0 + e1 e1) + e2 e2.  The pair is an
 *                   EDGE iff G2 <= gate2 (a NaN is no edge).
 *   2. Association: the edges in ascending (G2, track id, j); an edge MATCHES iff neither of its ends is matched yet.  This order is
 *                   the definition: it decides every tie.
 *   3. Matched:     instance j of track u gets track = u, prev_row = the track's last_row, gap = f - (the frame of that match),
 *                   age = ++hits, pred = (float)P; then P = (double)c_j, D = (double)disp_j, miss = 0, last_row = off1[f] + j.
 *   4. Births:      the unmatched instances open tracks in ascending j with the clip's next ids: prev_row -1, gap 0, age 1 (hits 1),
 *                   pred = c_j copied bit for bit; P, D, miss, last_row as in 3.
 *   5. Unmatched tracks: miss += 1, and the track dies iff miss > max_gap.  A surviving (coasting) track keeps P, and its D is
 *                   turned into the next frame's axes: D_r := (T[r][0] D_0 + T[r][1] D_1) + T[r][2] D_2.
 *   6. Capacity:    if matched tracks + coasting tracks + births exceed CMF_TRACK_MAX_LIVE, EVERY coasting track dies at this frame
 *                   and overflow[clip] += 1 (matched tracks + births = K <= 1024 always fit).
 *   7. Prediction into frame f+1, for every live track, with D as steps 3-5 left it:
 *                   P_r := (((T[r][0] P_0 + T[r][1] P_1) + T[r][2] P_2) + T[r][3]) + D_r
 *                   (disp is (p + flow) - T p, in scan-2 axes already: for a matched instance this is the mean of its points'
 *                   p + flow, up to rounding).
 *   8. The live list of frame f+1: the survivors in their old order, then the births -- ascending track id again.
 *   A frame with K = 0 (count 0, not selected when clustering, or without rows) has no instances: every track coasts.
 * Outputs in the instances' row space, (total): track, prev_row, gap, age int32, pred (total,3) float32 as above; the rows of an
 *   owned frame behind K hold track -1, prev_row -1, gap 0, age 0, pred 0.  point_track (total) int32: for point p of an owned frame,
 *   the track of instance label[p] where 0 <= label[p] < K, else -1.
 * Outputs in the clip's row space: track u of the clip is row base + u (the tracks of a clip are at most the sum of its K, at most
 *   its owned rows): birth, last int32, the global frames of its first and last match, hits int32.  The owned rows of the clip from
 *   base + ntracks on hold -1, -1, 0.  ntracks (nclips), overflow (nclips) int32.
 * Guarantees, as cmf_cluster_moving: every row of an owned frame is written, by the one thread that owns it (no atomics, no global
 *   scratch); rows outside every clip are not touched; every row written lies inside [0, total) whatever the offsets, counts, labels
 *   and clips hold: a bad argument gives wrong data (clips that overlap write the same rows more than once), never an access outside
 *   a buffer.  total <= INT_MAX.
 *   One workgroup of 1024 threads per clip, its frames in sequence; thread t owns live slot t (state in registers) and instance t.
 *   The association runs as mutual-best rounds (a track picks its best unmatched instance by (G2, j), an instance its best unmatched
 *   track by (G2, track id), pairs that pick each other match) whose fixed point is the sorted greedy matching above; a round reads
 *   only what the round before wrote, so the result does not depend on the schedule.  The launch keeps nclips CUs busy and lasts as
 *   long as its longest clip: the state is sequential.  tests/tracks_ref.py restates all of this in numpy, bit for bit. */
#define CMF_TRACK_MAX_LIVE 1024
#define CMF_TRACK_MAX_GAP 16
int cmf_track_instances(int nclips, int nframes, const int *clips, const int *off1, long long total, const int *count,
                        const int *label, const float *centroid, const float *disp, const float *T, double gate2, int max_gap,
                        int *track, int *prev_row, int *gap, int *age, float *pred, int *point_track, int *birth, int *last,
                        int *hits, int *ntracks, int *overflow, void *stream);

/* ---- per-track object states: smoothed kinematics and oriented boxes (cmflow_amd/objects.py) ----------------------
 * cmf_track_states: for every match of every track of cmf_track_instances, the track's position and velocity at that frame from a
 * fixed-interval smoother over ALL of the track's matches (a constant-velocity Kalman filter forwards, Rauch-Tung-Striebel
 * backwards), a heading from the smoothed velocity and a box oriented along it -- a definition, not an approximation of one.
 *   clips, off1, total, count, label, centroid, disp: as cmf_track_instances takes them; track, prev_row, gap (total) int32: its
 *   outputs.  tab1 / ld_tab: the split's cloud-1 table (xyz at columns 0..2; ld_tab >= 3).  poses (nframes,16) float64: the output of
 *   cmf_pose_chain on the transforms the instances were clustered with and the SAME clip ranges: A_f = poses[f] is the pose of scan
 *   2 of frame f in the clip's axes (the scan-1 axes of the clip's first frame); the pose of scan 1 of frame f is W_f = poses[f-1],
 *   and at the clip's first frame (f == first after clamping) W_f is the identity, taken as the numbers 1.0 and 0.0 through the same
 *   expressions.  Only the upper three rows of a pose are read.  rp = sigma_pos^2, rd = sigma_disp^2, q = sigma_acc^2,
 *   min_disp2 = min_disp^2, products of doubles formed by the host (rp, rd > 0; q, min_disp2 >= 0; none NaN).
 * Rows: the clamping of a clip, base, top, the frames that OWN rows and K_f are those of cmf_track_instances, word for word; row0_f =
 *   off1[f], the INSTANCE rows of frame f are row0_f .. row0_f + K_f - 1, N = last - first after clamping.
 * Everything below is float64 from the float32 / int32 entries, only + - * / and sqrt, every operation rounded on its own (no
 * contraction), in exactly the grouping written.
 *   1. Links.  For an instance row r of frame f: row_frame[r] = f, and next_row[r] = the first row r' with prev_row[r'] == r and
 *      track[r'] == track[r] among the instance rows of the frames f+1 .. min(f + CMF_TRACK_MAX_GAP + 1, last - 1) that own rows,
 *      frames ascending (top carried on from frame f), rows ascending inside a frame; -1 where there is none.  So a successor
 *      lies in a strictly later frame, no row has two predecessors that count, and no chain of links is longer than N.
 *      r is a HEAD unless p = prev_row[r] satisfies base <= p < row0_f and next_row[p] == r.  Every instance row of tables that
 *      cmf_track_instances produced lies on the chain of exactly one head: the track's matches in frame order.
 *   2. Measurements of row k at frame f, c = centroid[k], d = disp[k] (disp is in scan-2 axes, cmf_track_instances step 7):
 *        zp_r = ((W[r][0] c0 + W[r][1] c1) + W[r][2] c2) + W[r][3]   (W = W_f)
 *        zd_r = (A[r][0] d0 + A[r][1] d1) + A[r][2] d2                (A = A_f)
 *   3. Filter, along a head's chain.  The state per axis r is (p_r, v_r), v in metres per frame; the covariance (a, b, c) =
 *      (P_pp, P_pv, P_vv) is one for the three axes.  At the head: p = zp, v = zd, (a, b, c) = (rp, 0, rd).  At every later row
 *      k, with g = (double)min(max(gap[k], 1), CMF_TRACK_MAX_GAP + 1):
 *        PREDICT  pm_r = p_r + g v_r                                 (the velocity is kept)
 *                 am = (a + g ((2 b) + g c)) + (q ((g g) g)) / 3     bm = (b + g c) + (q (g g)) / 2     cm = c + q g
 *        UPDATE   (H = I, R = diag(rp, rd), the gain by the closed-form inverse of the innovation covariance)
 *                 s11 = am + rp   s12 = bm   s22 = cm + rd   det = s11 s22 - s12 s12
 *                 k11 = (am s22 - bm s12) / det   k12 = (bm s11 - am s12) / det
 *                 k21 = (bm s22 - cm s12) / det   k22 = (cm s11 - bm s12) / det
 *                 ep_r = zp_r - pm_r   ev_r = zd_r - v_r
 *                 p_r = pm_r + (k11 ep_r + k12 ev_r)   v_r = v_r + (k21 ep_r + k22 ev_r)
 *                 a = am - (k11 am + k12 bm)   b = bm - (k11 bm + k12 cm)   c = cm - (k21 bm + k22 cm)
 *      and filt[k] = (p0 p1 p2 v0 v1 v2), fcov[k] = (a b c).
 *   4. Smoother, backwards over the same chain from the filtered values alone.  At the chain's last row state = filt, scov = fcov.
 *      For a row j whose successor is k (g from gap[k] as above; (p, v, a, b, c) the FILTERED values of j, (ps, vs, as, bs, cs) the
 *      SMOOTHED values of k), the prediction is formed again by the expressions of PREDICT, then
 *        m11 = a + g b   m12 = b   m21 = b + g c   m22 = c   dm = am cm - bm bm
 *        c11 = (m11 cm - m12 bm) / dm   c12 = (m12 am - m11 bm) / dm   c21 = (m21 cm - m22 bm) / dm   c22 = (m22 am - m21 bm) / dm
 *        dp_r = ps_r - pm_r   dv_r = vs_r - v_r
 *        state[j] = (p_r + (c11 dp_r + c12 dv_r), v_r + (c21 dp_r + c22 dv_r))
 *        da = as - am   db = bs - bm   dc = cs - cm
 *        e11 = c11 da + c12 db   e12 = c11 db + c12 dc   e21 = c21 da + c22 db   e22 = c21 db + c22 dc
 *        scov[j] = (a + (e11 c11 + e12 c12), b + (e11 c21 + e12 c22), c + (e21 c21 + e22 c22))
 *   5. Back into the frame's own scan-1 axes, for every instance row with (x, v) = state[r] and W = W_f, by the rigid inverse
 *      (R^T, -R^T t) of cmf_pose_chain, whether or not R is exactly orthonormal:
 *        ti_r = -((W[0][r] W[0][3] + W[1][r] W[1][3]) + W[2][r] W[2][3])
 *        P_r = ((W[0][r] x0 + W[1][r] x1) + W[2][r] x2) + ti_r        V_r = (W[0][r] v0 + W[1][r] v1) + W[2][r] v2
 *      pos = (float)P, vel = (float)V.
 *   6. Heading.  s2 = V_0 V_0 + V_1 V_1.  If s2 >= min_disp2 and s2 > 0 (a NaN is neither): s = sqrt(s2), heading = ((float)(V_0 / s),
 *      (float)(V_1 / s)), heading_src = 1.  Otherwise heading = (1, 0), heading_src = 0: the axis-aligned box the instance has.
 *   7. Box, over the frame's member points i (label[row0_f + i] == the instance's number, i = 0 .. n_f - 1 ascending) with their
 *      float32 positions x, y, z from tab1, (hx, hy) the float32 heading AS WRITTEN taken back to float64 and c the float32 centroid:
 *        dx = (double)x - (double)c0   dy = (double)y - (double)c1   a_i = hx dx + hy dy   b_i = (-hy) dx + hx dy
 *      amin, amax, bmin, bmax by comparison from the first member (replaced only where a value is smaller, larger), lo_z, hi_z
 *      likewise over the float32 z, as the instances' lo / hi.  ma = (amin + amax) / 2, mb = (bmin + bmax) / 2 and
 *        box_size   = ((float)(amax - amin), (float)(bmax - bmin), (float)((double)hi_z - (double)lo_z))
 *        box_center = ((float)((double)c0 + (ma hx - mb hy)), (float)((double)c1 + (ma hy + mb hx)), (float)(((double)lo_z + (double)hi_z) / 2))
 *      An instance without a member point has box_size 0 and box_center = the centroid, copied.
 * Outputs, all in the instances' row space: row_frame, next_row (total) int32; filt, state (total,6), fcov, scov (total,3) float64,
 *   in the clip's axes; pos, vel, box_center, box_size (total,3), heading (total,2) float32, heading_src (total) int32, in the
 *   frame's scan-1 axes.  The rows of an owned frame behind K hold row_frame -1, next_row -1, heading_src -1 and zeros.
 * Guarantees, as cmf_track_instances: no atomics and no global scratch; every element of an owned frame's rows is written by one
 *   thread (steps 1 and 5-7 and the rows behind K by the row's own thread, steps 3-4 by the thread of the chain's head); rows
 *   outside every clip are not touched.  For tables that cmf_track_instances produced the result is fully defined and independent
 *   of the schedule.  For any other tables -- prev_row out of range or in a cycle, gap <= 0 or huge, labels, counts, offsets or
 *   clips that do not fit -- the result is wrong data, never an access outside a buffer and never an unbounded loop: a link is
 *   only ever followed to a row that step 1 found by its search, which lies in a strictly later owned frame of the clip, every
 *   walk is capped by N as well, and gap is clamped.  (An instance row whose prev_row points at a row of the clip that no frame
 *   owns may be left on no chain; its filt, state, fcov and scov are then not written.)  total <= INT_MAX.
 *   One workgroup per clip, barriers between the phases: links (one thread per instance row), chains (sequential per track,
 *   parallel over the heads), boxes (one thread per instance over its frame's labels); each phase works on sixteen frames side by
 *   side from a table of the clip's rows in LDS.  A latency kernel: it keeps nclips CUs busy and lasts as long as its longest clip.  tests/objects_ref.py restates all of this in numpy, bit for bit. */
int cmf_track_states(int nclips, int nframes, const int *clips, const int *off1, long long total, const int *count, const int *label,
                     const float *centroid, const float *disp, const int *track, const int *prev_row, const int *gap,
                     const float *tab1, int ld_tab, const double *poses, double rp, double rd, double q, double min_disp2,
                     int *row_frame, int *next_row, double *filt, double *fcov, double *state, double *scov, float *pos, float *vel,
                     float *heading, int *heading_src, float *box_center, float *box_size, void *stream);

/* ---- two sides of the analysis chain scored against each other (cmflow_amd/score.py) ------------------------------
 * cmf_score_tracks: per frame the instances of a "gt" and a "pred" side of the chain (cmf_cluster_moving .. cmf_track_instances on the
 * SAME split) matched by their point overlap, and per clip the identity walk of MOTS over the gt side's tracks -- a definition, not
 * an approximation of one.  Integers everywhere but one float64 division per candidate pair.
 *   clips, off1, total: as cmf_track_instances takes them.  iou_min in [0.5, 1).  gt_count / pred_count (nframes), gt_label /
 *   pred_label (total) int32: cmf_cluster_moving's count and label of either side (a frame a side did not select has count 0 there);
 *   gt_track / pred_track, gt_prev_row (total) int32: cmf_track_instances' track of either side and the gt side's prev_row.  The
 *   size tables are not read.
 * Rows: the clamping of a clip, base, top and the frames that OWN rows are those of cmf_track_instances, word for word; in a frame
 *   that owns its n_f rows, K_side = count_side[f] clamped to [0, min(n_f, 1024)], except that a frame of more than
 *   CMF_INST_MAX_POINTS rows has K = 0 on both sides (cmf_cluster_moving gives it no instances).  A frame that owns no rows has no
 *   instances on either side.  SOLID, the clip's gap-free rows: solid = base at the start, and a frame that owns [start, stop) with
 *   start == solid moves solid to stop.  For offsets that ascend inside the tables solid == top throughout: every row of the clip
 *   so far.  (Only a frame that owns no rows in the middle of a clip leaves rows behind solid.)
 * Per frame, over its points i = 0 .. n_f - 1:
 *   Labels.   g_i = gt_label[row0 + i] where 0 <= gt_label < K_gt, else -1; p_i likewise from the pred side.
 *   Sizes.    |G| = the points with g_i == G, |P| = those with p_i == P, c(G,P) = those with both: counted from the labels.
 *   Matching. G and P MATCH iff c > 0 and (double)c / (double)(|G| + |P| - c) > iou_min: one float64 division, a strict compare.
 *             At most one P passes for a G and one G for a P: a correctly rounded quotient is monotone and 1/2 is a float64, so a
 *             pair that passes has c / (|G| + |P| - c) > 1/2 as rationals, i.e. 3c > |G| + |P|; with c <= |P| this gives 2c > |G| --
 *             P holds more than half of G's points, and the instances of a side are disjoint, so no second P does; the same with G
 *             and P exchanged.  No assignment problem, no greedy order: the result does not depend on any order.
 *   Outputs in the instances' row space: match[row0 + P] = row0 + G or -1 and iou[row0 + P] = that quotient or 0.0, on pred rows;
 *             match_gt[row0 + G] = row0 + P or -1 on gt rows.  frame_tp[f] = the matched pairs, frame_fp[f] = K_pred - tp,
 *             frame_fn[f] = K_gt - tp; a frame of the clip that owns no rows gets 0, 0, 0.
 *   Identity, over the gt instances G = 0 .. K_gt - 1 in ascending order, t = gt_track[row0 + G]: G HAS IDENTITY iff t >= 0 and base + t
 *             < solid (solid with this frame taken in) and no lower instance of the frame carries the same t.  An instance without
 *             identity counts in tp / fp / fn and gt_total and in nothing below.  The track's row is base + t (the clip's row space,
 *             as cmf_track_instances' birth / last / hits): seen += 1; and if G matched P, with u = pred_track[row0 + P] where that is
 *             >= 0 and base + u < solid, else -1:
 *               if covered > 0 (the track was matched before):
 *                  switch[row0 + G] = last_partner != u                        -- the id switch of MOTS
 *                  frag[row0 + G]   = NOT (base <= r < row0 and r < solid and match_gt[r] >= 0), r = gt_prev_row[row0 + G]
 *                                                                            -- the track's instance directly before was not matched
 *               covered += 1, last_partner = u.
 *             switch and frag are 0 wherever this does not set them.
 *   The rows of an owned frame behind K_pred hold match -1 and iou 0, those behind K_gt match_gt -1, switch 0, frag 0; seen, covered
 *   and last_partner of a frame's rows start at 0, 0, -1 when the frame is reached.
 * Per clip (nclips): tp, fp, fn, gt_total (the sum of K_gt) int32, the sums over its frames; ids, frags int32, the sums of switch
 *   and frag; iou_units int64, the sum over the matches of (long long)floor(iou * 2^30) -- integers, exact in any order.
 * Guarantees, as cmf_track_states: no global scratch; every element of an owned frame's rows, every frame_* entry of a clip's frames
 *   and every per-clip entry is written, rows and frames outside every clip are not touched; for ANY tables the result is wrong
 *   data at worst, never an access outside a buffer and never an unbounded loop: a label indexes a table only after it is clamped to
 *   the frame's K, a track only after base + t < solid, which is a row of an owned frame of this clip at or before the current one,
 *   prev_row only after it is found inside the clip's solid rows before the frame, and every loop runs over a frame's rows or
 *   the workgroup's threads.  Clips that overlap write the same rows more than once.  total <= INT_MAX.
 *   One workgroup of 1024 threads per clip, its frames in sequence: one thread per point and per instance, the labels as packed keys
 *   in LDS, |G| and |P| by LDS integer atomics, c by a scan of the frame's keys (every lane reads the same address: a broadcast), the
 *   passing pairs published by LDS atomicMax (all points of a pair publish the same numbers); a gt track is touched by one thread
 *   per frame, and a frame reads the per-track rows the frames before wrote behind a barrier.  28 KB of LDS, no scratch.  The launch
 *   keeps nclips CUs busy and lasts as long as its longest clip.  tests/score_ref.py restates all of this in numpy, bit for bit. */
int cmf_score_tracks(int nclips, int nframes, const int *clips, const int *off1, long long total, double iou_min,
                     const int *gt_count, const int *gt_label, const int *gt_track, const int *gt_prev_row, const int *pred_count,
                     const int *pred_label, const int *pred_track, int *match, int *match_gt, double *iou, int *switches, int *frag,
                     int *frame_tp, int *frame_fp, int *frame_fn, int *seen, int *covered, int *last_partner, int *tp, int *fp,
                     int *fn, int *ids, int *frags, int *gt_total, long long *iou_units, void *stream);

/* Library / device identification: returns a static NUL-terminated string. */
const char *cmf_version(void);

#ifdef __cplusplus
}
#endif
#endif /* CMFLOW_HIP_H */
