/*
 * pdfops.h -- C ABI of libpdfops.so, the MI355X (gfx950) replacement for the reference's
 * libs/pointops CUDA extension (`pointops._C`).
 *
 * Each entry point replaces one `extern "C"` launcher of the reference (file:line cited per
 * function, paths relative to the reference root).  Signatures keep the reference's parameter
 * lists and add
 *   - `b`      : the scene count, where the reference inferred it by scanning `offset`,
 *   - `stream` : a hipStream_t passed as void* (the reference launched on the legacy stream),
 * and return an int status: 0 = ok, PDF_ERR_* (<0) = argument error, >0 = hipError_t.
 *
 * Contract (same as the reference unless noted):
 *   - all pointers are DEVICE pointers owned by the caller; the library never allocates,
 *     never synchronises and keeps NO mutable state -- no globals, no per-stream tables (re-entrant, any thread, any stream; since
 *     ABI 4 the reduced-precision mode of the Linear products is a per-call argument, `mma_input` below).  The only process-wide inputs
 *     are a few read-only PDFOPS_* environment variables that select kernel variants / grid caps for experiments and tests
 *     (PDFOPS_KNN_*, PDFOPS_PT_BLOCKS_*, PDFOPS_PT_CAP_<pass>; defaults are the measured best), read once per process, and
 *     PDFOPS_FPS_KERNEL (single | multi | mw8 | mw16: the kernel of the bucketed FPS) and PDFOPS_RL_FORM (auto | slab | group: the form
 *     of the streaming Linear kernels at K >= 128, bit-identical results), read at every launch;
 *   - float data is fp32, indices/offsets are int32, `offset` arrays hold CUMULATIVE scene ends;
 *   - kNN placeholder for scenes with fewer than `nsample` points: idx = -1, dist2 = 1e10;
 *   - outputs written by plain stores need no initialisation (grouping/subtraction/
 *     interpolation/aggregation forward, knn, fps, aggregation grad_position);
 *     outputs that are ACCUMULATED into must be pre-zeroed by the caller exactly as the
 *     reference's Python wrappers do: every grad_* scatter target and the attention_* forward outputs;
 *   - gather kernels treat idx < 0 as a zero row (the reference dereferences it: undefined).
 */
#ifndef PDFOPS_H
#define PDFOPS_H

#ifdef __cplusplus
extern "C" {
#endif

#define PDF_OK 0
#define PDF_ERR_BAD_ARG (-1)      /* null pointer / negative size */
#define PDF_ERR_NSAMPLE (-2)      /* nsample outside 1..128 (reference: best_dist[128], knn_query_cuda_kernel.cu:82) */
#define PDF_ERR_UNSUPPORTED (-3)  /* shape outside what the kernels are built for */
#define PDF_ERR_NOT_CONVERGED (-4) /* an iteration with a proven bound on its rounds ran past it (pdf_pg_cluster_labels) */

/* ABI version of THIS header.  pdf_abi_version() returns the version the loaded library was built with: a caller built against another
 * version must refuse to call (parameter lists differ; pointcloudpdf_amd/_native.py does).  History: 1 = rounds 1-3 (signatures changed
 * without a bump, see ADVICE of round 3); 4 = round 4: `mma_input` per call on the pdf_rowlin_ / pdf_block_ / pdf_bottleneck_ / pdf_linbn_ /
 * pdf_td_ entries, pdf_set_mma_input / pdf_get_mma_input / pdf_tickets_* removed, pdf_sgd_step takes a found-inf flag;
 * 5 = round 5: pdf_wa_* (atomic-free window-attention backward, fused logits), pdf_layernorm_*, pdf_region_* / *_dev (sync-free pseudo-label pass) added;
 * 7 = pdf_adam_step / pdf_adam_grad_unscale added (no existing parameter list changed);
 * 8 = pdf_fragment_bounds / pdf_fragment_gather / pdf_fragment_vote added (no existing parameter list changed);
 * 9 = pdf_radius_neighbors_self_adaptive added (no existing parameter list changed);
 * 10 = pdf_lovasz_workspace_bytes / pdf_lovasz_forward / pdf_lovasz_backward added (no existing parameter list changed);
 * 11 = pdf_openset_metrics_workspace_bytes / pdf_openset_metrics added (no existing parameter list changed);
 * 12 = pdf_scene_bounds / pdf_window_keys_scene added (no existing parameter list changed);
 * 13 = pdf_criteria_workspace_floats / pdf_ce_ex_* / pdf_focal_* / pdf_dice_* / pdf_bfocal_* added (no existing parameter list changed);
 * 14 = pdf_grid_pool_* / pdf_grid_unpool_forward / pdf_gva_* added (no existing parameter list changed);
 * 15 = pdf_cac_* added (no existing parameter list changed);
 * 16 = pdf_spconv_* added (no existing parameter list changed);
 * 17 = pdf_serial_* added (no existing parameter list changed);
 * 18 = pdf_pg_* and PDF_ERR_NOT_CONVERGED added (no existing parameter list changed);
 * 19 = pdf_transition_up_* and the two-problem entries pdf_bn_coef_from_partial2 / pdf_bn_act_backward2 / pdf_rowlin_wgrad2 added (no
 *      existing parameter list changed);
 * 20 = pdf_rowlin_forward_stats2 / pdf_rowlin_dgrad2 / pdf_rowlin_wgrad2_paired added (no existing parameter list changed);
 * 21 = pdf_msc_* added (no existing parameter list changed);
 * 22 = pdf_rowlin_wgrad_group_dgrad / pdf_rowlin_wgrad2_roww added; pdf_td_fwd_scratch_floats is the SUM of its two workspaces, which pdf_td_forward now uses side
 *      by side (no existing parameter list changed). */
#define PDF_ABI_VERSION 22
int pdf_abi_version(void);
const char *pdf_build_info(void);
/* Arithmetic of the squared distance in this library's geometry kernels (kNN, ball query, FPS): 0 = the reference's expression as
 * written in IEEE fp32 (libpdfops.so), 1 = fmaf(dz,dz,fmaf(dy,dy,dx*dx)), 2 = fmaf(dz,dz,fmaf(dx,dx,dy*dy)) (libpdfops_fma{1,2}.so:
 * the contractions an `nvcc -O2` build of knn_query_cuda_kernel.cu:92 / sampling_cuda_kernel.cu:54 may compute; csrc/pdfops_common.h). */
int pdf_dist_fma_mode(void);
/* `mma_input` (argument of every entry that runs the streaming per-point Linear products): the reduced-precision variant the reference
 * trains this path with (torch.cuda.amp.autocast: configs/s3dis/openseg-pt-v1-0-msp.py:6, pointcept/engines/train.py:340-363).
 * 0: fp32 operands, v_mfma_f32_16x16x4_f32 -- the parity path; 1: the operands of the products (forward, input gradient, weight gradient;
 * channel widths 32..512) are rounded to fp16 in registers and multiplied with v_mfma_f32_16x16x16_f16; 2: the same with bfloat16.
 * Tensors stay fp32 in memory and every accumulation is fp32 in all modes (what autocast does to nn.Linear, minus the rounding of the
 * OUTPUT to half).  Shapes the streaming kernels do not cover run in fp32 whatever the mode.  Any other value: PDF_ERR_BAD_ARG. */
#define PDF_MMA_F32 0
#define PDF_MMA_F16 1
#define PDF_MMA_BF16 2

/* replaces knn_query_cuda_launcher, libs/pointops/src/knn_query/knn_query_cuda_kernel.h:13
 * (kernel knn_query_cuda_kernel.cu:60-104).  idx (m,nsample), dist2 (m,nsample) = SQUARED distances. */
int pdf_knn_query(int m, int nsample, const float *xyz, const float *new_xyz,
                  const int *offset, const int *new_offset, int b,
                  int *idx, float *dist2, void *stream);

/* Same results through a uniform grid (exact: queries whose answer could depend on the reference's tie-breaking
 * are re-run by the scan kernel).  n = number of source points, workspace from pdf_knn_workspace_bytes(b, n, m). */
long pdf_knn_workspace_bytes(int b, int n, int m);
int pdf_knn_grid_supported(int nsample);
int pdf_knn_query_ws(int m, int nsample, int n, const float *xyz, const float *new_xyz, const int *offset,
                     const int *new_offset, int b, int *idx, float *dist2, void *workspace, long workspace_bytes,
                     void *stream);
/* The two halves of pdf_knn_query_ws on their own: one grid per set of SOURCE points (pdf_knn_grid_build), any number of query sets and
 * nsample values (3 / 8 / 16) over it (pdf_knn_query_grid).  workspace_bytes >= pdf_knn_workspace_bytes(b, n, m) for the largest m. */
int pdf_knn_grid_build(int n, const float *xyz, const int *offset, int b, void *workspace, long workspace_bytes, void *stream);
int pdf_knn_query_grid(int m, int nsample, int n, const float *xyz, const float *new_xyz, const int *offset, const int *new_offset, int b,
                       int *idx, float *dist2, void *workspace, long workspace_bytes, void *stream);
/* measurement aid: the same with the grid kernel counting the candidate distances it evaluates (*pairs, device counter zeroed by the
 * caller, += count).  The grid prunes by design, so "pairs per second" of this path must be quoted on EVALUATED pairs, not on the
 * m * n_scene pairs of the brute force it replaces. */
int pdf_knn_query_ws_counted(int m, int nsample, int n, const float *xyz, const float *new_xyz, const int *offset,
                             const int *new_offset, int b, int *idx, float *dist2, void *workspace, long workspace_bytes,
                             unsigned long long *pairs, void *stream);
/* the exact scan restricted to qlist[0 .. *qcount) (device pointers); qlist == NULL: all m queries */
int pdf_knn_query_list(int m, int nsample, const float *xyz, const float *new_xyz, const int *offset,
                       const int *new_offset, int b, int *idx, float *dist2, const int *qlist, const int *qcount,
                       void *stream);

/* replaces ball_query_cuda_launcher, libs/pointops/src/ball_query/ball_query_cuda_kernel.h:9-17 (kernel
 * ball_query_cuda_kernel.cu:58-123): points with d2 <= 1e-5 or min_radius^2 <= d2 < max_radius^2, collected in index
 * order, permuted by the reference's heap_sort, then the first candidates (<= nsample, padded with idx -1 / dist2 1e10) or
 * every (count / nsample)-th one (dist2 then holds the candidate INDEX as float, as upstream :120).  The reference's
 * per-thread list holds 2048 candidates and overruns beyond; here the first 2048 accepted points are kept.
 * nsample <= 2048, min_radius < max_radius. */
int pdf_ball_query(int m, int nsample, float min_radius, float max_radius, const float *xyz, const float *new_xyz,
                   const int *offset, const int *new_offset, int b, int *idx, float *dist2, void *stream);

/* replaces random_ball_query_cuda_launcher, libs/pointops/src/random_ball_query/random_ball_query_cuda_kernel.h:9-17
 * (kernel random_ball_query_cuda_kernel.cu:58-108): the first nsample accepted points along the caller's per-scene
 * permutation `order` (n ints, global row ids), padded with idx -1 / dist2 1e10. */
int pdf_random_ball_query(int m, int nsample, float min_radius, float max_radius, const int *order, const float *xyz,
                          const float *new_xyz, const int *offset, const int *new_offset, int b, int *idx, float *dist2,
                          void *stream);

/* replaces farthest_point_sampling_cuda_launcher, libs/pointops/src/sampling/sampling_cuda_kernel.h:13
 * (kernel sampling_cuda_kernel.cu:14-129).  `n` = size of the largest scene (fixes the reference's
 * block size opt_n_threads(n), cuda_utils.h:11-14, which fixes its arg-max tie rule).
 * `tmp` (N floats) is scratch and need NOT be pre-filled (the reference wants 1e10). */
int pdf_farthest_point_sampling(int b, int n, const float *xyz, const int *offset,
                                const int *new_offset, float *tmp, int *idx, void *stream);

/* log2 of the block size the reference would launch for a largest-scene size n (cuda_utils.h:11-14) */
int pdf_fps_reference_block_log2(int n);

/* Bucketed exact FPS (same results as pdf_farthest_point_sampling, far fewer point updates).
 * Host-side sizes: n_total = offset[b-1].  Workspace from pdf_fps_workspace_bytes(). */
long pdf_fps_workspace_bytes(int b, int n_total);
long pdf_fps_stats_offset(int b, int n_total); /* 4 x u32 per scene: bucket updates, super visits, samples, buckets */
int pdf_farthest_point_sampling_bucketed(int b, int n, int n_total, const float *xyz, const int *offset,
                                         const int *new_offset, void *workspace, long workspace_bytes,
                                         int *idx, void *stream);

/* replaces grouping_{forward,backward}_cuda_launcher, libs/pointops/src/grouping/grouping_cuda_kernel.h:14-15 */
int pdf_grouping_forward(int m, int nsample, int c, const float *input, const int *idx, float *output, void *stream);
int pdf_grouping_backward(int m, int nsample, int c, const float *grad_output, const int *idx, float *grad_input, void *stream);
/* The forward gathers with an optional VISITING ORDER of the queries (`order`: a permutation of 0 .. m-1, e.g. the Morton order of the
 * query points that the geometry pre-pass keeps per level; NULL = storage order): identical outputs.  Neighbouring queries share most
 * of their rows, and the kernels give every XCD one contiguous stretch of the order, so the repeats hit that XCD's L2 instead of
 * crossing the fabric (csrc/gather_ops.hip: grouping2 forward 51 % -> 69 % of the HBM peak).  The reference-ABI entries above are
 * these with order = NULL. */
int pdf_grouping_forward_ordered(int m, int nsample, int c, const float *input, const int *idx, const int *order, float *output, void *stream);
int pdf_group_forward_ordered(int m, int nsample, int c, int with_xyz, const float *feat, const float *xyz, const float *new_xyz,
                              const int *idx, const int *order, float *output, void *stream);
int pdf_interpolation_forward_ordered(int n, int c, int k, const float *input, const int *idx, const float *weight, const int *order,
                                      float *output, void *stream);
int pdf_subtraction_forward_ordered(int n, int nsample, int c, const float *input1, const float *input2, const int *idx, const int *order,
                                    float *output, void *stream);
int pdf_aggregation_forward_ordered(int n, int nsample, int c, int w_c, const float *input, const float *position, const float *weight,
                                    const int *idx, const int *order, float *output, void *stream);

/* replaces interpolation_{forward,backward}_cuda_launcher, libs/pointops/src/interpolation/interpolation_cuda_kernel.h:14-15 */
int pdf_interpolation_forward(int n, int c, int k, const float *input, const int *idx, const float *weight, float *output, void *stream);
int pdf_interpolation_backward(int n, int c, int k, const float *grad_output, const int *idx, const float *weight, float *grad_input, void *stream);

/* replaces subtraction_{forward,backward}_cuda_launcher, libs/pointops/src/subtraction/subtraction_cuda_kernel.h:14-15 */
int pdf_subtraction_forward(int n, int nsample, int c, const float *input1, const float *input2, const int *idx, float *output, void *stream);
int pdf_subtraction_backward(int n, int nsample, int c, const int *idx, const float *grad_output, float *grad_input1, float *grad_input2, void *stream);

/* replaces aggregation_{forward,backward}_cuda_launcher, libs/pointops/src/aggregation/aggregation_cuda_kernel.h:14-15 */
int pdf_aggregation_forward(int n, int nsample, int c, int w_c, const float *input, const float *position,
                            const float *weight, const int *idx, float *output, void *stream);
int pdf_aggregation_backward(int n, int nsample, int c, int w_c, const float *input, const float *position,
                             const float *weight, const int *idx, const float *grad_output,
                             float *grad_input, float *grad_position, float *grad_weight, void *stream);

/* replace attention_{relation,fusion}_step_{forward,backward}_cuda_launcher,
 * libs/pointops/src/attention/attention_cuda_kernel.h:31-53 */
int pdf_attention_relation_step_forward(int m, int g, int c, const float *query, const float *key, const float *weight,
                                        const int *index_target, const int *index_refer, float *output, void *stream);
int pdf_attention_relation_step_backward(int m, int g, int c, const float *query, float *grad_query,
                                         const float *key, float *grad_key, const float *weight, float *grad_weight,
                                         const int *index_target, const int *index_refer, const float *grad_output, void *stream);
int pdf_attention_fusion_step_forward(int m, int g, int c, const float *weight, const float *value,
                                      const int *index_target, const int *index_refer, float *output, void *stream);
int pdf_attention_fusion_step_backward(int m, int g, int c, const float *weight, float *grad_weight,
                                       const float *value, float *grad_value,
                                       const int *index_target, const int *index_refer, const float *grad_output, void *stream);

/* ---- fused entry points of our own (no reference launcher; they fuse the reference's Python-side
 *      compositions so the (m,nsample,c) temporaries never reach HBM) ---- */

/* pointops.grouping(idx, feat, xyz, new_xyz, with_xyz) -- libs/pointops/functions/grouping.py:36-60.
 * output (m, nsample, 3*with_xyz + c): [ (xyz[idx]-new_xyz) masked by idx>=0 | feat[idx] ], idx<0 -> zeros. */
int pdf_group_forward(int m, int nsample, int c, int with_xyz, const float *feat, const float *xyz,
                      const float *new_xyz, const int *idx, float *output, void *stream);
/* gradient w.r.t. feat only (xyz carries no gradient on this path); grad_feat (n,c) pre-zeroed. */
int pdf_group_backward(int m, int nsample, int c, int with_xyz, const float *grad_output, const int *idx,
                       float *grad_feat, void *stream);

/* inverse-distance weights of pointops.interpolation -- libs/pointops/functions/interpolation.py:14-17:
 * weight[n,j] = (1/(sqrt(dist2[n,j])+1e-8)) / sum_j(...) */
int pdf_interpolation_weights(int n, int k, const float *dist2, float *weight, void *stream);

/* Fused PointTransformerLayer (point_transformer_seg.py:45-78 incl. the three BatchNorm-as-LayerNorm norms,
 * pointcept/models/point_transformer/utils.py:7-14), forward.  Supported: nsample in {8,16}, c in {32,64,128}
 * (pdf_pt_layer_supported).  weights[8] = Wp1,bp1,Wp2,bp2,Ww1,bw1,Ww2,bw2 (host array of device pointers);
 * bn_params[6] = gamma/beta of linear_p[1], linear_w[0], linear_w[3]; bn_buffers[6] = their running mean/var
 * (updated in place when training).  bn (2*(3+c+c/8) floats) receives the scale/shift of the three norms,
 * saved (same size) their batch mean / rstd (training), H (n*nsample*c/8) the pre-norm attention hidden,
 * partial = pdf_pt_layer_partial_floats(...) floats of scratch, out (n,c). */
int pdf_pt_layer_supported(int nsample, int c);
long pdf_pt_layer_partial_floats(int n, int nsample, int c);
int pdf_pt_layer_forward(int n, int nsample, int c, const float *xq, const float *xk, const float *xv,
                         const float *p, const int *idx, const float *const *weights,
                         const float *const *bn_params, float *const *bn_buffers, int training, float eps,
                         float momentum, float *bn, float *saved, float *H, float *partial, float *out,
                         int storage_bf16, const int *order, void *stream);
/* The same with the batch's relative-coordinate sums (pdf_knn_rel_moments, summed over the batch's scenes: 9 doubles in device
 * memory) or NULL: in train mode the geometry branch's BatchNorm then comes from them (5 launches per layer instead of 7).
 * out_stat_rows (host int, may be NULL): when given, the last pass also leaves *out_stat_rows partial rows [sum out (c) | sum out^2 (c)]
 * in `partial` (train mode; 0 in eval mode) -- the statistics of a BatchNorm that reads `out` (the Bottleneck's bn2,
 * point_transformer_seg.py:187) for pdf_bn_coef_from_partial, instead of a statistics pass over `out`. */
int pdf_pt_layer_forward_m(int n, int nsample, int c, const float *xq, const float *xk, const float *xv,
                           const float *p, const int *idx, const float *const *weights,
                           const float *const *bn_params, float *const *bn_buffers, int training, float eps,
                           float momentum, float *bn, float *saved, float *H, float *partial, float *out,
                           int storage_bf16, const int *order, const double *moments, int *out_stat_rows, void *stream);

/* Backward of the fused PointTransformerLayer (train mode).  gxq / gxk / gxv are overwritten: the scatters of g_xk and g_xv run as
 * segmented gathers over the INVERSE of the kNN table (inv_off (n+1), inv_entry, entry_base -- see pdf_seg_sum_rows), so they are
 * deterministic and atomics-free; Wsm (n*nsample*c/8) and GR (n*nsample*c) are scratch (softmax weights, g_r rows).  sums needs
 * pdf_pt_layer_bwd_sums_floats(c) + 2*(3+c+c/8) floats and returns the parameter-gradient sections documented in
 * csrc/fused_layer.hip.  storage_bf16 (forward AND backward of a layer must agree): the row arrays only the layer itself reads --
 * H (saved), G2 / Wsm / GR (scratch) -- hold bfloat16 (round-to-nearest-even) in the first half of the same buffers; every sum and
 * product stays fp32.  The reduced-precision variant behind `bench.py --storage bf16` (the reference trains under AMP). */
long pdf_pt_layer_bwd_partial_floats(int n, int nsample, int c);
long pdf_pt_layer_bwd_sums_floats(int c);
int pdf_pt_layer_backward(int n, int nsample, int c, const float *xq, const float *xk, const float *xv,
                          const float *p, const int *idx, const float *const *weights, const float *bn,
                          const float *saved, const float *H, const float *gout, float *gxq, float *gxk,
                          float *gxv, float *G2, float *G3, float *Wsm, float *GR, const int *inv_off, const int *inv_entry,
                          int entry_base, float *partial, float *sums, int storage_bf16, const int *order, const double *moments,
                          void *stream);   /* moments: the batch's relative-coordinate sums (pdf_knn_rel_moments) or NULL: with them d Wp1 / d bp1 come in
                                              closed form from the sums of the third pass (no fourth pass over the rows) */

/* BatchNorm1d over (n, c) rows fused with the residual add and ReLU that follow it in the Bottleneck
 * (point_transformer_seg.py:184-192).  c must be a power of two in 4..1024.  coef (4c floats) = scale|shift|mean|rstd,
 * partial = pdf_bn_partial_floats(n, c) floats of scratch; backward: sums (2c) receives [d beta | d gamma]. */
int pdf_bn_supported(int c);
long pdf_bn_partial_floats(long n, int c);
int pdf_bn_act_forward(long n, int c, const float *x, const float *res, const float *gamma, const float *beta,
                       float *running_mean, float *running_var, int training, float eps, float momentum, int relu,
                       float *coef, float *partial, float *y, void *stream);
int pdf_bn_act_backward(long n, int c, const float *gy, const float *x, const float *res, const float *coef,
                        int training, int relu, float *partial, float *sums, float *gx, float *gres, void *stream);
/* coefficients only (statistics pass + finalize, or running statistics) */
int pdf_bn_coef(long n, int c, const float *x, const float *gamma, const float *beta, float *running_mean,
                float *running_var, int training, float eps, float momentum, float *coef, float *partial, void *stream);
/* y = relu?(x * scale + shift + res) with coefficients computed elsewhere (no statistics pass) */
int pdf_bn_apply(long n, int c, const float *x, const float *res, const float *coef, int relu, float *y, void *stream);

/* Dense per-point Linear on the fp32 matrix cores (csrc/rowlin.hip).  y (+)= f(x) Wt + bias with f = identity or the
 * folded BatchNorm-affine (+ReLU) of the producer (scale/shift over the k input channels); partial (optional,
 * pdf_rowlin_partial_floats) receives per-row-block column sums / sums of squares of y for the BatchNorm that follows.
 * transpose_w = 1 computes the input gradient dX = G W with the layer's (out, in) weight. */
long pdf_rowlin_partial_floats(long n, int o);
int pdf_rowlin_partial_rows(long n, int k, int o);
int pdf_rowlin_forward(long n, int k, int o, const float *x, long ldx, const float *w, int transpose_w,
                       const float *bias, const float *scale, const float *shift, int relu, float *y, long ldy,
                       int accumulate, float *partial, int mma_input, void *stream);
/* dW (o,k) = G^T f(X), db (o) = column sums of G (db may be NULL): both WRITTEN.  No float atomics: every workgroup stores its
 * partial block into a slab of ws (pdf_rowlin_wgrad_ws_floats(n, k, o, ng) floats, ng = 1 here), a second launch sums the slabs in a
 * fixed order -- bit-reproducible gradients (the reference's atomicAdd scatters are not: grouping_cuda_kernel.cu:16-25). */
long pdf_rowlin_wgrad_ws_floats(long n, int k, int o, int ng);
int pdf_rowlin_wgrad(long n, int k, int o, const float *g, long ldg, const float *x, long ldx,
                     const float *scale, const float *shift, int relu, float *dw, float *db, float *ws, int mma_input, void *stream);
/* BatchNorm coefficients from column partials [rows][2c] (sum | sum of squares): coef = scale|shift|mean|rstd */
int pdf_bn_coef_from_partial(const float *partial, int rows, long n, int c, const float *gamma, const float *beta,
                             float *running_mean, float *running_var, float eps, float momentum, float *coef, void *stream);

/* Several Linear layers over the same rows in one launch: nin = 1, nout <= 3 (y[i] = f(x[0]) Wt[i] + bias[i]: the q/k/v
 * projections, point_transformer_seg.py:47-49) or nin <= 3, nout = 1 (y[0] (+)= sum_i x[i] Wt[i]: their input gradient);
 * pdf_rowlin_wgrad_multi: weight / bias gradients of up to three layers sharing the input x. */
int pdf_rowlin_multi(long n, int k, int o, int nin, int nout, const float *const *x, long ldx, const float *const *w,
                     int transpose_w, const float *const *bias, const float *scale, const float *shift, int relu,
                     float *const *y, long ldy, int accumulate, int mma_input, void *stream);
int pdf_rowlin_wgrad_multi(long n, int k, int o, int ng, const float *const *g, long ldg, const float *x, long ldx,
                           const float *scale, const float *shift, int relu, float *const *dw, float *const *db, float *ws, int mma_input, void *stream);
/* Up to five weight gradients of ONE shape (n, k, o) with their OWN inputs in one launch + one slab reduction -- the five c x c products
 * of a Bottleneck backward (linear3, q / k / v, linear1; point_transformer_seg.py:184-192): dW_i = G_i^T f_i(X_i), f_i = relu_i?(x *
 * scale_i + shift_i) where scale_i is non-null, else the identity; db_i (nullable, db itself may be null) = column sums of G_i.  Written,
 * not accumulated.  Streaming shapes only (k, o multiples of 32 up to 512): PDF_ERR_UNSUPPORTED otherwise.
 * ws: pdf_rowlin_wgrad_ws_floats(n, k, o, ng) floats. */
int pdf_rowlin_wgrad_group(long n, int k, int o, int ng, const float *const *g, long ldg, const float *const *x, long ldx,
                           const float *const *scale, const float *const *shift, const int *relu, float *const *dw,
                           float *const *db, float *ws, int mma_input, void *stream);
/* pdf_rowlin_wgrad_group and the independent input gradient gx (n, k) (+)= dy (n, o) W (W (o, k) row-major, i.e. pdf_rowlin_forward with
 * transpose_w = 1) over the same rows -- a Bottleneck's five weight gradients beside its gx += dy W1: ONE launch for both + the slab
 * reduction at the model's widths (k = o in {32, 64} in the slab form, {128, 256, 512} up to 16,384 rows in the group form), the
 * product's launch followed by pdf_rowlin_wgrad_group otherwise (other shapes or forms, mma_input != 0, PDFOPS_PAIR=0 in the
 * environment) -- the same bits.  gx must overlap neither an input of the gradients nor ws.  `paired` (nullable) receives 1 when the
 * product went out in the gradients' launch, 0 when on its own.  PDF_ERR_UNSUPPORTED as pdf_rowlin_wgrad_group: the product has been
 * issued then, the gradients have not. */
int pdf_rowlin_wgrad_group_dgrad(long n, int k, int o, int ng, const float *const *g, long ldg, const float *const *x, long ldx,
                                 const float *const *scale, const float *const *shift, const int *relu, float *const *dw,
                                 float *const *db, float *ws, const float *dy, const float *w, float *gx, int accumulate,
                                 int *paired, int mma_input, void *stream);

/* Rigid KPConv of the StratifiedTransformer stem (stratified_transformer_v1m1_origin.py:582-662 over torch_points3d's KPConvLayer): the
 * part that is not a matrix product.  weighted[n, k, c] = sum_m max(0, 1 - |support[nb[n, m]] - query[n] - k_points[k]| / extent) *
 * x[nb[n, m], c] (overwritten; nb = -1: no neighbour); out = weighted (N, KP * C_in) times weight (KP * C_in, C_out) is a pdf_rowlin_forward.
 * pdf_kpconv_scatter is its adjoint: grad_x[nb[n, m], c] += sum_k w grad_weighted[n, k, c] (grad_x zeroed by the caller; float atomics).
 * KP <= 16, C_in <= 16 (pdf_kpconv_supported), else PDF_ERR_UNSUPPORTED. */
int pdf_kpconv_supported(int kp, int cin);
int pdf_kpconv_gather(int n, int m, int kp, int cin, const float *query, const float *support, const int *neighbors, const float *x,
                      const float *k_points, float extent, float *weighted, void *stream);
int pdf_kpconv_scatter(int n, int m, int kp, int cin, const float *query, const float *support, const int *neighbors,
                       const float *grad_weighted, const float *k_points, float extent, float *grad_x, void *stream);
/* Input gradient y = sum_i x[i] W[i] (nin <= 3; W (k, o) = the layers' own (out, in) weights) of Linear layers reading a
 * BatchNorm(+ReLU) output bx -> bn -> relu, with that BatchNorm's backward sums as the product's epilogue: partial
 * (pdf_rowlin_partial_floats(n, o)) receives *partial_rows rows of [sum g' | sum g' xhat]; pdf_bn_act_backward_presummed then
 * finishes the BatchNorm backward without re-reading y and bx for the reduction.  PDF_ERR_UNSUPPORTED outside the streaming
 * shapes (callers then use pdf_rowlin_multi + pdf_bn_act_backward). */
int pdf_rowlin_dgrad_bstats(long n, int k, int o, int nin, const float *const *x, long ldx, const float *const *w, float *y, long ldy,
                            const float *bx, long ldb, const float *bcoef, int brelu, float *partial, int *partial_rows,
                            int mma_input, void *stream);
/* pdf_rowlin_forward + the coefficients (scale | shift | mean | rstd) of the train-mode BatchNorm behind it (column sums in the
 * product's epilogue + one finalizer launch). */
int pdf_rowlin_forward_bn(long n, int k, int o, const float *x, long ldx, const float *w, const float *bias, const float *scale,
                          const float *shift, int relu, float *y, long ldy, float *partial, const float *gamma, const float *beta,
                          float *running_mean, float *running_var, float eps, float momentum, float *coef, int mma_input, void *stream);
int pdf_bn_act_backward_presummed(long n, int c, const float *gy, const float *x, const float *coef, int training, int relu,
                                  const float *partial, int partial_rows, float *sums, float *gx, void *stream);

/* Dense halves of the Bottleneck (point_transformer_seg.py:184-192) as single host calls (csrc/block.hip documents the
 * pointer tables p[]): pre = linear1 + bn1 + ReLU + q/k/v projections, post = bn2 + ReLU + linear3 + bn3 + residual + ReLU. */
int pdf_bn_coef_eval_or_partial(const float *partial, int rows, long n, int c, const float *gamma, const float *beta,
                                float *running_mean, float *running_var, int training, float eps, float momentum,
                                float *coef, void *stream);
int pdf_block_pre_forward(long n, int c, void *const *p, int training, float eps, float momentum, int mma_input, void *stream);
int pdf_block_pre_backward(long n, int c, void *const *p, int training, int mma_input, void *stream);
int pdf_block_post_forward(long n, int c, void *const *p, int training, float eps, float momentum, int mma_input, void *stream);
int pdf_block_post_backward(long n, int c, void *const *p, int training, int mma_input, void *stream);
/* The whole Bottleneck (both halves + the fused attention layer) as one call per direction; tables in csrc/block.hip. */
int pdf_bottleneck_forward(long n, int nsample, int c, void *const *p, int training, float eps, float momentum, int storage_bf16, int mma_input, void *stream);
int pdf_bottleneck_backward(long n, int nsample, int c, void *const *p, int training, int entry_base, int storage_bf16, int mma_input, void *stream);
/* Linear (+ bias) -> BatchNorm1d -> (ReLU) as one call per direction (TransitionUp, heads); tables in csrc/block.hip. */
int pdf_linbn_forward(long n, int k, int o, void *const *p, int training, int relu, float eps, float momentum, int mma_input, void *stream);
int pdf_linbn_backward(long n, int k, int o, void *const *p, int training, int relu, int mma_input, void *stream);
/* The two-input TransitionUp, relu(bn1(x1 W1^T + b1)) + interpolation(relu(bn2(x2 W2^T + b2))) over (n1, 3) tables, as one call per direction:
 * 3 launches forward, 7 backward; train mode only; the same bits as two pdf_linbn_* calls + interpolation + add (tables in csrc/block.hip).
 * Arguments are validated before the first launch: PDF_ERR_BAD_ARG for null pointers / n < 1, PDF_ERR_UNSUPPORTED for widths outside
 * pdf_transition_up_supported (k1, k2 in {32, 64, 128, 256, 512}, o % 32 == 0, pdf_bn_supported(o)), eval mode or misaligned tensors. */
int pdf_transition_up_supported(int k1, int k2, int o);
int pdf_transition_up_forward(long n1, int k1, long n2, int k2, int o, void *const *p, int training, float eps, float momentum, int mma_input,
                              void *stream);
int pdf_transition_up_backward(long n1, int k1, long n2, int k2, int o, void *const *p, int entry_base, int mma_input, void *stream);
/* Two independent problems per launch (the building blocks of pdf_transition_up_*; tables in csrc/pointwise.hip, csrc/rowlin.hip): the
 * BatchNorm finalize of two norms, the BatchNorm(+ReLU) backward of two norms (3 launches), two weight gradients as ONE product launch
 * (equal vector widths; PDFOPS_PAIR=0: one each) with ONE slab reduction.
 * Each problem keeps the grid of its single call, so the results are the bits of two single calls. */
int pdf_bn_coef_from_partial2(int rows0, long n0, int c0, int rows1, long n1, int c1, void *const *p, float eps, float momentum, void *stream);
int pdf_bn_act_backward2(long n0, int c0, long n1, int c1, void *const *p, int relu, void *stream);
int pdf_rowlin_wgrad2(long n0, int k0, int o0, long n1, int k1, int o1, void *const *p, int mma_input, void *stream);
/* Two Linear layers of one output width o with the statistics epilogue, y_i (n_i, o) = x_i (n_i, k_i) W_i^T + b_i and the rows of
 * pdf_rowlin_forward's `partial`: one launch for the width pairs (k_0, k_1) = (32, 64), (64, 128), (128, 256), (256, 512), (512, 512), two
 * otherwise (other widths or forms, mma_input != 0, PDFOPS_PAIR=0 in the environment) -- the bits of two pdf_rowlin_forward calls.  `paired`
 * (nullable; also of the two entries below) receives 1 when the two products went out as one launch, 0 when as two.
 * p[5 i + ..]: x, W (o, k_i), bias or null, y (written), partial (pdf_rowlin_partial_floats(n_i, o) floats, written). */
int pdf_rowlin_forward_stats2(long n0, int k0, long n1, int k1, int o, void *const *p, int *paired, int mma_input, void *stream);
/* Two input gradients gx_i (n_i, k_i) = g_i (n_i, o) W_i of Linear layers that share the output width o: one launch where both products run
 * the same streaming kernel, two otherwise (and with PDFOPS_PAIR=0 in the environment) -- the bits of two pdf_rowlin_forward calls with
 * transpose_w = 1.  p[3 i + ..]: g, W (o, k_i), gx (written; null: not computed). */
int pdf_rowlin_dgrad2(long n0, int k0, long n1, int k1, int o, void *const *p, int *paired, int mma_input, void *stream);
/* pdf_rowlin_wgrad2 with the same report. */
int pdf_rowlin_wgrad2_paired(long n0, int k0, int o0, long n1, int k1, int o1, void *const *p, int *paired, int mma_input, void *stream);
/* The same with a per-row weight on problem 0's gradient rows, dW_0 = sum_n roww[n] g_0[n]^T x_0[n] (element stride rws; problem 1 of vector
 * width 2, i.e. o_1 = 32: the two Gram products of pdf_td_forward): one product launch, one each with PDFOPS_PAIR=0 or mma_input != 0. */
int pdf_rowlin_wgrad2_roww(long n0, int k0, int o0, long n1, int k1, int o1, void *const *p, const float *roww, long rws, int *paired,
                           int mma_input, void *stream);

/* Row-weighted variants of the streaming Linear kernels and the bare BatchNorm-backward sums (building blocks of pdf_td_*). */
int pdf_rowlin_forward_roww(long n, int k, int o, const float *x, long ldx, const float *w, int transpose_w, float *y, long ldy,
                            int accumulate, const float *roww, long rws, int mma_input, void *stream);
int pdf_rowlin_wgrad_roww(long n, int k, int o, const float *g, long ldg, const float *x, long ldx, float *dw, const float *roww,
                          long rws, float *ws, int mma_input, void *stream);
int pdf_bn_bwd_sums(long n, int c, const float *gy, const float *x, const float *coef, int relu, float *partial, float *sums,
                    void *stream);

/* Fused TransitionDown with stride (point_transformer_seg.py:96-119): grouping with relative coordinates + Linear(3+cin, cout) +
 * train/eval BatchNorm + ReLU + max over the 16 neighbours, forward and backward, without the (m, 16, .) intermediates.
 * Geometry-only inputs (memoised per Geometry): idx (m,16), rel4 (m,16,4) masked relative coordinates, Z (n,32) = [sum of the
 * relative coordinates of the rows gathering point j (3) | their count | 0...], consts (16) = [sum rel^T rel (9) | sum rel (3)].
 * Pointer tables: csrc/transition_down.hip. */
int pdf_td_supported(int nsample, int cin, int cout);
int pdf_td_tables(long m, int b, const float *p_src, const float *p_new, const int *idx, const int *new_offset, float *rel4, float *Z,
                  float *scene_sums, long n, const int *inv_off, const int *inv_entry, int entry_base,
                  void *stream);   /* Z (n,32) and scene_sums (b,16) zeroed by the caller; inv_* = the inverse of idx (or NULL: float atomics) */
long pdf_td_gram_floats(int cin);
long pdf_td_fwd_scratch_floats(long n, int cin);
long pdf_td_bwd_scratch_floats(long m, int cin, int cout);
int pdf_td_forward(long n, long m, int cin, int cout, void *const *p, int training, float eps, float momentum, int mma_input, void *stream);
int pdf_td_backward(long n, long m, int cin, int cout, void *const *p, int entry_base, int mma_input, void *stream);

/* ---- scatter-adds as segmented gathers over an inverse neighbour table (csrc/seg_gather.hip; no reference counterpart: the reference
 * scatters with atomicAdd -- grouping_cuda_kernel.cu:20-25, interpolation_cuda_kernel.cu:27-33, subtraction_cuda_kernel.cu:24-30,
 * aggregation_cuda_kernel.cu:30-39).  For a table idx (m, nsample) over n rows: inv_off (n + 1) ascending positions into inv_entry;
 * inv_entry holds entry ids e + entry_base (e = i * nsample + j) grouped by destination idx[e], ascending inside a destination
 * (fixed summation order); entries with idx < 0 lie outside every segment.  pdf_subtraction_backward / pdf_aggregation_backward
 * accept a NULL scatter target (grad_input2 / grad_input) when the caller forms it with these. */
int pdf_seg_sum_rows(long n, int c, const float *src, const int *inv_off, const int *inv_entry, int entry_base, float scale, float *out,
                     void *stream);
/* self tables: inverse-segment sums (scaled) and every point's own-row sums of src (n * nsample, c) in one walk (subtraction backward) */
int pdf_seg_sum_rows_own(long n, int c, int nsample, const float *src, const int *inv_off, const int *inv_entry, int entry_base, float scale,
                         const int *order, float *out, float *out_own, void *stream);
int pdf_seg_sum_rows_strided(long n, int c, const float *src, long src_stride, const int *inv_off, const int *inv_entry, int entry_base,
                             float scale, float *out, void *stream);
int pdf_seg_sum_rows_x(long n, int c, const float *src, long src_stride, int src_bf16, const int *inv_off, const int *inv_entry, int entry_base,
                       float scale, float *out, void *stream);     /* src rows fp32 or bfloat16 */
int pdf_seg_sum_weighted_x(long n, int c, int nsample, int w_c, const float *src, const float *w, int w_bf16, const int *inv_off,
                           const int *inv_entry, int entry_base, const int *order, float *out, void *stream);   /* w fp32 or bfloat16 */
int pdf_seg_sum_weighted_ordered(long n, int c, int nsample, int w_c, const float *src, const float *w, const int *inv_off,
                                 const int *inv_entry, int entry_base, const int *order, float *out, void *stream);   /* order: visiting order of the n destinations or NULL */
int pdf_seg_sum_weighted(long n, int c, int nsample, int w_c, const float *src, const float *w, const int *inv_off, const int *inv_entry,
                         int entry_base, float *out, void *stream);

/* Cross-entropy with an ignore label, mean over the counted rows (pointcept/models/losses/misc.py:14-39 as configured on
 * this path).  Forward: loss[0], acc (pdf_ce_workspace_floats() floats; the first two = [sum, count], the rest per-workgroup partial
 * sums added in a fixed order: no atomics, nothing to zero), grad (n*c) = softmax - onehot (0 on ignored rows); a target that is neither
 * `ignore` nor in [0, c) makes the loss NaN (torch raises a device-side assert there).  Backward: grad_out = dlogits * gy[0] /
 * count; dlogits (the forward's `grad`) is only read, so the node can be differentiated more than once; grad_out may alias it. */
long pdf_ce_workspace_floats(void);
int pdf_ce_forward(long n, int c, const float *logits, const long *target, long ignore, float *grad, float *acc, float *loss,
                   void *stream);
int pdf_ce_backward(long n, int c, const float *dlogits, const float *acc, const float *gy, float *grad_out, void *stream);

/* The remaining criteria of pointcept/models/losses/misc.py as capturable passes (csrc/criteria.hip): fp32 logits, int64 labels, no float
 * atomics (per-workgroup partial sums in their own slots, added by one workgroup in a fixed order, in double: bit-reproducible), nothing
 * to zero, no host read.  acc: pdf_criteria_workspace_floats(c) floats (c = 1 for the binary loss), 8-byte aligned; acc[0..2] receive
 * [sum, normaliser, scale] where `scale` is what the backward multiplies with.  Every forward leaves its unscaled gradient (dice: the
 * softmax) in a buffer the backward only reads, so a node can be differentiated more than once; grad_out may not alias it.
 * PDF_REDUCE_*: the `reduction` argument.  n < 1, c < 1, a NULL array, an unknown reduction, label_smoothing outside [0, 1]:
 * PDF_ERR_BAD_ARG before any launch. */
#define PDF_REDUCE_NONE 0
#define PDF_REDUCE_MEAN 1
#define PDF_REDUCE_SUM 2
long pdf_criteria_workspace_floats(int c);
/* nn.CrossEntropyLoss(weight, ignore_index, reduction, label_smoothing) over (n, c) logits, any c >= 1 (c <= 64: one lane per row; above:
 * one wave per row).  weight: (c) floats or NULL (all 1).  Row with label t != ignore: l = (1 - eps) w[t] (-lp[t]) + eps / c sum_j w[j]
 * (-lp[j]), lp = log_softmax.  mean: loss[0] = sum l / sum w[t] (NaN when no row is counted); sum: loss[0] = sum l; none: loss (n) = l,
 * 0 on ignored rows.  A label that is neither `ignore` nor in [0, c) makes the loss (none: its row) NaN; its gradient row is 0.
 * grad (n*c) = d l / d logits.  Backward: grad_out = dlogits * gy[0] * acc[2] (none: * gy[row], gy (n)). */
int pdf_ce_ex_forward(long n, int c, const float *logits, const long *target, const float *weight, float label_smoothing, int reduction,
                      long ignore, float *grad, float *acc, float *loss, void *stream);
int pdf_ce_ex_backward(long n, int c, const float *dlogits, const float *acc, const float *gy, int reduction, float *grad_out, void *stream);
/* FocalLoss (misc.py:97-172) over the rows with target != ignore: per element of the one-hot target t against x = logits,
 * BCE_with_logits(x, t) * (alpha t + (1 - alpha)(1 - t)) * (t ? 1 - sigmoid(x) : sigmoid(x)) ^ gamma; alpha_vec: (c) floats or NULL (then
 * the scalar alpha).  mean: over (valid rows * c) elements, counted on the device, 0 with a zero gradient when every row is ignored; sum
 * likewise (PDF_REDUCE_NONE: PDF_ERR_BAD_ARG).  A bad label makes the loss NaN.  Backward: grad_out = dlogits * gy[0] * acc[2]. */
int pdf_focal_forward(long n, int c, const float *logits, const long *target, const float *alpha_vec, float alpha, float gamma, int reduction,
                      long ignore, float *grad, float *acc, float *loss, void *stream);
int pdf_focal_backward(long n, int c, const float *dlogits, const float *acc, const float *gy, float *grad_out, void *stream);
/* DiceLoss (misc.py:176-223), loss_weight 1: over the rows with target != ignore, p = softmax(logits), y = onehot(clamp(target, 0, c - 1))
 * (labels are clamped, not refused: the reference's behaviour); per class i: num = 2 sum p_i y_i + smooth, den = sum (p_i ^ exponent + y_i)
 * + smooth; loss[0] = sum_{i != ignore} (1 - num / den) / c (the divisor stays c when class `ignore` is skipped: the reference's
 * behaviour).  prob (n*c) receives p; acc also keeps the per-class coefficients the backward reads.  exponent > 0 (2: a fast path).
 * Backward: grad_out = d loss / d logits * gy[0], from prob, target and acc. */
int pdf_dice_forward(long n, int c, const float *logits, const long *target, float smooth, float exponent, long ignore, float *prob,
                     float *acc, float *loss, void *stream);
int pdf_dice_backward(long n, int c, const float *prob, const long *target, long ignore, float exponent, const float *acc, const float *gy,
                      float *grad_out, void *stream);
/* BinaryFocalLoss (misc.py:60-93) over n elements with float targets (probabilities allowed): bce = logits ? BCE_with_logits(x, t) :
 * BCE(x, t) (logs clamped at -100 as F.binary_cross_entropy); f = (alpha t + (1 - alpha)(1 - t)) (1 - exp(-bce)) ^ gamma bce.  reduce != 0:
 * loss[0] = mean f; reduce == 0: loss (n) = f.  grad (n) = d f / d x.  Backward: grad_out = dpred * gy[0] * acc[2] (reduce == 0: * gy[e]). */
int pdf_bfocal_forward(long n, const float *pred, const float *target, float alpha, float gamma, int logits, int reduce, float *grad,
                       float *acc, float *loss, void *stream);
int pdf_bfocal_backward(long n, const float *dpred, const float *acc, const float *gy, int reduce, float *grad_out, void *stream);

/* Head of the context-aware classifier (pointcept/models/context_aware_classifier/context_aware_classifier_v1m1_base.py) as capturable
 * passes (csrc/cac.hip): n rows in `scenes` scenes (offset: the scenes' ends, int32 on the device), K classes, c channels, fp32 data,
 * int64 labels.  No float atomics (chunk slabs added in a fixed order: bit-reproducible), nothing to zero, no host read.  The fused
 * class is pdf_cac_supported(K, c): c a multiple of 4 up to 64, K <= 256, the (K, c) slab and its row tiles within LDS -- it contains
 * (20, 48), (13, 48), (13, 24) and (200, 48).  ws: pdf_cac_workspace_floats(n, K, c, scenes) floats.  n < 1, scenes < 1, a NULL array
 * or a shape outside the class: PDF_ERR_BAD_ARG before any launch.
 *   soft prototypes: w_nk = softmax(logits_n)_k [max_k softmax >= conf_thresh] (conf_thresh <= 0: no mask), mass[s, k] = sum_{n in s} w_nk,
 *     proto[s, k, :] = sum_{n in s} w_nk feat_n / (mass + 1e-7).  Backward: gfeat (n, c) and, unless glogits is NULL, the gradient through
 *     the softmax and the normaliser into the logits (the mask is not differentiated).
 *   label prototypes: proto[k] = sum_{t_n = k} feat_n / (count_k + 1e-4) where count_k > 0, else base[k]; labels outside [0, K) are skipped.
 *     Backward: gfeat_n = gproto[t_n] / (count + 1e-4).
 *   cosine logits: out[n, k] = scale * normalize(x_n) . normalize(proto[s(n), k]) (F.normalize: max(norm, 1e-12)); scenes == 1: one
 *     prototype set, offset may be NULL.  Backward: gx and gproto, F.normalize's backward with its clamp branch.
 *   distillation loss (K <= 256, any c): l_n = -sum_k log_softmax(pred)_nk (smoothness softmax(soft)_nk + (1 - smoothness) onehot_nk),
 *     e_n = -sum_k sm_nk log(sm_nk + 1e-4); loss[0] = sum over the classes present among labels != -1 of
 *     (sum_{t=y} l e / (sum_{t=y} e + 1e-4)) / (#present + 1e-4), 0 when none is.  grad (n*K) receives the unscaled gradient, rowbuf (2 n)
 *     the row pairs, acc (pdf_cac_distill_workspace_floats(K) floats, 8-byte aligned) the class triples and coefficients.  A label that
 *     is neither -1 nor in [0, K) makes the loss NaN.  Backward: grad_out = grad * coefficient[t_n] * gy[0] (only reads). */
int pdf_cac_supported(int K, int c);
long pdf_cac_workspace_floats(long n, int K, int c, int scenes);
int pdf_cac_soft_proto_forward(long n, int K, int c, int scenes, const float *feat, const float *logits, const int *offset,
                               float conf_thresh, float *proto, float *mass, float *ws, void *stream);
int pdf_cac_soft_proto_backward(long n, int K, int c, int scenes, const float *feat, const float *logits, const int *offset,
                                float conf_thresh, const float *proto, const float *mass, const float *gproto, float *gfeat,
                                float *glogits, void *stream);
int pdf_cac_label_proto_forward(long n, int K, int c, const float *feat, const long *target, const float *base, float *proto,
                                float *count, float *ws, void *stream);
int pdf_cac_label_proto_backward(long n, int K, int c, const long *target, const float *count, const float *gproto, float *gfeat,
                                 void *stream);
int pdf_cac_cosine_forward(long n, int K, int c, int scenes, const float *x, const float *proto, const int *offset, float scale,
                           float *out, void *stream);
int pdf_cac_cosine_backward(long n, int K, int c, int scenes, const float *x, const float *proto, const int *offset, float scale,
                            const float *gout, float *gx, float *gproto, float *ws, void *stream);
long pdf_cac_distill_workspace_floats(int K);
int pdf_cac_distill_forward(long n, int K, const float *pred, const float *soft, const long *target, float smoothness, float *grad,
                            float *rowbuf, float *acc, float *loss, void *stream);
int pdf_cac_distill_backward(long n, int K, const float *grad, const long *target, const float *acc, const float *gy, float *grad_out,
                             void *stream);

/* Sparse 3-D convolutions (csrc/sparse_conv.hip; DESIGN.md "Sparse convolutions"): the three spconv operators of SpUNet-v1m1 over sites
 * indices (n, 4) int32 = [batch, d0, d1, d2], fp32 features, weights (C_out, k, k, k, C_in) with the offset's flat index (o0 k + o1) k + o2.
 * Keys: batch << 48 | d0 << 32 | d1 << 16 | d2 -- coordinates in [0, 65536), batch in [0, 32768).  No float atomics, fixed summation
 * orders, nothing allocated, every launch on `stream`.
 * Geometry (coordinate-only).  Every array is sized by the fine level (nmax rows); a level's count is an int on the device that the
 * kernels read there, so all levels are enqueued without a host read and the caller reads the counts and the status word once.
 *   pdf_spconv_sort_sites: skey (n) uint64 ascending keys, order (n) int32 the rows in that order (stable: equal sites keep their row
 *     order); status |= 1 a negative coordinate / batch, 2 a value outside the packing, 4 a duplicated site (never cleared here).
 *   pdf_spconv_subm_table: nbr (count, ksize^3) int32, entry [i, o] = the row of the site at coord_i + o - ksize / 2 of the same batch (the
 *     lowest row of a duplicated site), -1 where none is.  order NULL: the rows are in key order themselves (every coarse level).
 *   pdf_spconv_down: one kernel-2 stride-2 step.  limit (3 host ints or NULL): coarse sites outside it are dropped, their fine rows get
 *     parent -1.  -> parent / code (nmax), the coarse sites in ascending key order (coarse_indices (nmax, 4), coarse_skey), children
 *     (nmax, 8; -1: none; the lowest row of a duplicated site), the fine rows bucketed by code in tiles of 128 rows (bucket_perm:
 *     pdf_spconv_bucket_rows(nmax) ints, -1 padding; tile_code: one int per tile, -1 past the last bucket; bucket_ptr: 18 ints),
 *     count_out[0] = the number of coarse sites.  workspace: pdf_spconv_geometry_workspace_bytes(nmax) bytes, 256-byte aligned.
 * Products.  pdf_spconv_supported(k, cin, cout): 1 = the matrix-core class (cin, cout multiples of 32 up to 384, k <= 3), 2 = the small
 *   class of the stem (cin <= 16, cout 32 or 64, k <= 5), 0 = neither.
 *   pdf_spconv_gather: out[row, :] = bias + sum_k x[tbl[row, mirror ? K - 1 - k : k], :] . W_k over rows `row = perm ? perm[r] : r`,
 *     r < rows, 0 <= row < orows; table entries outside [0, xrows) read zeros; W_k element (kk, col) = w[kk w_kk + k w_k + col w_col];
 *     K <= 27.  tile_k (needs perm, K == 1): tile t of 128 list entries uses the tap tile_k[t] (a tile with tile_k < 0 is skipped) --
 *     the selected-weight product out[i] = x[parent[i]] W[code[i]] over pdf_spconv_down's buckets.
 *   pdf_spconv_small_forward / _dgrad: the same sum and its input gradient (through the mirrored table) for the small class.
 *   pdf_spconv_wgrad: dw (C_out, K, C_in) = sum_r G[tbl[r, k], :]^T D[r, :]; swap = 0: G = the input (ca = C_in), D = the output gradient
 *     (cb = C_out); swap = 1: G = the output gradient, D = the input.  cb a multiple of 32 up to 384, ca <= 384.  ws:
 *     pdf_spconv_wgrad_ws_floats floats of partial slabs, added in slab order.
 *   pdf_spconv_colsum: out[c] = sum_r g[r, c] (the bias gradient): chunk sums, then the chunks in order; ws: pdf_spconv_colsum_ws_floats. */
long pdf_spconv_geometry_workspace_bytes(long n);
long pdf_spconv_bucket_rows(long n);
int pdf_spconv_sort_sites(long n, const int *indices, unsigned long long *skey, int *order, int *status, void *workspace, void *stream);
int pdf_spconv_subm_table(long nmax, const int *count, const int *indices, const unsigned long long *skey, const int *order, int ksize,
                          int *nbr, void *stream);
int pdf_spconv_down(long nmax, const int *count, const int *indices, const int *limit, int *parent, int *code, int *coarse_indices,
                    unsigned long long *coarse_skey, int *children, int *bucket_perm, int *tile_code, int *bucket_ptr, int *count_out,
                    void *workspace, void *stream);
int pdf_spconv_supported(int k, int cin, int cout);
int pdf_spconv_gather(long rows, long orows, long xrows, int cin, int cout, int K, const float *x, const int *tbl, int mirror,
                      const int *perm, const int *tile_k, const float *w, long w_kk, long w_k, long w_col, const float *bias, float *out,
                      void *stream);
int pdf_spconv_small_forward(long rows, int cin, int cout, int K, const float *x, const int *tbl, const float *w, const float *bias,
                             float *out, void *stream);
int pdf_spconv_small_dgrad(long rows, int cin, int cout, int K, const float *g, const int *tbl, const float *w, float *dx, void *stream);
long pdf_spconv_wgrad_ws_floats(long rows, int K, int ca, int cb);
int pdf_spconv_wgrad(long rows, long grows, int K, int ca, int cb, const float *G, const float *D, const int *tbl, int swap, float *ws,
                     float *dw, void *stream);
long pdf_spconv_colsum_ws_floats(int c);
int pdf_spconv_colsum(long rows, int c, const float *g, float *ws, float *out, void *stream);

/* Distillation loss of the incremental learner (pointcept/incrLearners/ours/pointpdf_incr_v1m1_base.py:62-87, IncrDistillKlLoss):
 * student (n, cs) and teacher (n, ct) fp32 logits, labels (n) int64, ct <= cs <= 64.  Target row t = [softmax(teacher * inv_tt), 0 ..]
 * padded to cs columns, or onehot(label) where label != ignore; loss[0] = sum_rows sum_j (xlogy(t_j, t_j) - t_j log_softmax(student *
 * inv_tp)_j) / n (kl_div "batchmean": divided by ALL n rows).  grad (n*cs) receives softmax(student * inv_tp) * sum_j t_j - t; acc
 * (pdf_incr_kl_workspace_floats() floats) receives [sum, inv_tp / n] in its first two floats, the rest per-workgroup partial sums added
 * in a fixed order (no atomics, nothing to zero, bit-reproducible).  A label that is neither `ignore` nor in [0, cs) makes the loss NaN
 * (its row's gradient is 0).  n < 1, ct < 1 or ct > cs: PDF_ERR_BAD_ARG; cs > 64: PDF_ERR_UNSUPPORTED.  Backward: grad_out = dgrad *
 * gy[0] * inv_tp / n; dgrad (the forward's `grad`) is only read, so the node can be differentiated more than once. */
long pdf_incr_kl_workspace_floats(void);
int pdf_incr_kl_forward(long n, int cs, int ct, const float *student, const float *teacher, const long *labels, long ignore, float inv_tp,
                        float inv_tt, float *grad, float *acc, float *loss, void *stream);
int pdf_incr_kl_backward(long n, int cs, const float *dgrad, const float *acc, const float *gy, float *grad_out, void *stream);

/* Lovasz-softmax, multiclass, over the whole batch (pointcept/models/losses/lovasz.py:89-164, 241-257 with per_image=False): logits
 * (n, c <= 64) fp32, target (n) int64.  P = softmax(logits); for every class that occurs among the rows whose target != ignore (and,
 * with class_mask, whose mask byte is non-zero): e = |fg - P[:, class]| sorted descending (equal errors keep ascending row order: a
 * stable sort, so the subgradient is defined and reproducible), loss_class = sum_i e_i (J_i - J_{i-1}) with the Jaccard index J_i formed
 * from integer counts in double; loss[0] = mean over those classes (added in ascending class order), loss[1] = their number (0 when
 * every row is ignored: loss 0, gradient 0).  A target that is neither `ignore` nor in [0, c) makes the loss NaN.  prob (n*c) receives
 * P, dlogits (n*c) the finished d loss / d logits.  workspace: pdf_lovasz_workspace_bytes(n, c) bytes, every byte written before it is
 * read (nothing to zero, no atomics, bit-reproducible).  n < 1, n >= 2^31 - 1 or c < 1: PDF_ERR_BAD_ARG; c > 64: PDF_ERR_UNSUPPORTED.
 * Backward: grad_out = dlogits * gy[0] * scale; dlogits is only read, so the node can be differentiated more than once; grad_out may
 * alias it. */
long pdf_lovasz_workspace_bytes(long n, int c);
int pdf_lovasz_forward(long n, int c, const float *logits, const long *target, long ignore, const unsigned char *class_mask, float *prob,
                       float *dlogits, float *loss, void *workspace, void *stream);
int pdf_lovasz_backward(long n, int c, const float *dlogits, const float *gy, float scale, float *grad_out, void *stream);

/* Open-set metrics of n rows in one pass (pointcept/utils/misc.py:55-87; csrc/openset_metrics.hip): the class histograms of
 * intersection_and_union_gpu as exact counts and AUPR / AUROC as sklearn's average_precision_score / roc_auc_score define them.
 * Exactly one of logits (n, c) fp32 and pred (n) int64 is given; a prediction from logits is the lowest index among the row's maximal
 * values, a NaN counting as maximal (torch.max(1)[1]).  target (n) int64; rows with target == ignore are dropped.  hist (3, k) int64 =
 * intersection | union | target over the classes [0, k): a prediction or a label outside [0, k) is left out of its own histogram only.
 * score (n) fp32 or NULL; unknown: k bytes, 1 = the class id counts as positive (NULL: no class does).  record (4) double = [aupr, auroc,
 * n_pos, n_neg] over the kept rows: aupr = sum over the groups of equal score, descending, of (tp_g - tp_{g-1}) / n_pos * tp_g / (tp_g +
 * fp_g), summed in double in a fixed order; auroc = S / (2 n_pos n_neg) with the INTEGER S = sum_g (fp_g - fp_{g-1}) (tp_g + tp_{g-1})
 * (the tie-grouped trapezoid, independent of summation order).  -0.0 and +0.0 are one score, +-inf ordinary values.  n_pos == 0 (also:
 * no kept row): aupr = auroc = NaN; n_neg == 0: auroc = NaN; a NaN score on a kept row: aupr = auroc = NaN (the counts stay); score ==
 * NULL: record = NaN, NaN, 0, 0 and only the histogram kernels run.  Every element of hist and record is written.  workspace:
 * pdf_openset_metrics_workspace_bytes(n, c) bytes (the size depends on n alone; c is the logits' width or 0), 8-byte aligned, every byte
 * written before it is read (nothing to zero, no float atomics, bit-reproducible, capturable).  n < 1, n >= 2^31 - 1, k < 1, both or
 * neither of logits / pred, c < 1 with logits, a NULL target / hist / record / workspace: PDF_ERR_BAD_ARG before any launch; k > 1024:
 * PDF_ERR_UNSUPPORTED. */
long pdf_openset_metrics_workspace_bytes(long n, int c);
int pdf_openset_metrics(long n, int c, const float *logits, const long *pred, const float *score, const long *target, long ignore,
                        const unsigned char *unknown, int k, long long *hist, double *record, void *workspace, void *stream);

/* Per-scene sums of the relative coordinates rel = xyz[idx[i, j]] - xyz[i] of a SELF neighbour table (rows with idx < 0: rel = 0):
 * out (b, 9) double = [Sx Sy Sz | Mxx Mxy Mxz Myy Myz Mzz], WRITTEN (every workgroup lies inside one scene and stores its nine sums
 * into its own slot of ws -- pdf_knn_rel_moments_ws_doubles(b, n) doubles --, a second launch adds a scene's slots in order: no
 * atomics, bit-reproducible statistics).  The train-mode BatchNorm after the layer's
 * Linear(3, 3) (point_transformer_seg.py:27-29) is a closed form of these and the weights: pdf_pt_layer_forward_m takes the batch's sums
 * and skips its first statistics pass (csrc/geom_moments.hip). */
long pdf_knn_rel_moments_ws_doubles(int b, long m);
int pdf_knn_rel_moments(int b, long n, int nsample, const float *xyz, const int *offset, const int *idx, double *out, double *ws, void *stream);
/* the same for m queries new_xyz (scene ends new_offset) over other source points xyz: TransitionDown's grouping table */
int pdf_knn_rel_moments_q(int b, long m, int nsample, const float *xyz, const float *new_xyz, const int *new_offset, const int *idx,
                          double *out, double *ws, void *stream);

/* Morton keys of the points of a batch, scene by scene (visiting order of the forward gathers and layer passes: a stable sort of these keys;
 * pointcloudpdf_amd/geometry.py: Geometry.order -- no reference counterpart, nothing is stored in that order): keys[i] = scene(i) << 30 |
 * 30-bit Morton code of point i on a 1024^3 grid over ITS scene's bounding box.  bounds: 4 b floats of scratch (written). */
int pdf_scene_morton_keys(long n, int b, const float *xyz, const int *offset, float *bounds, long long *keys, void *stream);

/* SGD with momentum and weight decay (torch.optim.SGD, dampening 0, no Nesterov -- the optimizer the reference's configs build,
 * pointcept/utils/optimizer.py + configs/s3dis/openseg-pt-v1-0-*.py) over every parameter tensor in ONE launch.  tab: ntensors records
 * {float *param; const float *grad; float *momentum; long length} in device memory; chunks: nchunks {tensor, chunk} int32 pairs, one
 * per pdf_sgd_chunk() values of a tensor.  param / momentum are updated in place.
 * found_inf (device float, may be NULL): non-zero = the step is skipped as a whole (a GradScaler step that saw a non-finite gradient). */
int pdf_sgd_chunk(void);
int pdf_sgd_step(int nchunks, const void *tab, const int *chunks, float lr, float momentum, float weight_decay, const float *found_inf,
                 void *stream);
/* Dynamic loss scaling of the reference's AMP training (torch.cuda.amp.GradScaler, pointcept/engines/train.py:340-363) with every decision
 * on the device, so that a captured step replays: pdf_grad_unscale multiplies every gradient of the table (pdf_sgd_step's layout) by
 * *inv_scale in place and sets *found_inf = 1 when any value is inf / nan (found_inf must be 0 on entry); pdf_scaler_update applies
 * GradScaler.update(): found_inf -> scale *= backoff_factor, growth_tracker = 0; else growth_tracker += 1 and after growth_interval clean
 * steps scale *= growth_factor; leaves inv_scale = 1 / scale and found_inf = 0.  All four words are caller-owned device scalars. */
int pdf_grad_unscale(int nchunks, const void *tab, const int *chunks, const float *inv_scale, float *found_inf, void *stream);
int pdf_scaler_update(float *scale, float *inv_scale, int *growth_tracker, float *found_inf, float growth_factor, float backoff_factor,
                      int growth_interval, void *stream);
/* Adam / AdamW (torch.optim.Adam / torch.optim.AdamW, the single-tensor non-capturable arithmetic of torch/optim/adam.py; no amsgrad, no
 * maximize -- the optimizer of configs/scannet/openseg-pt-v1-0-*.py and of the openseg-st-v1m1 configs) over every tensor of one parameter
 * group.  tab: ntensors records {float *param; const float *grad; float *exp_avg; float *exp_avg_sq; float *step; long length; long pad[2]}
 * (64 bytes) in device memory; chunks as for pdf_sgd_step (pdf_sgd_chunk() values per chunk).  step points at that tensor's own float32 step
 * count on the device: a one-thread-per-tensor launch adds 1 to each, then the update launch reads it for the bias corrections
 * 1 - beta^step, formed in double from THIS call's betas (OneCycleLR moves beta1 between calls).  decoupled: 1 = AdamW (p *= 1 - lr wd),
 * 0 = Adam's L2 form (g += wd p).  param / exp_avg / exp_avg_sq / step are updated in place.
 * found_inf (device float, may be NULL): non-zero = parameters, both moments and every step count stay untouched.
 * PDF_ERR_BAD_ARG before any launch: null tables, nchunks < 0, ntensors <= 0 with chunks to run, lr < 0, eps < 0, weight_decay < 0, a
 * beta outside [0, 1) (NaN included).  pdf_adam_grad_unscale is pdf_grad_unscale over this 64-byte record. */
int pdf_adam_step(int nchunks, int ntensors, const void *tab, const int *chunks, double lr, double beta1, double beta2, double eps,
                  double weight_decay, int decoupled, const float *found_inf, void *stream);
int pdf_adam_grad_unscale(int nchunks, const void *tab, const int *chunks, const float *inv_scale, float *found_inf, void *stream);

/* ---- libs/pointops2 window attention: the CSR-by-query v2 / v3 launchers of
 * libs/pointops2/src/attention_v2/attention_cuda_kernel_v2.h and libs/pointops2/src/rpe_v2/relative_pos_encoding_cuda_kernel_v2.h,
 * same parameter lists + stream.  N = number of queries (index0_offsets has N + 1 entries), M = edges, C = h * d,
 * tables are (L, h, d, 3), rel_idx is (M, 3).  n_max (longest edge list) is accepted for parity and not needed.
 * Overwritten outputs: attn / output / grad_q / grad_attn.  Pre-zeroed by the caller: grad_k, grad_v, grad_table*. */
int pdf_attention_step1_forward_v2(int N, int M, int h, int C, unsigned n_max, const float *q, const float *k,
                                   const int *index0_offsets, const int *index1, float *attn, void *stream);
int pdf_attention_step1_backward_v2(int N, int M, int h, int C, unsigned n_max, const float *grad_out, const int *index0_offsets,
                                    const int *index1, const float *q, const float *k, float *grad_q, float *grad_k, void *stream);
int pdf_dot_prod_with_idx_forward_v3(int N, int M, int h, int hdim, unsigned n_max, const float *q, const int *index_q_offsets,
                                     const float *k, const int *index_k, const float *table_q, const float *table_k,
                                     const int *rel_idx, float *output, void *stream);
int pdf_dot_prod_with_idx_backward_v3(int N, int M, int h, int hdim, unsigned n_max, const float *grad_out, const float *q,
                                      const int *index_q_offsets, const float *k, const int *index_k, const float *table_q,
                                      const float *table_k, const int *rel_idx, float *grad_q, float *grad_k, float *grad_table_q,
                                      float *grad_table_k, void *stream);
int pdf_attention_step2_with_rel_pos_value_forward_v2(int N, int M, int h, int hdim, unsigned n_max, const float *attn, const float *v,
                                                      const int *index0_offsets, const int *index1, const float *table,
                                                      const int *rel_idx, float *output, void *stream);
int pdf_attention_step2_with_rel_pos_value_backward_v2(int N, int M, int h, int hdim, unsigned n_max, const float *grad_out,
                                                       const int *index0_offsets, const int *index1, const float *attn, const float *v,
                                                       const float *table, const int *rel_idx, float *grad_attn, float *grad_v,
                                                       float *grad_table, void *stream);

/* the three table ops with the table length L (rows of the tables) passed explicitly: per-head kernels that keep the head's
 * table slabs and the table gradients in LDS (fall back to the entry points above when d is not a power of two <= 64 or the
 * slabs exceed 64 KB) */
int pdf_dot_prod_with_idx_forward_v3_l(int N, int M, int h, int hdim, int L, const float *q, const int *index_q_offsets, const float *k,
                                       const int *index_k, const float *table_q, const float *table_k, const int *rel_idx, float *output,
                                       void *stream);
int pdf_dot_prod_with_idx_backward_v3_l(int N, int M, int h, int hdim, int L, const float *grad_out, const float *q,
                                        const int *index_q_offsets, const float *k, const int *index_k, const float *table_q,
                                        const float *table_k, const int *rel_idx, float *grad_q, float *grad_k, float *grad_table_q,
                                        float *grad_table_k, void *stream);
int pdf_attention_step2_with_rel_pos_value_backward_v2_l(int N, int M, int h, int hdim, int L, const float *grad_out,
                                                         const int *index0_offsets, const int *index1, const float *attn, const float *v,
                                                         const float *table, const int *rel_idx, float *grad_attn, float *grad_v,
                                                         float *grad_table, void *stream);

/* ---- GridSample voxel keys: replaces the numpy front half of pointcept/datasets/transform.py:813-823 and
 * fnv_hash_vec (:911-925) for a batch of scenes.  coord (n,3) f32, offset (b) cumulative ends, min_grid (b,3) int64 = per-scene
 * floor(min coord / grid) -> grid (n,3) int64 scene-relative voxel coordinates, key (n) uint64 FNV keys.  f32 = 0: float64
 * division (NumPy >= 2 promotion), f32 = 1: float32 division (NumPy 1.x). */
int pdf_grid_hash(long n, int b, const float *coord, const int *offset, double gx, double gy, double gz, int f32,
                  const long long *min_grid, long long *grid, unsigned long long *key, void *stream);
/* The same on float64 coordinates (S3DIS stores them as float64; RandomRotate promotes float32 ones): floor(coord / grid) in float64. */
int pdf_grid_hash_f64(long n, int b, const double *coord, const int *offset, double gx, double gy, double gz,
                      const long long *min_grid, long long *grid, unsigned long long *key, void *stream);

/* ---- training augmentation of raw scenes (csrc/augment.hip; pointcept/datasets/transform.py, the PDF configs' train lists).
 * pdf_philox4x64: out (n,4) = Philox4x64-10 blocks for key (key0, key1), counters ctr0 .. ctr0 + n - 1 (word 0; carry into word 1);
 *   numpy.random.Philox(counter=c, key=k).random_raw(4) is the block of counter c + 1.
 * pdf_aug_bounds: per-scene min / max of coord (n,3) f64 [and color (n,3) f64, may be NULL] -> bounds (b,12): coord min, coord max,
 *   colour min, colour max.  offset (b + 1) int64 scene starts; part: pdf_aug_bounds_workspace_doubles(b) doubles.  No atomics.
 * pdf_aug_points: one segment of `nop` ops on every point, in place on fp64 rows (coord, color, normal; color / normal may be NULL).
 *   table (b, 1 + nop, 16) f64: row 0 = the scene's 64-bit key (bit pattern), rows 1.. = op code, fired flag, parameters and the
 *   scene's current NumPy dtype per array (pointcloudpdf_amd/augment.py builds it); bounds (b,12) of the segment's start (may be NULL
 *   when no op reads it); rec (k, n, 3) f64 recorded per-point normals (may be NULL: drawn in the kernel).
 * pdf_aug_keys: out (n) uint64 = word 0 of the Philox block (scene_keys[s], stream_id; counter = index in the scene). */
int pdf_philox4x64(long n, long key0, long key1, long ctr0, unsigned long long *out, void *stream);
int pdf_aug_bounds_workspace_doubles(int b);
int pdf_aug_bounds(int b, const long long *offset, const double *coord, const double *color, double *part, double *bounds, void *stream);
int pdf_aug_points(int b, long n, const long long *offset, int nop, const double *table, const double *bounds, const double *rec,
                   double *coord, double *color, double *normal, void *stream);
int pdf_aug_keys(int b, long n, const long long *offset, const unsigned long long *scene_keys, long stream_id, unsigned long long *out,
                 void *stream);
/* ElasticDistortion, one (granularity, magnitude) stage.  vinfo (int64): voxel starts (b + 1) of the scenes' noise volumes, dims (b,3),
 * axis starts (b + 1); vol (total, 3) float32 C-order volumes.  pdf_aug_elastic_noise: standard normals (Philox, as pdf_aug_keys;
 * counter = voxel index in the scene).  pdf_aug_elastic_blur: one 3-tap 1/3 box pass along `axis` with zero boundary, in != out.
 * pdf_aug_elastic_apply: coord += trilinear sample of vol on the scene's axes (f64, zero outside) * magnitude, rounded to the scene's
 * dtype; params (b,2) f64 = fired, float32 flag; disp (n,3) f64 may be NULL (receives the sample). */
int pdf_aug_elastic_noise(int b, long total, const long long *vinfo, const unsigned long long *scene_keys, long stream_id, float *vol,
                          void *stream);
int pdf_aug_elastic_blur(int b, long total, const long long *vinfo, const float *in, float *out, int axis, void *stream);
int pdf_aug_elastic_apply(int b, long n, const long long *offset, const long long *vinfo, const double *axes, const float *vol,
                          const double *params, double magnitude, double *coord, double *disp, void *stream);

/* ---- test-time fragment voting (pointcept/engines/test.py:218-229, 243-251): pred[index[r], :] +=
 * softmax(logits[r, :]); score_sum[index[r]] += score[r]; score_cnt[index[r]] += 1.  index (n) int64, distinct within a call
 * (one point per voxel of a GridSample test fragment); score may be NULL. */
int pdf_vote_accumulate(long n, int c, const float *logits, const float *score, const long *index, float *pred,
                        float *score_sum, float *score_cnt, void *stream);

/* ---- batched test-time fragments of ONE augmented scene (csrc/fragments.hip; pointcept/datasets/transform.py:858-887,
 * datasets/defaults.py:96-129, engines/test.py:206-251).  The fragment table (voxelize.fragment_table): order (n) int64 = point ids,
 * key-sorted, original order inside a voxel; vstart (v) / count (v) int64 = every voxel's run in `order`; voxel_of (n) int64 = the voxel
 * of every sorted position.  Fragment f holds order[vstart[i] + f % count[i]] of every voxel i; a call covers fragments f0 .. f0 + g - 1,
 * row r = (f - f0) v + i.  Every entry validates before any launch -- PDF_ERR_BAD_ARG: a null table / output, n < 0, v < 0, v > n,
 * f0 < 0, g < 1 (gather: g > 256, or g v >= 2^31 -- out_offset is int32), f64 not 0 / 1 -- and is a no-op for v == 0.
 * pdf_fragment_bounds: bounds (g, 6) float64 = [min xyz | max xyz] of the selected coordinates (coord (n, 3) fp32, or fp64 with f64 = 1;
 *   exact either way); ws: pdf_fragment_bounds_ws_doubles(g) doubles.
 * pdf_fragment_gather: index (g v) int64; out_coord (g v, 3) fp32 = coord[p] - shift[f - f0], shift (g, 3) in coord's dtype, subtracted in
 *   that dtype and rounded once to fp32; out_feat (g v, c) fp32 = nseg (1..4) segments side by side: seg_src[k] == NULL -> the shifted
 *   coordinate (seg_w[k] must be 3), else the (n, seg_w[k] in 1..4) fp32 array seg_src[k] gathered; seg_src / seg_w are HOST arrays of
 *   nseg entries; out_grid (g v, 3) int64 = grid_src[p] (both NULL, or both given); out_offset (g) int32 = (k + 1) v.
 * pdf_fragment_vote: logits (g v, c), score (g v) or NULL, in gather order, folded into pred (n, c) / score_sum (n) / score_cnt (n)
 *   without atomics, a point's fragments in ascending order: bit-identical to g successive pdf_vote_accumulate calls. */
long pdf_fragment_bounds_ws_doubles(int g);
int pdf_fragment_bounds(long n, long v, int f0, int g, int f64, const void *coord, const long *order, const long *vstart,
                        const long *count, double *ws, double *bounds, void *stream);
int pdf_fragment_gather(long n, long v, int f0, int g, int f64, const void *coord, const long *order, const long *vstart,
                        const long *count, const void *shift, int nseg, const float *const *seg_src, const int *seg_w,
                        const long long *grid_src, long *index, float *out_coord, float *out_feat, long long *out_grid,
                        int *out_offset, void *stream);
int pdf_fragment_vote(long n, long v, int f0, int g, int c, const float *logits, const float *score, const long *order,
                      const long *vstart, const long *count, const long *voxel_of, float *pred, float *score_sum,
                      float *score_cnt, void *stream);

/* Fixed-radius neighbour table of a batch with itself over the kNN grid (cells >= radius): idx (n, nsample) = the first nsample
 * points of the query's scene in index order within `radius`, -1 / 1e10 padded -- the results of pdf_random_ball_query with the
 * identity permutation and min_radius 0 (stands in for torch_points_kernels.ball_query(..., mode="partial_dense") in the PDF
 * pseudo-label pass, pointpdf_v1m1_base.py:122-130).  Workspace: pdf_knn_workspace_bytes(b, n, 0); b <= 64. */
int pdf_radius_neighbors_self(int n, int nsample, float radius, const float *xyz, const int *offset, int b, int *idx, float *dist2,
                              void *workspace, long workspace_bytes, void *stream);
/* The same table with one radius PER SCENE, derived on the device (the reference's adaptive_radius=True, pointpdf_v1m1_base.py:137-149):
 * r_s = min over the three axes of ((max_a - min_a) + pad) / divisor, fp32 in exactly that order -- with divisor = 16, pad = 1e-6 the value
 * of ((c.max(0)[0] - c.min(0)[0] + 1e-6) / 16).min() on the scene's float32 coordinates.  The extents are the ones the grid setup reduces
 * anyway; r_s is written to radii[s] (b floats, out), sizes the scene's cells (cell >= r_s * 1.0001) and is the radius of every query of
 * scene s: accepted are d2 < r_s * r_s or d2 <= 1e-5, as above.  A one-point scene, coincident points or a flat axis give
 * r_s = pad / divisor: every point then still finds itself and everything within sqrt(1e-5) = 3.16 mm -- both entries size their cells by
 * max(radius, 3.1623 mm), so the 27 cells around a query cover that reach whatever the radius.  A scene without points gets r_s = pad / divisor.  No host read, no allocation: the call
 * can be recorded into a graph.  Same workspace, same b <= 64, same argument errors as the fixed entry, plus divisor <= 0, pad < 0 or a
 * null radii; n == 0 launches nothing and leaves radii untouched. */
int pdf_radius_neighbors_self_adaptive(int n, int nsample, float divisor, float pad, const float *xyz, const int *offset, int b,
                                       int *idx, float *dist2, float *radii, void *workspace, long workspace_bytes, void *stream);

/* The graph stage of the PDF pseudo-label pass (pointpdf_v1m1_base.py:309-380: scipy.sparse.csgraph.minimum_spanning_tree over the
 * region's neighbour similarities, :340; connected_components of the weak tree edges, :360) for ONE scene, one workgroup.
 * u, v (E directed entries, node ids < n), w (E weights, or NULL: all equal), active (E flags, or NULL: all), nodes (n_nodes ids,
 * repeats allowed, covering every endpoint of an active entry; an entry with an endpoint outside the list or outside [0, n) is ignored).  chosen (E bytes, or NULL) = 1 for the entries of the minimum
 * spanning forest under the strict order (weight, entry index); comp (n ints, written at the listed nodes only) = the root of the
 * node's connected component (one of its node ids).  workspace: pdf_graph_forest_workspace_bytes(n, E, n_nodes) bytes, 8-byte
 * aligned.  Lists of up to 12,288 nodes keep the per-round state in LDS. */
long pdf_graph_forest_workspace_bytes(long n, long E, long n_nodes);
int pdf_graph_forest(long n, int E, const long long *u, const long long *v, const float *w, const unsigned char *active,
                     const long long *nodes, int n_nodes, int *comp, unsigned char *chosen, void *workspace, long workspace_bytes,
                     void *stream);

/* Two-component 1-D Gaussian mixture by EM in double on m SORTED values: stands in for sklearn.mixture.GaussianMixture(n_components=2)
 * .fit(tree weights) (pointpdf_v1m1_base.py:343-345; reg_covar 1e-6, tol on the mean log-likelihood, max_iter) with a deterministic
 * start (quartiles, then 2-means) instead of sklearn's randomly seeded k-means.  resp: 2 m doubles of scratch; out (8 doubles): means,
 * variances, weights of the two components, iterations run, final mean log-likelihood. */
int pdf_gmm2_1d(int m, const float *sorted_x, double *resp, double *out, int iters, double tol, double reg, void *stream);

/* Softmax over the edges of every query, per head (x, y: (M, h); index0_offsets: N + 1 entries; h <= 64): stands in for
 * torch_scatter.scatter_softmax(src, index_0, dim=0) in WindowAttention.forward (stratified_transformer_v1m1_origin.py:322-324;
 * torch_scatter is an unvendored dependency).  backward: grad_x = y * (grad_y - sum over the query of y * grad_y). */
int pdf_segment_softmax_forward(int N, int M, int h, const int *index0_offsets, const float *x, float *y, void *stream);
int pdf_segment_softmax_backward(int N, int M, int h, const int *index0_offsets, const float *y, const float *grad_y, float *grad_x,
                                 void *stream);

/* Atomic-free building blocks of the three backward launchers above (csrc/window_attention_bwd.hip), for head dim 16, L <= 64.  The
 * reference scatters with one atomicAdd per (edge, channel) (attention_cuda_kernel_v2.cu:50-93, relative_pos_encoding_cuda_kernel_v2.cu:
 * 287-340, 441-484); here every such sum is a segmented sum over the edge list grouped by query (the CSR arrays of the forward) or by key
 * (the transposed list the caller builds once per edge table: key offsets, edge ids grouped by key, and the query / rel_idx of those
 * edges -- pointcloudpdf_amd/_native.py: window_csc), in ascending edge order: bit-reproducible, outputs written (not accumulated).
 *   pdf_wa_segment_rows: out[n, c] = sum_{e in [seg_off[n], seg_off[n+1])} w[eid(e), c / 16] * (X[other[e], c] + T(rel[e])[c]),
 *       eid(e) = seg_edge ? seg_edge[e] : e;  X (rows, with `other`) and table (with `rel`, (M, 3) in SEGMENT order) are each optional.
 *   pdf_wa_table_grad:   grad_table[r, c, a] = sum_n x[n, c] * sum_{e in seg(n), rel[e][a] == r} w[eid(e), c / 16]   (x = the segment
 *       owner's row: q or grad_out over the CSR list, k over the CSC list); ws: pdf_wa_table_grad_ws_floats(N, h, L) floats.
 *   pdf_wa_grad_attn:    grad_attn[m, hh] = <grad_out[q(m), hh, :], v[index1[m], hh, :] + T(m, hh, :)>.
 * Row operands carry a row stride in floats (ldx / ldo / ldg / ldv / ld >= h * 16: q, k, v may be slices of the (N, 3 C) rows the qkv Linear
 * writes, gradients may be written into slices of one (N, 3 C) buffer) and the scales that WindowAttention applies to the query
 * (xscale on gathered / owner rows, oscale on the result, qscale on the query rows of the logits).
 * PDF_ERR_UNSUPPORTED for other head dims / longer tables: the caller keeps the atomic launchers above. */
int pdf_wa_segment_rows(int N, int h, int d, int L, const int *seg_off, const int *seg_edge, const int *other, const int *rel,
                        const float *w, const float *X, long ldx, float xscale, const float *table, float *out, long ldo, float oscale, void *stream);
/* pdf_wa_segment_rows with a visiting order of the owners (a permutation of 0 .. N - 1, or null = storage order): same sums, same results;
 * owners of one window side by side gather the same rows (stratified.BasicLayer.window_tables hands the window-sorted order over). */
int pdf_wa_segment_rows_ordered(int N, int h, int d, int L, const int *seg_off, const int *seg_edge, const int *other, const int *rel,
                                const float *w, const float *X, long ldx, float xscale, const float *table, float *out, long ldo, float oscale,
                                const int *order, void *stream);
long pdf_wa_table_grad_ws_floats(int N, int h, int L);
int pdf_wa_table_grad(int N, int h, int d, int L, const int *seg_off, const int *seg_edge, const int *rel, const float *w,
                      const float *x, long ldx, float xscale, float *ws, float *grad_table, void *stream);
int pdf_wa_grad_attn(int N, int M, int h, int d, int L, const float *grad_out, long ldg, const int *offsets, const int *index1, const float *v,
                     long ldv, const float *table, const int *rel, float *grad_attn, void *stream);
/* attention_step1_forward_cuda_launcher_v2 + dot_prod_with_idx_forward_cuda_launcher_v3 in one pass over the key rows (their sum is what
 * WindowAttention.forward feeds the softmax, stratified_transformer_v1m1_origin.py:300-321):
 * logits[m, hh] = <q[q(m), hh], k[index1[m], hh] + T_q(m, hh)> + <k[index1[m], hh], T_k(m, hh)>. */
int pdf_wa_logits_forward(int N, int M, int h, int d, int L, const float *q, const float *k, long ld, float qscale, const int *offsets,
                          const int *index1, const float *table_q, const float *table_k, const int *rel, float *out, void *stream);
/* dst (M, h) = src[edge[m], :]: edge scalars (attention weights / logit gradients) brought into the order of the key-grouped edge list. */
int pdf_wa_permute_edges(int M, int h, const float *src, const int *edge, float *dst, void *stream);
/* pdf_wa_logits_forward / pdf_wa_grad_attn with the queries a workgroup takes given by a visiting order (see pdf_wa_segment_rows_ordered);
 * every output element is the same expression: identical results. */
int pdf_wa_logits_forward_ordered(int N, int M, int h, int d, int L, const float *q, const float *k, long ld, float qscale, const int *offsets,
                                  const int *index1, const float *table_q, const float *table_k, const int *rel, float *out, const int *order,
                                  void *stream);
int pdf_wa_grad_attn_ordered(int N, int M, int h, int d, int L, const float *grad_out, long ldg, const int *offsets, const int *index1,
                             const float *v, long ldv, const float *table, const int *rel, float *grad_attn, const int *order, void *stream);

/* Edge tables of the StratifiedTransformer's window partitions (stratified_transformer_v1m1_origin.py:45-127 get_indice_pairs / grid_sample +
 * the stable sort by query of :468-536, and WindowAttention's quantised relative positions :282-292), built per QUERY instead of by pair
 * expansion + an edge-sized sort (csrc/window_edges.hip).  Inputs: int64 keys per point (fine-window key kf, coarse-window key kc, packed
 * fine-window cell wk), kf in ascending order (kf_sorted) with the point ids in that order (order_f, ties ascending), and the same for the
 * m FPS-downsampled points by coarse key (kcd_sorted, order_cd, wkd = wk[order_cd]).
 *   pdf_window_edges_count : count (n) int32 = row length of every query, seg (n, 4) int32 (16-byte aligned) = its two segments
 *   pdf_window_edges_fill  : offsets (n + 1) = exclusive scan of count -> index0 (E) int64 ascending, index1 (E) int32, rel (E, 3) int32 or
 *                            null; *flag |= 1 if a quantised offset leaves [0, vmax] (the reference asserts that range) */
/* The keys themselves (the elementwise part of :468-499 -- torch_geometric's voxel_grid on the plain coordinates for even blocks, on the
 * coordinates shifted by half a window from the batch minimum for odd ones -- and the fine-window cell of :91-94), one launch per partition:
 * xyz (n, 3), ends (scenes) int32 scene ends, lo / hi (3) float32 DEVICE = per-axis minimum / maximum of xyz -> kf, kc, wk (n) int64.
 * Same floating-point steps as torch.div(.., rounding_mode="floor" / "trunc") on float32 tensors: bit-identical keys. */
int pdf_window_keys(int n, const float *xyz, const int *ends, int scenes, const float *lo, const float *hi, float window_size, int parity,
                    long long *kf, long long *kc, long long *wk, void *stream);
/* The same with ONE ORIGIN PER SCENE (the precise tester: a fragment's partition must not depend on its batch mates).
 *   pdf_scene_bounds      : lo, hi (scenes, 3) float32 = per-axis minimum / maximum of every scene's rows of xyz, one launch, exact
 *   pdf_window_keys_scene : lo / hi (scenes, 3) -> every scene's keys are those of the scene collated alone through pdf_window_keys, plus the
 *                           number of grid cells of the scenes in front of it: keys of two scenes never compare equal, and the edge tables
 *                           built from them are, scene by scene, the tables of the scene alone (rows and key ids moved by the scene's start) */
int pdf_scene_bounds(int n, const float *xyz, const int *ends, int scenes, float *lo, float *hi, void *stream);
int pdf_window_keys_scene(int n, const float *xyz, const int *ends, int scenes, const float *lo, const float *hi, float window_size,
                          int parity, long long *kf, long long *kc, long long *wk, void *stream);
int pdf_window_edges_count(int n, const long long *kf_sorted, const long long *kf, int m, const long long *kcd_sorted, const long long *kc,
                           const long long *wk, const long long *wkd, int *count, int *seg, void *stream);
int pdf_window_edges_fill(int n, const int *offsets, const int *seg, const int *order_f, const int *order_cd, const long long *wk,
                          const long long *wkd, const float *xyz, float c2w, float qs, int vmax, long long *index0, int *index1, int *rel,
                          int *flag, void *stream);

/* The PDF pseudo-label pass without a host in the loop (pointcept/recognizers/ours/pointpdf_v1m1_base.py:190-380; csrc/region_grow.hip,
 * csrc/graph_prune.hip).  All scenes of a batch per call; starts / sizes (scenes) int32 = the scenes' point ranges; neighbors (N, nsample)
 * int32 GLOBAL row ids, -1 padded (the table pdf_radius_neighbors_self writes); every size the next stage needs stays in device memory, and
 * every reduction is done here (torch's multi-block reductions are not replay-safe on this stack: docs/NOTEBOOK.md, round 5):
 *   pdf_region_stats : :190-205 -- ml_norm = (ml - min) / (max - min + 1e-6), stop = mean(score) - beta * std(score) per scene; clears mult
 *   pdf_region_seeds : :206-207 -- mult[p] += 1 for the point whose src value has rank dice[s, j] (radix select; stands in for sort + gather)
 *   pdf_region_grow  : all growth rounds of :233-305 on mult (N) int32 (in: multiplicities of the seed list, out: the region);
 *                      lists: 2 N ints of scratch; max_points: the largest scene (host value: sizes the LDS bitmaps);
 *                      info (scenes, 4) = [rounds, grew, list length, distinct points]
 *   pdf_region_edges : the region's ascending node list and the (row, col, weight) entries of its neighbour graph (:309-335, ours/utils.py:7-43)
 *                      at capacity sizes[s] / sizes[s] * nsample per scene; counts (scenes, 4) = [nodes, entries, any -1 padding, smallest id
 *                      touched]; comp / lab (N) = every point's own local id; rows_ws: 3 * n_total words; lists / grow_info:
 *                      pdf_region_grow's `lists` / `info` when its largest scene <= pdf_region_grow_list_points(), else NULL, NULL
 *   pdf_graph_forest_dev / pdf_gmm2_1d_dev: pdf_graph_forest / pdf_gmm2_1d with the sizes read from device memory ([nodes, entries] / [m])
 *   pdf_region_tree  : the forest's chosen entries compacted in entry order (tdev[s, 1] of them per scene), tdev (scenes, 2) = [nodes, tree edges]
 *   pdf_sort_floats_dev: the first tdev[s, 1] weights of every scene ascending (what the mixture fit takes); tmp: N words
 *   pdf_gmm2_weak_dev: :343-358 for every scene -- the two-component fit of the sorted weights (fit (scenes, 8) doubles as pdf_gmm2_1d) and
 *                      weak[e] = tw[e] < mean - 2 * covariance of the component with the larger mean (N bytes); resp: 2 N doubles
 *   pdf_region_mask  : :360-380 -- component sizes over the touched points, z-score > 2 -> mask (N bytes); cnt: N ints of workspace */
int pdf_region_stats(int scenes, const int *starts, const int *sizes, const float *msp, const float *ml, int score_is_ml, float beta,
                     float *ml_norm, float *stop, int *mult, void *stream);
int pdf_region_seeds(int scenes, const int *starts, const int *sizes, const float *src, const long long *dice, int num_seed, int *mult,
                     void *stream);
int pdf_region_grow(int scenes, const int *starts, const int *sizes, int max_points, const float *coord, const float *score,
                    const int *neighbors, int nsample, const float *stop, int slide_window, int max_rounds, int *mult, int *lists, float *sim,
                    int *info, void *stream);
int pdf_region_edges(int scenes, const int *starts, const int *sizes, const float *coord, const float *msp, const int *neighbors,
                     int nsample, const int *mult, const int *lists, const int *grow_info, long long *nodes_out, long long *eu, long long *ev,
                     float *ew, unsigned char *touched, int *comp, int *lab, int *counts, void *rows_ws, long n_total, void *stream);
long pdf_region_grow_list_points(void);   /* largest scene for which pdf_region_grow leaves the ascending member list in `lists` */
int pdf_region_tree(int scenes, const int *starts, const int *sizes, int nsample, const int *counts, const unsigned char *chosen,
                    const long long *eu, const long long *ev, const float *ew, long long *tu, long long *tv, float *tw, int *tdev, void *stream);
int pdf_graph_forest_dev(long n, int E, const long long *u, const long long *v, const float *w, const unsigned char *active,
                         const long long *nodes, int n_nodes, const int *dev, int *comp, unsigned char *chosen, void *workspace,
                         long workspace_bytes, void *stream);
int pdf_gmm2_1d_dev(int m_cap, const float *sorted_x, const int *m_dev, double *resp, double *out, int iters, double tol, double reg, void *stream);
/* pdf_graph_forest_dev for the scenes of a batch in ONE launch (grid = scenes).  starts / sizes: HOST arrays; u, v, w, active, chosen
 * (N * stride) / nodes, comp (N): the batch's arrays, scene s at starts[s] (* stride); dev + s * dev_stride = the scene's [nodes, entries];
 * workspace: the scenes' pdf_graph_forest_workspace_bytes(size, size * stride, size), each rounded up to 8 bytes, back to back. */
int pdf_graph_forest_batch_dev(int scenes, const int *starts, const int *sizes, int stride, const long long *u, const long long *v,
                               const float *w, const unsigned char *active, const long long *nodes, const int *dev, int dev_stride,
                               int *comp, unsigned char *chosen, void *workspace, long workspace_bytes, void *stream);
int pdf_sort_floats_dev(int scenes, const int *starts, const int *sizes, const int *tdev, const float *x, float *out, void *tmp, void *stream);
int pdf_gmm2_weak_dev(int scenes, const int *starts, const int *sizes, const int *tdev, const float *sorted_x, const float *tw, double *resp,
                      double *fit, unsigned char *weak, int iters, double tol, double reg, void *stream);
int pdf_region_mask(int scenes, const int *starts, const int *sizes, const int *lab, const unsigned char *touched, const int *counts, int *cnt,
                    unsigned char *mask, void *stream);

/* The TransitionUp head's per-scene context (point_transformer_seg.py:148-161: ``x_b.sum(0, True) / cnt`` and ``.repeat(cnt, 1)``) as one
 * launch each with a fixed summation order (csrc/scene_rows.hip; torch's multi-workgroup reduction is not replay-safe on this stack).
 * offset (scenes) int32 = the scenes' end rows; mean != 0: divide by the scene's row count (sum: the forward's mean / repeat: its backward). */
int pdf_scene_sum_rows(int scenes, const int *offset, int c, const float *x, long ldx, int mean, float *out, void *stream);
int pdf_scene_repeat_rows(int scenes, const int *offset, long n, int c, const float *rows, int mean, float *out, void *stream);

/* torch.nn.LayerNorm over the channel dim of (n, c) rows (StratifiedTransformer's norms: stratified_transformer_v1m1_origin.py:123-139,
 * 366-368, 566-569) as one pass per direction (csrc/layernorm.hip): forward saves mean / rstd (n each); backward writes gx, dgamma, dbeta
 * (partial: pdf_layernorm_partial_floats(n, c) floats; fixed summation order).  c % 4 == 0, c <= 512, 16-byte aligned pointers. */
int pdf_layernorm_supported(int c);
long pdf_layernorm_partial_floats(long n, int c);
int pdf_layernorm_forward(long n, int c, const float *x, const float *gamma, const float *beta, float eps, float *y, float *mean,
                          float *rstd, void *stream);
int pdf_layernorm_backward(long n, int c, const float *gy, const float *x, const float *mean, const float *rstd, const float *gamma,
                           float *gx, float *partial, float *dgamma, float *dbeta, void *stream);

/* Staging copy for hipGraph replay (pointcloudpdf_amd/engine.py: CapturedStep; no reference counterpart -- the reference issues its
 * step from Python): nseg (src -> dst, nbytes) segments in ONE launch.  src_offset (device int32, may be NULL): element offset (4-byte
 * units) added to src, read on the device; every 4-byte element has sub_const + *sub (device int32, may be NULL) subtracted. */
#define PDF_COPY_MAX_SEGS 72
typedef struct PdfCopySeg {
    const void *src;
    void *dst;
    long nbytes;            /* multiple of 4 */
    const int *src_offset;
    const int *sub;
    int sub_const;
    int src_elems;          /* > 0: number of 4-byte elements of the array src points into (reads of a device-offset window are clamped) */
} PdfCopySeg;
int pdf_stage_copy(int nseg, const PdfCopySeg *segs, void *stream);

/* ---- PointTransformer-V2 (point_transformer_v2m2_base.py): partition pooling / unpooling (csrc/grid_pool.hip) and the grouped vector
 * attention core (csrc/gva.hip).  No float atomics, fixed summation orders, nothing allocated.
 * pdf_grid_pool_partition (:244-264): key = cell id of voxel_grid(coord - lo[scene], size, start = 0) -- fp32 subtraction, torch's fp32
 *   floor division, x fastest, scene slowest, extents from the batch-wide maximum -- as int64; stable ascending sort (two 32-bit radix
 *   sorts) -> cluster (n) int64 = rank of the point's key among the distinct keys, sorted (n) int32 = the sort order (ties in point
 *   order), idx_ptr int32: n + 1 entries allocated, count[0] + 1 written, count (1) int32 = number of clusters.  xyz (n, 3); ends (scenes)
 *   int32 ascending scene ends; lo / hi (scenes, 3) from pdf_scene_bounds; workspace: pdf_grid_pool_workspace_bytes(n) bytes, 256-byte
 *   aligned.  n < 1, n >= 2^31 - 2, size <= 0, a null pointer: PDF_ERR_BAD_ARG before any launch.
 * pdf_grid_pool_reduce (:265-266): coord_out (m, 3) = segment mean (rows added in ascending sorted position in fp32, one fp32 division);
 *   feat_out (m, c) = segment max, arg_out (m, c) int32 = the fine row that holds it (first in point order wins a tie).  The coordinate
 *   pair and the feature triple are each optional (all NULL).
 * pdf_grid_pool_max_backward: grad_in (n, c)[i, ch] = grad_out[cluster[i], ch] where arg[cluster[i], ch] == i, else 0.
 * pdf_grid_unpool_forward (:308-309): out (n, c) = x (m, c)[cluster]; its backward is pdf_seg_sum_rows over (idx_ptr, sorted, base 0). */
long pdf_grid_pool_workspace_bytes(long n);
int pdf_grid_pool_partition(long n, const float *xyz, const int *ends, int scenes, const float *lo, const float *hi, float size,
                            long long *cluster, int *sorted, int *idx_ptr, int *count, void *workspace, void *stream);
int pdf_grid_pool_reduce(long n, long m, int c, const float *xyz, const float *feat, const int *idx_ptr, const int *sorted,
                         float *coord_out, float *feat_out, int *arg_out, void *stream);
int pdf_grid_pool_max_backward(long n, long m, int c, const float *grad_out, const long long *cluster, const int *arg, float *grad_in,
                               void *stream);
int pdf_grid_unpool_forward(long n, long m, int c, const float *x, const long long *cluster, float *out, void *stream);
/* Grouped vector attention (:109-129).  idx (n, s) int32 with values in [-1, nk): a negative entry reads a zero key row and is masked
 * AFTER the softmax (no renormalisation).  inv_off (nk + 1) / inv_entry: the inverse of idx in pdf_seg_sum_rows' table form, base 0.
 * relation: rel (n, s, c) = (key[idx] - query[n]) * pem + peb, pem / peb (n, s, c) or NULL; backward: g_query = - sum_s g_rel * pem,
 *   g_key = inverse-segment sums of g_rel * pem, g_pem = g_rel * (key[idx] - query) (each output nullable; g_peb is g_rel itself).
 * attend (c = 8 * groups, s <= 64: pdf_gva_supported, else PDF_ERR_UNSUPPORTED): p (n, s, groups) = softmax over s of the logits,
 *   out (n, c)[n, 8 g + j] = sum_s p * [idx >= 0] * (value[idx] + peb); backward: g_logits = p * (m d - sum_t p_t m_t d_t) with
 *   d = <g_out[n, group], value[idx] + peb>, g_value = inverse-segment sums of p * g_out, g_peb = p * m * g_out (the last two nullable). */
int pdf_gva_supported(int c, int groups, int s);
int pdf_gva_relation_forward(long n, long nk, int s, int c, const float *query, const float *key, const int *idx, const float *pem,
                             const float *peb, float *rel, void *stream);
int pdf_gva_relation_backward(long n, long nk, int s, int c, const float *g_rel, const float *query, const float *key, const int *idx,
                              const float *pem, const int *inv_off, const int *inv_entry, float *g_query, float *g_key, float *g_pem,
                              void *stream);
int pdf_gva_attend_forward(long n, long nv, int s, int c, int groups, const float *logits, const float *value, const float *peb,
                           const int *idx, float *out, float *p, void *stream);
int pdf_gva_attend_backward(long n, long nv, int s, int c, int groups, const float *g_out, const float *p, const float *value,
                            const float *peb, const int *idx, const int *inv_off, const int *inv_entry, float *g_logits, float *g_value,
                            float *g_peb, void *stream);

/* ---- PointTransformer-V3 (point_transformer_v3m1_base.py): serialization, code-shift pooling partition (csrc/serialization.hip) and
 * the patch attention over serialized order (csrc/serial_attention.hip).
 * pdf_serial_codes: code (k, n) int64, row j = batch << 3 depth | curve_j(grid_coord & (2^depth - 1)); the curve of row j is the 4-bit
 *   field j of `orders`: 0 z, 1 z-trans (x and y swapped), 2 hilbert, 3 hilbert-trans -- bit-identical to
 *   models/utils/serialization/{z_order,hilbert}.py (Skilling's transform per lane, no table).  1 <= k <= 8, 0 <= depth <= 16.
 * pdf_serial_sort: order (k, n) int64 = stable ascending order of every code row (two stable 32-bit radix sorts, low word first; equal
 *   codes keep row order), inverse (k, n) int64 with inverse[j, order[j, i]] = i.  workspace: pdf_serial_workspace_bytes(n), 256-byte aligned.
 * pdf_serial_pool_partition (SerializedPooling :384-396): key = code0[order0[i]] >> shift is ascending in i, so one flag + scan pass gives
 *   cluster (n) int64 = rank of the row's key among the distinct keys, idx_ptr (count + 1 of n + 1 written) int32, sorted (n) int32 = the rows
 *   cluster by cluster in ASCENDING ROW INDEX inside a cluster (what a stable sort of cluster yields), head (count of n written) int64 = the
 *   first of them, count (1) int32.  Same workspace.
 * pdf_serial_attn_*: qkv (n, 3 c) fp32 rows in original order [q | k | v], head h' = columns 16 h' .. 16 h' + 15 of each third; order (n)
 *   int64 = the serialized order; qtab (nq, 4) int32 {q_start, q_len <= 64, k_start, k_len}: the queries at serialized positions
 *   [q_start, q_start + q_len) attend to the keys at [k_start, k_start + k_len); ktab (nk, 8) int32 {k_start, k_len <= 64, qa_start, qa_len,
 *   qb_start, qb_len, shared_from, 0}: the keys of the chunk receive the queries of window a, then those of window b for the keys at
 *   positions >= shared_from (fixed order, no float atomics).  The q windows and the key chunks each partition [0, n): every element of
 *   out (n, c), lse (n, h, 2), delta (n, h) and g_qkv (n, 3 c) is written exactly once.  out = softmax(scale q k^T) v per head in fp32 on
 *   v_mfma_f32_16x16x4_f32 with an online softmax; lse = the row's log-sum-exp as the pair (m, l): row maximum and sum of exp(s - m).  Shapes outside pdf_serial_attn_supported (c == 16 h,
 *   c <= 512, k >= 1): PDF_ERR_UNSUPPORTED.  A table row that points outside [0, n) is skipped. */
int pdf_serial_attn_supported(int c, int h, int k);
long pdf_serial_workspace_bytes(long n);
int pdf_serial_codes(long n, int k, int orders, int depth, const int *grid_coord, const long long *batch, long long *code, void *stream);
int pdf_serial_sort(long n, int k, const long long *code, long long *order, long long *inverse, void *workspace, void *stream);
int pdf_serial_pool_partition(long n, int shift, const long long *code0, const long long *order0, long long *cluster, int *sorted,
                              int *idx_ptr, long long *head, int *count, void *workspace, void *stream);
int pdf_serial_attn_forward(long n, int c, int h, float scale, const float *qkv, const long long *order, const int *qtab, int nq,
                            float *out, float *lse, void *stream);
int pdf_serial_attn_backward(long n, int c, int h, float scale, const float *qkv, const float *out, const float *lse, const float *g_out,
                             const long long *order, const int *qtab, int nq, const int *ktab, int nk, float *delta, float *g_qkv,
                             void *stream);

/* ---- PointGroup (PG-v1m1: libs/pointgroup_ops, point_group_v1m1_base.py, InsSegEvaluator): csrc/point_group.hip.
 * Ball table (ballquery_batch_p as CSR): row q = the points of q's scene in ASCENDING index with d2 < radius^2 (strict; fp32, the as-written
 *   expression of the reference, the arithmetic of pdf_dist_fma_mode()), cut after the first 1,000.  offset (b) = scene ends, b <= 64
 *   (else PDF_ERR_UNSUPPORTED).  pdf_pg_ball_count writes start_len (n, 2) int32 = {exclusive scan of the row lengths in row order, length}
 *   and total (1) int64 on the device; the caller reads total, allocates idx (total) and calls pdf_pg_ball_fill with the SAME, untouched
 *   workspace (pdf_pg_ball_workspace_bytes(n, b), 256-byte aligned).  total >= 2^31: PDF_ERR_UNSUPPORTED (start_len is int32, as upstream).
 * Clustering (bfs_cluster): pdf_pg_cluster_labels runs directed min-label propagation over the equal-label edges to its fixed point
 *   (rounds in batches, one host read per batch, at most n + 1 rounds, else PDF_ERR_NOT_CONVERGED; synchronises the stream) and reads the
 *   clusters off: L (n) = smallest index that reaches the point, size (n) = class sizes at the roots, rank (n) = cluster number of a kept
 *   root (size >= threshold; ascending root index) or -1, offs (n + 1, count + 1 written) = cluster offsets, code (n) int64 = the point's
 *   cluster number or n, info (3) int64 = {clusters, points in clusters, rounds}, counters (64) = scratch.  The caller sorts `code` stably
 *   (pdf_serial_sort) and pdf_pg_cluster_fill writes cluster_idxs (s, 2) int32 = {cluster, point}: members in ascending index.
 * Proposals (point_group_v1m1_base.py:140-170): pdf_pg_proposals_select keeps the clusters with more than propose_points members: rank (nc) =
 *   proposal number or -1, new_offs (kept + 1 written), info (2) int64 = {kept, their members}; pdf_pg_proposals_fill writes, per kept cluster
 *   (cluster_idxs (ns, 2); a cluster whose offsets leave it is skipped),
 *   members (object_idxs[member], or the member itself with object_idxs == NULL; int32 indices into the npts points), prop_of[member] = proposal,
 *   classes (int64) = label[first member], scores = mean over the members of prob[member, class] (prob (npts, k) fp32; double accumulator,
 *   fixed order), and masks (kept, npts) int32 = 1 at the members when masks != NULL (zeroed by the caller, as prop_of is set to -1).
 * pdf_pg_intersections: for the m evaluated points j with p = prop_of[map ? map[j] : j] >= 0: table[p, slot[j]] += 1 (table (np, g), slots
 *   outside [0, g) skipped), vert[p] += 1, voidc[p] += isvoid[j] (bytes); integer atomics, outputs zeroed by the caller.
 * Bias losses (:74-86): loss (2) = {bias_l1_loss, bias_cosine_loss} in fp32, or in double with a float64 centroid (centroid_f64 != 0); d1, d2
 *   (n, 3) fp32 = the unscaled gradients of the two terms, acc = pdf_pg_bias_loss_workspace_doubles() doubles (nothing to zero; acc[0] = 1 /
 *   denominator).  Backward: grad = (d1 gy[0] + d2 gy[1]) acc[0], gy (2) of the loss' type.  Capturable: no host read, no memset, no atomics. */
long pdf_pg_ball_workspace_bytes(int n, int b);
int pdf_pg_ball_count(int n, int b, float radius, const float *xyz, const int *offset, int *start_len, long long *total, void *workspace,
                      long workspace_bytes, void *stream);
int pdf_pg_ball_fill(int n, int b, float radius, const float *xyz, const int *offset, const int *start_len, long total, int *idx,
                     void *workspace, long workspace_bytes, void *stream);
int pdf_pg_cluster_labels(int n, const int *label, const int *idx, long total, const int *start_len, int threshold, int *L, int *size, int *rank,
                          int *offs, long long *code, long long *info, unsigned *counters, void *stream);
int pdf_pg_cluster_fill(long n, long s, const long long *code, const long long *order, int *cluster_idxs, void *stream);
int pdf_pg_proposals_select(int nc, const int *offs, int propose_points, int *rank, int *new_offs, long long *info, void *stream);
int pdf_pg_proposals_fill(int nc, long npts, int k, long ns, const int *cluster_idxs, const int *offs, const int *rank, const int *new_offs,
                          const int *label, long nobj, const long long *object_idxs, const float *prob, int *members, int *prop_of,
                          long long *classes, float *scores, int *masks, void *stream);
int pdf_pg_intersections(long m, long nsrc, int np, int g, const int *prop_of, const long long *map, const int *slot,
                         const unsigned char *isvoid, int *table, int *vert, int *voidc, void *stream);
long pdf_pg_bias_loss_workspace_doubles(void);
int pdf_pg_bias_loss_forward(long n, const float *pred, const float *coord, const void *centroid, int centroid_f64, const long long *instance,
                             long long ignore, float *d1, float *d2, double *acc, void *loss, void *stream);
int pdf_pg_bias_loss_backward(long n, const float *d1, const float *d2, const double *acc, const void *gy, int f64, float *grad, void *stream);

/* ---- csrc/scene_contrast.hip: MSC-v1m1 (pointcept/models/masked_scene_contrast/masked_scene_contrast_v1m1_base.py) -------------------------
 * Matched-pair InfoNCE (:174-203) without a (p, p) array.  feat1 (n1, c), feat2 (n2, c) fp32, match (p, 2) int64 = rows of the two views
 * (an index outside its view acts as a zero row and receives no gradient), c a multiple of 32 up to 256 (pdf_msc_nce_supported), p >= 1.
 * Forward: out (3) = {loss = mean_i(lse_i - s_ii / t), pos_sim = mean_i s_ii, neg_sim = mean_i mean_j s_ij - pos_sim / p} with
 *   S = A^ B^T, A^ = a / (|a| + 1e-7) over the gathered rows; saved = pdf_msc_nce_saved_floats(p, c) floats (A^, B^, norms, lse: what the
 *   backward reads), workspace = pdf_msc_nce_workspace_bytes(p, c, 0) bytes, 256-byte aligned, nothing to zero.
 * Backward: g1 (n1, c), g2 (n2, c) = gy[0] * d loss / d feat, every row written (zeros where no pair points); a row matched by several
 *   pairs adds them in ascending pair order; workspace = pdf_msc_nce_workspace_bytes(p, c, 1) bytes.  No atomics, no memset, no host read:
 *   the order of every sum is a function of p and c. */
int pdf_msc_nce_supported(int c);
long pdf_msc_nce_saved_floats(long p, int c);
long pdf_msc_nce_workspace_bytes(long p, int c, int backward);
int pdf_msc_nce_forward(long p, int c, long n1, long n2, const float *feat1, const float *feat2, const long long *match, float temperature,
                        float *saved, float *out, void *workspace, long workspace_bytes, void *stream);
int pdf_msc_nce_backward(long p, int c, long n1, long n2, const float *feat1, const float *feat2, const long long *match, float temperature,
                         const float *saved, const float *gy, float *g1, float *g2, void *workspace, long workspace_bytes, void *stream);
/* Masked reconstruction head (:274-307) over both views: pred = feat weight^T + bias (weight (3, c), c as above) on the rows whose mask
 * byte is set; kind 0 (color): term = sum (pred - target)^2, kind 1 (normal): term = sum pred / (|pred| + 1e-10) * target;
 * loss (1) = sum of the terms / masked rows (NaN without one).  dpred (n1 + n2, 3) = d term / d pred of the masked rows, acc =
 * pdf_msc_recon_acc_doubles() doubles (acc[0] = 1 / masked rows), both read by the backward: g1, g2 = d feat (zero rows where unmasked),
 * gw (3, c), gb (3) from per-workgroup slabs (slab: pdf_msc_recon_slab_floats(n1 + n2, c) floats) added in slab order.  gy (1) on the device. */
int pdf_msc_recon_supported(int c);
long pdf_msc_recon_acc_doubles(void);
long pdf_msc_recon_slab_floats(long n, int c);
int pdf_msc_recon_forward(long n1, long n2, int c, int kind, const float *feat1, const float *feat2, const unsigned char *mask1,
                          const unsigned char *mask2, const float *weight, const float *bias, const float *target1, const float *target2,
                          float *dpred, double *acc, float *loss, void *stream);
int pdf_msc_recon_backward(long n1, long n2, int c, const float *feat1, const float *feat2, const unsigned char *mask1, const unsigned char *mask2,
                           const float *weight, const float *dpred, const double *acc, const float *gy, float *g1, float *g2, float *gw, float *gb,
                           float *slab, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PDFOPS_H */
