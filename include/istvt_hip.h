/*
 * istvt_hip.h — C ABI of libistvt_hip.so, the MI355X (gfx950) kernels behind the ISTVT
 * video-clip forward/backward hot path.
 *
 * The reference (Vill-Lab/2023-TIFS-ISTVT) is pure PyTorch: it has no FFI for this path; its
 * "interface" is the chain of torch ops inside network/xception.py, network/vivit/module.py
 * and network/vivit/vivit.py.  Each entry point below names the reference ops it replaces
 * (file:line into /root/reference).  INTEGRATION.md shows the ctypes stubs that bind them.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer owned by the caller (PyTorch allocates everything);
 *     kernels never allocate, free, or retain pointers, and only enqueue on `stream`
 *     (istvt_stream_t is HIP's own hipStream_t, spelled out below so that this header needs no HIP include and stays
 *     valid C; no host synchronisation).  libistvt_hip.so is compiled against this header: a definition that
 *     disagrees with its prototype here does not build.
 *   - `dtype`: storage type of activations: 0 = float32 (parity mode), 1 = bfloat16.
 *     Parameters, statistics, parameter gradients and all accumulation are float32.
 *   - return value: ISTVT_OK (0); ISTVT_ERR_DTYPE (-2) = bad dtype; ISTVT_ERR_SHAPE (-3) = bad shape/argument;
 *     ISTVT_ERR_LAUNCH (-4) = the runtime refused to prepare a launch (a kernel's dynamic-LDS limit could not be raised);
 *     -(1000+e) = hipError_t e raised by the launch.  Nothing throws, nothing exits.
 *   - "accumulate" outputs (parameter gradients) are added to, so the caller zeroes them
 *     (they are the .grad buffers).
 *   - row-major everywhere; activations of the transformer are [M = B*F*P][D] with rows
 *     ordered (clip b, frame f, token p); stem activations are NHWC [frames][H][W][C].
 *   - `ld*` arguments are row strides in ELEMENTS (>= the row width, multiples of 8).  The host
 *     keeps transformer activations and the bf16 GEMM operand copies of the weights with rows
 *     padded so that every row starts on a 128-byte line and spans an ODD number of lines
 *     (ops.pad_ld: 728 -> 832, 2912 -> 3008, 512 -> 576, 1536 -> 1600 elements): the LDS-DMA
 *     staging of the GEMMs is priced per cache line touched (tools/dma_probe.hip), and with an
 *     even line count the rows of a column panel fall on half of the memory channels.  The
 *     kernels only require 16-byte aligned rows; pad columns are never read as data and never
 *     written.
 */
#ifndef ISTVT_HIP_H
#define ISTVT_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ihipStream_t* istvt_stream_t; /* HIP's definition of hipStream_t */

#define ISTVT_OK 0
#define ISTVT_ERR_DTYPE (-2)
#define ISTVT_ERR_SHAPE (-3)
#define ISTVT_ERR_LAUNCH (-4)

#define ISTVT_F32 0
#define ISTVT_BF16 1

/* ---- GEMM with fused epilogue -------------------------------------------------------------
 * C[m][n] = epi(alpha * sum_k A(m,k) B(n,k)) ; a_kc/b_kc = 1: operand stored [rows][K]
 * (K contiguous), 0: stored [K][rows].
 * Replaces nn.Linear (module.py:27,30,74,77,182,183,186; vivit.py:129), 1x1 convs
 * (xception.py:44,57) and the im2col'd 3x3 convs (xception.py:118,122): forward (1,1),
 * input gradient (1,0) and weight gradient (0,0).
 * bias: float[N] or NULL.  residual: T[M][ldr] or NULL (added after activation handling).
 * epi: 0 none; 1 GELU forward (exact erf, module.py:28): C = pre-activation, C2 = gelu;
 *      2 GELU backward: C = acc * gelu'(C2).
 * out_mode: 0 store T; 1 store float; 2 atomicAdd into float C; 3 split z stores its float partial
 *           at C + z*M*ldc (caller sums them with istvt_splitk_reduce).  splitk > 1 needs 2 or 3.
 * col_sum / col_sumsq (both or neither; NULL = off): replica-0 rows of a double[R][2][N] statistics accumulator (R =
 *           istvt_stats_replicas()); the kernel adds the per-column sum and sum of squares of the values it stores --
 *           the train-mode BatchNorm statistics of a 1x1 convolution's output (xception.py:44,57 -> :58,69,75) without a
 *           second pass.  Only the persistent bf16 NT kernel does this (forward of a >= 64-wide, 16-byte aligned
 *           problem with epi 0, no residual, out_mode 0); any other combination returns -3.
 *           col_sum alone (col_sumsq NULL) with epi 2: only the column sums -- the bias gradient of FeedForward's hidden
 *           layer (module.py:27), whose dy is exactly this GEMM's output; fold with istvt_stats_reduce_add.
 * flags:    bit 0 (float32 only): blocked summation -- every 32-deep step of the reduction is summed from zero and added
 *           to the running total, so the rounding error grows with 32 + K/32 terms instead of K (the transformer's
 *           Linears and every weight gradient use it: 10x closer to the float64 reference run on golden G5).  0 = one
 *           sequential fp32 FMA chain: the order that reproduces the reference CPU convolutions' ReLU / arg-max
 *           decisions in the Xception stem (forward and input gradient of its convolutions).
 *           bit 1 (bfloat16 forward on the persistent NT kernel only, -3 otherwise): A is TWO planes of M rows, the
 *           second directly behind the first (A + M * lda elements); output columns at or past 64 * (flags >> 16), a
 *           multiple of 256, take their rows from the second plane.  TemporalResidualAttention (module.py:193-196): q | k
 *           are projections of the frame-differenced LayerNorm output, v of the plain one -- one 728 -> 1536 GEMM.
 *           bit 4 (with epi 1 or 2, -3 otherwise): the GELU pair exchanges the DERIVATIVE instead of the pre-activation.
 *           epi 1 then stores C = gelu'(u) (computed from the fp32 u with the erf / exp of gelu itself), C2 = gelu(u); epi 2
 *           computes C = acc * C2 with C2 = that saved derivative.  FeedForward's backward (module.py:27-30) needs u for
 *           nothing else, so the same bytes carry what the backward would recompute per element; in float32 the result is
 *           bit-identical to the u form.
 *           bits 8..15: CUs, in units of 8 (at most 24 = 192 CUs, -3 otherwise), that a launch of the persistent NT kernel
 *           leaves free: set while a collective's kernels occupy CUs (the data-parallel gradient all-reduce that overlaps
 *           the stem backward, train_CNN.py:185-186 -> parallel.GradBucket), so that every persistent workgroup is resident
 *           at once instead of queueing behind a whole tile list.  An argument of each launch: the library keeps no state
 *           (results are bit-identical for every value: one workgroup computes an output tile in one fixed order). */
/* Smallest output edge (M and N of a bf16 forward, N_i and K_i of a weight gradient) that goes to the 256x256 LDS-DMA
 * kernels; the host routes by it too (weight copies, grouped weight gradients, workspace sizes). */
#define ISTVT_G256_MIN 64
int istvt_gemm(const void* A, long lda, int a_kc, const void* B, long ldb, int b_kc, void* C, long ldc, int M, int N,
               int K, const float* bias, const void* residual, long ldr, void* C2, int epi, int out_mode, int splitk,
               float alpha, double* col_sum, double* col_sumsq, int flags, int dtype, istvt_stream_t stream);

/* out[i] += sum_z ws[z*n + i]: second pass of a split-K weight gradient written as partial slabs */
int istvt_splitk_reduce(const float* ws, int splits, long n, float* out, istvt_stream_t stream);

/* Weight gradients of up to 8 nn.Linear layers in one launch pair (the eight of one transformer layer: module.py:27,30,
 * 74,77,182,183,186 as they come out of the backward pass): out_i[N_i][K_i] += dy_i^T x_i, dy_i bf16 [M][N_i] (row
 * stride lddy_i), x_i bf16 [M][K_i] (row stride ldx_i), out_i contiguous float.  The problems share the reduction
 * length M, so one grid of (tile, split) workgroups covers all of them with few reduction splits; ws: scratch of at
 * least splits * sum(N_i K_i) floats.  splits <= 0: chosen so that the grid fills the chip
 * (istvt_wgrad_group_splits returns that count, for sizing ws).  ISTVT_ERR_SHAPE when a problem is not one the
 * 256x256 bf16 weight-gradient kernel takes (N_i, K_i >= 64 and multiples of 8, 16-byte aligned rows). */
int istvt_wgrad_group(int count, const void* const* dy, const long* lddy, const void* const* x, const long* ldx,
                      float* const* out, const int* N, const int* K, int M, int splits, float* ws, long ws_elems,
                      istvt_stream_t stream);
int istvt_wgrad_group_splits(int count, const int* N, const int* K, int M);

/* ---- LayerNorm (module.py:15-21 PreNorm; vivit.py:89,128) ---------------------------------- */
int istvt_layernorm_fwd(const void* x, long ldx, const float* gamma, const float* beta, void* y, long ldy, float* mean,
                        float* rstd, long M, int D, float eps, int dtype, istvt_stream_t stream);
/* The same plus the frame difference of module.py:193 taken in fp32 before the rounding to the storage type:
 * diff[(b, f, p)] = y[(b, f, p)] for f < 2, y[(b, f, p)] - y[(b, f - 1, p)] for f >= 2; rows ordered (b, f, p). */
int istvt_layernorm_fwd_diff(const void* x, long ldx, const float* gamma, const float* beta, void* y, long ldy, void* diff,
                             long ldd, float* mean, float* rstd, int B, int F, int P, int D, float eps, int dtype,
                             istvt_stream_t stream);
/* dres (may be NULL) = gradient arriving through the residual connection, added to dx.  dgamma / dbeta accumulate.
 * dcol (may be NULL) accumulates the column sums of dx: the bias gradient of the nn.Linear whose output this LayerNorm
 * normalises (module.py:30,77,186).  ws: float scratch of >= istvt_layernorm_bwd_ws_elems(M, D) elements for the
 * per-workgroup partial sums; the parameter gradients are reduced in a fixed order (bit-reproducible, no atomics). */
int istvt_layernorm_bwd(const void* dy, long ld_dy, const void* x, long ld_x, const float* mean, const float* rstd,
                        const float* gamma, const void* dres, long ld_res, void* dx, long ld_dx, float* dgamma,
                        float* dbeta, float* dcol, float* ws, long ws_elems, long M, int D, int dtype,
                        istvt_stream_t stream);
int istvt_layernorm_bwd_ws_elems(long M, int D);
/* istvt_layernorm_bwd in two halves, for a caller that folds the partial rows off its critical path (another stream, or
 * later): _partial = the row kernel alone (dx, and the per-workgroup partial rows in ws; with_dcol: a third accumulator,
 * the column sums of dx), _reduce = the fixed-order fold of that ws into dgamma / dbeta (and dcol, non-NULL exactly when the
 * partial call had with_dcol).  Same arithmetic and order as the one-call form: bit-identical results. */
int istvt_layernorm_bwd_partial(const void* dy, long ld_dy, const void* x, long ld_x, const float* mean, const float* rstd,
                                const float* gamma, const void* dres, long ld_res, void* dx, long ld_dx, int with_dcol,
                                float* ws, long ws_elems, long M, int D, int dtype, istvt_stream_t stream);
int istvt_layernorm_bwd_reduce(const float* ws, long ws_elems, long M, int D, float* dgamma, float* dbeta, float* dcol,
                               istvt_stream_t stream);

/* ---- spatial attention (SpatialOnlyAttention.forward core, module.py:84-91) ---------------
 * qkv [BF*P][3*heads*dh] (q|k|v, 'b n (h d)') with row stride ldqkv (elements; also dqkv's), out / dout
 * [BF*P][heads*dh] with row stride ldo; lse [BF*P][heads][2] = softmax statistics (row max in the log2 domain,
 * 1/row sum).  Row strides are multiples of 8 elements; line-aligned, odd-line-count rows (ops.pad_ld) are what the
 * GEMMs on either side want. */
int istvt_attn_spatial_fwd(const void* qkv, long ldqkv, void* out, long ldo, float* lse, int BF, int P, int heads,
                           int dh, float scale, int dtype, istvt_stream_t stream);
int istvt_attn_spatial_bwd(const void* qkv, long ldqkv, const void* out, const void* dout, long ldo, const float* lse,
                           float* delta_scratch, void* dqkv, int BF, int P, int heads, int dh, float scale, int dtype,
                           istvt_stream_t stream);
/* fp8 variant of the two entry points above (BASELINE.json configs[4]; bfloat16 storage only): Q, K, V and the
 * softmax probabilities enter the attention MFMAs as OCP e4m3 (v_mfma_f32_16x16x32_fp8_fp8); softmax, statistics,
 * accumulation and the remaining backward products are unchanged.  Same arguments. */
int istvt_attn_spatial_fwd_fp8(const void* qkv, long ldqkv, void* out, long ldo, float* lse, int BF, int P, int heads,
                               int dh, float scale, int dtype, istvt_stream_t stream);
int istvt_attn_spatial_bwd_fp8(const void* qkv, long ldqkv, const void* out, const void* dout, long ldo, const float* lse,
                               float* delta, void* dqkv, int BF, int P, int heads, int dh, float scale, int dtype,
                               istvt_stream_t stream);

/* ---- temporal attention (TemporalResidualAttention.forward core, module.py:192-205) --------
 * qk [B*F*P][2*heads*dh] (q|k) with row stride ldqk (also dqk's); v / dv [B*F*P][heads*dh] with row stride ldv;
 * out / dout [B*F*P][heads*dh] with row stride ldo; rows (b,f,p); F <= 17 (float32), <= 32 (bfloat16).
 * qk and v may be column ranges of ONE [B*F*P][3*heads*dh] projection (v = qk + 2*heads*dh, ldv = ldqk).
 * diff != 0: q and k are the projections of the UN-differenced LayerNorm output; the kernels take the frame
 * difference of module.py:193 on them (q'[f] = q[f] - q[f-1] for f >= 2; exact because to_qk has no bias,
 * module.py:182) and the backward returns gradients with respect to the un-differenced rows.  diff == 0: plain
 * attention over frames (TemporalOnlyAttention, module.py:145-172).  diff == 2 (bfloat16 only, -3 otherwise): q and k
 * ARRIVE differenced (projections of istvt_layernorm_fwd_diff's second output: the reference's own order, the rounding
 * to bfloat16 at the magnitude of the difference); the forward is plain attention, the backward returns dq, dk with
 * respect to the UN-differenced projections (d q[f] = d q'[f] - d q'[f+1] for f >= 1) so that one input-gradient GEMM
 * over [dq | dk | dv] follows as with diff == 1. */
int istvt_attn_temporal_fwd(const void* qk, long ldqk, const void* v, long ldv, void* out, long ldo, int B, int F, int P,
                            int heads, int dh, float scale, int diff, int dtype, istvt_stream_t stream);
int istvt_attn_temporal_bwd(const void* qk, long ldqk, const void* v, long ldv, const void* dout, long ldo, void* dqk,
                            void* dv, int B, int F, int P, int heads, int dh, float scale, int diff, int dtype,
                            istvt_stream_t stream);

/* ---- relevance maps: gradient-weighted attention rollout (DESIGN.md "Relevance maps") -------------------------
 * One rollout step r_out[j] = r[j] + (1/H) sum_h sum_i r[i] max(0, A_h[i, j] dA_h[i, j]) with A the softmax output and
 * dA = dO V^T its gradient; fp32 r / r_out, r_out != r.  Spatial: per frame (r, r_out [BF][P]); qkv / ldqkv / lse as
 * istvt_attn_spatial_fwd wrote them, dout [BF*P][heads*dh] with row stride ldo; P recomputed from lse.  Temporal: per
 * (clip, position) (r, r_out [B*P][F], F <= 17); qkv [B*F*P][3*heads*dh] (q|k|v), the softmax recomputed in full with
 * the forward's diff code (0, 1, 2).  dh in {32, 64}. */
int istvt_attn_spatial_relevance(const void* qkv, long ldqkv, const void* dout, long ldo, const float* lse, const float* r,
                                 float* r_out, int BF, int P, int heads, int dh, float scale, int dtype, istvt_stream_t stream);
int istvt_attn_temporal_relevance(const void* qkv, long ldqkv, const void* dout, long ldo, const float* r, float* r_out, int B,
                                  int F, int P, int heads, int dh, float scale, int diff, int dtype, istvt_stream_t stream);
/* cam [maps][g][g] fp32 -> out [maps][g*s][g*s] fp32: bilinear upsampling (align_corners=False) by the integer factor s,
 * then (x - min) / (max - min) per map (visualize_rel.py:262-265).  g <= 64. */
int istvt_relevance_heatmap(const float* cam, float* out, int maps, int g, int s, istvt_stream_t stream);
/* Whole videos (DESIGN.md "Explaining whole videos"): the rollouts of W sliding windows, r_s [W][T+1][P], r_t [W][P][T+1],
 * logits [W][nc], fused per frame.  starts int32 [W] on the device: first frame of every window, ascending, 0 <= s <= N - T
 * (validated by the caller).  Window w covers frame n as its frame t = n - starts[w] when 0 <= t < T.  Per frame, the plain
 * mean over the covering windows in ascending window order of r_s[w][t+1][1..] (frame_s [N][P-1]), r_t[w][1..][t+1]
 * (frame_t [N][P-1]), r_t[w][0][t+1] (frame_weight [N]) and logits[w][index] (frame_logit [N]); count int32 [N] the number
 * of covering windows, a frame without one gets zeros.  One writer per element, fixed order, no atomics. */
int istvt_relevance_fuse_windows(const float* r_s, const float* r_t, const float* logits, const int* starts, float* frame_s,
                                 float* frame_t, float* frame_weight, float* frame_logit, int* count, int W, int T, int P,
                                 int nc, int index, int N, istvt_stream_t stream);
/* The heat map on the frame (visualize_rel.py:39-44) for N frames: frames uint8 [N][S][S][3], maps fp32 [N][g][g], lut uint8
 * [256][3] -> out uint8 [N][g*s][g*s][3].  m = istvt_relevance_heatmap's value, k = trunc(255 m) (k = 0 for a constant
 * map), cam = lut[k] / 255 + frame / 255 (the frame sampled bilinearly with half-pixel centres when S != g*s),
 * out = trunc(255 cam / max of cam over the frame).  ws: 4 floats of scratch per frame.  g <= 64, N <= 65535. */
int istvt_relevance_overlay_u8(const void* frames, const float* maps, const void* lut, float* ws, void* out, int N, int S,
                               int g, int s, istvt_stream_t stream);
/* A set of videos (DESIGN.md "Scoring a set of videos").  logits fp32 [W][nc], the windows of V videos one after the other;
 * offsets int32 [V+1] on the device: video v owns the windows [offsets[v], offsets[v+1]), 0 = offsets[0] < ... <
 * offsets[V] = W (validated by the caller; the kernel forces the table into [0, W]) -> logit_mean, prob_mean fp32 [V][nc]:
 * the mean of the video's logits and of 1 / (1 + exp(-logit)) (fp32).  One workgroup per video, every lane sums a strided
 * share of the windows in ascending order in fp64, the lane partials are added in lane order and the mean is rounded once
 * to fp32.  One writer per element, no atomics. */
int istvt_windows_reduce(const float* logits, const int* offsets, float* logit_mean, float* prob_mean, int W, int V, int nc,
                         istvt_stream_t stream);
/* scores fp32 [V], labels int32 [V] (0: negative, anything else: positive) -> counts int64 [6] = greater, equal, positives,
 * negatives, nonfinite, correct and auc fp64 [1] = (greater + equal / 2) / (positives * negatives), NaN when a class is
 * empty.  greater / equal: the (positive, negative) pairs with s_p > s_n / s_p == s_n in which both scores are finite; a
 * video with a NaN or infinite score is in `nonfinite`, in its class's count, in no pair and never correct.  correct:
 * (score > threshold) == positive.  Two launches: 256 videos per workgroup against all videos, six 64-bit counts per
 * workgroup into ws (ws_elems >= 6 * ceil(V / 256) 8-byte elements of caller-owned scratch), then one workgroup sums them.
 * Integer counts: exact, independent of order, no atomics. */
int istvt_auc_pairs(const float* scores, const int* labels, float threshold, void* ws, long ws_elems, long long* counts,
                    double* auc, int V, istvt_stream_t stream);

/* ---- token assembly (DSTTr.forward, vivit.py:133-142) -------------------------------------- */
int istvt_tokens_fwd(const void* feats, const float* space, const float* temporal, const float* pos, void* x, long ldx,
                     int B, int F, int P, int D, int pos_rows, int dtype, istvt_stream_t stream);
/* The same assembly for W sliding windows over one video (inference, forward only): bank [cap][P-1][D] (dtype) holds one
 * feature map per frame, idx int32 [W][F-1] names the bank slot of every frame of every window (0 <= idx < cap, validated by
 * the caller; a slot outside the bank contributes zero).  Bit-identical to istvt_tokens_fwd on the windows copied out. */
int istvt_tokens_gather_fwd(const void* bank, const int* idx, const float* space, const float* temporal, const float* pos,
                            void* x, long ldx, int W, int F, int P, int D, int pos_rows, int cap, int dtype,
                            istvt_stream_t stream);
/* dspace / dtemporal / dpos accumulate; ws = float scratch of (P + F - 1) * D elements (per-workgroup partial rows of the
 * two token gradients, folded in a fixed order: no floating-point atomics) */
int istvt_tokens_bwd(const void* dx, long lddx, void* dfeats, float* dspace, float* dtemporal, float* dpos, float* ws,
                     int B, int F, int P, int D, int pos_rows, int dtype, istvt_stream_t stream);

/* frame difference of module.py:193 (adjoint = 1: its transpose, for the backward) */
int istvt_frame_diff(const void* x, void* out, int B, int F, int P, int D, int adjoint, int dtype,
                     istvt_stream_t stream);

/* ==== Xception entry flow (network/xception.py:193-206), NHWC activations [frames][H][W][C] ====
 * A finalized BatchNorm travels as ONE device pointer `bnp` to a float[4][C] pack
 * {mean, rstd, scale = gamma*rstd, beta}; consumers apply z = (u - mean)*scale + beta. */

/* Per-channel statistics accumulators are double[R][2][C] with R = istvt_stats_replicas(): producers
 * (bn_stats, bn_bwd_stats, the fused sums of dwconv3x3) take pointers to replica 0's two rows and add
 * into replica (workgroup % R) to spread same-address atomics; istvt_stats_reduce folds replicas
 * 1..R-1 into replica 0, which finalize / bwd_apply then read. */
int istvt_stats_replicas(void);
int istvt_stats_reduce(double* acc, int C, istvt_stream_t stream);
/* out[c] += sum over the replicas of row 0: folds column sums accumulated by istvt_gemm(col_sum, NULL) into a float gradient */
int istvt_stats_reduce_add(const double* acc, int C, float* out, istvt_stream_t stream);

/* train-mode nn.BatchNorm2d (xception.py:58,69,75,119,123): sum/sumsq = rows 0/1 of replica 0 */
int istvt_bn_stats(const void* x, double* sum, double* sumsq, long M, int C, int dtype, istvt_stream_t stream);
/* use_batch=1: batch statistics (+ running-stat update, momentum/unbiased var as torch);
 * use_batch=0: running statistics (eval mode).  Writes the pack. */
int istvt_bn_finalize(const double* sum, const double* sumsq, double count, const float* gamma, const float* beta,
                      float* running_mean, float* running_var, float momentum, float eps, float* bnp, int C,
                      int use_batch, int update_running, istvt_stream_t stream);
int istvt_bn_apply(const void* x, const float* bnp, void* y, long M, int C, int relu, int dtype,
                   istvt_stream_t stream);
/* s1 += sum dz, s2 += sum dz*xhat (double[C]);  du = gamma*rstd*(dz - s1/M - xhat*s2/M), dgamma += s2, dbeta += s1 */
int istvt_bn_bwd_stats(const void* dz, const void* u, const float* bnp, double* s1, double* s2, long M, int C,
                       int dtype, istvt_stream_t stream);
/* batch_stats = 0: eval-mode BatchNorm (running statistics are constants): du = gamma*rstd*dz */
int istvt_bn_bwd_apply(const void* dz, const void* u, const float* bnp, const float* gamma, const double* s1,
                       const double* s2, void* du, float* dgamma, float* dbeta, long M, int C, int batch_stats,
                       int dtype, istvt_stream_t stream);
/* The BatchNorm-backward apply above, the 1x1 convolution's input gradient and its weight gradient in one pass (bf16;
 * (Cin, Cout) = (64, 128) or (128, 128), anything else is ISTVT_ERR_SHAPE and nothing is touched):
 *   du = bn_bwd_apply(dz, u) [M][Cout] (never stored), dd [M][Cin] = du . W, wgrad_out [Cout][Cin] += du^T . d.
 * d [M][ldd], wt = W^T [Cin][ldwt], dd contiguous; ws = caller-owned float workspace of istvt_pw_bwd_grid(M) slabs of
 * Cout * Cin, summed in slab order into wgrad_out (istvt_splitk_reduce): two runs give the same bits, and they are the bits
 * of the split-K weight gradient istvt_gemm + istvt_splitk_reduce give on the stored du (same chunks of rows, same order).
 * Operands must be smaller than 2 GiB each.  istvt_pw_bwd_rows(): rows per block of a workgroup's chunk. */
int istvt_pw_bwd(const void* dz, const void* u, const float* bnp, const float* gamma, const double* s1, const double* s2,
                 const void* d, long ldd, const void* wt, long ldwt, void* dd, float* ws, float* wgrad_out,
                 float* dgamma, float* dbeta, long M, int Cin, int Cout, int batch_stats, int dtype,
                 istvt_stream_t stream);
int istvt_pw_bwd_grid(long M);
int istvt_pw_bwd_rows(void);
/* tail of a stride-1 Block (xception.py:91-100 without the MaxPool): out = bn_x(x) + (bns ? bn_s(skip) : skip) */
int istvt_bn_add_fwd(const void* x, const float* bnx, const void* skip, const float* bns, void* out, long M, int C,
                     int dtype, istvt_stream_t stream);

/* conv1 (3->32, 3x3, s2, p0; xception.py:118): NCHW float clip -> col[M][32] ((dy,dx,ci) + 5 zero cols); adjoint */
int istvt_im2col_conv1(const float* x, void* col, int frames, int S, int dtype, istvt_stream_t stream);
int istvt_col2im_conv1(const void* dcol, float* dx, int frames, int S, int dtype, istvt_stream_t stream);
/* conv2 (32->64, 3x3, p0; xception.py:122): NHWC source with optional BN pack (+ReLU) on load -> col[M][9*C];
 * adjoint gathers dcol and masks by relu'(bn(u)) */
int istvt_im2col3x3(const void* src, const float* bnp, int relu, void* col, int frames, int H, int W, int C,
                    int dtype, istvt_stream_t stream);
int istvt_col2im3x3(const void* dcol, const void* u, const float* bnp, void* dz, int frames, int H, int W, int C,
                    int dtype, istvt_stream_t stream);

/* The same two convolutions computed directly (no im2col matrix in HBM); xception.py:118-123,193-199.
 * conv1_fwd: x float [frames][3][S][S], w float [32][3][3][3] (conv1.weight as stored) -> u1 [frames*Ho*Wo][32] (dtype).
 * conv2_* are bf16 only: u1 = raw conv1 output [frames][H][W][32], bnp = bn1's finalized pack (ReLU implied),
 * w = bf16 [64][(dy,dx,ci)].  fwd -> u2 [frames][H-2][W-2][64]; dgrad: du2 -> dz1 [frames][H][W][32] masked by
 * relu'(bn1(u1)); wgrad: dw float [64][(dy,dx,ci)] += sum over pixels, slabs = caller-owned float workspace of
 * istvt_conv2_wgrad_slabs() * 64 * 288 elements. */
int istvt_conv1_fwd(const float* x, const float* w, void* u1, int frames, int S, int dtype, istvt_stream_t stream);
/* conv1 forward from decoded frames (inference, no weight gradient): x uint8 [frames][S][S][3], mean / std float [3];
 * every byte is normalised as v = (float(u) / 255 - mean[c]) / std[c], each operation rounded on its own, and the sums run in
 * istvt_conv1_fwd's order: u1 is bit-identical to istvt_conv1_fwd on the float tensor torch makes from the same bytes.
 * S <= 4096. */
int istvt_conv1_fwd_u8(const void* x, const float* mean, const float* std, const float* w, void* u1, int frames, int S,
                       int dtype, istvt_stream_t stream);
/* conv1 weight gradient: du1 [frames*Ho*Wo][32] (dtype; rounded to bf16 for the MFMA), x as above ->
 * dw float [32][32] +=, column k = ci*9 + dy*3 + dx (conv1.weight's own order; columns 27..31 unused);
 * slabs = caller-owned float workspace of istvt_conv1_wgrad_slabs() * 1024 elements.  Ho <= 128. */
int istvt_conv1_wgrad(const void* du1, const float* x, float* slabs, float* dw, int frames, int S, int dtype,
                      istvt_stream_t stream);
int istvt_conv1_wgrad_slabs(void);
/* conv1 from a VIEW of decoded frames (the training entry): x uint8 [frames][Hs][Ws][3], `total` bytes readable at x
 * (>= frames*Hs*Ws*3; nothing outside [x, x + total) is read, x needs no alignment); view int32 [frames][3] = (y0, x0,
 * flip) on the device, or null for (0, 0, 0): output pixel (y, x) of frame f is source pixel (y0 + y, x0 + (flip ?
 * S-1-x : x)), 3 <= S <= min(Hs, Ws), channel order kept.  Bytes are normalised as in istvt_conv1_fwd_u8.  Each gives the
 * bits of its float twin (istvt_conv1_fwd / istvt_conv1_wgrad / istvt_im2col_conv1) on the float32 NCHW tensor the host
 * makes of the view, ((u / 255) - mean) / std.  conv1_wgrad_u8: slabs and limit (Ho <= 128) as istvt_conv1_wgrad. */
int istvt_conv1_fwd_u8_view(const void* x, long total, int Hs, int Ws, const int* view, const float* mean,
                            const float* std, const float* w, void* u1, int frames, int S, int dtype, istvt_stream_t stream);
int istvt_conv1_wgrad_u8(const void* du1, const void* x, long total, int Hs, int Ws, const int* view, const float* mean,
                         const float* std, float* slabs, float* dw, int frames, int S, int dtype, istvt_stream_t stream);
int istvt_im2col_conv1_u8(const void* x, long total, int Hs, int Ws, const int* view, const float* mean, const float* std,
                          void* col, int frames, int S, int dtype, istvt_stream_t stream);
/* Frames and boxes: frames uint8 [n][Hs][Ws][3] (`total` bytes readable at frames, >= n*Hs*Ws*3; nothing outside
 * [frames, frames + total) is read, no alignment needed), boxes int32 [n][4] = (y0, x0, h, w) on the device, every box
 * inside its frame with 1 <= h, w <= 8 S (the kernel forces a box that is not) -> out uint8 [n][S][S][3]: the box cut out
 * and resized as torch's interpolate(mode='bilinear', align_corners=False, antialias=True) resizes the cropped image --
 * per axis scale = n_in / S, sup = max(scale, 1), c = (i + 0.5) * scale, taps j in [max(int(c - sup + 0.5), 0),
 * min(int(c + sup + 0.5), n_in)) with w_j = max(0, 1 - |(j - c + 0.5) / sup|) divided by their sum; horizontal pass first,
 * kept in fp32, then vertical; byte = clamp(floor(v + 0.5), 0, 255).  h = w = S reproduces the slice.  S <= 480 (LDS). */
int istvt_crop_resize_u8(const void* frames, long total, int Hs, int Ws, const int* boxes, void* out, int n, int S,
                         istvt_stream_t stream);
/* NV12 frames: n frames of Hs rows of Y followed by Hs / 2 rows of Ws / 2 interleaved (Cb, Cr) pairs, uint8, `pitch` bytes
 * from row to row and `fstride` bytes from frame to frame (`total` bytes readable at frames, >= (n - 1) * fstride + (3 Hs / 2
 * - 1) * pitch + Ws; nothing outside is read, no alignment needed); Hs, Ws even, pixel (y, x) takes the pair (y >> 1,
 * x >> 1).  coef = (ky, yoff, krv, kgu, kgv, kbu) on the host, each in [0, 2^20), yoff <= 255; with Cb' = Cb - 128, Cr' =
 * Cr - 128 and yy = ky (Y - yoff), in int32: R = clamp((yy + krv Cr' + 32768) >> 16), G = clamp((yy - kgu Cb' - kgv Cr' +
 * 32768) >> 16), B = clamp((yy + kbu Cb' + 32768) >> 16), arithmetic shifts, clamp to 0..255.
 * istvt_nv12_to_rgb_u8 -> out uint8 [n][Hs][Ws][3] (contiguous, no alignment needed, no overlap with the frames).
 * istvt_crop_resize_nv12 -> out uint8 [n][S][S][3]: istvt_crop_resize_u8 (the same boxes, the same filter code) on those
 * RGB frames, bit for bit, without making them: only the Y and chroma bytes of the box rows are read.  S <= 480 (LDS). */
int istvt_nv12_to_rgb_u8(const void* frames, long total, int Hs, int Ws, long pitch, long fstride, const int* coef, void* out,
                         int n, istvt_stream_t stream);
int istvt_crop_resize_nv12(const void* frames, long total, int Hs, int Ws, long pitch, long fstride, const int* coef,
                           const int* boxes, void* out, int n, int S, istvt_stream_t stream);
/* Similarity warp (aligned crops): frames as istvt_crop_resize_u8 / istvt_crop_resize_nv12 take them, M float32 [n][2][3] on
 * the device -> out uint8 [n][S][S][3].  M[f] takes the centre of output pixel (ox, oy) to the continuous source point
 * c = M[f] (ox + .5, oy + .5, 1), source pixel j covering [j, j + 1).  With u = (m00, m10), v = (m01, m11), e1 = u / |u|,
 * e2 = v / |v|, s = sqrt|det|, sup = max(s, 1) and d = (jx + .5, jy + .5) - c, over every integer (jx, jy):
 * w = max(0, 1 - |d . e1| / sup) * max(0, 1 - |d . e2| / sup), value = sum w * frame[clamp(jy)][clamp(jx)] / sum w in double,
 * byte = clamp(floor(value + .5), 0, 255): the crop's antialiased triangle in the rotated frame of the output, the border
 * replicated.  An entry with a non-finite number, s outside [2^-6, 8], |u| or |v| outside [2^-7, 16] or the image of the
 * output centre (S / 2, S / 2) outside [0, Ws] x [0, Hs] gives a frame of zeros and reads nothing of its frame.
 * istvt_warp_similarity_nv12: the bits of istvt_warp_similarity_u8 on istvt_nv12_to_rgb_u8's frames, without making them. */
int istvt_warp_similarity_u8(const void* frames, long total, int Hs, int Ws, const float* M, void* out, int n, int S,
                             istvt_stream_t stream);
int istvt_warp_similarity_nv12(const void* frames, long total, int Hs, int Ws, long pitch, long fstride, const int* coef,
                               const float* M, void* out, int n, int S, istvt_stream_t stream);
/* Pasting relevance maps onto whole frames, IN PLACE: frames uint8 [n][Hs][Ws][3] (istvt_relevance_paste_u8; `total` bytes at
 * frames, >= n*Hs*Ws*3, no alignment needed) or NV12 as istvt_crop_resize_nv12 takes them (istvt_relevance_paste_nv12; pitch >=
 * Ws, frames that do not overlap); maps float32 [n][g][g], g <= 19; A double [n][2][3]: u = (a00 (sx + .5) + a01 (sy + .5)) +
 * a02, v likewise, take the centre of source pixel (sx, sy) to crop coordinates, the crop covering [0, S)^2; rect int32 [n][4] =
 * (y0, x0, h, w): where to look (clamped into the frame by the kernel, NV12: then aligned outward to even coordinates; nothing
 * outside it is read or written); lut uint8 [256][3]: R'G'B' for packed frames, (Y, Cb, Cr) for NV12; alpha float32 [n]; all on
 * the device.  Per frame, in double with one rounding per operation: mhat = (map - min) / (max - min) over the cells; in the
 * region 0 <= u, v < S: gu = u (g / S) - .5, x = floor(gu), fx = gu - x, cells clamped to [0, g - 1], a + fx (b - a) along x for
 * both rows and then along y: m; k = clamp(floor(255 m + .5), 0, 255), w = clamp(floor((256 alpha) m + .5), 0, 256), w = 0
 * outside the region.  Packed: out_c = (frame_c (256 - w) + lut[k][c] w + 128) >> 8.  NV12: Y likewise with lut[k][0]; per 2 x 2
 * block C_out = (C (1024 - sum w_i) + sum w_i lut[k_i][c] + 512) >> 10 for Cb (c = 1) and Cr (c = 2).  A frame whose map, A or
 * alpha holds a non-finite number is left untouched, as is one with a constant map or alpha <= 0.  One launch, one writer per
 * byte, no atomics: the bits of clips.paste_maps_host wherever 255 m and 256 alpha m are not within rounding of n + 1/2. */
int istvt_relevance_paste_u8(void* frames, long total, int Hs, int Ws, const float* maps, int g, const double* A,
                             const int* rect, const void* lut, const float* alpha, int n, int S, istvt_stream_t stream);
int istvt_relevance_paste_nv12(void* frames, long total, int Hs, int Ws, long pitch, long fstride, const float* maps, int g,
                               const double* A, const int* rect, const void* lut, const float* alpha, int n, int S,
                               istvt_stream_t stream);
/* JPEG round trip: frames uint8 [n][H][W][3] (`total` bytes readable at frames, >= n*H*W*3; nothing outside is read, no
 * alignment needed), quality int32 [n] on the device -> out uint8 [n][H][W][3] (no overlap with frames: ISTVT_ERR_SHAPE), the
 * RGB a baseline JPEG encoder and decoder hand back: libjpeg's 16-bit fixed-point colour transforms, edge replication to whole
 * MCUs, 2x2 box chroma downsample (subsampling = 2, 4:2:0) or none (0, 4:4:4), the 13-bit "slow integer" DCT, Annex K tables
 * scaled by the frame's quality (s = 5000 / q below 50, else 200 - 2 q; entry (base * s + 50) / 100 in 1..255), quantisation
 * half away from zero, the inverse DCT, the "fancy" triangle chroma upsample, clamp.  Quality 1..100 compresses (larger counts
 * as 100), <= 0 copies the frame.  int32 arithmetic only: the bits of clips.jpeg_roundtrip_host.  scratch: 8-byte aligned
 * planes, n * Hp * Wp * 3 / 2 bytes at 4:2:0 (Hp, Wp = H, W rounded up to multiples of 16) and n * Hp * Wp * 3 at 4:4:4
 * (multiples of 8).  Two launches, no synchronisation, no atomics.  H, W <= 16384. */
int istvt_jpeg_roundtrip_u8(const void* frames, long total, int n, int H, int W, const int* quality, int subsampling,
                            void* scratch, long scratch_bytes, void* out, istvt_stream_t stream);
/* JPEG files: a batch of baseline JPEG files, packed on the host by clips.jpeg_batch, decoded from their compressed bytes ->
 * out uint8 [n][Hc][Wc][3]: image i in the top left H_i x W_i of its canvas, 0 elsewhere; sizes int32 [n][2] = (H, W) and
 * status int32 [n] (0 fine, 1 the scan ended early, 2 a code or DC category no table holds, 3 a run past coefficient 63) on
 * the device.  The bits of clips.jpeg_decode_host where the status is 0: canonical Huffman decoding per restart interval
 * (T.81 F.2.2), the file's own quantisation tables, then the inverse half of the round trip above.  Three launches (entropy:
 * one lane per restart interval; IDCT; colour onto the canvas), no synchronisation, no global state.
 *   bytes      uint8 [nbytes]: the scans of all files, end to end
 *   images     int32 [n][20]: H, W, chroma step (2 or 1), MCU columns, MCU rows, quantisation slot of Y, Cb, Cr, (DC, AC)
 *              Huffman slots of Y, Cb, Cr, first block, first IDCT workgroup (24 blocks each), first segment, segments,
 *              blocks, layout code.  An image's blocks: those of Y, row by row of the plane padded to whole MCUs, then Cb's,
 *              then Cr's.  Layout code 0: three components, the chroma step on both axes (4:2:0: MCUs of 16 x 16 pixels and
 *              2 x 2 Y blocks; 4:4:4: 8 x 8 and one).  ISTVT_JPEG_LAYOUT_422: three components, the chroma step (2) is
 *              horizontal only, MCUs of 16 x 8 pixels with two Y blocks side by side.  ISTVT_JPEG_LAYOUT_GREY: Y alone, the
 *              chroma step is 1, MCUs of 8 x 8 pixels and one block, no Cb or Cr blocks; the Cb and Cr slots repeat Y's and
 *              nothing is read through them.  Any other code, or a chroma step the code does not go with, is -3.
 *   segments   int32 [nseg][5]: image, first byte, end byte, first MCU, MCUs; sorted by image, then by MCU
 *   qtabs      int32 [nq][64], natural order;  htabs int32 [nh][288]: limit[16], offset[16], values[256]
 *   scratch    16-byte aligned, blocks * 192 + nseg * 4 bytes; nothing is read from it before it is written
 * images_host / segments_host are host copies of the two tables: the entry checks them against the counts, nbytes, the
 * canvas and each other before any launch and returns -3 on a null pointer, a bad count, a canvas smaller than an image,
 * an out that overlaps bytes or an inconsistent table.  Every other pointer is a device pointer. */
#define ISTVT_JPEG_IMAGE_INTS 20   /* a row of images */
#define ISTVT_JPEG_SEGMENT_INTS 5  /* a row of segments */
#define ISTVT_JPEG_HUFF_INTS 288   /* a table of htabs */
#define ISTVT_JPEG_IDCT_BLOCKS 24  /* blocks per IDCT workgroup: what "first IDCT workgroup" of an images row counts in */
#define ISTVT_JPEG_LAYOUT_422 1    /* layout code of an images row: 4:2:2 */
#define ISTVT_JPEG_LAYOUT_GREY 2   /* ... one component */
typedef struct istvt_jpeg_decode_args {
    const void* bytes;
    long nbytes;
    const int* images;
    const int* images_host;
    const int* segments;
    const int* segments_host;
    const int* qtabs;
    const int* htabs;
    void* scratch;
    long scratch_bytes;
    void* out;
    int* sizes;
    int* status;
    istvt_stream_t stream;
    int n, nseg, nq, nh, Hc, Wc;
} istvt_jpeg_decode_args;
int istvt_jpeg_decode_u8(const istvt_jpeg_decode_args* a);
/* JPEG files without restart markers: istvt_jpeg_decode_u8 with another entropy kernel, one workgroup per restart interval
 * and one lane per chunk of it, for intervals that are long (a whole file where there are no markers).  The same argument
 * block, the same checks and the same bytes in out, sizes and status.  An interval of `length` bytes is cut into chunks of
 * max(chunk_bytes, ceil(length / 256)) bytes, at least one; the lanes start from guessed decoder states and relax them to the
 * sequential decoder's (csrc/jpeg_entropy_split.h), then decode their chunks.  chunk_bytes >= 16, and segments lie in the
 * order of their bytes (first byte >= the end byte of the segment before), or -3.
 *   scratch    16-byte aligned; the layout above in front, then from the next multiple of 16 bytes int32
 *              [nbytes / chunk_bytes + nseg][8], the state rows: those of segment s start at row (first byte) / chunk_bytes
 *              + s.  A row: the lane's entry state (byte index in `bytes`, bits of that byte taken, block within the MCU
 *              (0..5 at 4:2:0, 0..2 at 4:4:4, 0..3 at 4:2:2, 0 for greyscale), coefficient index), blocks it started, its
 *              first block within the interval, the status of its decode, the rounds in which a state of the interval
 *              changed.  clips.jpeg_split_plan has the sizes. */
#define ISTVT_JPEG_STATE_INTS 8    /* a state row */
int istvt_jpeg_decode_split_u8(const istvt_jpeg_decode_args* a, int chunk_bytes);
/* JPEG bank: the files of a whole set stay on the device with their tables (clips.jpeg_bank), and a call decodes the m of them
 * that `index` names, in that order and with repeats -> out uint8 [m][Hc][Wc][3], sizes int32 [m][2], status int32 [m] as
 * above, and two more statuses: 4 the index is outside [0, n), 5 the bank's row holds no decodable file (its segment count
 * is 0: istvt_jpeg_bank_ingest marks files so); either leaves size (0, 0) and a frame of zeros.  The bits of
 * clips.jpeg_bank_decode_host.  Four launches: jpeg_bank_plan_kernel writes batch-local images and segments tables into the
 * scratch, then the three kernels of istvt_jpeg_decode_u8 read those.  Place j gets first block j * block_stride, first IDCT
 * workgroup j * block_stride / 24 and first segment j * seg_max, so every grid is known from m alone; segment rows behind an
 * image's real count name image -1, which the entropy kernel rejects, and are not part of the image's status.  No
 * synchronisation, no global state, nothing allocated.  The argument block is istvt_jpeg_decode_args, read as follows:
 *   bytes, nbytes, images, segments, qtabs, htabs, n, nseg, nq, nh    the bank, on the device; nbytes < 2^31
 *   images_host    NOT a host pointer here: the index, int32 [m] on the device.  segments_host is not read.
 *   scratch        16-byte aligned; nothing is read from it before it is written.  m * block_stride * 192 bytes of
 *                  coefficients and planes | int32 [m * seg_max + m]: the segment statuses, then a word per place (0, 4 or 5),
 *                  which a place that cannot be decoded names as its one segment | from the next multiple of 16 bytes the
 *                  planned images int32 [m][20] | the planned segments int32 [m * seg_max][5].
 *                  clips.jpeg_bank_scratch_bytes has the sum.
 *   out, sizes, status, Hc, Wc, stream    as above, with m in the place of n
 * seg_max: the most segments of any file of the bank; block_stride: the most blocks of any, a multiple of 24; Hmax, Wmax: the
 * largest height and width.  The entry looks at scalars alone and returns -3 on a null pointer, a bad count or stride, a
 * canvas smaller than Hmax x Wmax, a scratch too small or misaligned, or an out that overlaps bytes; the bank's tables were
 * checked when it was built, and the plan kernel turns a row that does not fit the strides or the canvas into status 5. */
int istvt_jpeg_decode_indexed_u8(const istvt_jpeg_decode_args* a, int m, int seg_max, int block_stride, int Hmax, int Wmax);
/* JPEG bank, split: istvt_jpeg_decode_indexed_u8 for a bank whose files have long restart intervals (no markers at all, as
 * cameras and most encoders write them).  Four launches: the plan, then the split entropy kernel of
 * istvt_jpeg_decode_split_u8 on m * seg_max workgroups -- of 64 lanes where chunk_rows <= 64, else 256 -- then the IDCT and
 * canvas kernels.  The same argument block, the same bytes in out, sizes and status.  The split is a property of the bank:
 *   chunk_bytes    >= 16: an interval of `length` bytes is cut into chunks of max(chunk_bytes, ceil(length / 256)) bytes
 *   chunk_rows     1..256: the state rows reserved per planned segment row, at least the chunks of any interval of up to
 *                  seg_bytes_max bytes: min(256, max(1, ceil(seg_bytes_max / chunk_bytes))).  This is the second row addressing
 *                  of the split kernel: planned segment s = j * seg_max + k (place j, its segment k) owns rows [s * chunk_rows,
 *                  (s + 1) * chunk_rows), whatever the place of its bytes in the bank (the batch call addresses rows by byte
 *                  offset over the call's bytes, which for a bank are the whole set).  An interval of more chunks than
 *                  chunk_rows gets segment status 2 and nothing of it is written.
 *   seg_bytes_max  the longest interval of the bank in bytes, as its builder knows it: the plan kernel turns a place whose
 *                  file has a longer one into status 5, so a device table that differs from the host's number stays inside
 *                  the scratch.  Negative: no limit (chunk_rows = 256 then holds any interval).
 *   scratch        the layout of istvt_jpeg_decode_indexed_u8 in front, then from the next multiple of 16 bytes the state
 *                  rows int32 [m * seg_max * chunk_rows][8], a row as istvt_jpeg_decode_split_u8 describes it with byte
 *                  indices into the bank.  Rows behind an interval's chunks are not written.  clips.jpeg_bank_scratch_bytes
 *                  has the sum.
 * Checks on scalars alone, -3 as above and for chunk_bytes < 16 or chunk_rows outside 1..256.  No synchronisation, no
 * allocation, no global state. */
int istvt_jpeg_decode_indexed_split_u8(const istvt_jpeg_decode_args* a, int m, int seg_max, int block_stride, int Hmax, int Wmax,
                                       int chunk_bytes, int chunk_rows, int seg_bytes_max);
/* Batch draw: which B clips of T frames a training step takes from a bank and how each is augmented, drawn on the device as a
 * pure function of (seed, step); the bits of clips.batch_draw_host.  The plan, the step counter and the drawn tables live in
 * one int32 tensor on the device, the draw block of block_ints ints (csrc/batch_draw.h names the words):
 *   [0, 36)   header: magic 'BDRW', block_ints, B, T, stride, V, N, K, nk, jpeg lo, jpeg hi, 0 | as (low, high) pairs the
 *             thresholds round(p * 2^32) of flip, jpeg and perturb, the seed and the step | status, 0, the step that was
 *             drawn (low, high) | the offsets in ints of videos, base, shapes, kinds, boxes, quality, view, perturb, label | 0
 *   [36, 36 + B*T)   index: the place of the bank every frame is
 *   the nine parts at their offsets, in that order, each behind the one before: videos [V][3] = (first place, frames, label),
 *   base [N][4] = (y0, x0, h, w) per place, shapes [K][2] = Q16 (rh, rw), kinds [nk][3] = (kind, lo, hi), which are read, and
 *   boxes [B*T][4], quality [B*T], view [B][3], perturb [B][4], label [B], which are written.
 * The argument block is istvt_jpeg_decode_args, as the bank's entries take it; istvt_batch_draw reads two fields:
 *   images_host    NOT a host pointer here: the draw block, int32 [block_ints] on the device
 *   stream
 * One launch of ONE workgroup: every lane reads the step, and behind a barrier lane 0 stores step + 1, the step drawn and
 * status 0.  A block whose header disagrees with B, T or block_ints, or names a part outside the block or in front of the part
 * before it, gets status 1; one whose videos rows leave the base table or are shorter than (T - 1) * stride + 1 frames gets
 * status 2; either way no other word is written and the step stays.  Nothing outside the block is read or written.  No
 * synchronisation, nothing allocated.  -3 for a null block, B or T < 1, or block_ints < 36 + B * T. */
int istvt_batch_draw(const istvt_jpeg_decode_args* a, int B, int T, int block_ints);
/* The draw followed by istvt_jpeg_decode_indexed_u8 with m = B * T on the index it wrote: five launches.  images_host is the
 * draw block as above; every other field, and seg_max, block_stride, Hmax and Wmax, are the indexed decode's.  Statuses 4
 * and 5 are what they were; a refused block leaves its index as it was, which the plan kernel checks like any other. */
int istvt_jpeg_decode_drawn_u8(const istvt_jpeg_decode_args* a, int B, int T, int block_ints, int seg_max, int block_stride,
                               int Hmax, int Wmax);
/* The draw followed by istvt_jpeg_decode_indexed_split_u8 with m = B * T on the index it wrote: five launches.  chunk_bytes,
 * chunk_rows and seg_bytes_max are that entry's, everything else is istvt_jpeg_decode_drawn_u8's. */
int istvt_jpeg_decode_drawn_split_u8(const istvt_jpeg_decode_args* a, int B, int T, int block_ints, int seg_max, int block_stride,
                                     int Hmax, int Wmax, int chunk_bytes, int chunk_rows, int seg_bytes_max);
/* PNG files: a batch of 8-bit, non-interlaced PNG files of colour type 0 (grey), 2 (RGB) or 6 (RGBA), packed on the host by
 * clips.png_batch, decoded from their raw DEFLATE streams -> out uint8 [n][Hc][Wc][3]: image i in the top left H_i x W_i of its
 * canvas (grey replicated, alpha dropped), 0 elsewhere; sizes int32 [n][2] = (H, W) and status int32 [n] on the device.  The
 * bytes of clips.png_decode_host.  Status: 0 fine, 1 the stream ends early, 2 a reserved block type or a stored block whose
 * length and complement disagree, 3 code lengths over-subscribed or incomplete or a code no table holds, 4 a distance beyond
 * the bytes produced, 5 more or fewer bytes than H (1 + W bpp), 6 a filter byte above 4; a file whose status is not 0 gets an
 * all-zero canvas.  Two launches of n workgroups of one wave (inflate into the scratch; unfilter and colour onto the canvas),
 * no synchronisation, no global state, nothing allocated.  The argument block is istvt_jpeg_decode_args, as istvt_batch_draw
 * takes it; the entry reads
 *   bytes, nbytes  uint8 [nbytes], 16-byte aligned, nbytes <= ISTVT_PNG_MAX_BYTES: the DEFLATE streams end to end, each starting at a multiple of 16 bytes;
 *                  no byte outside a file's [begin, end) is read for it
 *   images         int32 [n][8]: H, W, colour type, bytes per pixel (1, 3 or 4), begin, end, 0, 0;  images_host: its host copy
 *   scratch        16-byte aligned, n * raw_stride bytes; file i's H (1 + W bpp) filtered bytes go to scratch + i * raw_stride and
 *                  nothing else of the scratch is written
 *   out, sizes, status, stream, n, Hc, Wc
 * and no other field.  raw_stride: a multiple of 16, at least every file's H (1 + W bpp).  -3 on a null pointer, a bad count,
 * a canvas smaller than an image, an out that overlaps bytes or a table row that disagrees with any of this. */
#define ISTVT_PNG_IMAGE_INTS 8     /* a row of a PNG batch's images */
#define ISTVT_PNG_MAX_BYTES 2147479552   /* nbytes at the most, 2^31 - 4096: byte offsets and a 256-byte window stay ints */
int istvt_png_decode_u8(const istvt_jpeg_decode_args* a, int raw_stride);
/* PNG files by their bands: the batch of istvt_png_decode_u8 packed with clips.png_batch(bands='index'), every file's stream
 * taken apart where its `baND` chunk says a band begins (a file without a usable chunk is one band), one wave per band in
 * place of one per file.  The bytes and statuses of clips.png_decode_bands_host: a band's window starts at its own first
 * output byte, a band that is not its file's last stops behind the stored block that ends at its end byte, and status 7 says
 * that the index disagrees with the stream (BFINAL in such a band); the file's status is that of its first failing band.
 * The entry reads what istvt_png_decode_u8 reads, and
 *   segments, segments_host, nseg   int32 [nseg][ISTVT_PNG_BAND_INTS]: file, first byte in `bytes`, end byte, first output byte
 *                  within the file's filtered rows, output bytes; sorted by file, then by band
 *   images[i][6], images[i][7]      file i's first row of segments and its count of them
 *   scratch        n * raw_stride bytes of filtered rows as above, then int32 [nseg] band statuses; scratch_bytes >= n *
 *                  raw_stride + 4 nseg.  Nothing else of it is written.
 * Two launches (inflate, nseg workgroups of one wave; unfilter and colour, n workgroups of one wave: the rows of a file stay
 * serial, since a band's first row may be filtered against the row above it), no synchronisation, nothing allocated.  -3
 * before any launch as above, and where the host tables disagree: a band outside its file's [begin, end), rows that are not
 * in file order, a file's output ranges that do not follow one another from 0 to H (1 + W bpp). */
#define ISTVT_PNG_BAND_INTS 5      /* a row of a PNG batch's bands */
int istvt_png_decode_bands_u8(const istvt_jpeg_decode_args* a, int raw_stride);
/* PNG bank: the files of a whole set stay on the device with their tables (clips.png_bank), and a call decodes the m of them
 * that `index` names by their bands, in that order and with repeats -> out uint8 [m][Hc][Wc][3], sizes int32 [m][2], status
 * int32 [m] as istvt_png_decode_bands_u8 writes them, and two more statuses: 8 the index is outside [0, n), 9 the bank's row
 * for the place, or one of its band rows, does not fit the call (only a device table that differs from what clips.png_bank
 * built gives it); either leaves size (0, 0) and a frame of zeros.  The bytes of clips.png_bank_decode_host.  The bank may
 * hold more than 2^31 bytes: a file is addressed by a 64-bit base, everything inside it by 32-bit offsets from that base.
 * Two launches and no plan kernel: png_bank_inflate_kernel, m * band_max workgroups of one wave, wave b being band b % band_max
 * of place b / band_max (a wave whose file has fewer bands leaves at once), and png_bank_unfilter_kernel, m workgroups of one
 * wave; both look the index up themselves and check the rows they use (csrc/png_bank.h).  No synchronisation, no global
 * state, no atomics, nothing allocated.  The argument block is istvt_jpeg_decode_args, read as follows:
 *   bytes, nbytes  uint8 [nbytes], 16-byte aligned: the bank's DEFLATE streams, each starting at a multiple of 16 bytes; nbytes
 *                  is a long and may exceed 2^31.  No byte outside a drawn file's [base, base + stream bytes) is read
 *   images, n      int32 [n][ISTVT_PNG_BANK_IMAGE_INTS]: H, W, colour type, bytes per pixel, base low word, base high word,
 *                  stream bytes, first band row, band count, flags (not read by this entry)
 *   segments, nseg int32 [nseg][ISTVT_PNG_BAND_INTS] as above, with the first byte and the end byte counted from the file's base
 *   images_host    NOT a host pointer here: the index, int32 [m] on the device.  segments_host is not read.
 *   scratch        16-byte aligned; m * raw_stride bytes of filtered rows, place j's at scratch + j * raw_stride, then int32
 *                  [m * band_max] band statuses, band k of place j at word j * band_max + k; scratch_bytes >= m * raw_stride +
 *                  4 m band_max (clips.png_bank_scratch_bytes).  Nothing is read from it before it is written.
 *   out, sizes, status, Hc, Wc, stream    as above, with m in the place of n
 * band_max: the most bands of any file of the bank; raw_stride: a multiple of 16, at least every file's H (1 + W bpp).  The
 * entry looks at scalars alone and returns -3 on a null pointer, a count below 1, a raw_stride below 16 or not a multiple of
 * 16, m * band_max beyond an int, a canvas outside 1..16384, a scratch too small or misaligned, or an out that overlaps bytes. */
#define ISTVT_PNG_BANK_IMAGE_INTS 10   /* a row of a PNG bank's images */
int istvt_png_decode_bank_u8(const istvt_jpeg_decode_args* a, int m, int band_max, int raw_stride);
/* The draw followed by istvt_png_decode_bank_u8 with m = B * T on the index it wrote: three launches.  images_host is the
 * draw block as istvt_batch_draw reads it; every other field, and band_max and raw_stride, are the bank decode's.  A refused
 * block leaves its index as it was, which the bank's kernels check like any other (status 8 outside the bank). */
int istvt_png_decode_bank_drawn_u8(const istvt_jpeg_decode_args* a, int B, int T, int block_ints, int band_max, int raw_stride);
/* PNG bands that stand alone.  A file whose `baND` chunk carries ISTVT_PNG_BAND_ALONE in its R word says that no band's first
 * row is filtered against the row above (types 2, 3, 4 on a row k R, k >= 1), so a band is decoded to pixels with no other
 * band.  istvt_png_decode_alone_u8 takes the block of istvt_png_decode_bands_u8 (clips.png_batch(bands='index', alone=True))
 * with its checks and its inflate launch, and
 *   qtabs, htabs, nq, nh   int32 [n] on the device and its host copy: file i's flag, 1 where its bands stand alone, else 0;
 *                  nq == nh == n
 * The unfilter launch has nseg workgroups of one wave, one per band row.  The waves of a flagged file each settle the file's
 * status for themselves -- the first failing band status in band order, then 6 for a filter byte above 4, then 10: the file
 * lies, a band's first row reads the row above -- and then reconstruct, or zero, rows [k R, min(H, (k + 1) R)) of the canvas
 * with the margin right of them; the wave of band 0 writes status and sizes and zeroes the margin below.  A file without the
 * flag is unfiltered whole by one wave as istvt_png_decode_bands_u8 does it: wave f of the launch for file f, so that the
 * long serial jobs start first; its own waves leave.  The bytes and statuses of clips.png_decode_alone_host.  -3 before any launch as there, and on a null qtabs or htabs, another nq or nh,
 * a flag word with bits other than bit 0, or a flagged file whose band rows are not the R-row bands of an index, R = the
 * output bytes of its band row 0 / (1 + W bpp): count == ceil(H / R), row k writes k R (1 + W bpp) and on for rows_k (1 + W
 * bpp) bytes (csrc/png_alone.h) -- so no canvas row is written twice or left unwritten.
 * istvt_png_decode_bank_alone_u8 is istvt_png_decode_bank_u8 in every argument, check and its inflate launch, for a bank
 * packed with clips.png_bank(alone=True): bit 0 of images[i][9] is file i's flag.  Its unfilter launch has m * band_max
 * workgroups, mapped as the inflate's; a flagged file whose band rows fail the check above has status 9.  The bytes of
 * clips.png_bank_decode_host.  istvt_png_decode_bank_alone_drawn_u8 is the draw in front of it, as above. */
#define ISTVT_PNG_BAND_ALONE 0x80000000u   /* bit 31 of the R word of a baND chunk: the bands stand alone */
int istvt_png_decode_alone_u8(const istvt_jpeg_decode_args* a, int raw_stride);
int istvt_png_decode_bank_alone_u8(const istvt_jpeg_decode_args* a, int m, int band_max, int raw_stride);
int istvt_png_decode_bank_alone_drawn_u8(const istvt_jpeg_decode_args* a, int B, int T, int block_ints, int band_max, int raw_stride);
/* PNG windows: files whose bands stand alone, decoded through one box (y0, x0, h, w) per place.  Only the bands the box touches
 * are inflated and unfiltered, kfirst = y0 / R to klast = (y0 + h - 1) / R, into out uint8 [m][Hc][Wc][3] whose place j is a
 * window: rows [w0, w1) = [kfirst R, min(H, (klast + 1) R)) of the image in its rows [0, w1 - w0) and columns [0, W), 0
 * elsewhere.  The bytes of clips.png_bank_window_host.  Status int32 [m]: 8 and 9 as the bank has them; 11 the file's index does
 * not say its bands stand alone; 12 the box does not lie in the image (h < 1, w < 1, y0 < 0, x0 < 0, y0 + h > H, x0 + w > W),
 * its window has more than Hc rows or more than win_bands bands; then the first status that is not 0 of the touched bands in
 * band order, 6 for a filter byte above 4 in rows [w0, w1), 10 for a row k R, k >= 1, of type 2, 3 or 4 among them, in that
 * order.  Damage in a band the box does not touch is not seen.  A place with a status has a window of zeros, origin 0 and the
 * moved box (0, 0, 1, 1); sizes int32 [m][2] are (H, W), or (0, 0) with 8 and 9.  Two launches of m * win_bands workgroups of
 * one wave, wave b being slot b % win_bands of place b / win_bands and taking band kfirst + slot (a wave whose window has no
 * such band, or whose place has a status, leaves at once); every wave checks the rows it uses (csrc/png_window.h).  No
 * synchronisation, no global state, no atomics, nothing allocated.  The argument block is istvt_jpeg_decode_args.
 * istvt_png_decode_bank_window_u8 reads the bank's fields as istvt_png_decode_bank_alone_u8 does, and
 *   qtabs, nq      int32 [m][4] on the device: the boxes; nq == m
 *   Hc, Wc         the window height `rows` and the canvas width: a file's W is compared with Wc, its H is not compared with Hc
 *   scratch        16-byte aligned; m * win_stride bytes of filtered rows, the window of place j at scratch + j * win_stride |
 *                  int32 [m * win_bands] band statuses, slot t of place j at word j * win_bands + t; a slot without a band is
 *                  not written | from the next multiple of 16 bytes int32 [m][4], the boxes moved into their windows, (y0 - w0,
 *                  x0, h, w) | int32 [m], the origins w0.  clips.png_window_scratch_bytes has the sum.
 *   out, sizes, status, stream, images_host (the index, on the device)    as there
 * win_bands: 1..band_max, the slots of a place; win_stride: a multiple of 16, at least min(H, Hc) (1 + W bpp) of every file
 * (a file of more gets status 9).  The entry looks at scalars alone and returns -3 on what istvt_png_decode_bank_u8 refuses,
 * asked with win_bands and win_stride in the place of band_max and raw_stride, on a band_max below 1, a raw_stride below 16 or
 * not a multiple of 16, a null qtabs, nq != m, win_bands outside 1..band_max, a win_stride below 16 or not a multiple of 16, m *
 * win_bands beyond an int, a scratch smaller than the layout, or an out that overlaps bytes.
 * istvt_png_decode_window_u8 is the batch of istvt_png_decode_alone_u8 (clips.png_batch(bands='index', alone=True)): m == n and
 * place j is file j.  It reads the fields of istvt_png_decode_bands_u8 and makes its checks of the host tables, with
 *   qtabs, nq      the boxes, as above; nq == n
 *   htabs, nh      int32 [n] on the HOST: file i's flag; nh == n.  -3 unless every flag is 1 and every file's band rows are the
 *                  R-row bands of an index, as istvt_png_decode_alone_u8 asks of a flagged file
 *   Hc, Wc, scratch    as above, with n in the place of m
 * istvt_png_decode_bank_window_drawn_u8 is the draw in front of the bank's entry with m = B * T: three launches.  images_host
 * is the draw block as istvt_batch_draw reads it, and qtabs points at the boxes inside it, which the draw has just written. */
int istvt_png_decode_window_u8(const istvt_jpeg_decode_args* a, int win_bands, int win_stride);
int istvt_png_decode_bank_window_u8(const istvt_jpeg_decode_args* a, int m, int band_max, int raw_stride, int win_bands, int win_stride);
int istvt_png_decode_bank_window_drawn_u8(const istvt_jpeg_decode_args* a, int B, int T, int block_ints, int band_max, int raw_stride,
                                          int win_bands, int win_stride);
/* JPEG files out: frames uint8 [n][H][W][3] (`total` bytes readable at frames, >= n*H*W*3) -> n baseline JFIF files laid end
 * to end in data, the bytes of clips.jpeg_encode_host: the forward half of the round trip above (colour in, padding, 4:2:0
 * downsample at subsampling = 2 or none at 0, the slow-integer DCT, the quantiser of the frame's quality), Huffman coding with
 * the Annex K.3 tables, a restart marker every restart_interval MCUs (0: none; 0..65535).  All frames of a call share H, W,
 * subsampling and restart interval; quality int32 [n] on the device is per frame.  Four launches (coefficients; one lane per
 * restart interval counts; one workgroup takes the prefix sum; the same lanes store), no synchronisation, no global state,
 * nothing allocated.
 *   header     the bytes SOI .. SOS header that every file of the call starts with (clips.jpeg_header), on the device; the 64
 *              bytes at dqt0 and at dqt1 are the two quantisation tables, filled per frame from its quality
 *   scratch    16-byte aligned, 128 bytes per 8 x 8 block (int16 coefficients in zig-zag order; per frame the blocks of Y row
 *              by row of the plane padded to whole MCUs, then Cb's, then Cr's) + 16 bytes per restart interval
 *   data       uint8 [capacity], no overlap with frames;  offsets int64 [n + 1]: file i is data[offsets[i] .. offsets[i + 1])
 *   status     int32 [n]: 0 fine | 1 the file does not fit in data: nothing of it is written, offsets still hold the true
 *              sizes, so offsets[n] is the capacity a retry needs | 2 quality <= 0: an empty file | 3 a coefficient outside
 *              baseline's categories, coded clamped (not reachable from 8-bit samples)
 * Returns -3 before any launch on a null pointer, a bad count or size, a scratch too small or misaligned, or an overlap. */
typedef struct istvt_jpeg_encode_args {
    const void* frames;
    long total;
    const int* quality;
    const void* header;
    long header_bytes;
    void* scratch;
    long scratch_bytes;
    void* data;
    long capacity;
    long* offsets;
    int* status;
    istvt_stream_t stream;
    int n, H, W, subsampling, restart_interval, dqt0, dqt1;
} istvt_jpeg_encode_args;
int istvt_jpeg_encode_u8(const istvt_jpeg_encode_args* a);
/* JPEG files out with optimised Huffman tables: istvt_jpeg_encode_u8 with every file coded by its own four tables, those
 * libjpeg's jpeg_gen_optimal_table makes of the file's symbol counts -> the bytes of clips.jpeg_encode_host(optimize=True).
 * The same argument block, the same checks, and offsets and status as above.  `header` is the same standard header;
 * [dht0, dht1) are the bytes of its four Huffman table segments (dqt1 + 64 <= dht0 < dht1 <= header_bytes), which every file
 * replaces by its own, so a file's header is at most header_bytes long.  Five launches on the stream (coefficients; one
 * workgroup per image counts symbols in LDS and builds the tables; one workgroup per image counts the bytes of its restart
 * intervals; one workgroup takes the prefix sum with the per-image header lengths; the same lanes store), no
 * synchronisation, no global atomics, nothing allocated, nothing that has to be zeroed.
 *   scratch    16-byte aligned, 128 bytes per 8 x 8 block + 16 bytes per restart interval as above, then
 *              ISTVT_JPEG_OPT_ROW_BYTES per image: int32 header length (16 bytes), four Huffman table segments of up to 277
 *              bytes 288 bytes apart (DC 0, DC 1, AC 0, AC 1), then 544 code words (code << 8 | length; 16 + 16 DC, 256 + 256
 *              AC).  A row of an image whose quality is <= 0 is not written. */
#define ISTVT_JPEG_OPT_ROW_BYTES 3344
int istvt_jpeg_encode_opt_u8(const istvt_jpeg_encode_args* a, int dht0, int dht1);
/* JPEG files out in the layouts 4:2:2 and greyscale: the two entries above for layout = ISTVT_JPEG_LAYOUT_422 (MCUs of 16 x
 * 8 pixels: two Y blocks side by side, Cb, Cr; chroma is the mean of horizontal pairs, (a + b + (chroma column & 1)) >> 1) or
 * ISTVT_JPEG_LAYOUT_GREY (MCUs of 8 x 8 pixels and one block: Y of the colour transform alone, coded with table id 0) -> the
 * bytes of clips.jpeg_encode_host(layout=).  The same argument block with subsampling = 0, the same checks, and offsets and
 * status as above; any other layout or subsampling is -3.  restart_interval counts the layout's MCUs.  `header` is
 * clips.jpeg_header(layout=); it holds both quantisation tables and all four Huffman tables in either layout.
 * dht0 == dht1 == 0: the Annex K.3 tables, the four launches and the scratch of istvt_jpeg_encode_u8.  Otherwise [dht0, dht1)
 * are the header's four Huffman table segments, checked as istvt_jpeg_encode_opt_u8 checks them, and every file is coded with
 * its own tables in that entry's five launches and scratch; a greyscale file's two id-1 tables are empty (19 bytes each).
 * Blocks per frame: 4 per MCU at 4:2:2, 1 for greyscale.  No synchronisation, no global atomics, nothing allocated, nothing
 * that has to be zeroed. */
int istvt_jpeg_encode_layout_u8(const istvt_jpeg_encode_args* a, int layout, int dht0, int dht1);
/* JPEG bank, ingest: the result of one istvt_jpeg_encode_u8 / istvt_jpeg_encode_layout_u8 call with the Annex K.3 tables
 * (dht0 == dht1 == 0) -> the tables of a bank over the same `data`, without a host parse.  Two launches:
 * jpeg_bank_qtabs_kernel de-zigzags the 2 x 64 bytes at dqt0 / dqt1 of every file; jpeg_bank_scan_kernel, one workgroup per
 * file, finds the FF D0..D7 pairs of its scan in tiles of 256 lanes x 16 bytes and writes its segment rows and its images
 * row.  No synchronisation, no atomics, nothing allocated.  The argument block is istvt_jpeg_encode_args as the encoder call
 * had it -- data, capacity (< 2^31), offsets, status (read here), header_bytes, dqt0, dqt1, n, H, W, subsampling,
 * restart_interval, stream -- except that frames, quality and header are not read and
 *   scratch        is the result, 16-byte aligned: segments int32 [n * seg_max][5] with byte offsets into data (seg_max =
 *                  ceil(MCUs / restart_interval), 1 where that is 0) | qtabs int32 [2 n][64], file i's at rows 2 i, 2 i + 1 |
 *                  images int32 [n][20], whose Huffman slots are 0..3 in the order DC 0, AC 0, DC 1, AC 1 (0, 1 for greyscale).
 * layout: 0 with the call's subsampling, or ISTVT_JPEG_LAYOUT_422 / ISTVT_JPEG_LAYOUT_GREY with subsampling 0.  A file whose
 * status is not 0, that is shorter than header_bytes + 2, does not end with EOI or does not hold seg_max - 1 restart markers
 * gets 0 segments in its images row: istvt_jpeg_decode_indexed_u8 reports status 5 for it.  -3 as above. */
int istvt_jpeg_bank_ingest(const istvt_jpeg_encode_args* a, int layout);
/* PNG files out: a batch of frames uint8 [n][H][W][bpp], bpp = 1 (grey), 3 (RGB) or 4 (RGBA) -> n complete PNG files (signature,
 * IHDR, one IDAT, IEND) end to end in `data`, the bytes of clips.png_encode_banded_host.  Rows [k R, min(H, (k + 1) R)) with
 * their filter bytes are band k, R = min(band_rows, H): one dynamic-Huffman block of literals and distance-1 matches and an
 * empty stored block, so every band starts and ends on a byte and can be inflated alone.  filter: 0..4 on every row, or 5: per
 * row the type with the smallest sum of min(r, 256 - r) over its residuals, the lowest on a tie; the row above is the source's.
 * The block is istvt_jpeg_encode_args, of which this entry reads
 *   frames, total  the pixels, total >= n H W bpp bytes readable; no alignment needed
 *   scratch        16-byte aligned, scratch_bytes >= n * raw_stride + n * ceil(H / R) * ISTVT_PNG_BAND_ROW_BYTES: file i's
 *                  filtered rows at i * raw_stride (raw_stride >= H (1 + W bpp), a multiple of 16), then one row of 432 ints per
 *                  band: 288 literal/length code words (bit-reversed code << 8 | length), 136 dwords of block-header bits, then
 *                  header bits, the band's bytes in the stream, Adler-32 parts a, b, the band's filtered bytes, the distance
 *                  code's word, the band's offset in the stream, 0
 *   data, capacity the files; data may not overlap frames
 *   offsets        long [n + 1]: file i is data[offsets[i] .. offsets[i + 1])
 *   status         int [n]: 0 fine, 1 the file does not fit: nothing of it is written, offsets still hold true sizes and
 *                  offsets[n] is the capacity a retry needs
 *   stream, n, H, W (H, W <= 16384)
 * and no other field.  Four launches (filter and count, one wave per band; prefix sum, one workgroup; store, the same waves;
 * container with Adler-32 and CRC-32s, one workgroup of 512 threads per file), no synchronisation, no global atomics, nothing allocated, nothing
 * that has to be zeroed.  -3 before any launch: a null pointer, a bad count, size, bpp, band_rows or filter, a misaligned or
 * short scratch, data overlapping frames. */
#define ISTVT_PNG_BAND_ROW_BYTES 1728
int istvt_png_encode_u8(const istvt_jpeg_encode_args* a, int bpp, int band_rows, int filter, int raw_stride);
/* PNG files out with their band index: istvt_png_encode_u8 in every argument, check, scratch row and launch, and every file
 * carries between IHDR and IDAT the private ancillary chunk `baND` of 12 + 8 + 4 (nb + 1) bytes, nb = ceil(H / R): big-endian
 * uint32 words R, nb and nb + 1 offsets into the zlib stream, off[0] = 2, off[nb] = the stream's length - 4; band k is stream
 * bytes [off[k], off[k + 1]).  The bytes of clips.png_encode_banded_host(index=True).  The prefix kernel adds the chunk's
 * length to every file; the container kernel writes it from the bands' offsets in the scratch rows and folds its CRC-32 as it
 * folds the IDAT's.  Status 1 and offsets as above. */
int istvt_png_encode_indexed_u8(const istvt_jpeg_encode_args* a, int bpp, int band_rows, int filter, int raw_stride);
/* ... with bands that stand alone: istvt_png_encode_indexed_u8 in checks, scratch and its four launches.  The filter kernel
 * restricts every band's first row to the types that do not read the row above -- 'adaptive' takes the cheaper of 0 and 1, of
 * equal sums 0; a fixed 2 becomes 0, a fixed 3 or 4 becomes 1 -- and the container kernel writes R | ISTVT_PNG_BAND_ALONE as
 * the chunk's first word.  The bytes of clips.png_encode_banded_host(index=True, alone=True). */
int istvt_png_encode_alone_u8(const istvt_jpeg_encode_args* a, int bpp, int band_rows, int filter, int raw_stride);
/* Perturbations: frames uint8 [n][H][W][3] (`total` bytes readable at frames, >= n*H*W*3; nothing outside is read, no
 * alignment needed), table int32 [n][4] = (kind, param, frame_id, stream) per frame on the device -- or, with per_clip_T = T >
 * 0, [n / T][4] per clip: frame f reads row f / T and adds f % T to its frame_id -> out uint8 [n][H][W][3] (no overlap with
 * frames: ISTVT_ERR_SHAPE).  int32 arithmetic with arithmetic shifts only, the bits of clips.perturb_host; v = a byte, Y = (19595
 * R + 38470 G + 7471 B + 32768) >> 16 of its pixel, clamp to 0..255.  kind 0: v.  1 (brightness, param = gain in Q8): clamp((v p
 * + 128) >> 8).  2 (contrast, Q8): clamp(m + (((v - m) p + 128) >> 8)), m = (sum of Y over the frame + H W / 2) / (H W).  3
 * (saturation, Q8): clamp(Y + (((v - Y) p + 128) >> 8)).  4 (noise, param = sigma in Q4 grey levels, <= 1023): clamp(v + (((z p)
 * 887 + (1 << 21)) >> 22)), z = the sum of the 16 bytes of Philox4x32-10(counter ((y W + x) 3 + c, frame_id, stream, 0), key
 * (seed & 0xffffffff, seed >> 32)) less 2040.  5 (blur, param = a row of taps): clamp((sum_j t[j] sum_i t[i] v(y + j - 10, x + i
 * - 10) + (1 << 21)) >> 22), coordinates clamped into the frame; taps int32 [taps_rows][21] on the device, taps_rows <= 16, every
 * row symmetric about index 10, non-negative, summing to 2048 (a null taps blurs nothing).  6 (pixelate, param = block side k in
 * 2..32): (S + cnt / 2) / cnt over the k x k block that holds the pixel, blocks laid from the frame's corner and cut to it.  A
 * kind outside 0..6 copies; a param outside its range is forced into it for kinds 5 and 6.  scratch: 8-byte aligned, n * min(32,
 * ceil(H W / 2048)) * 8 bytes.  Three launches, no synchronisation, no atomics, no state.  H, W <= 16384. */
int istvt_perturb_u8(const void* frames, long total, int n, int H, int W, const int* table, int per_clip_T, const int* taps,
                     int taps_rows, unsigned long long seed, void* scratch, long scratch_bytes, void* out, istvt_stream_t stream);
int istvt_conv2_fwd(const void* u1, const float* bnp, const void* w, void* u2, int frames, int H, int W,
                    istvt_stream_t stream);
int istvt_conv2_dgrad(const void* du2, const void* w, const void* u1, const float* bnp, void* dz1, int frames, int H,
                      int W, istvt_stream_t stream);
int istvt_conv2_wgrad(const void* du2, const void* u1, const float* bnp, float* slabs, float* dw, int frames, int H,
                      int W, istvt_stream_t stream);
int istvt_conv2_wgrad_slabs(void);

/* depthwise 3x3 s1 p1 (SeparableConv2d.conv1, xception.py:43), LDS-tiled.  w: float[9][C] (tap-major);
 * the weight gradient dw is float[C][9] (PyTorch order).
 * forward: in_bn (+in_relu) = the preceding BatchNorm+ReLU applied on load (xception.py:67,73).
 * input gradient (flip=1): epilogue = ReLU mask of msrc (optionally through m_bn) before (mask_pre) /
 * after (mask_post) adding the stride-2 skip-path gradient addsrc[f][y/2][x/2] (Ha = (H-1)/2+1, Wa likewise) or, for
 * the stride-1 blocks, the full-resolution one addsrc[f][y][x] (Ha = H, Wa = W), plus fused
 * BatchNorm-backward sums st_s1/st_s2 (double[C]) of the result w.r.t. m_bn. */
int istvt_dwconv3x3(const void* in, const float* w, void* out, int frames, int H, int W, int C, const float* in_bn,
                    int in_relu, int flip, const void* msrc, const float* m_bn, int mask_pre, int mask_post,
                    const void* addsrc, int Ha, int Wa, double* st_s1, double* st_s2, int dtype,
                    istvt_stream_t stream);
/* dw float [C][9] accumulates; ws = float scratch of istvt_dwconv3x3_wgrad_ws_elems(...) elements (one partial slab
 * per workgroup slot, folded in slot order: bit-reproducible) */
int istvt_dwconv3x3_wgrad(const void* in, const float* in_bn, int in_relu, const void* dout, float* dw, float* ws,
                          long ws_elems, int frames, int H, int W, int C, int dtype, istvt_stream_t stream);
int istvt_dwconv3x3_wgrad_ws_elems(int frames, int H, int W, int C);

/* Block tail (xception.py:88,91-100): out = maxpool3x3s2p1(bn_x(x)) + bn_s(skip); argmax: uint8 per output element */
int istvt_pool_add_fwd(const void* x, const float* bnx, const void* skip, const float* bns, void* out,
                       unsigned char* argmax, int frames, int H, int W, int C, int dtype, istvt_stream_t stream);
/* u (NULL = off): the input of the block's last BatchNorm (xception.py:75), whose output the pooling consumed; with it
 * bnp (that BatchNorm's pack) and s1 / s2 (replica-0 rows of a double[R][2][C] accumulator): the kernel adds the
 * BatchNorm-backward sums  sum dz,  sum dz * xhat  of the values it stores -- no istvt_bn_bwd_stats pass over dz and u */
int istvt_pool_bwd(const void* dout, const unsigned char* argmax, void* dz, int frames, int H, int W, int C,
                   const void* u, const float* bnp, double* s1, double* s2, int dtype, istvt_stream_t stream);
/* input of the stride-2 1x1 skip conv (xception.py:57): out[f][y][x] = in[f][2y][2x] */
int istvt_subsample2(const void* in, void* out, int frames, int H, int W, int C, int dtype, istvt_stream_t stream);

/* ==== next rows: Xception exit flow head, ablation transformers, dropout ==== */
/* Xception.logits (xception.py:208-213): out[f][c] = mean_hw relu(x[f][hw][c]) on NHWC features; relu = 0: plain mean */
int istvt_relu_avgpool_fwd(const void* x, void* out, int frames, int HW, int C, int relu, int dtype,
                           istvt_stream_t stream);
int istvt_relu_avgpool_bwd(const void* x, const void* dout, void* dx, int frames, int HW, int C, int relu, int dtype,
                           istvt_stream_t stream);
/* Token assembly of ViViT / VanillaTr (vivit.py:60-67,74-75,180-186): S sequences of n rows -> n + 1 rows,
 * out[s][0] = tok (+ pos[s % period][0]), out[s][1+i] = src[s][i] (+ pos[s % period][1+i]); pos float
 * [period][pos_rows][D] or NULL.  bwd: dsrc (may be NULL), dtok / dpos accumulate (float). */
int istvt_prepend_fwd(const void* src, const float* tok, const float* pos, void* out, long ldo, long S, int n, int D,
                      int period, int pos_rows, int dtype, istvt_stream_t stream);
/* ws (needed with dtok) = float scratch of istvt_prepend_bwd_ws_rows(S, period, dpos != NULL) * D elements */
int istvt_prepend_bwd(const void* dout, long ldd, void* dsrc, float* dtok, float* dpos, float* ws, long S, int n, int D,
                      int period, int pos_rows, int dtype, istvt_stream_t stream);
int istvt_prepend_bwd_ws_rows(long S, int period, int has_pos);
/* x.mean(dim=1) of [S][n][D] (ViViT pool='mean', vivit.py:79) and its adjoint */
int istvt_seq_mean_fwd(const void* x, long ldx, void* out, long S, int n, int D, int dtype, istvt_stream_t stream);
int istvt_seq_mean_bwd(const void* dout, void* dx, long ldx, long S, int n, int D, int dtype, istvt_stream_t stream);
/* nn.Dropout(p) in training mode (module.py:29,31,78,187; models_copy.py:41-44): Philox4x32-10 keyed by `seed`,
 * mask = one byte per element (1 = kept), y = mask ? x / (1 - p) : 0; backward applies the stored mask. */
int istvt_dropout_fwd(const void* x, long ldx, void* y, long ldy, unsigned char* mask, long M, int D, float p,
                      unsigned long long seed, int dtype, istvt_stream_t stream);
int istvt_dropout_bwd(const void* dy, long ldy, const unsigned char* mask, void* dx, long ldx, long M, int D, float p,
                      int dtype, istvt_stream_t stream);
/* out = a + b on row-strided [M][D] views: the residual add behind an active Dropout (module.py:78,187 with p > 0) */
int istvt_add(const void* a, long lda, const void* b, long ldb, void* out, long ldo, long M, int D, int dtype,
              istvt_stream_t stream);

/* ---- helpers -------------------------------------------------------------------------------- */
/* out[n] += sum_m x[m][n]  (bias gradients); ws = float scratch of istvt_colsum_ws_elems(M, N) elements (one partial row
 * per row block, folded in a fixed order) */
int istvt_colsum(const void* x, float* out, long M, int N, long ld, float* ws, long ws_elems, int dtype,
                 istvt_stream_t stream);
int istvt_colsum_ws_elems(long M, int N);
/* out[i] += sum_{r < rows} ws[r * n + i], rows added in index order by one writer per element: the second stage of every
 * per-column sum of this library (fp32 split-K slabs of narrow weight gradients, bias / token / BatchNorm-affine
 * gradients).  No kernel adds float32 values with atomics; the only atomics left are the double-precision statistics
 * accumulators (BatchNorm sums, the GELU-backward column sums), whose addends are float32 partial sums: a 53-bit
 * accumulator adds 24-bit addends exactly over any realistic spread of magnitudes, so their order does not change
 * the result.  A training step gives the same bits on every run (tests/test_model_gpu.py). */
int istvt_rows_reduce(const float* ws, int rows, long n, float* out, istvt_stream_t stream);
int istvt_cast(const void* in, int in_dtype, void* out, int out_dtype, long n, istvt_stream_t stream);
/* rows x cols cast between row-strided buffers (bf16 operand copies of fp32 weights with line-aligned rows) */
int istvt_cast2d(const void* in, int in_dtype, long ldi, void* out, int out_dtype, long ldo, long rows, int cols,
                 istvt_stream_t stream);
/* fp32 [R][C] -> bf16 [R][C] (row stride ldo) and its transpose bf16 [C][R] (row stride ldt) in one pass: the
 * operand copies of a Linear weight for the forward and the input-gradient GEMMs (R, C multiples of 8) */
int istvt_cast_transpose(const float* in, long ldi, void* out, long ldo, void* outT, long ldt, int R, int C,
                         istvt_stream_t stream);
/* the same for `count` weights in one launch (groups of 32): the bf16 operand copies of every nn.Linear weight the
 * optimizer has just changed, refreshed at the start of a step instead of one launch per weight */
int istvt_cast_transpose_group(int count, const float* const* in, const long* ldi, void* const* out, const long* ldo,
                               void* const* outT, const long* ldt, const int* R, const int* C, istvt_stream_t stream);

/* ---- fused optimizer steps over flat float buffers (train_CNN.py:196-201: torch.optim.SGD(momentum) / AdamW) ----
 * p, g, state: n floats each, 16-byte aligned (parallel.GradBucket(flatten_params=True)).  Semantics are torch.optim's:
 * sgd: g' = g + wd p; buf = first_step ? g' : momentum buf + (1 - dampening) g'; p -= lr (nesterov ? g' + momentum buf : buf)
 * adamw (amsgrad off): p *= 1 - lr wd; m, v moments; p -= lr / (1 - b1^step) * m / (sqrt(v) / sqrt(1 - b2^step) + eps)
 * zero_grad != 0 also writes zeros over g (the next step's zero-grad pass).  grad_scale multiplies g on load: the
 * 1 / world_size of the data-parallel gradient mean (the all-reduce then only sums; no separate scaling pass).
 * momentum == 0 ignores dampening, as torch does. */
int istvt_sgd_momentum(float* p, float* g, float* buf, long n, float lr, float momentum, float dampening,
                       float weight_decay, int nesterov, int first_step, int zero_grad, float grad_scale,
                       istvt_stream_t stream);
int istvt_adamw(float* p, float* g, float* m, float* v, long n, float lr, float beta1, float beta2, float eps,
                float weight_decay, long step, int zero_grad, float grad_scale, istvt_stream_t stream);

/* ---- around the fused step: global gradient norm (clipping, non-finite skip) and per-group hyper-parameters ----
 * istvt_grad_norm: total_norm = || grad_scale * g ||_2 over the n floats of g (16-byte aligned), two stages in a fixed
 * order: every workgroup reduces one contiguous chunk (fp32 per lane over 16 elements, fp64 from there on) into one double
 * of ws (>= istvt_grad_norm_ws_elems(n) doubles), one workgroup sums those.  Chunk and grid depend on n alone and there are
 * no atomics: the same bucket gives the same bits on every rank and in every run.  The second stage writes the STEP-INFO
 * BLOCK `info` (device memory, 8 x 32-bit words). */
typedef struct istvt_step_info {
    float total_norm;  /* || grad_scale * g ||_2 */
    float scale;       /* what the step multiplies g by -- grad_scale x min(1, max_norm / (total_norm + 1e-6)), torch's
                          clip_grad_norm_ coefficient; just grad_scale with max_norm <= 0; 0 for a skipped step */
    int finite;        /* total_norm is finite */
    int applied_steps; /* with skipped_steps touched only with skip_nonfinite != 0 -- a non-finite norm counts as a skipped */
    int skipped_steps; /* step, any other as an applied one (the caller zeroes the block once, or sets applied_steps when it
                          resumes a run) */
    int reserved[3];
} istvt_step_info;
int istvt_grad_norm(const float* g, long n, float grad_scale, float max_norm, int skip_nonfinite, double* ws,
                    long ws_elems, void* info, istvt_stream_t stream);
int istvt_grad_norm_ws_elems(long n);
/* The steps above with {lr, weight_decay} per parameter group (at most 8).  seg_end / seg_group: DEVICE arrays of nseg
 * entries -- sorted end offsets (the last one is n) and the group of the elements [seg_end[i-1], seg_end[i]); boundaries
 * fall at any offset.  group_lr / group_wd: HOST arrays of ngroups floats, passed on to the kernel by value (a scheduler's
 * change costs no copy to the device).  The arithmetic is that of the plain entry points, bit for bit.
 * info (nullable): a step-info block written by istvt_grad_norm on the same stream; its `scale` then replaces grad_scale.
 * skip_nonfinite != 0 (needs info): with finite == 0 parameters and state stay untouched (g is still zeroed when zero_grad
 * is set), and which step this is -- sgd's first-step rule, adamw's bias corrections -- comes from the block's
 * applied_steps instead of first_step / step, so a skipped step leaves no trace. */
int istvt_sgd_momentum_groups(float* p, float* g, float* buf, long n, const long* seg_end, const int* seg_group, int nseg,
                              const float* group_lr, const float* group_wd, int ngroups, float momentum, float dampening,
                              int nesterov, int first_step, int zero_grad, float grad_scale, const void* info,
                              int skip_nonfinite, istvt_stream_t stream);
int istvt_adamw_groups(float* p, float* g, float* m, float* v, long n, const long* seg_end, const int* seg_group, int nseg,
                       const float* group_lr, const float* group_wd, int ngroups, float beta1, float beta2, float eps,
                       long step, int zero_grad, float grad_scale, const void* info, int skip_nonfinite,
                       istvt_stream_t stream);

/* ---- the criterion: nn.BCEWithLogitsLoss, the accuracy count and the epoch meters (train_CNN.py:148,526-536) ----
 * THE METER BLOCK: ten 8-byte words of device memory that istvt_bce_logits ADDS one call to.  One lane updates it with a
 * plain read-modify-write: calls that share a block run on one stream (single writer, stream-ordered, no atomics).  The
 * caller zeroes it (one fill) where an epoch starts. */
typedef struct istvt_loss_meter {
    double loss_sum;       /* sum of the per-sample losses, fp64 */
    double batch_loss_sum; /* sum of the reduced values the calls returned (each rounded to fp32 once): what
                              `train_loss += loss.item()` accumulates; with reduction none, the call's sum */
    long long seen;        /* samples */
    long long correct;     /* tp + tn */
    long long tp, tn, fp, fn; /* prediction z > threshold against y > 0.5 (the unsmoothed target) */
    long long calls;
    long long reserved;
} istvt_loss_meter;
#define ISTVT_TARGET_F32 0
#define ISTVT_TARGET_I64 1
#define ISTVT_TARGET_I32 2
#define ISTVT_TARGET_U8 3
#define ISTVT_REDUCE_NONE 0
#define ISTVT_REDUCE_MEAN 1
#define ISTVT_REDUCE_SUM 2
/* One launch, one workgroup.  z: float logits, sample i at z[i * stride] (stride >= 1 elements: a column of a (B, nc)
 * tensor needs no copy); y: n targets of the type y_kind names, contiguous; w: float[n] per-sample weights or NULL.
 *   y' = y (1 - label_smoothing) + label_smoothing / 2                                 0 <= label_smoothing < 1
 *   l_i = w_i [ (1 - y') z + (1 + (pos_weight - 1) y') (log1p(exp(-|z|)) + max(-z, 0)) ]     (torch's formula; computed as
 *         w_i [ (1 - y') softplus(z) + pos_weight y' softplus(-z) ], the same function without the cancellation)
 *   reduced = sum_i l_i (ISTVT_REDUCE_SUM, and _NONE) or that sum / n (ISTVT_REDUCE_MEAN: by n, as torch, not by sum w)
 *   d_i = d reduced / d z_i = w_i [ (1 - y') sigmoid(z) - pos_weight y' sigmoid(-z) ], times 1 / n for the mean
 * Outputs, each nullable: loss float[n] (per sample), reduced float[1], d float[n] (the UNSCALED logit gradient:
 * istvt_bce_logits_bwd multiplies it by the incoming gradient), meter (an istvt_loss_meter, added to).
 * Per-sample arithmetic is fp32.  The sum is fp64 in a fixed order -- lane t of T = min(1024, max(64, 2^ceil(log2 n)))
 * adds samples t, t + T, ... in ascending order, a binary tree in LDS folds the lanes -- and is rounded to fp32 once; counts
 * are integers.  Two calls give the same bits.  A NaN logit predicts negative (NaN > threshold is false), as the
 * reference's (outputs > 0) does, and makes the sums NaN.  1 <= n <= 2^30; the one workgroup walks n samples in
 * ceil(n / 1024) rounds (DESIGN.md section 16 has the times). */
int istvt_bce_logits(const float* z, long stride, const void* y, int y_kind, const float* w, float pos_weight,
                     float label_smoothing, int reduction, float threshold, long n, float* loss, float* reduced, float* d,
                     void* meter, istvt_stream_t stream);
/* grad[i] = d[i] * (g_per_sample ? g[i] : g[0]); g in DEVICE memory (the gradient autograd hands the criterion: one
 * element for mean / sum, n for none), so (loss * s).backward() needs no host read. */
int istvt_bce_logits_bwd(const float* d, const float* g, int g_per_sample, float* grad, long n, istvt_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* ISTVT_HIP_H */
