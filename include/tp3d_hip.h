/*
 * tp3d_hip.h -- C-ABI of libtp3d_hip.so, the MI355X (gfx950) implementation of the
 * torch_points_kernels hot path used by torch-points3d.
 *
 * The reference has no FFI table for this path: it binds the third-party Python package
 * `torch_points_kernels` by import name (reference torch_points3d/core/spatial_ops/sampling.py:7,
 * core/spatial_ops/neighbour_finder.py:5, core/base_conv/dense.py:19, modules/pointnet2/dense.py:4).
 * Each entry point below is what that package's Python function would bind for one call; the
 * Python wrapper lives in torch_points3d_amd/torchpoints.py and INTEGRATION.md shows the ctypes stub.
 *
 * Conventions
 *  - plain pointers and sizes only; every pointer is DEVICE memory owned by the caller
 *    (the library never allocates, frees or synchronises);
 *  - all tensors are dense, row-major, contiguous; float = IEEE fp32; indices are int64 (the
 *    reference feeds them to torch.gather, core/base_conv/dense.py:75-76);
 *  - `stream` is a hipStream_t passed as void* (NULL = the null stream); work is enqueued, not awaited;
 *  - return 0 on success, a negative TP3D_E_* code otherwise (no exception crosses the boundary);
 *    tp3d_strerror() gives text, tp3d_last_hip_error() the hipError_t of a failed launch;
 *  - squared distances are evaluated as (dx*dx + dy*dy) + dz*dz, fp32, no fused multiply-add, so that
 *    index outputs are bit-exact against the CPU oracle (oracle/tpk_ref_cpu.c).
 */
#ifndef TP3D_HIP_H
#define TP3D_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TP3D_OK 0
#define TP3D_E_BADARG (-1)   /* negative / inconsistent sizes, null pointer with non-empty work */
#define TP3D_E_LAUNCH (-2)   /* hipGetLastError() != hipSuccess after the launch */
#define TP3D_E_UNSORTED (-3) /* reserved: batch vector not sorted (checked by the host wrapper) */
#define TP3D_E_TOOBIG (-4)   /* size exceeds what the kernel's index arithmetic supports */

#define TP3D_ABI_VERSION 39

int tp3d_abi_version(void);
const char *tp3d_strerror(int code);
int tp3d_last_hip_error(void);

/*
 * furthest_point_sample(xyz, npoint)            [reference call: core/spatial_ops/sampling.py:100]
 *   xyz (B,N,3) f32 -> out_idx (B,npoint) int64.  sel[0]=0, then argmax of the running min squared
 *   distance, ties -> lowest index.  scratch: B*N floats (used only when N > TP3D_FPS_MAX_REG_POINTS).
 */
#define TP3D_FPS_MAX_REG_POINTS 32768
int tp3d_fps_f32(const float *xyz, int B, int N, int npoint, float *scratch, int64_t *out_idx, void *stream);

/*
 * fps(pos, batch, ratio) on a ragged batch      [reference call: core/spatial_ops/sampling.py:53-63 (FPSSampler)]
 *   pos (M,3) f32; cloud b owns the rows seg_in[b] .. seg_in[b+1]) and selects seg_out[b+1] - seg_out[b] of them
 *   (seg_in, seg_out: (clouds+1) int64 DEVICE arrays of offsets).  out_idx (seg_out[clouds]) int64 receives GLOBAL
 *   row indices in selection order at out_idx[seg_out[b] ..].  One workgroup per cloud, the arithmetic of
 *   tp3d_fps_f32: first selected = the cloud's first row, running min of (dx*dx+dy*dy)+dz*dz, ties -> lowest index;
 *   equal clouds give tp3d_fps_f32's indices (+ the cloud's first row) bit for bit.
 *   max_cloud_points: the largest cloud (picks the register template; a larger cloud than stated writes nothing).
 *   A cloud without points or with a quota of 0 writes nothing; a quota above the cloud's size is the caller's
 *   error (the host wrapper raises; the kernel stops at the cloud's size).
 *   scratch: M floats, used only when max_cloud_points > TP3D_FPS_MAX_REG_POINTS.
 */
int tp3d_fps_ragged_f32(const float *pos, const int64_t *seg_in, const int64_t *seg_out, int64_t M, int clouds,
                        int max_cloud_points, float *scratch, int64_t *out_idx, void *stream);

/*
 * ball_query(radius, nsample, x, y, mode="dense", sort)
 *                                               [reference call: core/spatial_ops/neighbour_finder.py:164,
 *                                                core/losses/dirichlet_loss.py:52]
 *   x (B,N,3), y (B,np,3) -> idx (B,np,nsample) int64, dist2 (B,np,nsample) f32.
 *   sort=0: hits (d2 < r*r, strict) in ascending index order, first nsample; remaining slots repeat the
 *           first hit (0 if none); dist2 = -1 in padded slots.
 *   sort=1: the nsample closest hits, closest first (ties by index), padded with the closest.
 *   workspace (optional, tp3d_ball_query_workspace_bytes(B, B*N, N) bytes): with it, clouds of >= 2048 points are
 *   searched through a uniform grid (27 cells per query) with bit-identical output; NULL = brute force.
 */
int tp3d_ball_query_dense_f32(const float *x, const float *y, int B, int N, int np, float radius, int nsample,
                              int sort, int64_t *idx, float *dist2, void *workspace, size_t workspace_bytes,
                              void *stream);
size_t tp3d_ball_query_workspace_bytes(int num_clouds, int64_t rows, int max_cloud_points);

/*
 * ball_query(..., mode="partial_dense", batch_x, batch_y)
 *                                               [reference call: core/spatial_ops/neighbour_finder.py:31-37]
 *   x (M,3) with ascending batch_x (M) int64, y (Nq,3) with batch_y (Nq) int64.
 *   idx (Nq,nsample) int64 = global rows of x, padded with -1; dist2 padded with -1.
 *   Optional grid acceleration: seg_x (num_clouds+1) int64 device array of cloud row offsets into x,
 *   max_cloud_points = the largest cloud, workspace = tp3d_ball_query_workspace_bytes(num_clouds, M,
 *   max_cloud_points) bytes; pass NULL / 0 for the brute-force scan of each query's cloud segment.
 *   reuse_grid != 0: the workspace still holds the grid the previous call on it built for the SAME x, seg_x,
 *   max_cloud_points and radius (e.g. the last block of a KPConv level and the strided block of the next level
 *   search the same support with the same radius, modules/KPConv/blocks.py:52): the build is skipped.
 */
int tp3d_ball_query_partial_dense_f32(const float *x, const float *y, const int64_t *batch_x,
                                      const int64_t *batch_y, int64_t M, int64_t Nq, float radius, int nsample,
                                      int sort, int64_t *idx, float *dist2, const int64_t *seg_x, int num_clouds,
                                      int max_cloud_points, void *workspace, size_t workspace_bytes, int reuse_grid,
                                      void *stream);

/*
 * three_nn(unknown, known) -> (dist, idx)       [reference call: core/base_conv/dense.py:136]
 *   unknown (B,n,3), known (B,m,3), m >= 3 -> dist (B,n,3) f32 Euclidean (sqrt), idx (B,n,3) int64;
 *   ascending distance, ties -> lowest index.
 */
int tp3d_three_nn_f32(const float *unknown, const float *known, int B, int n, int m, float *dist, int64_t *idx,
                      void *stream);

/*
 * three_interpolate(features, idx, weight)      [reference call: core/base_conv/dense.py:140]
 *   features (B,C,m), idx (B,n,3) int64, weight (B,n,3) -> out (B,C,n) = (w0*f0 + w1*f1) + w2*f2.
 *   bwd: grad_out (B,C,n) -> grad_features (B,C,m) (overwritten, not accumulated); atomic-free and bitwise
 *        reproducible; needs tp3d_scatter_workspace_bytes(B, 3*n, m, 1) bytes of device workspace.
 */
int tp3d_three_interpolate_fwd_f32(const float *features, const int64_t *idx, const float *weight, int B, int C,
                                   int m, int n, float *out, void *stream);
int tp3d_three_interpolate_bwd_f32(const float *grad_out, const int64_t *idx, const float *weight, int B, int C,
                                   int m, int n, float *grad_features, void *workspace, size_t workspace_bytes,
                                   void *stream);

/*
 * Device workspace (bytes) of the two scatter-add backward entry points: the inverse index of an
 * index table with L slots per cloud pointing into nbins destinations (+ the permuted weights).
 */
size_t tp3d_scatter_workspace_bytes(int B, int L, int nbins, int with_weights);

/*
 * grouping_operation(features, idx)             [reference call: modules/pointnet2/dense.py:38,45]
 *   features (B,C,N), idx (B,np,ns) int64 -> out (B,C,np,ns); bwd scatters grad_out into (B,C,N)
 *   (overwritten, not accumulated); atomic-free and bitwise reproducible; needs
 *   tp3d_scatter_workspace_bytes(B, np*ns, N, 0) bytes of device workspace.
 */
int tp3d_group_fwd_f32(const float *features, const int64_t *idx, int B, int C, int N, int np, int ns, float *out,
                       void *stream);
int tp3d_group_bwd_f32(const float *grad_out, const int64_t *idx, int B, int C, int N, int np, int ns,
                       float *grad_features, void *workspace, size_t workspace_bytes, void *stream);

/* =====================================================================================================
 * Grouped-MLP aggregation in channel-last ("rows") layout: the work PointNetMSGDown / DenseFPModule /
 * GlobalDenseBaseModule do around their 1x1-conv GEMMs (reference modules/pointnet2/dense.py:36-75,
 * core/base_conv/dense.py:102-184, core/common_modules/dense_modules.py:5-29).  Activations are (rows, C)
 * row-major fp32; the GEMMs themselves are plain library GEMMs issued by the host wrapper.
 * ===================================================================================================== */

/* out[(b,j,s), :] = [ (pos[b,idx[b,j,s]] - new_pos[b,j]) (/ radius if normalize), x_cl[b,idx[b,j,s], 0:C], 0.. ]
 * pos (B,N,3), new_pos (B,np,3), x_cl (B,N,C) or NULL when C == 0, idx (B,np,ns) -> out (B*np*ns, ld),
 * ld >= 3+C; columns past 3+C are written as zeros (row padding for 16-byte aligned GEMM operands). */
int tp3d_group_concat_fwd_f32(const float *pos, const float *new_pos, const float *x_cl, const int64_t *idx, int B,
                              int N, int np, int ns, int C, int ld, float radius, int normalize, float *out,
                              void *stream);

/* Scatter-add of row gradients back onto their source points, atomic-free (inverse index + gather-sum):
 *   grad_x_cl[b,k,0:C] = sum over slots l of cloud b with idx[b,l] == k (ascending l) of
 *                        weight[b,l] * grad_rows[(b, l/div), col0 : col0+C]          (weight NULL -> 1)
 * grad_rows (B, L/div, ld); idx (B, L) with values in [0, nbins); grad_x_cl (B, nbins, C).
 * workspace: tp3d_scatter_workspace_bytes(B, L, nbins, weight != NULL). */
int tp3d_rows_scatter_bwd_f32(const float *grad_rows, const int64_t *idx, const float *weight, int B, int L, int div,
                              int nbins, int ld, int col0, int C, float *grad_x_cl, void *workspace,
                              size_t workspace_bytes, void *stream);
/* The same in two halves: the inverted table depends on idx / weight only (geometry, not features), so it can be built
 * ahead of the backward pass -- tp3d_rows_scatter_invert fills `workspace` (same size query), tp3d_rows_scatter_apply_f32
 * consumes a table built for the same (idx, weight, B, L, div, nbins); with_weights = the table was built with weights.
 * Sums run in ascending slot order; a destination with more than 128 slots is summed in 16 contiguous pieces that are
 * then added in order (fixed association: reproducible, not the sequential sum bit for bit). */
int tp3d_rows_scatter_invert(const int64_t *idx, const float *weight, int B, int L, int div, int nbins, void *workspace,
                             size_t workspace_bytes, void *stream);
int tp3d_rows_scatter_apply_f32(const float *grad_rows, int B, int L, int div, int nbins, int ld, int col0, int C,
                                int with_weights, float *grad_x_cl, void *table, size_t table_bytes, void *stream);

/* BatchNorm statistics of Y (M, C): mean, invstd, scale = gamma*invstd and shift = beta; the normalised value is
 * always formed as (y - mean)*scale + shift (a folded shift beta - mean*scale would cancel against y*scale in fp32
 * when |mean| >> std).  Batch statistics are accumulated as shifted sums per row chunk and merged with Chan's formula.
 * training != 0: batch mean / biased variance (running stats updated in place with `momentum`, unbiased var;
 * *num_batches_tracked, if given, incremented on the device -- BatchNorm's counter without a launch of its own);
 * training == 0: running statistics.  workspace: tp3d_bn_workspace_floats(M, C) floats. */
size_t tp3d_bn_workspace_floats(int64_t M, int C);
int tp3d_bn_stats_f32(const float *Y, int64_t M, int C, float eps, float momentum, const float *gamma,
                      const float *beta, float *running_mean, float *running_var, int64_t *num_batches_tracked,
                      int training, float *mean, float *invstd, float *scale, float *shift, float *workspace,
                      void *stream);

/* out = LeakyReLU_slope((Y - mean)*scale + shift) over (M, C);  the pooled form also takes the max over each group of
 * ns consecutive rows (first maximum wins) and records its row in argmax (G, C). */
int tp3d_bn_act_f32(const float *Y, const float *mean, const float *scale, const float *shift, float slope, int64_t M,
                    int C, float *out, void *stream);
int tp3d_bn_act_maxpool_f32(const float *Y, const float *mean, const float *scale, const float *shift, float slope,
                            int64_t G, int ns, int C, float *out, int *argmax, void *stream);

/* Backward of out = act(BN(Y)): dbeta, dgamma (C) and dY (M, C).  dA is (M, C), or -- with argmax != NULL --
 * the gradient (M/ns, C) of the pooled output.  workspace: tp3d_bn_workspace_floats(M, C) floats. */
int tp3d_bn_act_bwd_f32(const float *dA, const int *argmax, const float *Y, const float *scale, const float *shift,
                        const float *mean, const float *invstd, float slope, int64_t M, int ns, int C, int training,
                        float *dbeta, float *dgamma, float *dY, float *workspace, void *stream);
/* Only the reductions of that backward pass: dbeta, dgamma (C) and the two per-channel terms the fused GEMMs
 * (tp3d_gemm_rows_bnbwd_sp_f32, tp3d_gemm_tn_bn_narrow_f32) subtract while they form dY:  c1 = dbeta / M,  c2 = invstd * dgamma / M
 * (both zero with training == 0).  Same arguments and workspace as tp3d_bn_act_bwd_f32, no dY. */
int tp3d_bn_bwd_reduce_f32(const float *dA, const int *argmax, const float *Y, const float *scale, const float *shift,
                           const float *mean, const float *invstd, float slope, int64_t M, int ns, int C, int training,
                           float *dbeta, float *dgamma, float *c1, float *c2, float *workspace, int reverse,
                           void *stream);

/* out[(b,i), :] = [ (w0*f0 + w1*f1) + w2*f2 , skip_cl[b,i,0:C2], 0.. ],  f_t = feat_cl[b, idx[b,i,t], 0:C1]
 * feat_cl (B,m,C1), idx/weight (B,n,3), skip_cl (B,n,C2) or NULL -> out (B*n, ld), ld >= C1+C2 (zero padded). */
int tp3d_interp_concat_fwd_f32(const float *feat_cl, const int64_t *idx, const float *weight, const float *skip_cl,
                               int B, int m, int n, int C1, int C2, int ld, float *out, void *stream);

/* `reverse` (tp3d_gemm_tn_x3_act_red_f32, tp3d_gemm_rows_narrow_f32, tp3d_gemm_tn_bn_narrow_f32, tp3d_gemm_rows_bnact_sp_f32, tp3d_gemm_rows_bnact_x3_f32, tp3d_gemm_rows_bnbwd_sp_f32, tp3d_gemm_tn_x3_f32,
 * tp3d_gemm_tn_x3_act_f32, tp3d_bn_bwd_reduce_f32): 1 = walk the row blocks of the (M, .) operands last to first.  The result
 * is the same set of products / sums (the contractions over rows sum their blocks in the walked order: reproducible per
 * direction, the two directions differ by rounding).  A chain of kernels over 268 MB activation matrices alternates the
 * direction so that each kernel starts on the rows its predecessor touched last -- what the 256 MB memory-side cache
 * still holds (measured: 7.92 -> 7.76 ms per training step of the headline network). */
/* Tall-skinny GEMM of a shared-MLP layer, fp32 MFMA:  C[M,N] = A[M,K] * Bt[N,K]^T  (row-major, K % 4 == 0).
 * Forward: A = rows, Bt = W exactly as nn.Conv2d stores it (Cout x Cin).  With stat_partial != NULL the epilogue also
 * writes shifted partial column sums of C: stat_partial[chunk][4][N] = sum d, sum d^2 (d = value - shift), shift, rows;
 * chunk < tp3d_gemm_rows_stat_chunks(M, N); the buffer holds tp3d_gemm_rows_stat_floats(M, N) floats;
 * tp3d_bn_finalize_f32 turns them into the BatchNorm statistics -- no separate statistics pass over C.
 * Without statistics and with `workspace` (tp3d_gemm_rows_workspace_floats(M, N, K) floats, 0 = not needed) a long
 * contraction with few output tiles is split over K-ranges into partial slabs summed in fixed order. */
size_t tp3d_gemm_rows_stat_floats(int64_t M, int N);
int tp3d_gemm_rows_stat_chunks(int64_t M, int N);
size_t tp3d_gemm_rows_workspace_floats(int64_t M, int N, int K);
int tp3d_gemm_rows_f32(const float *A, const float *Bt, int64_t M, int N, int K, float *C, float *stat_partial,
                       float *workspace, void *stream);
/* The same contraction with the eval-mode BatchNorm + LeakyReLU of its OUTPUT applied to the accumulators:
 *   C = LeakyReLU((A Bt^T - mean[n]) * scale[n] + beta[n])      (mean / scale / beta: N floats, as tp3d_bn_stats_f32 leaves them)
 * -- one launch per Linear -> BatchNorm (running statistics) -> activation layer of an inference pass
 * (core/common_modules/base_modules.py: FastBatchNorm1d + activation after nn.Linear).  workspace as for
 * tp3d_gemm_rows_f32 without statistics (K-split slabs; the epilogue then runs in the slab sum, which needs N % 4 == 0). */
int tp3d_gemm_rows_epi_f32(const float *A, const float *Bt, int64_t M, int N, int K, const float *mean, const float *scale,
                           const float *beta, float slope, float *C, float *workspace, void *stream);
/* The same fused contraction on the split-role kernel (csrc/gemm_rows_sp.hip: four MFMA waves fed by four loader waves
 * that apply the prologue on their way into LDS, so it costs the MFMA waves nothing).  act_out != NULL additionally
 * receives the activated rows (M,K) the backward pass of the next layer contracts with (training); stat_partial as for
 * tp3d_gemm_rows_f32 but with tp3d_gemm_rows_sp_chunks(M, N, K, act_out != NULL) chunks of 4 * N floats.  Shapes: K % 4 == 0,
 * 4 <= K <= 512, N <= 64 or (N % 128 not in 1..64 and N <= 1024 in 1, 2, 4 or 8 column tiles), at least 512 output
 * tiles --
 * tp3d_gemm_rows_sp_chunks returns 0 for a shape that is not served (TP3D_E_BADARG from the launch).
 * Replaces the Conv2d -> BatchNorm2d -> LeakyReLU hand-over between two layers of MLP2D
 * (core/common_modules/dense_modules.py:25-29). */
int tp3d_gemm_rows_sp_chunks(int64_t M, int N, int K, int with_act_out);
int tp3d_gemm_rows_bnact_sp_f32(const float *Y, const float *mean, const float *scale, const float *beta, float slope,
                                const float *Bt, int64_t M, int N, int K, float *C, float *stat_partial, float *act_out,
                                int reverse, void *stream);
/* tp3d_gemm_rows_bnact_sp_f32 with the fp32 contraction carried by the bf16 matrix pipe (csrc/gemm_rows_x3.hip): every operand
 * value split exactly into three bf16 terms by the loader waves (x3_split.h), the product as the six term pairs of weight
 * >= 2^-15, each a v_mfma_f32_32x32x16_bf16 with fp32 accumulation.  Same arguments, outputs and statistics layout;
 * tp3d_gemm_rows_x3_chunks is its chunk count / shape rule (0: not served -- more than 64 output columns, K <= 512). */
int tp3d_gemm_rows_x3_chunks(int64_t M, int N, int K, int with_act_out);
int tp3d_gemm_rows_bnact_x3_f32(const float *Y, const float *mean, const float *scale, const float *beta, float slope,
                                const float *Bt, int64_t M, int N, int K, float *C, float *stat_partial, float *act_out,
                                int reverse, void *stream);

/* Input-gradient GEMM of a layer on the split-role kernel, with the layer's BatchNorm + activation BACKWARD formed by the
 * loader waves:  C[M,N] = dY[M,K] * Bt[N,K]^T,  dY = scale*((dA*act'(z) - c1) - (Y - mean)*c2),  z = (Y - mean)*scale + beta.
 * Y (M,K) pre-BatchNorm output of the layer, dA (M,K) gradient of its activated output -- or, with argmax != NULL, the
 * gradient (M/ns, K) of its max-pooled output and the winning rows (tp3d_bn_act_maxpool_f32; ns a power of two >= 64) --, c1 / c2 (K) from
 * tp3d_bn_bwd_reduce_f32, Bt (N,K) = W^T of the layer (N = its input width).  dY_out (M,K), if not NULL, receives dY for the weight-gradient contraction; ldc >= N is the row stride of C in
 * floats (the gradient of a column range of wider rows: the grouped rows' feature columns) and the pad_lo <= 32 columns
 * in front of / pad_hi <= 32 behind that range are written as zeros.  Shapes: as tp3d_gemm_rows_bnact_sp_f32 with K <= 256
 * (tp3d_gemm_rows_bnbwd_sp_serves).  Autograd of Conv2d -> BatchNorm2d -> LeakyReLU
 * (core/common_modules/dense_modules.py:25-29). */
int tp3d_gemm_rows_bnbwd_sp_serves(int64_t M, int N, int K);
int tp3d_gemm_rows_bnbwd_sp_f32(const float *Y, const float *dA, const float *mean, const float *scale, const float *beta,
                                const float *c1, const float *c2, float slope, const float *Bt, int64_t M, int N, int K,
                                float *C, int ldc, int pad_lo, int pad_hi, float *dY_out, const int *argmax, int ns,
                                int reverse, void *stream);
/* `partial` is consumed: with more than 64 chunks they are first folded, in place, into 32 slices. */
int tp3d_bn_finalize_f32(float *partial, int chunks, int64_t M, int C, float eps, float momentum, const float *gamma,
                         const float *beta, float *running_mean, float *running_var, int64_t *num_batches_tracked,
                         float *mean, float *invstd, float *scale, float *shift, void *stream);

/* Weight gradient of the FIRST layer of a shared MLP on grouped rows (K <= 16 input channels, K % 4 == 0) with dY formed
 * on the fly:  out[n,k] = sum_r dY[r,n] * A[r,k],  dY = BatchNorm + LeakyReLU backward of (Y, dA) as in
 * tp3d_gemm_rows_bnbwd_sp_f32 (c1_n / c2_n from tp3d_bn_bwd_reduce_f32).  Y, dA (M,N), A (M,K) -> out (N,K).
 * One streaming pass over Y and dA (2*M*N*K flops against 8*M*N bytes: HBM-bound); fixed summation order.
 * workspace: tp3d_gemm_tn_bn_narrow_workspace_floats(M, N, K) floats.
 * Autograd of Conv2d -> BatchNorm2d -> LeakyReLU (core/common_modules/dense_modules.py:25-29). */
int tp3d_gemm_tn_bn_narrow_serves(int64_t M, int N, int K);
/* The forward contraction of such a layer (same shape rule):  Y (M,N) = A (M,K) W (N,K)^T, k ascending per output, one
 * streaming pass (4 M (N + K) bytes: write-dominated; the MFMA tile kernel pads K to its 32-wide step and runs at 3 TB/s).
 * stat_partial != NULL: tp3d_gemm_rows_narrow_chunks(M) chunks of [4][N] floats (sum d, sum d^2, shift, rows) in the layout
 * tp3d_bn_finalize_f32 folds.  Conv2d 1x1 bias=False of core/common_modules/dense_modules.py:25-29. */
int tp3d_gemm_rows_narrow_chunks(int64_t M);
int tp3d_gemm_rows_narrow_f32(const float *A, const float *W, int64_t M, int N, int K, float *Y, float *stat_partial,
                              int reverse, void *stream);
size_t tp3d_gemm_tn_bn_narrow_workspace_floats(int64_t M, int N, int K);
int tp3d_gemm_tn_bn_narrow_f32(const float *Y, const float *dA, const float *mean_n, const float *scale_n,
                               const float *beta_n, const float *c1_n, const float *c2_n, float slope_n, const float *A,
                               int64_t M, int N, int K, float *out, float *workspace, int reverse, void *stream);

/* Weight gradient of a 1x1 conv / shared-MLP layer:  out[n,k] = sum_r dY[r,n] * A[r,k]
 * dY (M,N), A (M,K) row-major -> out (N,K); rows split over the grid, fp32 MFMA, fixed-order reduction of the
 * splits (reproducible).  workspace: tp3d_gemm_tn_workspace_floats(M, N, K) floats. */
size_t tp3d_gemm_tn_workspace_floats(int64_t M, int N, int K);
int tp3d_gemm_tn_f32(const float *dY, const float *A, int64_t M, int N, int K, float *out, float *workspace,
                     void *stream);

/* The same contraction with the fp32 products carried by the bf16 matrix pipe (csrc/gemm_tn_x3.hip): every operand value is
 * split exactly into three bf16 terms (3 x 8 significand bits) by the loader waves of a split-role kernel, and the product
 * is the sum of the term pairs -- terms = 9: all nine, every product exact as in the fp32 MFMA; terms = 6: the six of
 * weight >= 2^-16 -- each a v_mfma_f32_32x32x16_bf16 with fp32 accumulation.  The contraction then runs at the rate HBM
 * delivers the rows instead of at the fp32 MFMA rate.  Serves M >= 131072, N >= 64, K >= 64 (not both 64), N % 4 == 0, K % 4 == 0, M * max(N, K) < 2^30, and an output that
 * fills at least 80 % of at most two tiles (128- or 64-wide, or 128 + a 32-column strip)
 * (tp3d_gemm_tn_x3_serves); other shapes: tp3d_gemm_tn_f32.  workspace: tp3d_gemm_tn_x3_workspace_floats floats.
 * Reference: the weight gradient of Conv2d 1x1 in MLP2D (core/common_modules/dense_modules.py:5-12), autograd's
 * grad_output^T @ input. */
int tp3d_gemm_tn_x3_serves(int64_t M, int N, int K);
size_t tp3d_gemm_tn_x3_workspace_floats(int64_t M, int N, int K);
int tp3d_gemm_tn_x3_f32(const float *dY, const float *A, int64_t M, int N, int K, int terms, float *out, float *workspace,
                        int reverse, void *stream);
/* ... with the A operand formed on the fly: dW = dY^T * LeakyReLU((Yp - mean_k) * scale_k + beta_k), Yp (M, K) the previous
 * layer's pre-BatchNorm output, mean_k / scale_k / beta_k its statistics rows (K floats each).  The loader waves evaluate
 * the forward kernels' expression in their order, so the result is bit for bit that of the plain entry point on the
 * activated rows -- which the forward pass then need not write. */
int tp3d_gemm_tn_x3_act_f32(const float *dY, const float *Yp, const float *mean_k, const float *scale_k, const float *beta_k,
                            float slope_k, int64_t M, int N, int K, int terms, float *out, float *workspace, int reverse, void *stream);
/* ... and, from one more operand stream, the BatchNorm-backward REDUCTIONS of the layer Yp belongs to: dA_k (M,K) is the
 * gradient of that layer's activated output, invstd_k (K) its statistics row; red_out (4,K) = dbeta, dgamma,
 * c1 = dbeta / M, c2 = invstd * dgamma / M (zero with training == 0) -- what tp3d_bn_bwd_reduce_f32(dA_k, Yp) returns,
 * without that pass (its 8 M K bytes become 4 M K here: Yp is already streaming through this kernel's loader waves).
 * tp3d_gemm_tn_x3_red_chunks(M,N,K): 0 = shape not served (needs one tile column, K <= 128, and a 128 x 128, 128 x 64 or 64 x 64 tile), else the chunks of
 * [2][K] floats red_workspace must hold.  terms == 6. */
int tp3d_gemm_tn_x3_red_chunks(int64_t M, int N, int K);
int tp3d_gemm_tn_x3_act_red_f32(const float *dY, const float *Yp, const float *mean_k, const float *scale_k,
                                const float *beta_k, const float *invstd_k, float slope_k, const float *dA_k, int training,
                                int64_t M, int N, int K, int terms, float *out, float *workspace, float *red_out,
                                float *red_workspace, int reverse, void *stream);

/* KPConv rigid convolution, stage 1 (reference modules/KPConv/convolution_ops.py:19-98):
 *   weighted[q, k, :] = sum_n h(|(support[nbr[q,n]] - query[q]) - k_points[k]|) * features[nbr[q,n], :]
 * query (Nq,3), support (M,3), neighbors (Nq,Mn) int64 with -1 (or >= M) = shadow neighbour, features (M,Cin),
 * k_points (KP,3), KP <= 16 -> weighted (Nq, KP, Cin).  influence: 0 constant, 1 linear (max(1 - d/extent, 0)),
 * 2 gaussian (sigma = 0.3*extent); closest != 0 keeps only the nearest kernel point per neighbour.
 * Stage 2 (:101-105) is one GEMM  (Nq, KP*Cin) x (KP*Cin, Cout)  issued by the host wrapper. */
int tp3d_kpconv_weighted_f32(const float *query, const float *support, const int64_t *neighbors,
                             const float *features, const float *k_points, int64_t Nq, int64_t M, int Mn, int Cin,
                             int KP, float extent, int influence, int closest, float *weighted, void *stream);

/* Backward of stage 1 wrt the input features (autograd through convolution_ops.py:92-98):
 *   d_features[m, :] = sum over (q,n) with neighbors[q,n] == m of sum_k h(...) * d_weighted[q, k, :]
 * d_weighted (Nq, KP, Cin) = d_out @ W2^T (host GEMM) -> d_features (M, Cin), overwritten; atomic-free and
 * reproducible: per-slot gradient rows (Nq*Mn, Cin) are formed per query and summed per support point in slot order
 * through the inverted neighbour table.
 *   inverse: tp3d_kpconv_bwd_workspace_bytes(M, Nq*Mn) bytes holding the inverted table; it is (re)built by the call
 *            unless inverse_ready != 0, i.e. the caller kept the buffer of an earlier call on the SAME neighbours / M
 *            (tp3d_nbr_maxpool_bwd_f32 shares it: a strided block inverts its table once for both; with precomputed
 *            neighbour tables it is built once for the whole training run);
 *   workspace: tp3d_kpconv_grad_workspace_bytes(M, Nq*Mn, Cin) bytes for the per-slot rows. */
size_t tp3d_kpconv_bwd_workspace_bytes(int64_t M, int64_t slots);
size_t tp3d_kpconv_grad_workspace_bytes(int64_t M, int64_t slots, int Cin);
int tp3d_kpconv_bwd_features_f32(const float *query, const float *support, const int64_t *neighbors,
                                 const float *k_points, const float *d_weighted, int64_t Nq, int64_t M, int Mn,
                                 int Cin, int KP, float extent, int influence, int closest, float *d_features,
                                 void *inverse, size_t inverse_bytes, int inverse_ready, void *workspace,
                                 size_t workspace_bytes, void *stream);

/* KPConv deformable convolution, stage 1 (reference modules/KPConv/convolution_ops.py:110-235, KPConv_deform_ops).
 * The rigid arguments plus offsets (Nq,KP,3) and modulations (Nq,KP) or NULL (= 1).  With
 *   rel[q,n] = support[nbr[q,n]] - query[q]   (shadow neighbour: the point (1e6,1e6,1e6), zero features),
 *   dk[q,k]  = k_points[k] + offsets[q,k],    d2[q,n,k] = |rel[q,n] - dk[q,k]|^2  ((dx*dx + dy*dy) + dz*dz, no fma),
 *   in_range[q,n] = any_k d2[q,n,k] < extent^2   (extent^2 formed in double, rounded to fp32),
 * it writes
 *   weighted[q,k,:] = modulations[q,k] * sum_n in_range[q,n] * h(d2[q,n,k]) * features[nbr[q,n], :]      (Nq,KP,Cin)
 *   kp_min_d2[q,k]  = min over ALL Mn slots of d2[q,n,k]  (or NULL), kp_argmin[q,k] its slot, first minimum (int32, or NULL;
 *                     needs kp_min_d2) -- the only use the reference makes of its (Nq,Mn,KP) distances (losses.py:12).
 * h: 0 constant (d2 < extent^2), 1 linear (max(1 - sqrt(d2)/extent, 0)), 2 gaussian (exp(-d2 / (2 (0.3 extent)^2 + 1e-9))).
 * Sum aggregation only (the reference's deformable "closest" raises).  M, Mn >= 1, KP <= 16.  Mn <= 64 runs on the fp32
 * matrix pipe, larger tables on the per-lane-FMA kernel.  Stage 2 is the same host GEMM as for the rigid convolution. */
int tp3d_kpconv_deform_weighted_f32(const float *query, const float *support, const int64_t *neighbors,
                                    const float *features, const float *k_points, const float *offsets,
                                    const float *modulations, int64_t Nq, int64_t M, int Mn, int Cin, int KP, float extent,
                                    int influence, float *weighted, float *kp_min_d2, int32_t *kp_argmin, void *stream);

/* Backward of the deformable stage 1.  d_weighted (Nq,KP,Cin) = d_out @ W2^T (host GEMM; the gradient of the MODULATED
 * weighted features), d_kp_min_d2 (Nq,KP) or NULL (then kp_argmin may be NULL), kp_argmin as the forward wrote it.
 *   s[q,n,k]           = in_range[q,n] * sum_c features[nbr[q,n],c] * d_weighted[q,k,c]
 *   d_offsets[q,k,:]   = sum_n modulations[q,k] * s[q,n,k] * dh/d dk  -  2 d_kp_min_d2[q,k] * (rel[q,argmin] - dk[q,k])
 *   d_modulations[q,k] = sum_n s[q,n,k] * h(d2[q,n,k])                                     (NULL without modulations)
 *   d_features[m,:]    = sum over (q,n) with nbr[q,n] == m of sum_k modulations * in_range * h * d_weighted[q,k,:]
 *                        (NULL: not wanted; then inverse / workspace are not touched)
 * No gradient flows through in_range, positions or k_points.  linear influence: the term of a pair with d2 == 0 (the
 * reference: NaN) and of a pair at or beyond the extent is 0.  All outputs are overwritten; atomic-free, fixed
 * summation order.  inverse / inverse_ready / workspace: exactly as for tp3d_kpconv_bwd_features_f32
 * (tp3d_kpconv_bwd_workspace_bytes, tp3d_kpconv_grad_workspace_bytes); the inverted table is shared with it. */
int tp3d_kpconv_deform_bwd_f32(const float *query, const float *support, const int64_t *neighbors, const float *features,
                               const float *k_points, const float *offsets, const float *modulations,
                               const float *d_weighted, const float *d_kp_min_d2, const int32_t *kp_argmin, int64_t Nq,
                               int64_t M, int Mn, int Cin, int KP, float extent, int influence, float *d_features,
                               float *d_offsets, float *d_modulations, void *inverse, size_t inverse_bytes,
                               int inverse_ready, void *workspace, size_t workspace_bytes, void *stream);

/* Geometric relation rows of Relation-Shape convolution (reference modules/RSConv/dense.py:86-101):
 *   out[(b,j,s), 0:10] = [ |d|, new_pos[b,j] (3), p (3), d (3) ],  p = pos[b, idx[b,j,s]],  d = p - new_pos[b,j];
 *   columns 10 .. ld-1 are zero.  pos (B,N,3), new_pos (B,np,3), idx (B,np,ns) -> out (B*np*ns, ld), ld >= 10. */
int tp3d_relation_rows_f32(const float *pos, const float *new_pos, const int64_t *idx, int B, int N, int np, int ns,
                           int ld, float *out, void *stream);

/* inverse-distance weights of DenseFPModule (core/base_conv/dense.py:137-139): dist (rows,3) -> weight (rows,3) */
int tp3d_idw_weights_f32(const float *dist, int64_t rows, float *weight, void *stream);

/* GridSampling3D (reference core/data_transform/grid_transform.py:84-141; sampler of the strided KPConv blocks,
 * modules/KPConv/blocks.py:60-61,79).  pos (N,3) f32, batch (N) int64 or NULL, voxel edge `size`:
 *   coords = round_half_even(pos / size);  points sharing (batch, coords) form a cluster;  clusters are numbered in
 *   ascending (batch, z, y, x) order (torch_cluster grid_cluster key + torch.unique(sorted), :117-122).
 * Three steps, because the reference's own pipeline has two device->host waits (extent of the key, number of
 * clusters) and this library never synchronises:
 *   1. tp3d_voxel_bounds_f32   -> bounds[8] int32 on the DEVICE: min xyz, max xyz of coords, max batch, bad-input flag;
 *                                 the host copies them back and passes them to step 2 as a HOST array;
 *   2. tp3d_voxel_cluster_f32  -> cluster (N) id of each point; order (N) point indices sorted by (cluster, index);
 *                                 cluster_start (N+1; [0..K] valid) slot range of each cluster in `order`;
 *                                 last (N; [0..K) valid) highest point index of each cluster = the reference's
 *                                 unique_pos_indices (consecutive_cluster's scatter_, last write wins);
 *                                 meta (1 + clouds) int64 on the device, clouds = bounds[6] + 1 (1 without batch):
 *                                 meta[0] = K, meta[1 + b] = clusters of clouds 0..b together (0 for a cloud without
 *                                 points): the row offsets of the sampled batch vector.  workspace:
 *                                 tp3d_voxel_workspace_bytes(N);
 *   3. tp3d_cluster_mean_f32   -> out (K,C) = scatter_mean(x (N,C)) summed in ascending point order (:78), and
 *      tp3d_cluster_majority_i64 -> out (K) = majority label, ties -> lowest (:72-76); num_classes = max-min+1.
 */
int tp3d_voxel_bounds_f32(const float *pos, const int64_t *batch, int64_t N, float size, int32_t *bounds, void *stream);
size_t tp3d_voxel_workspace_bytes(int64_t N);
int tp3d_voxel_cluster_f32(const float *pos, const int64_t *batch, int64_t N, float size, const int32_t *bounds_host,
                           int64_t *cluster, int64_t *order, int64_t *cluster_start, int64_t *last, int64_t *meta,
                           void *workspace, size_t workspace_bytes, void *stream);
int tp3d_cluster_mean_f32(const float *x, const int64_t *order, const int64_t *cluster_start, int64_t K, int C,
                          float *out, void *stream);
int tp3d_cluster_majority_i64(const int64_t *labels, const int64_t *order, const int64_t *cluster_start, int64_t K,
                              int64_t min_label, int64_t num_classes, int64_t *out, void *stream);

/* Exact k nearest neighbours (reference call sites: core/spatial_ops/interpolate.py:27,69 -- KNNInterpolate /
 * FPModule_PD, k = 1 in the KPConv decoders; core/spatial_ops/neighbour_finder.py:42-47 -- KNNNeighbourFinder, k = 16
 * in RandLA-Net; both go through torch_cluster `knn`).
 *   partial_dense: x (M,3) support with sorted batch ids, seg_x (num_clouds+1) row offsets of the clouds in x,
 *                  y (Nq,3) queries with batch_y (Nq) -> idx (Nq,k) global rows of x, dist2 (Nq,k) squared distances;
 *   dense:         x (B,N,3), y (B,np,3) -> idx (B,np,k) cloud-local, dist2 (B,np,k).
 *   Closest first, ties by lower index; slots a cloud of fewer than k points cannot fill hold -1 / -1.0.
 *   cell: preferred grid cell edge (e.g. the sampling grid size); <= 0 lets the library choose.
 *   workspace: tp3d_knn_workspace_bytes(num_clouds, rows of x, largest cloud) bytes. */
size_t tp3d_knn_workspace_bytes(int num_clouds, int64_t rows, int max_cloud_points);
int tp3d_knn_partial_dense_f32(const float *x, const float *y, const int64_t *batch_y, const int64_t *seg_x,
                               int num_clouds, int max_cloud_points, int64_t M, int64_t Nq, int k, float cell,
                               int64_t *idx, float *dist2, void *workspace, size_t workspace_bytes, void *stream);
int tp3d_knn_dense_f32(const float *x, const float *y, int B, int N, int np, int k, float cell, int64_t *idx,
                       float *dist2, void *workspace, size_t workspace_bytes, void *stream);

/* knn_interpolate + skip concatenation of FPModule_PD (core/base_conv/partial_dense.py:136-140):
 *   w_j = 1 / max(dist2[i,j], 1e-16);  out[i, 0:C] = (sum_j x[idx[i,j], :] * w_j) / (sum_j w_j)   (slot order, -1 skipped)
 *   out[i, C:C+C2] = skip[i, :];  columns up to ld are zero.   x (M,C), idx/dist2 (Nq,k), skip (Nq,C2) or NULL.
 *   wnorm (Nq,k) or NULL receives w_j / sum_j w_j (0 in -1 slots): the weights of the backward scatter
 *   (tp3d_rows_scatter_bwd_f32 with B = 1). */
int tp3d_knn_interpolate_fwd_f32(const float *x, const int64_t *idx, const float *dist2, const float *skip, int64_t Nq,
                                 int k, int C, int C2, int ld, float *out, float *wnorm, void *stream);

/* RandLA-Net local feature aggregation over a fixed-k neighbour table (modules/RandLANet/modules.py:9-54; the reference
 * runs it as a torch_geometric MessagePassing over the edge list of torch_cluster's knn).  Edge e = q*k + n.
 *
 * relative position encoding (modules.py:36-41): out (Nq*k, 12) rows
 *   [q_pos[q] (3), s_pos[j] (3), q_pos[q] - s_pos[j] (3), |q_pos[q] - s_pos[j]| (1), 0, 0],  j = nbr[e];
 *   a missing neighbour (j < 0 or j >= M) gives a zero row. */
int tp3d_randla_relpos_f32(const float *q_pos, const float *s_pos, const int64_t *nbr, int64_t Nq, int k, int64_t M,
                           float *out, void *stream);

/* attentive pooling (modules.py:46-52 with aggr="add"):  out[q, c] = sum_n softmax_c(g[e, :])[c] * f[e, c]
 *   g (Nq*k, ldg) attention scores, f (Nq*k, ldf) edge features (C <= ldg, ldf; C, ldf <= 256), out (Nq, C).
 *   nbr (Nq*k) or NULL: edges with nbr[e] < 0 are left out of the sum.
 * backward: dg (Nq*k, ldg) columns [0, C) and df (Nq*k, ldf) all columns (padding zeroed) are overwritten:
 *   df = s * dout[q];  dg = s * (f * dout[q] - sum_c s * f * dout[q]),  s = softmax_c(g[e, :]). */
int tp3d_attn_pool_fwd_f32(const float *g, const float *f, const int64_t *nbr, int64_t Nq, int k, int C, int ldg, int ldf,
                           float *out, void *stream);
int tp3d_attn_pool_bwd_f32(const float *g, const float *f, const float *dout, const int64_t *nbr, int64_t Nq, int k, int C,
                           int ldg, int ldf, float *dg, float *df, void *stream);

/* The whole eval-mode edge chain of RandlaKernel.message + aggr="add" in one kernel (csrc/randla_lfa.hip): nothing of
 * size Nq*k is written to memory.  k must be 16; nbr (Nq, 16) rows of the support, no -1 slots.
 *   rel  = [q_pos[q], s_pos[j], q_pos[q] - s_pos[j], |q_pos[q] - s_pos[j]|]                       (10)
 *   rij  = L2(L1(rel))                              L1: 10 -> P1, L2: P1 -> P2          (point_pos_nn)
 *   f    = [x[j] | rij]                             C = Cx + P2; x NULL: x[j] = s_pos[j], Cx must be 3
 *   g    = L4(L3(f))                                L3: C -> A1, L4: A1 -> C            (attention_nn)
 *   out[q, :] = sum over n = 0..15, in that order, of softmax_c(g) * f                 (Nq, C)
 * L(v) = LeakyReLU_0.2(scale * (W v) + shift): nn.Linear's weight W (N, K) with the bias and the eval-mode BatchNorm
 * folded by the caller, scale = gamma / sqrt(var + eps), shift = beta + scale * (bias - mean).
 * consts: one dense float buffer, per layer L1..L4 in turn  W (N*K), scale (N), shift (N).
 * Limits: C, P1, P2 <= 64, A1 <= 128 (TP3D_E_TOOBIG beyond).  fp32 products on the matrix pipe, no atomics. */
int tp3d_randla_lfa_eval_f32(const float *q_pos, const float *s_pos, const float *x, const int64_t *nbr, int64_t Nq,
                             int64_t M, int k, int Cx, int P1, int P2, int A1, const float *consts, float *out,
                             void *stream);

/* Skinny row GEMM of the edge-wise MLPs (modules/RandLANet/modules.py:20-22; nn.Linear inside MLP,
 * core/common_modules/base_modules.py:29-43):  Y (M, N) = A (M, K; row stride lda >= K) * W (N, K)^T,  N, K <= 32.
 * One row per lane, k ascending per output.  Y is dense (row stride N).
 * With lda a multiple of 4 and A 16-byte aligned the rows are read as whole float4: the columns [K, pad4(K)) of A are
 * then read and meet a zero weight, so they must hold finite values (producers write zeros); columns from pad4(K) on are
 * never read.  Any other lda / alignment reads exactly the K columns. */
int tp3d_gemm_skinny_f32(const float *A, const float *W, int64_t M, int N, int K, int lda, float *Y, void *stream);
/* The same with BatchNorm (given statistics rows mean / scale / beta of N: eval mode) and LeakyReLU applied to every
 * output before it is stored: one pass over the rows instead of three (Linear, affine, activation). */
int tp3d_gemm_skinny_bnact_f32(const float *A, const float *W, int64_t M, int N, int K, int lda, const float *mean,
                               const float *scale, const float *beta, float slope, float *out, void *stream);

/* Strided shortcut of the KPConv ResnetBBlock (modules/KPConv/blocks.py:206-210):
 *   out[q, c] = max over n of x[neighbors[q,n], c], a shadow neighbour (-1 or >= M) contributing 0.0
 * x (M,C), neighbors (Nq,Mn) -> out (Nq,C); argmax (Nq,C) int32 or NULL = winning slot n (first maximum).
 * Backward: d_x (M,C) overwritten, atomic-free (inverse neighbour table); inverse / inverse_ready as for
 * tp3d_kpconv_bwd_features_f32. */
int tp3d_nbr_maxpool_fwd_f32(const float *x, const int64_t *neighbors, int64_t Nq, int64_t M, int Mn, int C, float *out,
                             int32_t *argmax, void *stream);
int tp3d_nbr_maxpool_bwd_f32(const float *grad_out, const int32_t *argmax, const int64_t *neighbors, int64_t Nq,
                             int64_t M, int Mn, int C, float *d_x, void *inverse, size_t inverse_bytes,
                             int inverse_ready, void *stream);

/* PosPool position pooling of PPNet (modules/PPNet/ops.py:44-109), csrc/pospool.hip:
 *   rel = (support[neighbors[q,n]] - query[q]) / radius
 *   out[q, c] = sum over n of geo(rel, c) * features[neighbors[q,n], c]     a shadow neighbour (-1 or >= M) adds nothing
 * embedding 0 (xyz, C % 3 == 0): geo = rel[c / (C/3)].  embedding 1 (sin_cos, C % 6 == 0 with F = C/6, or C == 9 with
 * F = 1): c = axis * 2F + t, geo = sin(100 rel[axis] / dim_mat[t]) for t < F, cos(100 rel[axis] / dim_mat[t - F])
 * otherwise; C == 9: channels 6..8 are rel itself.  dim_mat: device (F,) table 1000^(j/F) (unused for xyz, may be NULL).
 * reduction 0 sum, 1 avg: out / (n_q + 1e-5), n_q = slots of row q whose index, shadows mapped to M, is < *padding;
 * padding: DEVICE int64, the maximum of the table with its shadows mapped to M (tp3d_pospool_padding_i64) -- what the
 * reference's torch.max(neighbors) returns after its gather has rewritten -1 to M.
 * counts (Nq) or NULL: n_q + 1e-5 as float, what the backward divides by.
 * Backward: d_features (M,C) overwritten (positions carry no gradient); atomic-free and bit-reproducible through the
 * inverted neighbour table, inverse / inverse_ready as for tp3d_kpconv_bwd_features_f32; counts may be NULL for sum. */
int tp3d_pospool_padding_i64(const int64_t *neighbors, int64_t slots, int64_t M, int64_t *padding, void *stream);
int tp3d_pospool_fwd_f32(const float *query, const float *support, const int64_t *neighbors, const float *features,
                         const int64_t *padding, const float *dim_mat, int64_t Nq, int64_t M, int Mn, int C, float radius,
                         int embedding, int reduction, float *out, float *counts, void *stream);
int tp3d_pospool_bwd_f32(const float *query, const float *support, const int64_t *neighbors, const float *grad_out,
                         const float *counts, const float *dim_mat, int64_t Nq, int64_t M, int Mn, int C, float radius,
                         int embedding, int reduction, float *d_features, void *inverse, size_t inverse_bytes,
                         int inverse_ready, void *stream);

/* =====================================================================================================
 * Message-passing PointNet++ (modules/pointnet2/message_passing.py:9-31 SAModule = FPSSampler +
 * MultiscaleRadiusNeighbourFinder + torch_geometric PointConv; core/base_conv/message_passing.py:132-151
 * GlobalBaseModule): neighbourhoods of varying size as an edge list in CSR form.
 * ===================================================================================================== */

/* radius(x, y, r, batch_x, batch_y, max_num_neighbors) as edges      [core/spatial_ops/neighbour_finder.py:31-33,141-144]
 *   table (Nq, max_num) int64: the -1 padded output of tp3d_ball_query_partial_dense_f32 (sort = 0).
 *   edge_start (Nq+1) = exclusive scan of the number of slots >= 0 per row (edge_start[Nq] = E, which the caller
 *   reads back to size col);  col (E) = the slots >= 0, row-major, in slot order (ascending support row). */
int tp3d_table_edge_start_i64(const int64_t *table, int64_t Nq, int max_num, int64_t *edge_start, void *stream);
int tp3d_table_edge_col_i64(const int64_t *table, const int64_t *edge_start, int64_t Nq, int max_num, int64_t E,
                            int64_t *col, void *stream);

/* message of PointConv: cat([x_j, pos_j - pos_i])                     [modules/pointnet2/message_passing.py:20,26]
 *   for edge e of query i (edge_start[i] <= e < edge_start[i+1]) with support row j = col[e]:
 *   out[e, :] = [ x[j, 0:C] | pos_s[j] - pos_q[i] | 0 .. ];  x (M,C) or NULL when C == 0, pos_s (M,3), pos_q (Nq,3),
 *   out (E, ld), ld >= C+3; columns past C+3 are written as zeros (16-byte row alignment, as
 *   tp3d_group_concat_fwd_f32).  A col outside [0, M) gives a zero row.  Gradient wrt x: tp3d_rows_scatter_bwd_f32
 *   with B = 1, L = E, div = 1, idx = col, col0 = 0. */
int tp3d_pointconv_rows_f32(const float *x, const float *pos_s, const float *pos_q, const int64_t *edge_start,
                            const int64_t *col, int64_t Nq, int64_t M, int64_t E, int C, int ld, float *out,
                            void *stream);

/* max over segments of rows: aggr="max" of PointConv (seg = edge_start) and global_max_pool of GlobalBaseModule
 * (seg = the cloud offsets)                                           [core/base_conv/message_passing.py:136,145]
 *   rows (E, ld), seg (S+1) int64 ascending with seg[0] = 0, seg[S] = E -> out[s, c] = max over rows seg[s] ..
 *   seg[s+1]) of rows[r, c], c < C <= ld; argmax (S,C) int64 = the winning row r (the first maximum); an empty
 *   segment gives 0.0 and -1.
 *   bwd: d_rows (E, ld) OVERWRITTEN: dout[s, c] at the winning row, zero elsewhere, padding columns zero.
 *   Atomic-free (every row belongs to one segment), bitwise reproducible. */
int tp3d_segment_max_fwd_f32(const float *rows, const int64_t *seg, int64_t S, int64_t E, int C, int ld, float *out,
                             int64_t *argmax, void *stream);
int tp3d_segment_max_bwd_f32(const float *dout, const int64_t *argmax, const int64_t *seg, int64_t S, int64_t E, int C,
                             int ld, float *d_rows, void *stream);

/* =====================================================================================================
 * Message-passing RSConv (modules/RSConv/message_passing.py:10-60 Convolution, RSConvDown): the relation rows of
 * the edges and the fused "gather x weight -> max" aggregation over the same CSR edge list (csrc/rsconv_mp.hip).
 * ===================================================================================================== */

/* relation vector h_ij of Convolution.message                        [modules/RSConv/message_passing.py:35-38]
 *   for edge e of query i with support row j = col[e], d = pos_q[i] - pos_s[j] (query minus support):
 *   out[e, :] = [ sqrt(dx^2 + dy^2 + dz^2) | d | pos_q[i] | pos_s[j] | 0 .. ];  out (E, ld), ld >= 10, columns past
 *   10 are written as zeros.  A col outside [0, M) gives a zero row.  No gradient (positions carry none). */
int tp3d_rsconv_relation_rows_f32(const float *pos_s, const float *pos_q, const int64_t *edge_start, const int64_t *col,
                                  int64_t Nq, int64_t M, int64_t E, int ld, float *out, void *stream);

/* aggr="max" of the messages M_ij * x_j                             [modules/RSConv/message_passing.py:42-44]
 *   w (E, ldw), x (M, ldx), C <= ldw, ldx -> out[i, c] = max over the edges e of query i of w[e, c] * x[col[e], c];
 *   arg (Nq, C) int64 = the winning edge (absolute index, the first maximum); a query without an edge gives 0.0 and
 *   -1: the comparison rule of tp3d_segment_max_fwd_f32, and bit-equal to it on the rows w * x[col].  A col outside
 *   [0, M) counts as a zero feature row.
 *   bwd: d_w (E, ldw) OVERWRITTEN: dout[i, c] * x[col[e], c] at the winning edge, zero elsewhere, padding columns
 *   zero.  g_x (E, ldw) or NULL, OVERWRITTEN alike with dout[i, c] * w[e, c]: the sparse edge rows whose sum per
 *   support row is the gradient wrt x -- tp3d_rows_scatter_bwd_f32 with B = 1, L = E, div = 1, idx = col, ld = ldw,
 *   col0 = 0.  Atomic-free, bitwise reproducible. */
int tp3d_rsconv_msgmax_fwd_f32(const float *w, int ldw, const float *x, int ldx, const int64_t *col,
                               const int64_t *edge_start, int64_t Nq, int64_t M, int64_t E, int C, float *out,
                               int64_t *arg, void *stream);
int tp3d_rsconv_msgmax_bwd_f32(const float *dout, const int64_t *arg, const float *w, int ldw, const float *x, int ldx,
                               const int64_t *col, const int64_t *edge_start, int64_t Nq, int64_t M, int64_t E, int C,
                               float *d_w, float *g_x, void *stream);

/* Sparse voxel convolution (csrc/sparseconv.hip)      [modules/SparseConv3d/nn/torchsparse.py, modules/SparseConv3d/modules.py]
 *   coords (N, 4) int32 rows [x, y, z, batch], 0 <= batch < 2^9; a voxel of tensor stride ts covers [c, c + ts) per axis and
 *   is accepted when that holds a coordinate of (-2^18, 2^18): |c| < 2^18 at ts = 1, -2^18 allowed at a coarser stride.
 *   A coordinate SET is (keys (rows) int64 sorted, rows (rows) int32 = owner row of each sorted slot, meta 16 int32 =
 *   [min x, y, z | max x, y, z | max batch | bad flags | row count | 0...]); bad flags: 1 = a value out of range, 2 = two equal
 *   voxels (input set only), 4 = bounding box * batches does not fit the 64-bit key.  The host reads meta once per new set.
 *   tp3d_sparse_set_build_i32: ts = the tensor stride of `coords` (the range rule above).  down == 0: the set of `coords` themselves, rows in the caller's order (keys_out, rows_out: N).
 *     down > 0: the distinct floor(c / down) * down per axis (batch kept), ascending (batch, x, y, z): keys_out, rows_out
 *     (= iota) and coords_out (., 4) sized for N rows, meta[8] of them written.
 *   tp3d_sparse_set_build_clouds_i32: the same with the caller's exclusive bound on the batch index, 1 <= cloud_limit <=
 *     tp3d_sparse_cloud_limit_max() = 2^24 (else TP3D_E_BADARG), in place of 2^9: a sparse tensor with one cloud per
 *     cluster.  Flag 4 still guards the key: extents * (highest batch + 1) must stay below 4e18.  Kernel maps and the
 *     products read the batch through the key only and take any such set.
 *   tp3d_sparse_kmap_i32: table (Nq, ksize^3) int32 = the row of the set's voxel at qcoords[q] + sign * offset_k * step, -1
 *     where absent; offsets {-(k / 2) .. k / 2} (ksize 3 or 5), {0, 1} (ksize 2), {0} (ksize 1) per axis, x slowest, z
 *     fastest.  The convolution and weight gradient take K <= 125.
 *   tp3d_sparse_kmap_mirror_i32: inverse[i][k] = forward[i][K - 1 - k] (stride 1, odd kernel).
 *   tp3d_sparse_conv_f32: y (Nout, Cout) = sum_k x[table[r][k]] . W[k], x (Nsrc, Cin); W (K, Cin, Cout), or with
 *     w_transposed != 0 W is (K, Cout, Cin) and W[k]^T is applied.  An entry outside [0, Nsrc) counts as absent.  fp32
 *     MFMA over LDS-staged gathered rows; Cin <= 4 plain FMA.  No atomics: bit-reproducible.
 *   tp3d_sparse_wgrad_f32: dW (K, Cin, Cout) = sum_r x[table[r][k]]^T . dy[r], x (Nsrc, Cin), dy (N, Cout), table (N, K);
 *     tp3d_sparse_wgrad_chunks(N, K, Cin, Cout) row chunks, each summed in ascending row order, their partials
 *     (workspace: tp3d_sparse_wgrad_workspace_floats, 0 for one chunk) summed in ascending chunk order.
 *   The wide first layer, 27 < K <= 125 and Cin <= 4 (a 5^3 kernel on a surface finds few of its offsets):
 *   tp3d_sparse_conv_wide_f32: the sum of tp3d_sparse_conv_f32 (W (K, Cin, Cout) only) over the PRESENT offsets of a row,
 *     compacted per wave with a ballot, k then ci ascending; W staged in LDS.  tp3d_sparse_conv_wide_serves is 0 where W
 *     and the hit lists do not fit the LDS (TP3D_E_BADARG from the launch): the generic kernel serves those.
 *   tp3d_sparse_wgrad_wide_f32: dW as tp3d_sparse_wgrad_f32; a workgroup per row chunk, per-wave accumulators in LDS (no
 *     atomics), rows of a wave, then waves, then chunks summed in ascending order: bit-reproducible.  Each dy row and table
 *     row is read once.  tp3d_sparse_wgrad_wide_chunks is 0 (and the launch TP3D_E_BADARG) where one wave's K * Cin * Cout
 *     accumulators do not fit the LDS; workspace: tp3d_sparse_wgrad_wide_workspace_floats, 0 for one chunk. */
size_t tp3d_sparse_workspace_bytes(int64_t N);
int tp3d_sparse_set_build_i32(const int32_t *coords, int64_t N, int ts, int down, int64_t *keys_out, int32_t *rows_out,
                              int32_t *coords_out, int32_t *meta, void *workspace, size_t workspace_bytes, void *stream);
int tp3d_sparse_cloud_limit_max(void);
int tp3d_sparse_set_build_clouds_i32(const int32_t *coords, int64_t N, int ts, int down, int cloud_limit, int64_t *keys_out,
                                     int32_t *rows_out, int32_t *coords_out, int32_t *meta, void *workspace,
                                     size_t workspace_bytes, void *stream);
int tp3d_sparse_kmap_i32(const int32_t *qcoords, int64_t Nq, int ksize, int step, int sign, const int64_t *keys,
                         const int32_t *rows, const int32_t *meta, int64_t Ns, int32_t *table, void *stream);
int tp3d_sparse_kmap_mirror_i32(const int32_t *forward, int64_t N, int K, int32_t *inverse, void *stream);
int tp3d_sparse_conv_f32(const float *x, const int32_t *table, const float *W, int64_t Nout, int64_t Nsrc, int K, int Cin,
                         int Cout, int w_transposed, float *y, void *stream);
int tp3d_sparse_wgrad_chunks(int64_t N, int K, int Cin, int Cout);
size_t tp3d_sparse_wgrad_workspace_floats(int64_t N, int K, int Cin, int Cout);
int tp3d_sparse_wgrad_f32(const float *x, const float *dy, const int32_t *table, int64_t N, int64_t Nsrc, int K, int Cin,
                          int Cout, float *dW, float *workspace, size_t workspace_floats, void *stream);
int tp3d_sparse_conv_wide_serves(int K, int Cin, int Cout);
int tp3d_sparse_conv_wide_f32(const float *x, const int32_t *table, const float *W, int64_t Nout, int64_t Nsrc, int K, int Cin,
                              int Cout, float *y, void *stream);
int tp3d_sparse_wgrad_wide_chunks(int64_t N, int K, int Cin, int Cout);
size_t tp3d_sparse_wgrad_wide_workspace_floats(int64_t N, int K, int Cin, int Cout);
int tp3d_sparse_wgrad_wide_f32(const float *x, const float *dy, const int32_t *table, int64_t N, int64_t Nsrc, int K, int Cin,
                               int Cout, float *dW, float *workspace, size_t workspace_floats, void *stream);

/* Multi-scale fusion (csrc/scale_fuse.hip)                        [models/registration/ms_svconv3d.py apply_nn]
 *   xs, dxs: HOST arrays of S <= 8 device pointers, each (N, C) fp32.  xhat_s = x_s / (||x_s||_2 + eps) per row; mode 0 cat:
 *   out (N, S * C), scale s in columns [s C, (s + 1) C); mode 1 max, 2 mean over the scales: out (N, C).  norm (N, S) =
 *   ||x_s||_2 (read by the backward); xhat (S, N, C) or NULL: the normalised rows (modes 1, 2); arg (N, C) uint8 = the
 *   winning scale, ties to the lowest (mode 1 only, else NULL).  A group of 8 / 16 / 32 / 64 lanes owns a row; sums are
 *   butterfly reductions in a fixed order.  No atomics: bit-reproducible.
 *   tp3d_scale_fuse_bwd_f32: dxs[s] = g_s / d - x_s <g_s, x_s> / (n d^2), d = n + eps (evaluated as (g_s - h <g_s, h> d / n) / d,
 *   h = x_s / d), and g_s / d where n == 0; g_s = the
 *   cotangent of xhat_s: gout's columns (cat), gout / S (mean), gout where arg == s (max), plus gxhat[s] (S, N, C) when not
 *   NULL; gout may be NULL (= 0). */
int tp3d_scale_fuse_fwd_f32(const float *const *xs, int S, int64_t N, int C, int mode, float eps, float *out, float *xhat,
                            float *norm, unsigned char *arg, void *stream);
int tp3d_scale_fuse_bwd_f32(const float *const *xs, int S, int64_t N, int C, int mode, float eps, const float *gout,
                            const float *gxhat, const float *norm, const unsigned char *arg, float *const *dxs, void *stream);

/* Point-voxel operations of PVCNN (csrc/pointvoxel.hip)                                     [modules/PVCNN/utils.py]
 *   Features fp32, tables int32, -1 = absent; an index outside its row range counts as absent.  No float atomics: every
 *   result is bit-reproducible.  The lookups are tp3d_sparse_kmap_i32 over the coordinates of tp3d_pv_quantize_f32
 *   (ksize 1: the point's voxel row; ksize 2, step s, sign 1: the 8 corner rows, x slowest, z fastest).
 *   tp3d_pv_quantize_f32: pc (N, 4) = [x, y, z, batch] -> q (N, 4) int32 = [floor(x / s) * s, ..., (int)batch]; division
 *     and floor in fp32 (floor, not truncation), s >= 1.
 *   tp3d_pv_trilinear_f32: w (N, 8); corner k = 4 dx + 2 dy + dz: w = a_x a_y a_z with a = (pf + s) - p (d = 0) or p - pf
 *     (d = 1), pf = floor(p / s) * s; then / s^3; then 0 where idx8[p][k] is absent (outside [0, Nv)); then
 *     / (sum_k w + 1e-8); all fp32 in that order.  nearest != 0: afterwards corners 1..7 get w = 0 and idx8 = -1 (written
 *     to idx8), no renormalisation.
 *   tp3d_pv_invert_i32: table (N, K), K = 1 or 8, into Nv rows -> start (Nv + 1), order (N * K ints, the first start[Nv]
 *     written): order[start[v] .. start[v + 1]) = the slots l = p * K + k with table[l] == v in ascending l (stable radix
 *     sort); absent slots are dropped.  workspace: tp3d_pv_invert_workspace_bytes(N, K).
 *   tp3d_pv_gather_f32: out (N, C): out[p] = sum_k wk * src[table[p][k]] over the present slots, k ascending; wk =
 *     w[p][k], or with w NULL scale[table[p][k]], or 1 with both NULL.  src (Nsrc, C).
 *   tp3d_pv_runsum_f32: out (Nv, C): out[v] = scale[v] * sum over l in order[start[v] .. start[v + 1]) of w[l] *
 *     src[l / K]; w (Nsrc * K) and scale (Nv) may each be NULL (= 1); src (Nsrc, C); an empty run gives zeros.  A run of
 *     more than 64 slots is summed in 16 contiguous pieces of ceil(n / 16) slots, each in ascending order, the pieces
 *     added in order (fixed association by run length: reproducible, not the sequential sum bit for bit).
 *   Lanes run across channels, float4 where C % 4 == 0 and src / out are 16-byte aligned. */
int tp3d_pv_quantize_f32(const float *pc, int64_t N, int s, int32_t *q, void *stream);
int tp3d_pv_trilinear_f32(const float *pc, int32_t *idx8, int64_t N, int64_t Nv, int s, int nearest, float *w, void *stream);
size_t tp3d_pv_invert_workspace_bytes(int64_t N, int K);
int tp3d_pv_invert_i32(const int32_t *table, int64_t N, int K, int64_t Nv, int32_t *start, int32_t *order, void *workspace,
                       size_t workspace_bytes, void *stream);
int tp3d_pv_gather_f32(const float *src, const int32_t *table, const float *w, const float *scale, int64_t N, int K,
                       int64_t Nsrc, int C, float *out, void *stream);
int tp3d_pv_runsum_f32(const float *src, const int32_t *start, const int32_t *order, const float *w, const float *scale,
                       int64_t Nv, int K, int64_t Nsrc, int C, float *out, void *stream);

/* Cluster voxel mean of PointGroup's sparse scorers (csrc/cluster_voxel.hip)   [models/panoptic/pointgroup.py:123-141]
 *   The clusters are a CSR over member slots: slot e holds the point members[e] (E int64).  Every slot belongs to one
 *   voxel: voxel v owns the slots order[vstart[v] .. vstart[v + 1]) (int64, ascending slot: tp3d_voxel_cluster_f32 over
 *   the slots), and slot_voxel[e] (E int64) names it.  x (N, ldx) fp32 are the rows of the points, C <= ldx.
 *   tp3d_cluster_voxel_mean_fwd_f32: out (V, C): out[v] = (sum over the voxel's slots e, ascending, of x[members[e]]) / n_v.
 *     x is read through voxel -> slot -> point; no (E, C) rows are written.
 *   tp3d_cluster_voxel_mean_bwd_f32: dx (N, C) OVERWRITTEN: dx[p] = sum over the slots e with members[e] == p, ascending e,
 *     of dout[slot_voxel[e]] / n_voxel; exact zeros for a point in no slot.  dout (V, C) dense.  pstart (N + 1), porder (E)
 *     int32: the point -> slots index, porder[pstart[p] .. pstart[p + 1]) = the slots of p ascending -- tp3d_pv_invert_i32
 *     of `members` with K = 1 and Nv = N.
 *   Both: a run of more than 64 slots is summed in 16 contiguous pieces of ceil(n / 16) slots, each ascending, the pieces
 *   added in order (the association of tp3d_pv_runsum_f32); an index outside its range counts as absent.  Lanes run across
 *   channels, float4 where C % 4 == 0 and every row is 16-byte aligned.  No float atomics: repeats are bit-equal. */
int tp3d_cluster_voxel_mean_fwd_f32(const float *x, int ldx, const int64_t *members, const int64_t *order, const int64_t *vstart,
                                    int64_t N, int64_t E, int64_t V, int C, float *out, void *stream);
int tp3d_cluster_voxel_mean_bwd_f32(const float *dout, const int64_t *slot_voxel, const int64_t *vstart, const int32_t *pstart,
                                    const int32_t *porder, int64_t N, int64_t E, int64_t V, int C, float *dx, void *stream);

/* Region growing of PointGroup (csrc/region_grow.hip)           [models/panoptic/pointgroup.py:98-121, region_grow]
 *   The connected components of the graph that joins points i, j when labels[i] == labels[j], batch[i] == batch[j], the
 *   label is not one of ignore[0 .. n_ignore) and (dx*dx + dy*dy) + dz*dz < radius * radius in fp32 -- the membership
 *   test of tp3d_ball_query_partial_dense_f32, uncapped.  pos (N,3), labels (N), batch (N, ascending); ignore is DEVICE
 *   memory.  Components of at least min_cluster_size points are written as a CSR, ordered by (label ascending, lowest
 *   member ascending), members in ascending point index:
 *     members (N; [0, M) valid) point indices;  member_cluster (N; [0, M) valid) cluster of each member slot;
 *     starts (N + 1; [0, K] valid) slot range of each cluster;  cluster_label, cluster_cloud (N; [0, K) valid);
 *     stats (8 int32): [0] largest neighbour count of a point (itself and duplicates included: the row length an
 *     uncapped ball query would have), [1] K, [2] M, [3] flags: 1 a kept label outside [0, 4094], 2 a cloud id outside
 *     [0, 1023], 4 a coordinate beyond +-2^24 cells, 8 more than 16382 cells of 1.01 * radius along an axis.  A point
 *     that raises a flag is left out of every cluster (nothing wraps; a coordinate beyond the limit also stays out of
 *     the cell box); the caller reads stats back once and decides.
 *   The result does not depend on the execution order (min-root union-find: a component's root is its lowest index);
 *   no float atomics.  Memory proportional to N: workspace tp3d_region_grow_workspace_bytes(N) (0: N not served). */
size_t tp3d_region_grow_workspace_bytes(int64_t N);
int tp3d_region_grow_f32(const float *pos, const int64_t *labels, const int64_t *batch, int64_t N, const int64_t *ignore,
                         int n_ignore, float radius, int64_t min_cluster_size, int64_t *members, int64_t *member_cluster,
                         int64_t *starts, int64_t *cluster_label, int64_t *cluster_cloud, int32_t *stats, void *workspace,
                         size_t workspace_bytes, void *stream);

/* Registration descriptors (csrc/registration.hip)   [core/losses/metric_losses.py, utils/registration.py, geometry.py]
 *   tp3d_feature_nn_f32: a (P, C), b (S, C) fp32 -> dist2 (P) fp32, idx (P) int64: dist2[i] = min over the allowed j of
 *     sum_c (a[i][c] - b[j][c])^2, idx[i] the LOWEST such j among exact ties.  The difference form in fp32: per tile of
 *     32 / 64 / 128 channels (the least that holds C; 64 for C > 128, tiles added in ascending order) four fma chains over
 *     c = k, k + 4, ... ascending, combined as (s0 + s1) + (s2 + s3).  pos_a (P, 3) and pos_b (S, 3), both or neither:
 *     j is allowed only if sqrt(((dx*dx + dy*dy) + dz*dz) + 1e-7) > min_dist in fp32 (pdist(..., "L2") > min_dist).  A row
 *     without an allowed candidate (S == 0 included) gets idx = -1, dist2 = +inf; a NaN distance never wins.  S is split
 *     over workgroups and the per-split minima of (distance bits << 32 | j) are combined by an integer minimum: no float
 *     atomics, repeats are bit-equal.  workspace: tp3d_feature_nn_workspace_bytes(P, S, C) (0: nothing to do or too big).
 *   Fast Global Registration, one iteration = tp3d_fgr_accumulate_f32 + tp3d_fgr_solve with the same N, iter, workspace
 *     (tp3d_fgr_workspace_bytes(N): the pose T_res and mu in double, then the per-block partial sums), iter = 0, 1, ... in
 *     order.  accumulate: s = R p + t with the pose of the workspace (identity at iter 0), the Geman-McClure weight
 *     w = mu / (mu + |q - s|^2) (1 at iter 0), and the 21 + 6 distinct entries of A^T A and A^T b of get_matrix_system
 *     (rows w [-[s]x | I], right side w (q - s)) summed in double per block.  solve (one wave): the partials added in
 *     block order, the 6 x 6 system by Gaussian elimination with partial pivoting in double, T = the Rodrigues matrix of
 *     get_trans (identity rotation at theta == 0), T_res <- T T_res, mu <- mu_init at iter 0 and mu / 2 when iter > 0 and
 *     iter % 5 == 0 (it weighs the NEXT iteration, as in the reference); T (16 floats, row-major) receives T_res.  A pivot
 *     that is exactly 0, or a solution that is not finite, leaves T_res as it was (the reference raises).  The host reads
 *     nothing between the launches. */
size_t tp3d_feature_nn_workspace_bytes(int64_t P, int64_t S, int C);
int tp3d_feature_nn_f32(const float *a, const float *b, const float *pos_a, const float *pos_b, int64_t P, int64_t S, int C,
                        float min_dist, float *dist2, int64_t *idx, void *workspace, size_t workspace_bytes, void *stream);
size_t tp3d_fgr_workspace_bytes(int64_t N);
int tp3d_fgr_accumulate_f32(const float *xyz, const float *xyz_target, int64_t N, int iter, void *workspace,
                            size_t workspace_bytes, void *stream);
int tp3d_fgr_solve(int64_t N, int iter, double mu_init, float *T, void *workspace, size_t workspace_bytes, void *stream);

/* RANSAC over correspondences and the weighted Kabsch refit (csrc/ransac.hip, csrc/ransac_horn.h)
 *                                                   [utils/registration.py:24-43, :141-163; open3d's correspondence RANSAC]
 *   xyz, xyz_target (N, 3) fp32: correspondence i pairs xyz[i] with xyz_target[i]; 3 <= N < 2^31 / 3.
 *   tp3d_ransac_score_f32: samples (H, n) int64, 3 <= n <= 8, entries in [0, N), repeats allowed -> poses (H, 12) fp32 (row-
 *     major [R | t]; NULL: kept in the workspace) and counts (H) int32.  The pose of a hypothesis maps its n sampled
 *     sources onto their targets in the least-squares sense, in double by Horn's closed form: centred cross-covariance,
 *     the symmetric 4 x 4 matrix, the unit eigenvector of its largest eigenvalue by cyclic Jacobi sweeps, that quaternion
 *     as R, t = mean(q) - R mean(p) -- Kabsch with the determinant correction, a proper rotation by construction.  One
 *     thread per hypothesis, the pose computed once.  counts[h] = the number of i with |R p_i + t - q_i|^2 <
 *     threshold^2 in fp32: s_a = fma(R_a0, px, fma(R_a1, py, fma(R_a2, pz, t_a))), d_a = s_a - q_a,
 *     d2 = fma(dz, dz, fma(dy, dy, dx * dx)).  A pose that is not finite (or a sampled row outside [0, N), which is
 *     never dereferenced) gives NaNs and the count 0.  N is split over workgroups in whole tiles of TP3D_RANSAC_TILE
 *     (tp3d_ransac_splits(N, H) splits) and the per-split counts are added as integers in split order: repeats are
 *     bit-equal, nothing of size H * N exists.
 *   tp3d_ransac_select: the hypothesis of the highest count, among equal counts the LOWEST index (the integer maximum
 *     of (count << 32) | (0xffffffff - h), H <= 2^31; open3d compares the inlier RMSE of equal counts instead).  Its
 *     index, count and pose (formed again in double) go to the head of the workspace; the host reads nothing.
 *   tp3d_kabsch_accumulate_f32 + tp3d_kabsch_solve with the same N, gate and workspace: the weighted Kabsch pose.  The
 *     weight of correspondence i is weight[i] (NULL: 1), and with gate != 0 only correspondences with |R p + t - q|^2 <
 *     threshold^2 in double under the pose of the workspace weigh in.  accumulate: per-block sums in double of w, w p,
 *     w q, w p_a q_b, the gated count and the gated sum of squared distances.  solve (one wave): the partials added in
 *     block order, centred, Horn as above; the pose goes to the workspace and, as 16 floats row-major, to T (may be
 *     NULL).  If the weight sum is 0, or with the gate fewer than 3 correspondences are gated in, the previous pose
 *     stays; without a previous pose (gate == 0 starts afresh) the result is the identity.  update == 0 leaves the pose
 *     and only records the stats.
 *   The head of the workspace, doubles: [0, 12) pose, 12 whether there is one, 13 best index, 14 best count, 15 gated
 *     count and 16 gated sum of d^2 of the last accumulate, 17 its weight sum.  tp3d_ransac_workspace_bytes(N, H): H = 0
 *     for the Kabsch entry points alone; 0 = not served. */
#define TP3D_RANSAC_TILE 256
#define TP3D_RANSAC_HYP_BLOCK 256
size_t tp3d_ransac_workspace_bytes(int64_t N, int64_t H);
int tp3d_ransac_splits(int64_t N, int64_t H);
int tp3d_ransac_score_f32(const float *xyz, const float *xyz_target, int64_t N, const int64_t *samples, int64_t H, int n,
                          float threshold, float *poses, int32_t *counts, void *workspace, size_t workspace_bytes, void *stream);
int tp3d_ransac_select(const float *xyz, const float *xyz_target, int64_t N, const int64_t *samples, int64_t H, int n,
                       const int32_t *counts, void *workspace, size_t workspace_bytes, void *stream);
int tp3d_kabsch_accumulate_f32(const float *xyz, const float *xyz_target, const float *weight, int64_t N, int gate,
                               double threshold, void *workspace, size_t workspace_bytes, void *stream);
int tp3d_kabsch_solve(int64_t N, int gate, int update, float *T, void *workspace, size_t workspace_bytes, void *stream);

/* Per-cloud row kernels of PointNet (csrc/segment_rows.hip)
 *                                  [core/common_modules/spatial_transform.py:44-49, modules/PointNet/modules.py:33-35, :108]
 *   seg (B + 1) int64: the row offsets of the clouds, ascending, seg[0] = 0, seg[B] = N, empty clouds allowed; fp32 data;
 *   row strides (ld*) in floats.  No float atomics, nothing of size N * k * k is written, repeats are bit-equal.
 *   tp3d_segment_transform_f32: x (N, ldx), T (B, k, k) -> out (N, ldo); for row i of cloud b
 *     out[i, c] = sum_j x[i, j] * T[b, j, c] (transpose != 0: T[b, c, j]) for c < k, one fp32 fma chain, j ascending;
 *     out[i, c] = x[i, c] for k <= c < C; 0 for C <= c < ldo.  1 <= k <= 64, k <= C <= ldx, ldo (else TP3D_E_BADARG).
 *     With T[b] the identity out[:, :C] is x bit for bit (up to the sign of a zero); transpose = 1 on dy is the input
 *     gradient.  out must not overlap x.  A workgroup serves tp3d_segment_tile_rows() consecutive rows.
 *   tp3d_segment_transform_wgrad_f32: dT (B, k, k): dT[b, j, c] = sum over the rows i of cloud b of x[i, j] * dy[i, c].
 *     Every cloud is cut into chunks of tp3d_segment_sum_chunk() rows from its first row; a chunk is summed in ascending
 *     row order (one fma chain per entry), a cloud's chunks are added in ascending order; an empty cloud gives zeros.
 *     workspace: tp3d_segment_transform_wgrad_workspace_bytes(N, B, k).
 *   tp3d_segment_bcast_cat_f32: x (N, ldx) or NULL with C1 = 0, g (B, ldg) -> out (N, ldo):
 *     out[i] = [ x[i, 0:C1] | g[b(i), 0:C2] | 0 .. ldo ).
 *   tp3d_segment_sum_f32: out (B, C): out[b, c] = scale[b] * sum over the rows i of cloud b of rows[i, col0 + c], rows
 *     (N, ld), scale (B) or NULL (= 1); the chunked order of the weight gradient.
 *     workspace: tp3d_segment_sum_workspace_bytes(N, B, C). */
int tp3d_segment_tile_rows(void);
int tp3d_segment_sum_chunk(void);
int tp3d_segment_transform_f32(const float *x, const float *T, const int64_t *seg, int64_t N, int64_t B, int k, int C, int ldx,
                               int ldo, int transpose, float *out, void *stream);
size_t tp3d_segment_transform_wgrad_workspace_bytes(int64_t N, int64_t B, int k);
int tp3d_segment_transform_wgrad_f32(const float *x, const float *dy, const int64_t *seg, int64_t N, int64_t B, int k, int ldx,
                                     int lddy, float *dT, void *workspace, size_t workspace_bytes, void *stream);
int tp3d_segment_bcast_cat_f32(const float *x, const float *g, const int64_t *seg, int64_t N, int64_t B, int C1, int C2, int ldx,
                               int ldg, int ldo, float *out, void *stream);
size_t tp3d_segment_sum_workspace_bytes(int64_t N, int64_t B, int C);
int tp3d_segment_sum_f32(const float *rows, const int64_t *seg, const float *scale, int64_t N, int64_t B, int col0, int C, int ld,
                         float *out, void *workspace, size_t workspace_bytes, void *stream);

/* Detection: box post-processing of VoteNet (csrc/detection.hip)
 *                       [utils/box_utils.py:28-182, modules/VoteNet/votenet_results.py:231-255, metrics/box_detection/ap.py:81-107]
 *   tp3d_box_nms_f32: nms_samecls for B scenes of P boxes in one launch, one workgroup per scene.  boxes (B, P, 6) fp32
 *     [xmin ymin zmin xmax ymax zmax], classes (B, P), order (B, P): the visiting order of each scene (box indices in
 *     [0, P), best first; the host wrapper sorts).  A live box i clears every later box j of the order with
 *     classes[i] == classes[j] and o > overlap_threshold, where in fp32, one rounding per operation, no fused multiply-add:
 *     area = ((x2 - x1) * (y2 - y1)) * (z2 - z1), l, w, h = max(0, min(hi) - max(lo)) per axis, inter = (l * w) * h,
 *     o = inter / ((area_i + area_j) - inter), o = o * (1 or 0 for equal classes).  0 / 0 compares false.
 *     keep (B, P) bytes, 1 = kept.  P <= TP3D_BOX_NMS_MAX_BOXES (else TP3D_E_TOOBIG); nothing of size P * P is written.
 *   tp3d_box3d_iou_f64: corners1 (n, 8, 3), corners2 (m, 8, 3) fp32 -> iou (n, m) float64, box3d_iou of every pair: rows
 *     0-3 the bottom face counter-clockwise seen from +z, rows 4-7 the top face.  The footprint of box 1 is clipped by
 *     the footprint of box 2 with polygon_clip's Sutherland-Hodgman (edge order, strict inside test, computeIntersection)
 *     in float64 on the promoted corners; the area is 0.5 * |sum_k (x_k * y_k+1 - x_k+1 * y_k)| in vertex order, 0 for an
 *     empty clip; height max(0, min(c1[4].z, c2[4].z) - max(c1[0].z, c2[0].z)); volumes as box3d_vol (three edge lengths);
 *     iou = inter / ((vol1 + vol2) - inter).  Where rounding splits two collinear edges (a rotated box against itself) the
 *     clip divides by zero and the result is NaN; the reference's hull raises on the same pairs.
 *   tp3d_box_best_gt_f64: for detection d (corners (D, 8, 3), class, scene) the first maximum of that IoU over the
 *     ground-truth boxes gt_scene_start[scene] .. gt_scene_start[scene + 1]) of its class (gt sorted by scene; S scenes):
 *     ovmax (D) float64, -inf without a candidate; jmax (D) the row of that box in gt_corners, -1 without a candidate.
 *     No (D, G) matrix is written.
 *   tp3d_ap_match: order (D) lists the detections grouped by (scene, class), inside a group by descending score (the
 *     host wrapper sorts).  Each group is walked in that order; tp[d, t] = 1 when ovmax[d] > thresholds[t] (strict) and
 *     jmax[d] has not been taken by an earlier detection of the group at that threshold.  thresholds (T) float64 DEVICE
 *     memory; taken (T * G) bytes of scratch (cleared here); tp (D, T) bytes. */
#define TP3D_BOX_NMS_MAX_BOXES 4096
int tp3d_box_nms_max_boxes(void);
int tp3d_box_nms_f32(const float *boxes, const int64_t *classes, const int64_t *order, int B, int P, float overlap_threshold,
                     uint8_t *keep, void *stream);
int tp3d_box3d_iou_f64(const float *corners1, const float *corners2, int64_t n, int64_t m, double *iou, void *stream);
int tp3d_box_best_gt_f64(const float *det_corners, const int64_t *det_class, const int64_t *det_scene, int64_t D,
                         const float *gt_corners, const int64_t *gt_class, const int64_t *gt_scene_start, int64_t G, int64_t S,
                         double *ovmax, int64_t *jmax, void *stream);
int tp3d_ap_match(const int64_t *order, const int64_t *det_class, const int64_t *det_scene, int64_t D, const double *ovmax,
                  const int64_t *jmax, int64_t G, const double *thresholds, int T, uint8_t *taken, uint8_t *tp, void *stream);

/* Segmentation metrics (csrc/seg_metrics.hip)
 *                       [metrics/confusion_matrix.py, segmentation_tracker.py, shapenet_part_tracker.py, s3dis_tracker.py,
 *                        segmentation_helpers.py]
 * Integer counters only: no float arithmetic in the counting kernels, no float atomics anywhere, results independent of
 * the launch geometry.  Nothing is read back and nothing of the size of the input is written.
 *   Row argmax (confusion and part counts): the prediction of a row is the LOWEST column holding the row's maximum over
 *     the given column range (numpy's argmax); the running maximum starts from the first column of the range, so rows
 *     of negative log-probabilities are served.  Rows holding NaN are outside the contract (the library is built with
 *     -fno-honor-nans): their prediction is unspecified, though always inside the range.
 *   tp3d_confusion_count_f32: cm is int64 (C * C + 1), ACCUMULATED into and never cleared here.  Row i of N:
 *       labels[i] == ignore_label: skipped (pass INT64_MIN for "no ignore label");
 *       row_index given and row_index[i] == -1: skipped; otherwise the scores row is row_index[i] (i without row_index);
 *       a label outside [0, C), a scores row outside [0, n_score_rows) or (pred mode) a prediction outside [0, C):
 *         cm[C * C] += 1, the "invalid" counter, and no matrix cell changes;
 *       else cm[label * C + prediction] += 1, prediction = col_lo + argmax of scores[row, col_lo .. col_hi), or pred[i].
 *     scores (n_score_rows, >= col_hi) fp32 with row stride ld >= col_hi, 0 <= col_lo < col_hi <= C; or scores = NULL and
 *     pred (N) int64 (then row_index must be NULL and ld, col_lo, col_hi are not read).  Rows are staged through LDS in
 *     tiles of tp3d_confusion_tile_rows() with coalesced loads, then one lane per row.  For
 *     C <= TP3D_CONFUSION_LDS_MAX_CLASSES a workgroup counts in C * C int32 LDS cells and adds its non-zero cells to cm
 *     once, with agent-scope 64-bit integer atomics; wider matrices are counted with those atomics directly.
 *     N <= 2^40 (TP3D_E_TOOBIG beyond).
 *   tp3d_part_iou_counts_f32 (ShapeNet protocol): B clouds, cloud b = rows seg[b] .. seg[b + 1]) of scores (N, C), row
 *     stride ld >= C, and labels (N).  part_lo[C], part_hi[C] (int32, device): for every label the range [lo, hi) of the
 *     labels of its category.  One workgroup per cloud.  The category is that of the cloud's FIRST label; a row's
 *     prediction is lo + argmax over columns [lo, hi) only.  counts (B, TP3D_PART_IOU_MAX_PARTS, 2) int32 =
 *     (intersection, union) of label == part and prediction == part for part = lo + p, zero for p >= hi - lo; a label
 *     outside [lo, hi) matches no part.  cat_lo (B) int32 = lo, -1 for an empty cloud, -2 (and zero counts) where the
 *     first label is outside [0, C), the tables give an empty, out-of-range or too wide category, or seg is not ascending
 *     inside [0, N].  max_parts = the widest category of the tables as the caller knows it:
 *     > TP3D_PART_IOU_MAX_PARTS is TP3D_E_TOOBIG.  "Absent part counts as 1" and the means are the host's.
 *   tp3d_vote_add_f32: votes[ids[i], :] += out[i, :], counts[ids[i]] += 1 for the n rows of out (n, C), row stride ld.
 *     votes (T, C) fp32 contiguous, counts (T) int32, workspace (T) int64 zeroed ONCE when allocated and then owned by
 *     these votes, errors (1) int64: += 1 per id outside [0, T) (that row adds nothing).  epoch: 1, 2, 3, ... one more
 *     per call on the same workspace (< 2^31).  With unique ids the result is bit-equal to the indexed add.  Duplicate
 *     rule: of the rows of ONE call naming the same target, only the one with the HIGHEST row index is added, and the
 *     count rises by one.  Pass 1 takes the integer maximum of (epoch << 32 | row) per target, so a word left by an
 *     earlier call never wins and nothing of size T is cleared; pass 2 lets the winning rows write with plain stores.
 *     n <= 2^31 - 1. */
#define TP3D_CONFUSION_LDS_MAX_CLASSES 80
#define TP3D_PART_IOU_MAX_PARTS 16
int tp3d_confusion_tile_rows(void);
int tp3d_confusion_lds_max_classes(void);
int tp3d_part_iou_max_parts(void);
int tp3d_confusion_count_f32(const float *scores, int64_t n_score_rows, int ld, const int64_t *pred, const int64_t *labels,
                             const int64_t *row_index, int64_t N, int C, int col_lo, int col_hi, int64_t ignore_label,
                             int64_t *cm, void *stream);
int tp3d_part_iou_counts_f32(const float *scores, int ld, const int64_t *labels, const int64_t *seg, int64_t N, int64_t B, int C,
                             const int32_t *part_lo, const int32_t *part_hi, int max_parts, int32_t *counts, int32_t *cat_lo,
                             void *stream);
int tp3d_vote_add_f32(const float *out, int ld, const int64_t *ids, int64_t n, int C, int64_t T, int64_t epoch, float *votes,
                      int32_t *counts, int64_t *workspace, int64_t *errors, void *stream);

/* Panoptic metrics (csrc/panoptic_metrics.hip)
 *                       [metrics/panoptic_tracker.py, models/panoptic/structures.py:6-49]
 * Clusters are a CSR: cluster k owns members[starts[k] .. starts[k + 1]) (point indices), member_cluster[e] = the cluster
 * of slot e (ascending).  Integer counters only, no float atomics, bit-equal repeats, nothing read back; memory is
 * proportional to the slots M, the clusters K, the instances G and the overlapping cluster pairs -- there is no (K, N),
 * (K, K) or (K, G) array.  K, M and the pair capacity are at most 2^31 - 1 (TP3D_E_TOOBIG beyond).
 *   tp3d_cluster_best_instance: column (N) = the ground-truth column of every point or -1; gt_size, gt_class (G);
 *     cluster_class, col_lo, col_hi (K): the columns [col_lo, col_hi) of the cluster's cloud (members with a column
 *     outside it are not counted).  One workgroup per cluster (one wave up to 256 members) counts the members per column
 *     in an LDS histogram of TP3D_CLUSTER_BEST_WINDOW columns, window after window.  With n = the cluster's slots:
 *       inter_all, col_all: the first maximum over the columns with inter > 0 of the fp32 value
 *         fp32(inter) / max((fp32(n) + fp32(gt_size)) - fp32(inter), 1), one rounding per operation; col_all = -1 and
 *         inter_all = 0 when no column has a member;
 *       inter_cls, col_cls: the first maximum over the columns with inter > 0 and gt_class == cluster_class of the
 *         float64 value inter / (n + gt_size - inter); -1 and 0 without such a column.
 *   Sparse overlaps, two calls that share `stats` (3 int64, device) and the count workspace:
 *     tp3d_cluster_overlap_count sorts the slots by point (stable, over the low point_bits bits: members in
 *       [0, 2^point_bits)) and counts, per slot, the other clusters that hold its point (a cluster that lists a point
 *       twice counts once); stats[0] = the number Q of ordered (cluster, other) pairs over all points, stats[1..2] = 0.
 *     tp3d_cluster_overlap_emit writes those pairs as keys cluster * K + other into `cap` slots, sorts them and reduces
 *       the runs: ov_start (K + 1), ov_other and ov_inter (cap; the first ov_start[K] entries are written): for cluster
 *       k the entries ov_start[k] .. ov_start[k + 1]) list the clusters it shares a point with, ascending, and the number
 *       of shared points; both directions are stored.  stats[1] = ov_start[K].  Q > cap: stats[2] = 1, ov_start is all
 *       zero and the entries are unspecified (nothing is written outside the buffers).
 *   tp3d_cluster_nms: order (K) = the visiting order (the host wrapper sorts); hot, keep (K) bytes.  A cluster that is
 *     alive when visited clears every neighbour j with fp32(inter) / ((fp32(n_i) + fp32(n_j)) - fp32(inter)) > threshold.
 *     Clusters without such a neighbour (hot = 0) are kept by a parallel pass; one workgroup walks the others in order,
 *     its lanes spread over the neighbour list of the visited cluster.  P = the entries of ov_other / ov_inter.
 *   tp3d_instance_ap_match: the sibling of tp3d_ap_match for instances.  order (K) lists the clusters grouped by (cloud,
 *     class), inside a group in visiting order.  tp[d] = 1 when valid[d], col_cls[d] >= 0, the float64 IoU
 *     inter_cls / (size + gt_size[col_cls] - inter_cls) >= threshold (not strict) and the instance has not been taken by
 *     an earlier cluster of the group.  taken (G) bytes of scratch (cleared here); tp (K) bytes, written for every d. */
#define TP3D_CLUSTER_BEST_WINDOW 1024
int tp3d_cluster_best_window(void);
int tp3d_cluster_best_instance(const int64_t *members, const int64_t *starts, int64_t M, int64_t K, const int64_t *column,
                               int64_t N, const int64_t *gt_size, const int64_t *gt_class, int64_t G,
                               const int64_t *cluster_class, const int64_t *col_lo, const int64_t *col_hi, int64_t *inter_all,
                               int64_t *col_all, int64_t *inter_cls, int64_t *col_cls, void *stream);
size_t tp3d_cluster_overlap_count_workspace_bytes(int64_t M);
size_t tp3d_cluster_overlap_emit_workspace_bytes(int64_t cap);
int tp3d_cluster_overlap_count(const int64_t *members, const int64_t *member_cluster, int64_t M, int64_t K, int point_bits,
                               int64_t *stats, void *workspace, size_t workspace_bytes, void *stream);
int tp3d_cluster_overlap_emit(const int64_t *member_cluster, int64_t M, int64_t K, int64_t cap, int64_t *ov_start,
                              int64_t *ov_other, int64_t *ov_inter, int64_t *stats, void *count_workspace,
                              size_t count_workspace_bytes, void *workspace, size_t workspace_bytes, void *stream);
int tp3d_cluster_nms(const int64_t *order, const int64_t *starts, int64_t K, const int64_t *ov_start, const int64_t *ov_other,
                     const int64_t *ov_inter, int64_t P, float threshold, uint8_t *hot, uint8_t *keep, void *stream);
int tp3d_instance_ap_match(const int64_t *order, const int64_t *cls, const int64_t *cloud, const uint8_t *valid, int64_t K,
                           const int64_t *size, const int64_t *inter_cls, const int64_t *col_cls, const int64_t *gt_size,
                           int64_t G, double threshold, uint8_t *taken, uint8_t *tp, void *stream);

/* Data transforms (csrc/transforms.hip)
 *                       [core/data_transform/transforms.py, grid_transform.py:169-226]
 * Region cut: which rows of pos (N, 3) lie in each of B regions of one kind.  Integer counters and plain stores, no float
 * atomics, bit-equal repeats, nothing of size N * B in memory: a count pass writes one int per (region, tile of
 * tp3d_region_tile_rows() rows), one block scan turns them into offsets, the emit pass orders the rows of a tile by
 * ballot and prefix, so every list is ascending.
 *   kind   0 sphere     d2 < r^2,  d2 = (dx dx + dy dy) + dz dz, d = p - c, r = param[b][0]
 *          1 cylinder   as the sphere with d2 = dx dx + dy dy
 *          2 box        |q_i| < param[b][i] for i = 0, 1, 2, q = R d (rot (B, 3, 3) row-major, null: q = d)
 *          3 ellipsoid  ((qx qx) / (a a) + (qy qy) / (b b)) + (qz qz) / (c c) < 1, (a, b, c) = param[b]
 *          4 mask       mask[row] != 0 (keep mode only, B = 0, no pos)
 *     The fp32 inputs are promoted to double, differences first, then products, sums left to right, one rounding per
 *     operation (no fma): a numpy float64 restatement is bit-equal.
 *   flags  1 closed: <= in place of <;  2 skip_zero: a row with d2 == 0 is outside (d2 of its kind; box and ellipsoid
 *          use the sphere's);  4 align_origin: pos_out has the fp32 centre subtracted in fp32 (x, y only for a cylinder)
 *   mode   0 each: start (B + 1), index / batch (capacity) / pos_out (capacity, 3): region b owns the entries
 *            start[b] .. start[b + 1]: its rows ascending, its id, and their positions.  batch, pos_out may be null.
 *          1 keep: one ascending list of the rows that lie in NO region (kind 4: whose mask byte is set); start = [0, T];
 *            seg_out (S + 1) = the kept rows below seg[s], the per-scene offsets of the kept rows (null: not wanted).
 *   seg (S + 1), scene (B): region b looks only at rows seg[scene[b]] .. seg[scene[b] + 1] (a scene outside [0, S)
 *     holds none) and its workgroups read no other tile; scene null: every row.
 *   tp3d_region_count_f32 fills the workspace and writes start and status = [T, T > capacity] (capacity < 0: no bound;
 *     T = all entries).  tp3d_region_emit_f32 takes the same arguments and workspace and writes the entries below
 *     `capacity`; after an overflow the lists are cut there (nothing is written past the buffers) and seg_out is zero.
 *   N <= 2^31 - 1 and N * B <= 2^31 - 1 in each mode (TP3D_E_TOOBIG beyond): the offsets are ints.
 * Elastic distortion of a ragged batch.  Cloud b owns a noise grid dims[b] = (d0, d1, d2) cells of 3 channels, C order,
 * at floats goff[b] .. goff[b + 1] of `noise`; total = goff[B].
 *   tp3d_elastic_blur_f32: `rounds` rounds of the 3-tap box blur along axis 0, 1, 2 with zero padding, in place (tmp:
 *     `total` floats).  A pass sums the taps in ascending order in double over the fp32 weight float(1) / float(3) and
 *     rounds once to fp32: scipy.ndimage.convolve(mode="constant") on float32 input.
 *   tp3d_elastic_apply_f32: out = fp32(pos + interp(pos) * magnitude) in double; interp is trilinear over the axes
 *     axes[b][d] = (start, step, stop) doubles, value i = i * step + start, the last one = stop (numpy.linspace); the
 *     interval is the one with grid[i] <= x < grid[i + 1] (the last closed), the eight corners are summed in the order
 *     and with the weight products ((1 w_x) w_y) w_z of scipy's RegularGridInterpolator; a row outside the axes of its
 *     cloud, or of no cloud of seg (B + 1), is copied. */
int tp3d_region_tile_rows(void);
size_t tp3d_region_workspace_bytes(int64_t N, int64_t B, int mode);
int tp3d_region_count_f32(const float *pos, int64_t N, const int64_t *seg, int64_t S, int kind, int mode, int flags,
                          const float *centre, const float *param, const float *rot, const int64_t *scene,
                          const uint8_t *mask, int64_t B, int64_t capacity, int64_t *start, int64_t *status, void *workspace,
                          size_t workspace_bytes, void *stream);
int tp3d_region_emit_f32(const float *pos, int64_t N, const int64_t *seg, int64_t S, int kind, int mode, int flags,
                         const float *centre, const float *param, const float *rot, const int64_t *scene,
                         const uint8_t *mask, int64_t B, int64_t capacity, const int64_t *status, int64_t *index,
                         int64_t *batch, float *pos_out, int64_t *seg_out, const void *workspace, size_t workspace_bytes,
                         void *stream);
int tp3d_elastic_blur_f32(float *noise, float *tmp, const int32_t *dims, const int64_t *goff, int64_t B, int64_t total,
                          int rounds, void *stream);
int tp3d_elastic_apply_f32(const float *pos, const int64_t *seg, int64_t B, int64_t N, const float *noise,
                           const int32_t *dims, const int64_t *goff, const double *axes, double magnitude, float *out,
                           void *stream);

/* =====================================================================================================
 * FPFH descriptors (csrc/fpfh.hip): open3d's estimate_normals + compute_fpfh_feature over a hybrid (radius, max_nn)
 * search, as restated in float64 numpy by torch_points3d_amd/fpfh.py -- that file is the definition of every rule.
 * Ragged batches: seg_x (clouds + 1) row offsets of x, batch_y the cloud of every query.
 *   tp3d_hybrid_search_f32: of the rows of the query's cloud with (dx*dx + dy*dy) + dz*dz < radius*radius in fp32 (the
 *     membership of tp3d_ball_query_partial_dense_f32), the max_nn <= TP3D_FPFH_MAX_NN smallest by (dist2, index), in that
 *     order: idx (Nq, max_nn) global rows, dist2 (Nq, max_nn), both padded with -1, and count (Nq).  Served from the grid
 *     (cell edge = radius) for every max_nn; M <= 2^31 - 1.
 *   tp3d_fpfh_normals_f32: per row the unit eigenvector of the smallest eigenvalue of the covariance of its count
 *     neighbours (mean and covariance in double, slot order; cyclic Jacobi), (0, 0, 1) for count < 3; signed towards
 *     viewpoint (N, 3) or, with viewpoint null, so that its largest component (lowest axis on ties) is positive.
 *   tp3d_spfh_counts_f32: counts (N, 33): how many of the slots 1 .. count - 1 of a row fall into each of the 11 bins of
 *     the three Darboux-frame features; integer adds only.  The angle bin is decided against the ten edge directions of
 *     tp3d_fpfh_edge_table (table[20] = (cos, sin) of -pi + 2 pi e / 11, e = 1 .. 10; a host function), not by atan2.
 *   tp3d_fpfh_f32: for r < R the row i = rows[r] (rows null: i = r): out[b] = (sum[b / 11] != 0 ? acc[b] * 100 /
 *     sum[b / 11] : 0) + spfh_i[b], acc and sum over the slots 1 .. count - 1 with d2 != 0 of spfh_j[b] / d2 in double,
 *     spfh_j = counts_j * (100 / (count_j - 1)); out64 (R, 33) and / or out32 = its one rounding.
 * ===================================================================================================== */
#define TP3D_FPFH_MAX_NN 256
int tp3d_fpfh_edge_table(double *table);
size_t tp3d_hybrid_search_workspace_bytes(int num_clouds, int64_t rows, int max_cloud_points);
int tp3d_hybrid_search_f32(const float *x, const float *y, const int64_t *batch_y, const int64_t *seg_x, int num_clouds,
                           int max_cloud_points, int64_t M, int64_t Nq, float radius, int max_nn, int32_t *idx,
                           float *dist2, int32_t *count, void *workspace, size_t workspace_bytes, void *stream);
int tp3d_fpfh_normals_f32(const float *pos, const int32_t *idx, const int32_t *count, int64_t N, int max_nn,
                          const float *viewpoint, float *normals, void *stream);
int tp3d_spfh_counts_f32(const float *pos, const float *normals, const int32_t *idx, const int32_t *count, int64_t N,
                         int max_nn, int32_t *counts, void *stream);
int tp3d_fpfh_f32(const float *pos, const int32_t *idx, const int32_t *count, const int32_t *counts, const int64_t *rows,
                  int64_t R, int64_t N, int max_nn, double *out64, float *out32, void *stream);

/* =====================================================================================================
 * TSDF fusion (csrc/tsdf.hip): the reference's datasets/registration/fusion.py (TSDFVolume) and utils.py (extract_pcd,
 * rgbd2pcd), as restated in float64 numpy by torch_points3d_amd/tsdf.py -- that file is the definition of every rule, and
 * the device equals it bit for bit.  One owner per voxel, plain stores, no atomics of any kind.
 *   tp3d_tsdf_integrate: F <= TP3D_TSDF_MAX_FRAMES frames (F, H, W) into tsdf, weight (X, Y, Z) fp32, C order, in place.
 *     One thread per voxel, consecutive threads along z; the frames are applied in order in registers, so every volume
 *     element is read once and written at most once whatever F is, and the result is bit-equal to F one-frame calls.
 *     consts (F, TP3D_TSDF_CONSTS) doubles per frame: rows 0 .. 2 of inv(cam_pose) (12), double(fp32(fx, fy, cx, cy)), the
 *     observation weight.  depth_kind 0: uint16 raw, metres = double(raw) / depth_scale, zeroed above depth_thresh (give
 *     +inf for none); 1: float64 metres, used as they are.  Per voxel and frame:
 *       p_a = fp32(o_a + fp32(fp32(voxel_size) * fp32(i_a)));  c_r = ((M_r0 p_x + M_r1 p_y) + M_r2 p_z) + M_r3 in double;
 *       skip unless c_z > 0;  px = rint(c_x * fx / c_z + cx) (half to even), py likewise; skip unless 0 <= px < W and
 *       0 <= py < H (in double);  d = depth[py, px]; skip unless d > 0 and diff = d - c_z >= -trunc;
 *       dist = min(1, diff / trunc);  w_new = fp32(double(w) + obs);
 *       t = fp32((double(fp32(w * t)) + obs * dist) / double(w_new));  w = w_new.
 *     X * Y * Z <= (2^31 - 1) * 256 and Y * Z <= 2^31 - 1 (TP3D_E_TOOBIG beyond).
 *   tp3d_tsdf_surface_count / _emit: the voxels with |t| < tsdf_thresh and w > weight_thresh (fp32 compares) in ascending
 *     voxel index: pos (capacity, 3) doubles = double(i_a) * voxel_size + double(o_a) and / or index (capacity) flat voxel
 *     ids (either may be null).  The predicate is evaluated on the fly in both passes over tiles of tp3d_tsdf_tile_rows()
 *     voxels (count per tile, one block scan, ballot-and-prefix emit: the pieces of the region cut); no mask of volume size
 *     is written.  _count writes status = [T, T > capacity] (capacity < 0: no bound); _emit writes the entries below
 *     `capacity` and nothing past them.  N = X * Y * Z <= 2^31 - 1 (TP3D_E_TOOBIG beyond).
 *   tp3d_depth_unproject_count / _emit: F raw uint16 frames (F, H, W) as one ragged list: start (F + 1); per kept pixel
 *     ((Z < max_depth) & (Z > 0), Z = double(raw) / depth_scale, ascending pixel index) the world row pos (capacity, 3)
 *     doubles and pixel (capacity) = f * H * W + y * W + x (either may be null).  consts (F, TP3D_UNPROJECT_CONSTS): rows
 *     0 .. 2 of the pose (12), K00, K11, K02, K12.  X = ((x + 0.5) - K02) * Z / K00, Y likewise with y, K12, K11;
 *     pos_a = ((X r_a0 + Y r_a1) + Z r_a2) + t_a.  status and capacity as above; F * H * W <= 2^31 - 1.
 * ===================================================================================================== */
#define TP3D_TSDF_MAX_FRAMES 64
#define TP3D_TSDF_CONSTS 17
#define TP3D_UNPROJECT_CONSTS 16
int tp3d_tsdf_tile_rows(void);
int tp3d_tsdf_integrate(float *tsdf, float *weight, int64_t X, int64_t Y, int64_t Z, float ox, float oy, float oz,
                        double voxel_size, double trunc, const void *depth, int depth_kind, int F, int H, int W,
                        const double *consts, double depth_scale, double depth_thresh, void *stream);
size_t tp3d_tsdf_surface_workspace_bytes(int64_t N);
int tp3d_tsdf_surface_count(const float *tsdf, const float *weight, int64_t N, float tsdf_thresh, float weight_thresh,
                            int64_t capacity, int64_t *status, void *workspace, size_t workspace_bytes, void *stream);
int tp3d_tsdf_surface_emit(const float *tsdf, const float *weight, int64_t X, int64_t Y, int64_t Z, float ox, float oy,
                           float oz, double voxel_size, float tsdf_thresh, float weight_thresh, int64_t capacity,
                           double *pos, int64_t *index, const void *workspace, size_t workspace_bytes, void *stream);
size_t tp3d_depth_unproject_workspace_bytes(int64_t F, int64_t HW);
int tp3d_depth_unproject_count(const uint16_t *depth, int64_t F, int64_t H, int64_t W, double depth_scale, double max_depth,
                               int64_t capacity, int64_t *start, int64_t *status, void *workspace, size_t workspace_bytes,
                               void *stream);
int tp3d_depth_unproject_emit(const uint16_t *depth, int64_t F, int64_t H, int64_t W, const double *consts,
                              double depth_scale, double max_depth, int64_t capacity, double *pos, int64_t *pixel,
                              const void *workspace, size_t workspace_bytes, void *stream);

/* =====================================================================================================
 * Launch plans (host arithmetic only, no device work): what an entry point WILL do for given sizes -- how it
 * splits the rows, how many partial rows it writes, how it carves its workspace.  tests/test_plans_cpu.py sweeps
 * them against the workspace-size queries above, so that "the extent a kernel writes <= the size the caller was
 * told to allocate" is checked for every shape without a GPU.  All return 0 or TP3D_E_BADARG.
 * ===================================================================================================== */
/* plan[8]: splits, rows per split, tile rows (N side), tile columns (K side), tiles, rows staged per step,
 * workspace floats written, first row of the last split */
int tp3d_gemm_tn_plan(int64_t M, int N, int K, int64_t *plan);
/* plan[0..7] = splits, rows per split, tile rows (n), tile columns (k, strip included), tiles, rows staged per step,
 * workspace floats, dynamic LDS bytes of tp3d_gemm_tn_x3_f32 */
int tp3d_gemm_tn_x3_plan(int64_t M, int N, int K, int64_t *plan);
/* plan[9]: column tiles, row blocks, work items, workgroups, statistics chunks written, 1 = one chunk set per
 * workgroup, wave rows per tile, K-ranges of a split launch (K = 0: not asked), tile columns */
int tp3d_gemm_rows_plan(int64_t M, int N, int K, int64_t *plan);
/* Few-row launches (at most 256 work items of 128 x 128, no K-split) run as 64 x 64 tiles, four workgroups per item;
 * plan[4]: 64 x 64 work items, workgroups (<= 1024), 1 = taken with statistics, 1 = taken without (a K-split launch
 * never is).  C, the statistics chunks and tp3d_gemm_rows_stat_chunks / _stat_floats are the same either way. */
int tp3d_gemm_rows_small_plan(int64_t M, int N, int K, int64_t *plan);
/* on = 1 (default): the few-row tile rules of tp3d_gemm_rows_f32 / _epi_f32 (above) and tp3d_gemm_tn_f32 (a smaller
 * tile where tiles x splits < 256; splits and rows per split untouched); on = 0: the plans without them.  Results are
 * bit-identical.  Process-wide and not synchronised: set it before plans are queried or a step is captured. */
int tp3d_set_few_row_tiles(int on);
/* plan[3]: rows per chunk, chunks, workspace floats written by tp3d_bn_stats_f32 (pooled_ns = 0) or
 * tp3d_bn_act_bwd_f32 (pooled_ns = its ns; 1 for the dense form) */
int tp3d_bn_plan(int64_t M, int C, int pooled_ns, int64_t *plan);
/* plan[9]: byte offsets of start, order, scratch, wsorted (-1 = none), merge_tmp; workspace bytes; 1 = table
 * inverted flat over the batch; ints of scratch that path needs; byte offset of the hub list (1 + B*nbins ints) */
int tp3d_scatter_plan(int B, int L, int nbins, int with_weights, int64_t *plan);

#ifdef __cplusplus
}
#endif
#endif /* TP3D_HIP_H */
