/*
 * ppea_depth.h -- C ABI of libppea_depth.so (gfx950 / MI355X).
 *
 * The drop-in boundary of the PPEA-Depth training hot path.
 * Every entry point replaces a stock ATen/cuDNN op sequence at the cited
 * reference call site (paths relative to /root/reference/ppeadepth/).
 *
 * Conventions
 *   - all pointers are DEVICE pointers into contiguous row-major (NCHW) buffers
 *     owned by the caller; kernels never allocate or free;
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); every
 *     call only enqueues work on that stream and returns;
 *   - the return value is a hipError_t (0 = hipSuccess); PPEA_ERR_UNSUPPORTED
 *     (= -1) is returned for argument combinations the library does not serve;
 *   - fp32 I/O entry points end in _f32, bf16 I/O (fp32 accumulate) in _bf16.
 */
#ifndef PPEA_DEPTH_H
#define PPEA_DEPTH_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PPEA_ERR_UNSUPPORTED (-1)
#define PPEA_ERR_ARG (-2)          /* inconsistent arguments (e.g. a required pointer is NULL) */

/* Library / build identification: returns the ABI version (bumped on any signature change). */
int ppea_abi_version(void);

/* Measurement aid (tools/step_timeline.py): a one-lane launch on `stream` that writes the device's constant-rate clock
 * (wall_clock64, 100 MHz) to *slot (uint64, device memory) -- a timestamp of that point of the stream that also works inside
 * a captured graph, where HIP events cannot be timed. */
int ppea_timestamp(void* slot, void* stream);

/* ------------------------------------------------------------------------------------------
 * A1  Large-kernel depthwise convolution  (networks/replknet_adapter.py:151-168 get_conv2d,
 *     :232-239 ReparamLargeKernelConv.forward).  stride 1, pad K/2, dilation 1, no bias.
 *     x [N,C,H,W]; w_big [C,1,K,K]; w_small [C,1,KS,KS] or NULL (then y_small is ignored).
 *     One launch produces both branches from one LDS-resident input tile.
 *     K odd, 7 <= K <= 31; KS in {0 (absent), 3, 5}.
 * ---------------------------------------------------------------------------------------- */
int ppea_dwconv_lk_fwd_f32(const float* x, const float* w_big, const float* w_small,
                           float* y_big, float* y_small,
                           int N, int C, int H, int W, int K, int KS, void* stream);
int ppea_dwconv_lk_fwd_bf16(const uint16_t* x, const float* w_big, const float* w_small,
                            uint16_t* y_big, uint16_t* y_small,
                            int N, int C, int H, int W, int K, int KS, void* stream);

/* dgrad of the pair: dx = corr(dy_big, flip(w_big)) + corr(dy_small, flip(w_small)).
 * dy_small / w_small may be NULL. */
int ppea_dwconv_lk_bwd_data_f32(const float* dy_big, const float* dy_small,
                                const float* w_big, const float* w_small, float* dx,
                                int N, int C, int H, int W, int K, int KS, void* stream);
int ppea_dwconv_lk_bwd_data_bf16(const uint16_t* dy_big, const uint16_t* dy_small,
                                 const float* w_big, const float* w_small, uint16_t* dx,
                                 int N, int C, int H, int W, int K, int KS, void* stream);

/* bf16 on the matrix cores (banded-Toeplitz MFMA kernel, csrc/dwconv_mfma.hip).  The filters are packed
 * ONCE per weight version (they are frozen in PPEA-Depth Stage 1/2, repdepth.py:47-50) into a bf16 image
 * from which every wave builds its register-resident Toeplitz fragments:
 *   ppea_dwconv_lk_packed_bytes(C, K)            size of the packed buffer for w [C,1,K,K]
 *   ppea_dwconv_lk_pack_bf16(w, packed, C, K, flip)   flip = 0 for fwd, 1 for dgrad (both axes reversed)
 *   ppea_dwconv_lk_fwd_bf16p / _bwd_data_bf16p   as the _bf16 entry points above, with packed filters
 *                                                (packed_small may be NULL; KS in {0, 5}; K in {31,29,27,13}).
 * Returns PPEA_ERR_UNSUPPORTED for shapes it does not serve; callers then use the _bf16 entry points. */
long ppea_dwconv_lk_packed_bytes(int C, int K);
int ppea_dwconv_lk_pack_bf16(const float* w, void* packed, int C, int K, int flip, void* stream);
int ppea_dwconv_lk_fwd_bf16p(const uint16_t* x, const void* packed_big, const void* packed_small,
                             uint16_t* y_big, uint16_t* y_small,
                             int N, int C, int H, int W, int K, int KS, void* stream);
/* Forward with the BatchNorm (+ ReLU) of the INPUT fused into the staging pass: RepLKBlock's pw1 conv_bn_relu -> large
 * kernel (replknet_adapter.py:305-308 with :182-197).  x = the 1x1 conv's output, `sums` [C][P][2] its epilogue's partial
 * (sum, sum of squares) (ppea_pwconv_stats_bf16), count = N*H*W.  Every wave finalises its channel's statistics (fp64, the
 * arithmetic of ppea_bn_finalize_sums_f32) and stages relu(gamma * (x - mean) * invstd + beta) rounded to bf16, zero
 * outside the plane; mean / invstd [C] are written for backward, running statistics updated unless NULL.  KS must be 5. */
int ppea_dwconv_lk_fwd_bn_bf16p(const uint16_t* x, const void* packed_big, const void* packed_small, uint16_t* y_big,
                                uint16_t* y_small, const float* sums, int P, long count, const float* gamma,
                                const float* beta, float eps, float momentum, float* running_mean, float* running_var,
                                float* mean, float* invstd, int N, int C, int H, int W, int K, int KS, void* stream);
/* forward + the statistics of the two BatchNorms that follow the re-parameterised pair (replknet_adapter.py:232-239):
 * stats [2][C][P][2] fp32, P = ppea_dwconv_lk_stats_partials(...) partial (sum, sum of squares) pairs per channel of the
 * stored y_big (first half) / y_small values; reduce each half with ppea_bn_finalize_sums_f32. */
int ppea_dwconv_lk_stats_partials(int N, int C, int H, int W, int K, int KS);
int ppea_dwconv_lk_fwd_stats_bf16p(const uint16_t* x, const void* packed_big, const void* packed_small, uint16_t* y_big,
                                   uint16_t* y_small, float* stats, int N, int C, int H, int W, int K, int KS,
                                   void* stream);
int ppea_dwconv_lk_bwd_data_bf16p(const uint16_t* dy_big, const uint16_t* dy_small,
                                  const void* packed_big_flip, const void* packed_small_flip,
                                  uint16_t* dx, int N, int C, int H, int W, int K, int KS, void* stream);

/* Depthwise 3x3, stride 1 or 2, pad 1, no bias (stem[1], stem[3], transitions[.][1];
 * replknet_adapter.py:414-416, 451-453).  w [C,1,3,3] fp32.  bwd_data: H, W are the forward INPUT sizes. */
int ppea_dwconv3x3_fwd_f32(const void* x, const float* w, void* y, int N, int C, int H, int W, int stride, void* stream);
int ppea_dwconv3x3_fwd_bf16(const void* x, const float* w, void* y, int N, int C, int H, int W, int stride, void* stream);
int ppea_dwconv3x3_bwd_data_f32(const void* dy, const float* w, void* dx, int N, int C, int H, int W, int stride, void* stream);
int ppea_dwconv3x3_bwd_data_bf16(const void* dy, const float* w, void* dx, int N, int C, int H, int W, int stride, void* stream);
/* The kernel these four and ppea_dwconv3x3_fwd_affine_* launch (host only, no device needed): elem_bytes 4 (f32) | 2 (bf16);
 * mode 0 forward, 1 data gradient, 2 affine forward.  Returns 0 the one-pixel-per-thread kernel, 1 dw3v_s1 (bf16, stride 1,
 * W % 8 == 0), 2 dw3v_s2_fwd / 3 dw3v_s2_bwd (bf16, stride 2, H and W even, Wo % 8 == 0), or PPEA_ERR_UNSUPPORTED exactly
 * where the entry points return it (stride not in {1, 2}, N * C > 65535, a size <= 0). */
int ppea_dwconv3x3_plan(int elem_bytes, int mode, int N, int C, int H, int W, int stride);

/* wgrad (only needed with --fullft_reb, repdepth.py:47, and by the plug-in's weight.grad):
 * dw[c,0,u,v] = sum_{n,i,j} dy[n,c,i,j] * x[n,c,i+u-K/2,j+v-K/2].  dw is overwritten. */
int ppea_dwconv_lk_bwd_filter_f32(const float* x, const float* dy, float* dw,
                                  int N, int C, int H, int W, int K, void* stream);
/* The same quantity for bf16 activations on the matrix cores (csrc/dwconv_wgrad.hip): per channel a 32 x 32 GEMM tile
 * over k = (n, input row, column), dw_c[u][v] = sum_k dy[n,c,r-u+K/2,j] * x[n,c,r,j+v-K/2].  BOTH filters of the
 * re-parameterised pair leave one launch that reads x once (dy_small / dw_small NULL iff KS == 0); dw_* are fp32 and
 * overwritten.  The (n, row band) parts go through `workspace` (ppea_dwconv_lk_bwd_filter_workspace_bytes bytes) and are
 * added in a fixed order by a second launch: no atomics.  Served: K in {31, 29, 27, 13}, KS in {0, 5}, W <= 4096 and
 * N * H < 2^30 (any C, planes smaller than the filter included); otherwise both return PPEA_ERR_UNSUPPORTED and the
 * caller keeps the _f32 entry point. */
long ppea_dwconv_lk_bwd_filter_workspace_bytes(int N, int C, int H, int W, int K, int KS);
int ppea_dwconv_lk_bwd_filter_bf16(const uint16_t* x, const uint16_t* dy_big, const uint16_t* dy_small,
                                   float* dw_big, float* dw_small, void* workspace,
                                   int N, int C, int H, int W, int K, int KS, void* stream);
/* wgrad of the depthwise 3x3 (stride 1 / 2, pad 1): dw[c,0,u,v] = sum_{n,i,j} dy[n,c,i,j] * x[n,c,i*s+u-1,j*s+v-1], fp32,
 * overwritten; x [N,C,H,W], dy [N,C,Ho,Wo].  Per-part sums through `workspace`, added in a fixed order (no atomics). */
long ppea_dwconv3x3_bwd_filter_workspace_bytes(int N, int C, int H, int W, int stride);
int ppea_dwconv3x3_bwd_filter_f32(const void* x, const void* dy, float* dw, void* workspace, int N, int C, int H, int W,
                                  int stride, void* stream);
int ppea_dwconv3x3_bwd_filter_bf16(const void* x, const void* dy, float* dw, void* workspace, int N, int C, int H, int W,
                                   int stride, void* stream);

/* ------------------------------------------------------------------------------------------
 * A5/A6  Pointwise (1x1) convolution on MFMA, NCHW bf16 (csrc/pwconv.hip): RepLKBlock.pw1/pw2,
 *     ConvFFN.pw1/pw2, stem[2], transitions[.][0] (replknet_adapter.py:270-271, 296-297, 415, 452).
 *     Y[b][m][p] = sum_k A[m][k] * X[b][k][p] (+ bias[m]);  A [M][K] bf16 row-major = the conv weight
 *     [Cout][Cin] for forward, its transpose for the data gradient.  X [B][K][HW], Y [B][M][HW].
 *     Fast path needs K % 32 == 0 and HW % 8 == 0; otherwise PPEA_ERR_UNSUPPORTED.
 * ---------------------------------------------------------------------------------------- */
int ppea_pwconv_bf16(const void* A, const void* X, const float* bias, void* Y, int B, int M, int K, int HW,
                     void* stream);

/* ------------------------------------------------------------------------------------------
 * A4  Adapters (replknet_adapter.py:20-47 `Adapter`: Linear -> GELU -> Linear over channels;
 *     :49-109 `B_Adapter`, adpt_test 4: Conv2d(C, C/4, 3, 1, 1) -> GELU -> Linear(C/4, C)), forward and
 *     all gradients, NCHW bf16 end to end (no layout changes), built from four entry points:
 *
 *   ppea_pwconv_ex_bf16   the GEMM above with an epilogue. epi 0: Y = A X + bias.  epi 1: Y = pre-activation,
 *                         Y2 = GELU(pre).  epi 2: Y = (A X) * GELU'(aux)  (aux, Y, Y2: [B][M][HW] bf16).
 *                         bias: fp32, or bf16 when bias_bf16 != 0.  a_transposed != 0: the matrix is passed as
 *                         At [K][M] (M % 8 == 0), so a data gradient consumes the forward weight unchanged.
 *   ppea_pwgrad_bf16      weight gradients: out[m*N + n] = sum_{b,p} P[b][m][p] Q[b][n][p] (fp32), followed by
 *                         the row sums of P (bias gradient) at out[M*N + m] when want_rowsum != 0.
 *                         P [B][M][HW], Q [B][N][HW] bf16, HW % 8 == 0.  `workspace`: device scratch of
 *                         ppea_pwgrad_workspace_bytes(B, M, N, HW) bytes (split-K partials; deterministic).
 *   ppea_tapsum_fwd_bf16  the 3x3 conv = GEMM with the tap-major weight matrix [9*Ch][C] (rows t*Ch + m,
 *                         t = 3*ky + kx) followed by this shift-and-add: pre[b][m][y][x] = bias[m] +
 *                         sum_t T[b][t*Ch+m][y+ky-1][x+kx-1] (zero padded), h = GELU(pre).  W % 4 == 0.
 *   ppea_tapsum_bwd_bf16  its adjoint: dT[b][t*Ch+m][y][x] = g[b][m][y-ky+1][x-kx+1].
 * ---------------------------------------------------------------------------------------- */
/* ppea_pwconv_bf16 + the statistics of the BatchNorm that follows it (conv_bn / conv_bn_relu, replknet_adapter.py:182-197):
 * stats [M][P][2] fp32 = per output channel (sum, sum of squares) of the stored bf16 values over P disjoint pixel sets,
 * P = ppea_pwconv_stats_partials(B, M, K, HW); ppea_bn_finalize_sums_f32 turns them into mean / biased var / invstd of
 * `count` values per channel and updates the running statistics (fp64 totals, fixed order) -- no statistics pass over Y. */
int ppea_pwconv_stats_partials(int B, int M, int K, int HW);
int ppea_pwconv_stats_bf16(const void* A, const void* X, const float* bias, void* Y, float* stats, int B, int M, int K,
                           int HW, void* stream);
int ppea_bn_finalize_sums_f32(const float* partial, int P, int C, long count, float eps, float momentum, float* mean,
                              float* var, float* invstd, float* running_mean, float* running_var, void* stream);
int ppea_pwconv_ex_bf16(const void* A, const void* X, const void* bias, int bias_bf16, int epi, const void* aux,
                        void* Y, void* Y2, int B, int M, int K, int HW, int a_transposed, void* stream);
/* Inference forms of the depthwise convs (eval-mode BatchNorm folded):
 *   ppea_dwconv_lk_fwd_bias_act_bf16p  y = act(DW_K(x; packed merged filter) + bias[c]) on the MFMA kernel: an eval-mode
 *       ReparamLargeKernelConv (+ ReLU) in one launch; packed = ppea_dwconv_lk_pack_bf16 of a_big W_k + pad(a_small W_5),
 *       bias = o_big + o_small; relu != 0: ReLU.  K in {31, 29, 27, 13}; unserved shapes: PPEA_ERR_UNSUPPORTED.
 *   ppea_dwconv_lk_fwd_bias_act_f32 / _bf16  the same on the fp32-arithmetic kernel with the fp32 filter [C][K][K].
 *   ppea_dwconv3x3_fwd_affine_f32 / _bf16    y = act(s[c] * DW3x3(x) + o[c]) (stem[1], stem[3], transitions[.][1]). */
int ppea_dwconv_lk_fwd_bias_act_bf16p(const uint16_t* x, const void* packed, const float* bias, int relu, uint16_t* y, int N,
                                      int C, int H, int W, int K, void* stream);
int ppea_dwconv_lk_fwd_bias_act_f32(const void* x, const float* w, const float* bias, int relu, void* y, int N, int C, int H,
                                    int W, int K, void* stream);
int ppea_dwconv_lk_fwd_bias_act_bf16(const void* x, const float* w, const float* bias, int relu, void* y, int N, int C, int H,
                                     int W, int K, void* stream);
int ppea_dwconv3x3_fwd_affine_f32(const void* x, const float* w, const float* s, const float* o, int relu, void* y, int N, int C,
                                  int H, int W, int stride, void* stream);
int ppea_dwconv3x3_fwd_affine_bf16(const void* x, const float* w, const float* s, const float* o, int relu, void* y, int N, int C,
                                   int H, int W, int stride, void* stream);
/* Inference form (eval-mode BatchNorm folded into a per-channel fp32 table applied to the accumulator; the matrix is the
 * training model's bf16 weight, unchanged):  t = act(s[m] * (A X)[m][p] + o[m]), act 0 none / 1 ReLU / 2 GELU(erf), s NULL = 1,
 * o NULL = 0;  Y = t (+ r1) (+ r2_scale * r2), r1 / r2 [B][M][HW] bf16 or NULL;  Y2 (optional) = s2[m] * Y + o2[m] of Y as
 * stored: the next block's first BatchNorm.  K % 32 == 0 and HW % 8 == 0, else PPEA_ERR_UNSUPPORTED. */
int ppea_pwconv_infer_bf16(const void* A, const void* X, const float* s, const float* o, int act, const void* r1,
                           const void* r2, float r2_scale, const float* s2, const float* o2, void* Y, void* Y2, int B, int M,
                           int K, int HW, void* stream);
long ppea_pwgrad_workspace_bytes(int B, int M, int N, int HW);
int ppea_pwgrad_bf16(const void* P, const void* Q, float* out, void* workspace, int B, int M, int N, int HW,
                     int want_rowsum, void* stream);
/* ppea_pwgrad_ex_bf16: same GEMM, results written straight into the parameter gradients: out_w fp32 or bf16
 * (out_w_bf16), [M][N] for taps = 1 or, for the tap-major 3x3 form (taps = 9, rows t*Ch + m), nn.Conv2d layout
 * [Ch][N][3][3]; out_b (may be NULL) = row sums of rows [b_row0, b_row0 + b_rows). */
int ppea_pwgrad_ex_bf16(const void* P, const void* Q, void* workspace, int B, int M, int N, int HW, void* out_w,
                        int out_w_bf16, int taps, void* out_b, int out_b_bf16, int b_row0, int b_rows, void* stream);
/* Two such problems over the same [B][.][HW] pixels (an adapter's D_fc2 and D_fc1 weight gradients, replknet_adapter.py:20-109)
 * in ONE GEMM launch and ONE reduce launch; every argument that differs is an array of two.  HW % 32 == 0, else
 * PPEA_ERR_UNSUPPORTED / a workspace size of -1: call ppea_pwgrad_ex_bf16 twice. */
long ppea_pwgrad_pair_workspace_bytes(int B, const int* M, const int* N, int HW);
int ppea_pwgrad_ex_pair_bf16(const void* const* P, const void* const* Q, void* workspace, int B, const int* M, const int* N,
                             int HW, void* const* out_w, const int* out_w_bf16, const int* taps, void* const* out_b,
                             const int* out_b_bf16, const int* b_row0, const int* b_rows, void* stream);
int ppea_tapsum_fwd_bf16(const void* T, const void* bias, int bias_bf16, void* pre, void* h, int B, int Ch, int H,
                         int W, void* stream);
int ppea_tapsum_bwd_bf16(const void* g, void* dT, int B, int Ch, int H, int W, void* stream);
/* Plans of the pointwise GEMM kernels (ABI 27).  Host only, no device call, no stream; each is answered by the function the
 * launch itself goes by, under the PPEA_PW_TILE / PPEA_PW_V2 / PPEA_PWGRAD_V2 hooks as the launch reads them (per call).
 *   ppea_pwconv_plan   what ppea_pwconv_bf16, _stats_bf16, _ex_bf16 (a_transposed as given) and _infer_bf16 (which serves
 *        version 2 only) launch for B, M, K, HW.  plan[8]:
 *          [0] version  1 pwconv_kernel<BM, ., WN, EPI, a_transposed, BK>, 2 pwconv2_kernel<BM, BK, EPI, a_transposed>
 *          [1] BM  [2] BK  [3] WN (pixel-waves per workgroup)  [4] [5] [6] grid x, y, z
 *          [7] P   statistics partials per channel (= ppea_pwconv_stats_partials for a_transposed == 0)
 *        PPEA_ERR_UNSUPPORTED exactly where those entry points return it for their shape arguments.
 *   ppea_pwgrad_plan   the split of ppea_pwgrad_bf16 / ppea_pwgrad_ex_bf16.  plan[9]:
 *          [0] pixel step of pwgrad2_kernel<step> (0: pwgrad_kernel, 64 pixels per step)  [1] steps per image
 *          [2] total steps  [3] steps per split  [4] S (splits = grid x)  [5] tiles along M  [6] tiles along N
 *          [7] [8] workspace bytes (= ppea_pwgrad_workspace_bytes): the low 31 bits, the bits above them
 *   ppea_pwgrad_pair_plan   the same for ppea_pwgrad_ex_pair_bf16 (pwgrad2_pair_kernel<32>): [5] [6] = tiles of problem 0,
 *        of problem 1;  [7] [8] = ppea_pwgrad_pair_workspace_bytes.  PPEA_ERR_UNSUPPORTED where the pair form is not served. */
int ppea_pwconv_plan(int B, int M, int K, int HW, int a_transposed, int* plan);
/* Test support, host only: ppea_pwconv_plan for one B and A mode over M = Mstep * (1..nM) x K = 32 * (1..nK) x
 * HW = 8 * (1..nHW); out[nM][nK][nHW], one byte per shape: bit 0 version 2, bits 1-2 BM (0: 32, 1: 64, 2: 128), bit 3
 * BK = 64; 0xff: not served.  summary[2] = shapes served, row-major shapes whose ppea_pwconv_stats_partials is not plan[7]. */
int ppea_pwconv_plan_sweep(int B, int a_transposed, int Mstep, int nM, int nK, int nHW, unsigned char* out, long* summary);
int ppea_pwgrad_plan(int B, int M, int N, int HW, int* plan);
int ppea_pwgrad_pair_plan(int B, const int* M, const int* N, int HW, int* plan);

/* ------------------------------------------------------------------------------------------
 * A2 (+A5/A6 glue)  Training-mode BatchNorm fused with its neighbours (csrc/bn_fused.hip):
 *     y = act( BN_a(z1) [+ BN_b(z2)] ) [* mask[n]] [+ r1] [+ r2_scale * r2]
 *   replaces conv_bn / conv_bn_relu (replknet_adapter.py:182-197), the two-branch sum of
 *   ReparamLargeKernelConv.forward (:232-239) and the residual / DropPath / adapter adds of
 *   RepLKBlock.forward (:315-326) and ConvFFN.forward (:283-289).  NCHW, HW = H*W.
 *   act: 0 none, 1 ReLU, 2 GELU(erf).  z2, mask [N], r1, r2 may be NULL.
 *   stats = host array of 8 DEVICE pointers {mean1, invstd1, gamma1, beta1, mean2, invstd2, gamma2, beta2}.
 *   forward : ppea_bn_stats_*   per-plane (mean, M2) -> partial [C][N][2]
 *             ppea_bn_finalize_f32  Chan-combine -> mean/var(biased)/invstd [C]; running stats updated
 *                                   (momentum, unbiased var) unless running_mean is NULL
 *             ppea_bn_apply_*
 *   backward: g = dy * mask[n] * act'(u);
 *             ppea_bn_bwd_reduce_*  -> partial [C][N][3] = sum g, sum g*zhat1, sum g*zhat2
 *             ppea_bn_bwd_finalize_f32 -> sums [3][C]  (d_beta = sums[0], d_gamma_k = sums[k])
 *             ppea_bn_bwd_apply_*   dz_k = gamma_k*invstd_k*(g - sums0*inv_count - zhat_k*sums_k*inv_count)
 * ---------------------------------------------------------------------------------------- */
int ppea_bn_stats_f32(const void* z, float* partial, int N, int C, int HW, void* stream);
int ppea_bn_stats_bf16(const void* z, float* partial, int N, int C, int HW, void* stream);
int ppea_bn_finalize_f32(const float* partial, int N, int C, int HW, float eps, float momentum,
                         float* mean, float* var, float* invstd, float* running_mean,
                         float* running_var, void* stream);
/* Small channels (N*HW <= 16384 elements, HW % 8 == 0, C >= 64): statistics (resp. backward sums) final in ONE
 * launch, one wave per channel over all N planes; PPEA_ERR_UNSUPPORTED otherwise (use the two-launch forms). */
int ppea_bn_stats_final_f32(const void* z, int N, int C, int HW, float eps, float momentum, float* mean, float* var,
                            float* invstd, float* running_mean, float* running_var, void* stream);
int ppea_bn_stats_final_bf16(const void* z, int N, int C, int HW, float eps, float momentum, float* mean, float* var,
                             float* invstd, float* running_mean, float* running_var, void* stream);
int ppea_bn_bwd_reduce_final_f32(const void* dy, const void* z1, const void* z2, const float* const* stats,
                                 const float* mask, float* sums, int act, int N, int C, int HW, void* stream);
int ppea_bn_bwd_reduce_final_bf16(const void* dy, const void* z1, const void* z2, const float* const* stats,
                                  const float* mask, float* sums, int act, int N, int C, int HW, void* stream);
/* SyncBatchNorm across ranks (one packed all-gather per BN forward, trainer.py:215-222 + get_bn rka.py:176-180):
 * local statistics in wire layout packed[2C+1] = mean[C] | biased var[C] | count, and the Chan combine of the
 * gathered [world][2C+1] table into mean / invstd (running statistics updated unless running_mean is NULL). */
int ppea_bn_finalize_packed_f32(const float* partial, int N, int C, int HW, float* packed, void* stream);
/* same wire layout straight from the tensor in one launch (small channels; PPEA_ERR_UNSUPPORTED otherwise) */
int ppea_bn_stats_packed_f32(const void* z, int N, int C, int HW, float* packed, void* stream);
int ppea_bn_stats_packed_bf16(const void* z, int N, int C, int HW, float* packed, void* stream);
int ppea_bn_sync_combine_f32(const float* gathered, int world, int C, float eps, float momentum, float* mean,
                             float* invstd, float* running_mean, float* running_var, void* stream);
/* One launch per BN and direction for small channels (N * HW <= 16384, HW % 8 == 0, C >= 64): the workgroup that
 * owns a channel keeps its values in registers, so statistics + apply (forward) and reduce + apply (backward) are one
 * kernel each.  prm = {gamma1, beta1, gamma2, beta2}; out = {running_mean1, running_var1, running_mean2, running_var2
 * (NULL: no update), mean1, invstd1, mean2, invstd2 (written)}; `sums` [3][C] as ppea_bn_bwd_reduce_final_*.
 * Same semantics as rka.py:182-197, 232-239, 283-289, 315-326 (training-mode BN + act + DropPath + residuals). */
int ppea_bn_fwd_channel_f32(const void* z1, const void* z2, const float* const* prm, float* const* out, float eps,
                            float momentum, const float* mask, const void* r1, const void* r2, float r2_scale, void* y,
                            int act, int N, int C, int HW, void* stream);
int ppea_bn_fwd_channel_bf16(const void* z1, const void* z2, const float* const* prm, float* const* out, float eps,
                             float momentum, const float* mask, const void* r1, const void* r2, float r2_scale, void* y,
                             int act, int N, int C, int HW, void* stream);
/* The same forward for ONE BatchNorm whose statistics come from the producing GEMM's epilogue (partial [C][P][2] from
 * ppea_pwconv_stats_bf16): no reduction over the activation, no workgroup barrier.  prm = {gamma, beta}; out =
 * {running_mean, running_var (NULL: no update), mean, invstd}.  Backward: ppea_bn_bwd_channel_*. */
int ppea_bn_fwd_channel_sums_f32(const void* z, const float* partial, int P, const float* const* prm, float* const* out,
                                 float eps, float momentum, const float* mask, const void* r1, const void* r2, float r2_scale,
                                 void* y, int act, int N, int C, int HW, void* stream);
int ppea_bn_fwd_channel_sums_bf16(const void* z, const float* partial, int P, const float* const* prm, float* const* out,
                                  float eps, float momentum, const float* mask, const void* r1, const void* r2, float r2_scale,
                                  void* y, int act, int N, int C, int HW, void* stream);
/* acc (or NULL): a gradient that reaches z1 through another consumer (the block's residual connection, rka.py:289, 326);
 * dz1 = BN-backward(dy) + acc in the same launch instead of a separate element-wise add. */
int ppea_bn_bwd_channel_f32(const void* dy, const void* z1, const void* z2, const float* const* stats, const float* mask,
                            float inv_count, const void* acc, void* dz1, void* dz2, float* sums, int act, int N, int C,
                            int HW, void* stream);
int ppea_bn_bwd_channel_bf16(const void* dy, const void* z1, const void* z2, const float* const* stats, const float* mask,
                             float inv_count, const void* acc, void* dz1, void* dz2, float* sums, int act, int N, int C,
                             int HW, void* stream);
/* An output with TWO consumers (RepLKBlock / ConvFFN: the first 1x1 conv and the adapter both read the block's first
 * BatchNorm, replknet_adapter.py:283-289, 315-326): dyb / dy2b = the second consumer's gradient.  The kernels start from
 * round(dy + dyb) -- what a separate element-wise add would have stored -- so results are bit-identical to that form. */
int ppea_bn_bwd_channel_dup_f32(const void* dy, const void* dyb, const void* z1, const void* z2, const float* const* stats,
                                const float* mask, float inv_count, const void* acc, void* dz1, void* dz2, float* sums,
                                int act, int N, int C, int HW, void* stream);
int ppea_bn_bwd_channel_dup_bf16(const void* dy, const void* dyb, const void* z1, const void* z2, const float* const* stats,
                                 const float* mask, float inv_count, const void* acc, void* dz1, void* dz2, float* sums,
                                 int act, int N, int C, int HW, void* stream);
int ppea_bn_bwd_channel_next_dup_f32(const void* dy2, const void* dy2b, const void* dskip, const void* z, const void* y,
                                     const float* const* stats, const float* mask, float inv_count, void* dz, void* dy,
                                     float* sums, int N, int C, int HW, void* stream);
int ppea_bn_bwd_channel_next_dup_bf16(const void* dy2, const void* dy2b, const void* dskip, const void* z, const void* y,
                                      const float* const* stats, const float* mask, float inv_count, void* dz, void* dy,
                                      float* sums, int N, int C, int HW, void* stream);
/* Several ranks (reduce -> all-reduce -> apply): the reduce launch merges the two gradients and stores dym = round(dy + dyb)
 * for the apply launch.  Limits of ppea_bn_bwd_reduce_final_*. */
int ppea_bn_bwd_reduce_final_dup_f32(const void* dy, const void* dyb, void* dym, const void* z1, const void* z2,
                                     const float* const* stats, const float* mask, float* sums, int act, int N, int C,
                                     int HW, void* stream);
int ppea_bn_bwd_reduce_final_dup_bf16(const void* dy, const void* dyb, void* dym, const void* z1, const void* z2,
                                      const float* const* stats, const float* mask, float* sums, int act, int N, int C,
                                      int HW, void* stream);
/* End of one block and the first BatchNorm of the next in one launch per direction (replknet_adapter.py:283-289,
 * 315-326 followed by the next block's prelkb_bn / preffn_bn, :281, :312): y = mask * BN_A(z) + r1 + r2_scale * r2,
 * y2 = BN_B(y) with BN_B's statistics taken of the stored y.  prm = {gammaA, betaA, gammaB, betaB}; out = {running_meanA,
 * running_varA, running_meanB, running_varB (NULL: no update), meanA, invstdA, meanB, invstdB (written)}.  Backward:
 * stats = {meanA, invstdA, gammaA, betaA, meanB, invstdB, gammaB, betaB}; dskip = gradient of y from its other consumer
 * (NULL: none); writes dz, dy (total gradient of y) and sums [4][C] = dbetaA | dgammaA | dbetaB | dgammaB.
 * Results are bit-identical to ppea_bn_fwd_channel_* / ppea_bn_bwd_channel_* applied twice. */
int ppea_bn_fwd_channel_next_f32(const void* z, const float* const* prm, float* const* out, float eps, float momentum,
                                 const float* mask, const void* r1, const void* r2, float r2_scale, void* y, void* y2,
                                 int N, int C, int HW, void* stream);
int ppea_bn_fwd_channel_next_bf16(const void* z, const float* const* prm, float* const* out, float eps, float momentum,
                                  const float* mask, const void* r1, const void* r2, float r2_scale, void* y, void* y2,
                                  int N, int C, int HW, void* stream);
int ppea_bn_bwd_channel_next_f32(const void* dy2, const void* dskip, const void* z, const void* y, const float* const* stats,
                                 const float* mask, float inv_count, void* dz, void* dy, float* sums, int N, int C, int HW,
                                 void* stream);
int ppea_bn_bwd_channel_next_bf16(const void* dy2, const void* dskip, const void* z, const void* y, const float* const* stats,
                                  const float* mask, float inv_count, void* dz, void* dy, float* sums, int N, int C, int HW,
                                  void* stream);
int ppea_bn_apply_f32(const void* z1, const void* z2, const float* const* stats, const float* mask,
                      const void* r1, const void* r2, float r2_scale, void* y, int act,
                      int N, int C, int HW, void* stream);
int ppea_bn_apply_bf16(const void* z1, const void* z2, const float* const* stats, const float* mask,
                       const void* r1, const void* r2, float r2_scale, void* y, int act,
                       int N, int C, int HW, void* stream);
int ppea_bn_bwd_reduce_f32(const void* dy, const void* z1, const void* z2, const float* const* stats,
                           const float* mask, float* partial, int act, int N, int C, int HW, void* stream);
int ppea_bn_bwd_reduce_bf16(const void* dy, const void* z1, const void* z2, const float* const* stats,
                            const float* mask, float* partial, int act, int N, int C, int HW, void* stream);
int ppea_bn_bwd_finalize_f32(const float* partial, int N, int C, float* sums, void* stream);
int ppea_bn_bwd_apply_f32(const void* dy, const void* z1, const void* z2, const float* const* stats,
                          const float* mask, const float* sums, float inv_count, void* dz1, void* dz2,
                          int act, int N, int C, int HW, void* stream);
int ppea_bn_bwd_apply_bf16(const void* dy, const void* z1, const void* z2, const float* const* stats,
                           const float* mask, const float* sums, float inv_count, void* dz1, void* dz2,
                           int act, int N, int C, int HW, void* stream);
/* ------------------------------------------------------------------------------------------
 * A2 across ranks  SyncBatchNorm on the fused kernels (csrc/bn_sync.hip).  Both encoders are nn.SyncBatchNorm in the
 *   reference (replknet_adapter.py:170-180; DDP step trainer.py:215-222): statistics of the GLOBAL batch.  One BatchNorm
 *   (+ act + DropPath + residual + adapter add) = TWO launches around ONE collective issued by the host:
 *     ppea_bn_sync_stats_* (or ppea_bn_sync_stats_from_sums_f32 after a GEMM that left partial sums)
 *         -> packed = mean1[C] | biased var1[C] [| mean2[C] | var2[C]] | count        (pitch 2C+1, or 4C+1 with z2)
 *     all-gather -> gathered [world][pitch]
 *     ppea_bn_sync_apply_*: Chan combine of the gathered rows inside the apply kernel (no combine launch), running
 *         statistics (momentum, unbiased variance of the global batch), out[4..7] = saved mean / invstd, y as
 *         ppea_bn_fwd_channel_*; packed_next (or NULL; needs N * HW <= 16384, C >= 64): the LOCAL statistics of the stored
 *         y in wire format (pitch 2C+1) -- the next BatchNorm over y (replknet_adapter.py:281, 312) then needs no
 *         statistics launch.  HW % 8 == 0, else PPEA_ERR_UNSUPPORTED (ppea_bn_sync_combine_f32 + ppea_bn_apply_*).
 *   prm / out as ppea_bn_fwd_channel_*.  ws: ppea_bn_sync_stats_workspace_bytes(N, C, HW, z2 != NULL) bytes (0 when one
 *   workgroup covers a channel).  Backward: ppea_bn_bwd_reduce(_final)_* -> all-reduce (sum) of sums [3][C] ->
 *   ppea_bn_sync_bwd_apply_* with inv_count = 1 / (global count); acc (shape of z1, or NULL): dz1 = round(dz1) + acc, the
 *   gradient reaching z1 through its other consumer (the block's residual connection, rka.py:289, 326); dgb [3][C] (or
 *   NULL) = sums * gscale: d beta | d gamma1 | d gamma2 with gscale = 1 / world -- the reference's DDP averages the
 *   per-rank LOCAL sums torch's SyncBatchNorm returns (trainer.py:215-222), which is (global sum) / world.
 * ---------------------------------------------------------------------------------------- */
long ppea_bn_sync_stats_workspace_bytes(int N, int C, int HW, int two);
int ppea_bn_sync_stats_f32(const void* z1, const void* z2, float* packed, float* ws, int N, int C, int HW, void* stream);
int ppea_bn_sync_stats_bf16(const void* z1, const void* z2, float* packed, float* ws, int N, int C, int HW, void* stream);
int ppea_bn_sync_stats_from_sums_f32(const float* sums, int P, int C, long count, float* packed, void* stream);
int ppea_bn_sync_apply_f32(const void* z1, const void* z2, const float* gathered, int world, const float* const* prm,
                           float* const* out, float eps, float momentum, const float* mask, const void* r1, const void* r2,
                           float r2_scale, void* y, float* packed_next, int act, int N, int C, int HW, void* stream);
int ppea_bn_sync_apply_bf16(const void* z1, const void* z2, const float* gathered, int world, const float* const* prm,
                            float* const* out, float eps, float momentum, const float* mask, const void* r1, const void* r2,
                            float r2_scale, void* y, float* packed_next, int act, int N, int C, int HW, void* stream);
int ppea_bn_sync_bwd_apply_f32(const void* dy, const void* z1, const void* z2, const float* const* stats,
                               const float* mask, const float* sums, float inv_count, const void* acc, void* dz1, void* dz2,
                               float* dgb, float gscale, int act, int N, int C, int HW, void* stream);
int ppea_bn_sync_bwd_apply_bf16(const void* dy, const void* z1, const void* z2, const float* const* stats,
                                const float* mask, const float* sums, float inv_count, const void* acc, void* dz1, void* dz2,
                                float* dgb, float gscale, int act, int N, int C, int HW, void* stream);

/* ------------------------------------------------------------------------------------------
 * A12 glue  nn.ReflectionPad2d(1) of the decoder's Conv3x3 (layers.py:119-135).  in [planes,H,W] ->
 *     out [planes,H+2,W+2]; backward is a gather (no atomics): din [planes,H,W] from dout.  H, W >= 3.
 * ---------------------------------------------------------------------------------------- */
int ppea_reflect_pad1_fwd_f32(const void* in, void* out, long planes, int H, int W, void* stream);
int ppea_reflect_pad1_fwd_bf16(const void* in, void* out, long planes, int H, int W, void* stream);
int ppea_reflect_pad1_bwd_f32(const void* dout, void* din, long planes, int H, int W, void* stream);
int ppea_reflect_pad1_bwd_bf16(const void* dout, void* din, long planes, int H, int W, void* stream);

/* ------------------------------------------------------------------------------------------
 * A18+A19  BackprojectDepth -> Project3D fused (layers.py:138-199; trainer.py:904-907).
 *     depth [B,1,H,W]; inv_K [B,4,4] (only [:3,:3] read); P [B,3,4] = (K @ T)[:, :3, :];
 *     grid [B,H,W,2] normalised to [-1,1] (x then y); eps added to z (1e-7).
 *     bwd: d_depth [B,1,H,W] and dP [B,3,4] overwritten; dP is summed from per-block partials in a caller-owned
 *     workspace of ppea_backproject_project_bwd_workspace_bytes(B, H, W) bytes in a FIXED order (no float atomics:
 *     the pose gradient is bitwise reproducible).  B is the grid's y extent and a pixel index an int: B > 65535 or
 *     H * W > 0x7fffff00 is PPEA_ERR_UNSUPPORTED, here and for the split entry points below.
 * ---------------------------------------------------------------------------------------- */
int ppea_backproject_project_fwd_f32(const float* depth, const float* inv_K, const float* P,
                                     float* grid, int B, int H, int W, float eps, void* stream);
long ppea_backproject_project_bwd_workspace_bytes(int B, int H, int W);
int ppea_backproject_project_bwd_f32(const float* depth, const float* inv_K, const float* P,
                                     const float* d_grid, float* d_depth, float* dP, void* workspace,
                                     int B, int H, int W, float eps, void* stream);

/* ------------------------------------------------------------------------------------------
 * A18, A19 as separate launches (layers.py:138-168 BackprojectDepth, 171-199 Project3D), for callers that keep the
 * reference's two modules or need the point cloud / the projected depth.  All fp32, one thread per pixel, no atomics.
 *   backproject: points [B,4,HW]: rows 0-2 = depth * (inv_K[:3,:3] @ (x, y, 1)), row 3 = 1; x, y from the thread index.
 *     bwd: d_depth [B,1,H,W] overwritten; d_inv_K [B,4,4] (NULL: not wanted, workspace unused) gets the 9 sums
 *     d_points[i] * depth * (x, y, 1)[j] in its upper-left 3x3 and zeros elsewhere.  Either may be NULL, not both.
 *   project3d: P is the whole [B,4,4] product K @ T, of which rows 0-2 are read in place (the reference's `[:, :3, :]`
 *     without a copy); cam = P[:3] @ points over all four rows (row 3 need not be 1); grid [B,H,W,2] as the fused kernel
 *     writes it; z [B,1,H,W] = cam[2] (NULL: not wanted).  bwd: d_z NULL = no gradient into z; d_points [B,4,HW] and
 *     dP [B,4,4] (12 sums, row 3 zeros) are overwritten, either may be NULL (not wanted), not both.
 *   Both backward passes sum per-block partials from a caller-owned workspace of *_bwd_workspace_bytes(B, H, W) bytes in a
 *   fixed order.  Where row 3 of `points` is 1, project3d(backproject(.)) and its gradients carry the fused kernels' bits.
 *   Note that `P` / `dP` here are [B,4,4], unlike the [B,3,4] `P` / `dP` of ppea_backproject_project_* above.
 * ---------------------------------------------------------------------------------------- */
int ppea_backproject_fwd_f32(const float* depth, const float* inv_K, float* points, int B, int H, int W, void* stream);
long ppea_backproject_bwd_workspace_bytes(int B, int H, int W);
int ppea_backproject_bwd_f32(const float* depth, const float* inv_K, const float* d_points, float* d_depth, float* d_inv_K,
                             void* workspace, int B, int H, int W, void* stream);
int ppea_project3d_fwd_f32(const float* points, const float* P, float* grid, float* z, int B, int H, int W, float eps,
                           void* stream);
long ppea_project3d_bwd_workspace_bytes(int B, int H, int W);
int ppea_project3d_bwd_f32(const float* points, const float* P, const float* d_grid, const float* d_z, float* d_points,
                           float* dP, void* workspace, int B, int H, int W, float eps, void* stream);

/* ------------------------------------------------------------------------------------------
 * A20  F.grid_sample(bilinear, align_corners=True)  (trainer.py:911-914 border;
 *      replk_matching_adapter.py:299 zeros).  src [B,C,Hi,Wi]; grid [B,Ho,Wo,2];
 *      out [B,C,Ho,Wo].  padding: 0 = zeros, 1 = border.
 *      bwd_grid: gradient w.r.t. the grid only (the source is data).
 * ---------------------------------------------------------------------------------------- */
int ppea_grid_sample_fwd_f32(const float* src, const float* grid, float* out,
                             int B, int C, int Hi, int Wi, int Ho, int Wo, int padding,
                             void* stream);
int ppea_grid_sample_bwd_grid_f32(const float* src, const float* grid, const float* d_out,
                                  float* d_grid, int B, int C, int Hi, int Wi, int Ho, int Wo,
                                  int padding, void* stream);

/* A15: axis-angle + translation -> 4x4 transformation (layers.py:26-42 `transformation_from_parameters`, 61-100
 * `rot_from_axisangle`): aa, tr [B][3] fp32 -> T [B][4][4]; invert != 0: R^T T(-t).  Backward: d aa, d tr from dT. */
int ppea_pose_matrix_fwd_f32(const float* aa, const float* tr, float* T, int B, int invert, void* stream);
int ppea_pose_matrix_bwd_f32(const float* aa, const float* tr, const float* dT, float* daa, float* dtr, int B, int invert,
                             void* stream);

/* A14/A15: the relative poses of the F <= 4 lookup frames from P <= 4 pose-network outputs in one launch
 * (repdepth.py:465-507), forward only (the reference computes them under no_grad).  aa, tr: HOST arrays of P device pointers;
 * sample b of output p is the three floats at aa[p] + b * stride (stride >= 3, in floats).  pair, invert, pred: HOST arrays
 * of F ints: frame f uses output pair[f], builds its matrix as ppea_pose_matrix_fwd_f32 does (invert[f]) and multiplies it
 * from the left onto the relative pose of frame pred[f] < f (-1: no predecessor), each element summed over k = 0, 1, 2, 3 in
 * that order.  keep [B][F] fp32 or NULL (keep all): 0 writes exact zeros for that (item, frame), and its successors in the chain multiply
 * with those zeros.  T [B][F][4][4]. */
int ppea_pose_chain_fwd_f32(const float* const* aa, const float* const* tr, int P, int stride, const int* pair,
                            const int* invert, const int* pred, const float* keep, float* T, int B, int F, void* stream);

/* The same chain on a video stream: ring [F][B][2][3] fp32 holds the pose decoder's raw (axisangle, translation) of the pairs
 * of consecutive frames, pair (t-j-1, t-j) at slot (head - j) mod F with head = state[0] (state [1 + B] int32 on the device,
 * as for ppea_cost_volume_ring_fwd_*).  aa_new / tr_new (sample b at + b * stride floats; both NULL: none) is the newest
 * pair and is stored into slot head first.  T(0 -> -1) = inv(pair 0), T(0 -> -(j+1)) = inv(pair j) @ T(0 -> -j), the
 * arithmetic of ppea_pose_chain_fwd_f32; exact zeros and present[b][j] = 0 where state[1 + b] <= j.  T [B][F][4][4],
 * present [B][F] bytes. */
int ppea_pose_chain_ring_fwd_f32(const float* aa_new, const float* tr_new, int stride, float* ring, const int32_t* state,
                                 float* T, uint8_t* present, int B, int F, void* stream);

/* ------------------------------------------------------------------------------------------
 * A21+A22 compute_reprojection_loss (trainer.py:995-1007; SSIM layers.py:226-257):
 *      out[b,0,i,j] = alpha * mean_c SSIM(pred,target) + (1-alpha) * mean_c |target-pred|.
 *      pred/target [B,C,H,W] (H,W >= 2); out has batch stride `out_bstride` elements so the
 *      result can be written straight into one channel of a [B,2,H,W] buffer.
 *      bwd: gradient w.r.t. pred (d_out has batch stride dout_bstride).
 * ---------------------------------------------------------------------------------------- */
int ppea_ssim_l1_fwd_f32(const float* pred, const float* target, float* out, long out_bstride,
                         int B, int C, int H, int W, float alpha, void* stream);
int ppea_ssim_l1_bwd_f32(const float* pred, const float* target, const float* d_out,
                         long dout_bstride, float* d_pred, int B, int C, int H, int W,
                         float alpha, void* stream);

/* ------------------------------------------------------------------------------------------
 * A23  get_smooth_loss (layers.py:210-223).  disp [B,1,H,W], img [B,C,H,W].
 *      partials [ppea_smooth_num_partials()][2]: per-workgroup partial sums (deterministic, no
 *      atomics); column 0 = sum |dx disp| e^{-mean_c|dx img|}, column 1 = same for dy.  The caller
 *      adds the rows and divides by the element counts B*H*(W-1) and B*(H-1)*W.
 *      bwd: d_disp = gx * d(sum_x)/d(disp) + gy * d(sum_y)/d(disp) with scalar weights.
 * ---------------------------------------------------------------------------------------- */
int ppea_smooth_num_partials(void);
int ppea_smooth_fwd_f32(const float* disp, const float* img, float* partials,
                        int B, int C, int H, int W, void* stream);
int ppea_smooth_bwd_f32(const float* disp, const float* img, float gx, float gy, float* d_disp,
                        int B, int C, int H, int W, void* stream);

/* ------------------------------------------------------------------------------------------
 * A24/A25  per-pixel loss selection (trainer.py:1069-1114): min over the S source frames, S in {1, 2},
 *      selec_reproj overwrite, identity min + tie-break noise, automask argmin.
 *      reproj, identity [B,S,H,W]; warped_0 / warped_1 [B,C,H,W], read for selec_reproj only and NULL
 *      otherwise; noise [B,1,H,W] (already * 1e-5) or NULL.  Outputs: sel [B,1,H,W] selected
 *      reprojection loss; src_idx uint8 [B,1,H,W] (0/1 = which of reproj's channels feeds `sel`,
 *      2 = forced zero); frame_idx int64 [B,1,H,W] (argmin over the frames, first minimum);
 *      auto_idx int64 [B,1,H,W] (argmin over [sel, identity_min+noise], first minimum).
 *      S = 1 (frame_ids [0, -1], the two-frame items of DDAD): sel is the only channel, src_idx = 0 and
 *      frame_idx = 0 everywhere, the identity minimum is the only identity channel (+ noise), auto_idx by
 *      the same first-minimum / NaN rule; no warped frame is read, and selec_reproj != 0 is
 *      PPEA_ERR_UNSUPPORTED (the reference reads the warped frame +1 there, trainer.py:1077-1083).
 * ---------------------------------------------------------------------------------------- */
int ppea_loss_select_f32(const float* reproj, const float* identity, const float* warped_0,
                         const float* warped_1, const float* noise, float* sel,
                         uint8_t* src_idx, int64_t* frame_idx, int64_t* auto_idx,
                         int B, int S, int C, int H, int W, int selec_reproj, void* stream);

/* Tail of compute_losses (trainer.py:1092-1139) after the per-pixel selection: mask (automask argmin == 0, or for the
 * multi-frame pass consistency_mask * (1 - augmentation_mask)), rl = sum(sel * mask) / (sum(mask) + 1e-7), and for the
 * multi-frame pass the consistency loss mean(|multi - mono| * (1 - mask)) and its target.  One pass + finalize forward, one
 * pass backward (d reproj [B][S][H][W], S in {1, 2}, routed by the selection's source index, d multi_depth; the forward
 * does not see the frames: it reads the selected loss); fixed summation order.
 *   sel, mask, target, multi, mono [B][1][H][W] fp32; auto_idx int64 or NULL; cons [B][H][W] or NULL; aug [B] or NULL;
 *   partial: ppea_loss_tail_blocks(B*H*W) * 3 floats; out[0] = rl, out[1] = consistency loss, out[2] = 1/(sum(mask)+1e-7);
 *   g_rl / g_con: device scalars (gradients of out[0] / out[1]) or NULL. */
int ppea_loss_tail_blocks(long total);
int ppea_loss_tail_fwd_f32(const float* sel, const int64_t* auto_idx, const float* cons, const float* aug, const float* multi,
                           const float* mono, float* mask, float* target, float* partial, float* out, int B, int H, int W,
                           int is_multi, void* stream);
int ppea_loss_tail_bwd_f32(const float* mask, const uint8_t* src, const float* out, const float* g_rl, const float* g_con,
                           const float* multi, const float* mono, float* d_reproj, float* d_multi, int B, int S, int H,
                           int W, void* stream);

/* ------------------------------------------------------------------------------------------
 * A12 / A14  Dense convolutions as implicit GEMMs on the matrix cores (csrc/conv_nhwc.hip, conv_wgrad.hip):
 *     bf16 channels-last activations, fp32 accumulation.  Replaces the library convolutions behind
 *       ConvBlock / Conv3x3            layers.py:103-135 (decoder: networks/depth_decoder_v2.py:172-245)
 *       ResNet-18 pose trunk          networks/resnet_encoder.py:25-72, 397-409
 *       PoseDecoder                   networks/pose_decoder.py:33-52
 *       reduce_conv                   networks/replk_matching_adapter.py:127-131
 *       RepLKNet stem[0]              networks/replknet_adapter.py:411
 *     forward and data gradient (one kernel: the data gradient runs it with the flipped / transposed operand image
 *     and, for a strided forward, over the zero-dilated output gradient) and weight gradient.
 *
 *   ppea_conv_packed_bytes(Cout, Cin, R, S, flip)   bytes of the operand image of w [Cout][Cin][R][S]
 *   ppea_conv_pack_weights(w, w_is_bf16, packed, Cout, Cin, R, S, flip)
 *        flip = 0: [R*S][Cout][Cin padded to 32] (forward); flip = 1: [R*S reversed][Cin][Cout padded to 32] (dgrad)
 *   ppea_conv_nhwc_bf16   y = act(bias + conv(x)):  x [N][H][W][Cin] (Cin % 8 == 0), y [N][Ho][Wo][Cout] or, with
 *        out_nchw, [N][Cout][Ho][Wo]; R, S <= 7; stride 1 | 2; pad = zero padding, or reflect != 0: reflection
 *        padding of `pad` <= 1 read through reflected indices (no padded copy); dil > 1: x is read as its zero-dilated
 *        image (data gradient of a strided conv); bias fp32 or (bias_bf16) bf16 or NULL; act 0 none, 1 ReLU, 2 ELU,
 *        3 sigmoid.
 *   ppea_conv_wgrad_nhwc_bf16   dw [Cout][Cin][R][S] (fp32 or bf16) = sum_pixels dz (x) x, split over output patches
 *        with fp32 partials in a caller-owned workspace of ppea_conv_wgrad_workspace_bytes(...) bytes
 *        (deterministic; Cin % 8 == 0, Cout % 8 == 0).
 *   ppea_image_to_nhwc_bf16   fp32 NCHW frames -> bf16 channels-last, channels zero-padded to Cp (% 8 == 0),
 *        y = (x - sub) / div  (resnet_encoder.py:399 normalisation for the pose trunk; sub 0, div 1 for stem[0]).
 *   ppea_conv_nhwc_plan / ppea_conv_wgrad_plan   host only, no device call, no stream: the kernel the two entry points
 *        above launch for these shape arguments, decided by the function they launch by.
 *        ppea_conv_nhwc_plan   plan[0..4] = NTC (conv3x3_resident_kernel<NTC, 1>; 0: the per-tile kernel), BN, RPS
 *        (conv_nhwc_kernel<BN, ., ., stride, out_nchw, R, RPS>; 0 with NTC > 0), TR, TC (pixel tile).
 *        ppea_conv_wgrad_plan  plan[0..11] = BM, BN, WK, splits, slabs, rows_per_block, rgroups, TR, TC, n_patches
 *        (conv_wgrad_kernel<stride, R, BM, BN>), split_rule (what set `splits`: 0 two waves of workgroups, 1 the
 *        workspace cap, 2 the floor min(two waves, 4) that a lower cap is raised to, 3 one workgroup per CU, 4 one patch per workgroup), tree_reduce (1: the
 *        slab sum runs on the parallel reducer, 0: on the flat one).
 * ---------------------------------------------------------------------------------------- */
long ppea_conv_packed_bytes(int Cout, int Cin, int R, int S, int flip);
int ppea_conv_pack_weights(const void* w, int w_is_bf16, void* packed, int Cout, int Cin, int R, int S, int flip,
                           void* stream);
int ppea_conv_nhwc_bf16(const void* x, const void* w_packed, const void* bias, int bias_bf16, void* y,
                        int N, int H, int W, int Cin, int Cout, int R, int S, int stride, int pad, int reflect, int dil,
                        int Ho, int Wo, int act, int out_nchw, void* stream);
long ppea_conv_wgrad_workspace_bytes(int N, int Cin, int Cout, int R, int S, int stride, int Ho, int Wo);
int ppea_conv_wgrad_nhwc_bf16(const void* dz, const void* x, void* dw, int dw_bf16, void* workspace,
                              int N, int H, int W, int Cin, int Cout, int R, int S, int stride, int pad, int reflect,
                              int Ho, int Wo, void* stream);
int ppea_image_to_nhwc_bf16(const float* x, void* y, int N, int C, int H, int W, int Cp, float sub, float div,
                            void* stream);
int ppea_conv_nhwc_plan(int N, int H, int W, int Cin, int Cout, int R, int S, int stride, int pad, int reflect, int dil,
                        int Ho, int Wo, int out_nchw, int* plan);
int ppea_conv_wgrad_plan(int N, int Cin, int Cout, int R, int S, int stride, int Ho, int Wo, int* plan);

/* Plans of the large-kernel depthwise kernels (ABI 22).  Host only, no device call, no stream; each is answered by the
 * function the launch itself goes by.
 *   ppea_dwconv_lk_plan   what ppea_dwconv_lk_fwd_bf16p (mode 0, variant 0), _fwd_stats_bf16p (0, 1), _fwd_bn_bf16p (0, 2),
 *        _fwd_bias_act_bf16p (0, 3; KS = 0) and _bwd_data_bf16p (mode 1, variant 0) launch for [N,C,H,W], K, KS.  plan[24]:
 *          [0] family   0 no MFMA kernel serves the shape (the entry point returns PPEA_ERR_UNSUPPORTED; the rest is 0),
 *                       1 row-band dwconv_mfma_kernel<K, KS, mode, NSEG, BN, WS, BA>,
 *                       2 batch-major dwconv_bm_kernel<K, KS, mode, H, NY, NTX, RS, BN>
 *          [1] partials statistics partials per channel (forward; = ppea_dwconv_lk_stats_partials; 0 for mode 1 and BA)
 *          [2] lds_bytes  dynamic LDS of the launch
 *          row-band:    [3] NSEG  [4] WS  [5] BN  [6] BA  [7] band  [8] G (planes stacked per item)  [9] bands per plane
 *                       [10] segs (column segments)  [11] items_per_channel  [12] wpc (waves per channel)
 *                       [13] ipw (items per wave)  [14] fast (1: prefetched staging)
 *          batch-major: [5] BN  [15] H  [16] NY  [17] NTX  [18] RS  [19] VEC (8: W % 8 == 0, else 4)  [20] gi (images per
 *                       group)  [21] ngroups  [22] wgpc (workgroups per channel block)  [23] cpw (column tiles per workgroup)
 *        Returns 0 (also with family 0), PPEA_ERR_ARG for plan == NULL or a mode / variant outside the lists.
 *   ppea_dwconv_lk_bwd_filter_plan   plan[0..5] = parts, rows_per_part, rounds (of a full part: ceil(rows_per_part / 4)),
 *        vec (1: W % 8 == 0, 16-byte dy loads), dynamic LDS bytes, rows of the last part, of ppea_dwconv_lk_bwd_filter_bf16;
 *        PPEA_ERR_UNSUPPORTED where that call returns it.
 *   ppea_dwconv_lk_f32_plan   plan[0] = index into CFGS_<K> (csrc/dwconv_lk.hip) of the tile the fp32 vector kernel
 *        (ppea_dwconv_lk_{fwd,bwd_data}_{f32,bf16}, KS in {0, 5}) picks for an H x W plane; -1: the generic kernel. */
int ppea_dwconv_lk_plan(int N, int C, int H, int W, int K, int KS, int mode, int variant, int* plan);
/* Test support, host only: ppea_dwconv_lk_plan over N 1..Nmax x C in Cs[nC] x H 1..Hmax x W 1..Wmax, folded into
 * seen[1 << 14] (one byte per packed plan key; the packing is documented at the definition in csrc/dwconv_mfma.hip) and
 * summary[4] = shapes served, largest lds_bytes, plans whose ipw / wpc do not cover the items exactly, shapes not served. */
int ppea_dwconv_lk_plan_sweep(int K, int KS, int mode, int variant, int Nmax, const int* Cs, int nC, int Hmax, int Wmax,
                              unsigned char* seen, long* summary);
int ppea_dwconv_lk_bwd_filter_plan(int N, int C, int H, int W, int K, int KS, int* plan);
int ppea_dwconv_lk_f32_plan(int H, int W, int K, int* plan);

/* fp32 dense convolutions / linear layers on the fp32 matrix cores (csrc/conv_f32.hip, v_mfma_f32_32x32x2_f32): the
 * fp32 (parity, BASELINE config 1) step's replacement for every library convolution and GEMM behind
 *   RepLKBlock / ConvFFN 1x1 convs, B_Adapter / Adapter     networks/replknet_adapter.py:20-109, 264-326
 *   ConvBlock / Conv3x3 / ConvTranspose2d (Stage 2)          layers.py:103-135, networks/depth_decoder_v2.py:172-245
 *   ResNet-18 pose trunk, PoseDecoder                        networks/resnet_encoder.py:367-409, networks/pose_decoder.py:27-52
 *   reduce_conv, RepLKNet stem[0]                            networks/replk_matching_adapter.py:127-131, replknet_adapter.py:411
 * One implicit-GEMM family for every kernel size, stride, zero padding and memory format: x / y / dy / dx are addressed
 * through four ELEMENT strides (n, c, h, w) -- NCHW, channels_last, or a [tokens][features] matrix viewed as
 * [1][features][tokens][1] (nn.Linear).  w / dw: [Cout][Cin][R][S] contiguous.  Ho = (H + 2 pad - R) / stride + 1.
 *   ppea_conv2d_f32_fwd     y = bias + conv(x)  (bias [Cout] or NULL)
 *   ppea_conv2d_f32_dgrad   dx (every element written) from dy
 *   ppea_conv2d_f32_wgrad   dw = sum over pixels, split over the grid with fp32 slabs in a caller-owned workspace of
 *                           ppea_conv2d_f32_wgrad_workspace_bytes(...) bytes summed in a fixed order (no atomics)
 * ---------------------------------------------------------------------------------------- */
int ppea_conv2d_f32_fwd(const float* x, const long* xs, const float* w, const float* bias, float* y, const long* ys, int N,
                        int Cin, int H, int W, int Cout, int R, int S, int stride, int pad, void* stream);
int ppea_conv2d_f32_dgrad(const float* dy, const long* dys, const float* w, float* dx, const long* dxs, int N, int Cin, int H,
                          int W, int Cout, int R, int S, int stride, int pad, int Ho, int Wo, void* stream);
long ppea_conv2d_f32_wgrad_workspace_bytes(int N, int Cin, int Cout, int R, int S, int Ho, int Wo);
int ppea_conv2d_f32_wgrad(const float* x, const long* xs, const float* dy, const long* dys, float* dw, float* workspace, int N,
                          int Cin, int H, int W, int Cout, int R, int S, int stride, int pad, int Ho, int Wo, void* stream);
/* The same family for bf16 weights / activations / results (widened as they are staged, fp32 products and sums on the same
 * instruction, one rounding at the store; bias and dw stay fp32): what the bf16 step uses for shapes the layout-specialised
 * bf16 kernels do not take (map widths that are not a multiple of 4 pixels, channel counts that are not multiples of
 * 8 / 32: reduced-size test configurations), so that no shape of either dtype reaches a library convolution or GEMM. */
int ppea_conv2d_bf16_fwd(const void* x, const long* xs, const void* w, const float* bias, void* y, const long* ys, int N,
                         int Cin, int H, int W, int Cout, int R, int S, int stride, int pad, void* stream);
int ppea_conv2d_bf16_dgrad(const void* dy, const long* dys, const void* w, void* dx, const long* dxs, int N, int Cin, int H,
                           int W, int Cout, int R, int S, int stride, int pad, int Ho, int Wo, void* stream);
int ppea_conv2d_bf16_wgrad(const void* x, const long* xs, const void* dy, const long* dys, float* dw, float* workspace, int N,
                           int Cin, int H, int W, int Cout, int R, int S, int stride, int pad, int Ho, int Wo, void* stream);

/* MaxPool2d(3, 2, 1) of the pose ResNet-18 (networks/resnet_encoder.py:376-392) on channels-last tensors
 * (csrc/nhwc_pool.hip): forward keeps a one-byte window index (3 r + s, torch's tie rule: first maximum in scan order), the
 * backward gathers (no atomics).  x [N][H][W][C], C % 8 == 0; y, idx [N][Ho][Wo][C] with Ho = (H - 1) / 2 + 1. */
int ppea_nhwc_maxpool3x3s2_fwd_f32(const void* x, void* y, void* idx, int N, int H, int W, int C, void* stream);
int ppea_nhwc_maxpool3x3s2_fwd_bf16(const void* x, void* y, void* idx, int N, int H, int W, int C, void* stream);
int ppea_nhwc_maxpool3x3s2_bwd_f32(const void* dy, const void* idx, void* dx, int N, int H, int W, int C, void* stream);
int ppea_nhwc_maxpool3x3s2_bwd_bf16(const void* dy, const void* idx, void* dx, int N, int H, int W, int C, void* stream);

/* Image-fed convolutions (csrc/conv_image.hip): RepLKNet stem[0] (networks/replknet_adapter.py:411, 3x3 stride 2) and
 * the pose ResNet-18 conv1 (networks/resnet_encoder.py:376-388, 7x7 stride 2).  The frame is channels-last bf16 with its
 * 3 / 6 channels zero-padded to 8 (ppea_image_to_nhwc_bf16); one MFMA contraction covers a whole filter ROW (S taps x 8
 * channels are contiguous in memory), weights packed [K][Cout][K*8 padded to 32].  Forward and weight gradient
 * (dw [Cout][Cin][K][K], Cin <= 8 real channels); no data gradient (the input is the frame). */
long ppea_conv_image_packed_bytes(int Cout, int K);
int ppea_conv_image_pack_weights(const void* w, int w_is_bf16, void* packed, int Cout, int Cin, int K, void* stream);
int ppea_conv_image_bf16(const void* x, const void* w_packed, void* y, int N, int H, int W, int Cout, int K, int stride,
                         int pad, int Ho, int Wo, int out_nchw, void* stream);
long ppea_conv_image_wgrad_workspace_bytes(int N, int Cout, int K, int Ho, int Wo);
int ppea_conv_image_wgrad_bf16(const void* dz, const void* x, void* dw, int dw_bf16, void* workspace, int N, int H, int W,
                               int Cin, int Cout, int K, int stride, int pad, int Ho, int Wo, void* stream);

/* ------------------------------------------------------------------------------------------
 * A9  match_features (replk_matching_adapter.py:261-340, the loop over the lookups :289-326): F = 1 .. 4 lookup frames per
 *      item in ONE launch (larger F: PPEA_ERR_UNSUPPORTED).  F = 1 is the former single-frame form: the entry points
 *      ppea_cost_volume_fwd_{f32,bf16} of ABI <= 15 are these with F = 1 and a required `skip`, same bits.
 *      cur [B,C,h,w]; lookup [B,F,C,h,w]; P [B,F,3,4] = (K @ T_f)[:, :3, :] at the matching scale; inv_K [B,4,4]; bins [D];
 *      skip [B,F] int32, required (non-zero = that frame's pose was zeroed: the frame adds nothing; every frame of an item
 *      skipped -> cost 0).  Per (item, bin, pixel): diff_f = mean_c|warp_f(lookup_f) - cur| for every frame that is not
 *      skipped and whose sample lies inside the edge mask;
 *      cost [B,D,h,w] = (((0 + diff_0) + diff_1) + ...) / (#{f: diff_f > 0} + 1e-7) in fp32, frames in order.
 *      bf16 features (the bf16 step): the kernel is bound by the bytes crossing the L1, so the (1 + F) maps are packed into
 *      channel-PAIR dwords first (`pairs`: caller-owned workspace of (1 + F) * B * C/2 * h * w uint32) and a corner load
 *      serves two channels.  Bit-identical to the fp32 form on the features widened to fp32.  C even.
 *      Refused before anything is launched or read: F outside 1 .. 4, C <= 0 (bf16: odd C), h or w < 5, D outside
 *      1 .. 65535, B > 65535 (B is a grid dimension) -> PPEA_ERR_UNSUPPORTED; then B == 0 -> 0; then a NULL cur / lookup /
 *      pairs / P / inv_K / bins / skip / cost -> PPEA_ERR_ARG (as the ring entries below, where only `skip` may be NULL).
 * A10 cost_volume_reduce (:446-456, :372-387): missing -> per-pixel max; confidence mask;
 *      argmin over bins after 0 -> 100 (int64, first minimum); lowest = 1/bins[argmin];
 *      cost_out = filled cost * confidence.  B > 65535 (a grid dimension): PPEA_ERR_UNSUPPORTED.
 * ---------------------------------------------------------------------------------------- */
int ppea_cost_volume_multi_fwd_f32(const float* cur, const float* lookup, const float* P, const float* inv_K,
                                   const float* bins, const int32_t* skip, float* cost, int B, int F, int C, int h, int w,
                                   int D, float eps, void* stream);
int ppea_cost_volume_multi_fwd_bf16(const void* cur, const void* lookup, void* pairs, const float* P, const float* inv_K,
                                    const float* bins, const int32_t* skip, float* cost, int B, int F, int C, int h, int w,
                                    int D, float eps, void* stream);
/* Video streaming (DepthPredictor.stream): the lookups are the last F frames, kept in a device ring.
 *      state [1 + B] int32 on the device: state[0] = head slot (taken mod F), state[1 + b] = frames item b has seen since its
 *      reset, clamped at F.  No entry below reads it on the host.
 *      ppea_cost_volume_ring_fwd_*: ppea_cost_volume_multi_fwd_* with lookup frame f of item b at slot (head - 1 - f) mod F of
 *      ring [F,B,C,h,w]; the frame is skipped where seen[b] <= f or skip[b][f] != 0 (skip may be NULL).  Same kernel, same bits
 *      as the multi entry on the frames gathered in order.  bf16: `cur_pairs` [B,C/2,h,w] and `ring_pairs` [F,B,C/2,h,w] are
 *      channel-pair dwords already (ppea_cv_ring_store_bf16 writes both).
 *      ppea_cv_ring_store_*: src [B,C,h,w] -> slot head of dst [F,B,..] (bf16: packed to channel pairs, C even); state NULL:
 *      dst is a plain [B,..] buffer.
 *      ppea_cv_ring_advance: head <- (head + 1) mod F, seen[b] <- min(max(seen[b], 0) + 1, F) for any word (INT_MAX gives F);
 *      enqueue after the sweep and the store. */
int ppea_cost_volume_ring_fwd_f32(const float* cur, const float* ring, const int32_t* state, const float* P,
                                  const float* inv_K, const float* bins, const int32_t* skip, float* cost, int B, int F,
                                  int C, int h, int w, int D, float eps, void* stream);
int ppea_cost_volume_ring_fwd_bf16(const void* cur_pairs, const void* ring_pairs, const int32_t* state, const float* P,
                                   const float* inv_K, const float* bins, const int32_t* skip, float* cost, int B, int F,
                                   int C, int h, int w, int D, float eps, void* stream);
int ppea_cv_ring_store_f32(const float* src, float* dst, const int32_t* state, int B, int F, int C, int h, int w,
                           void* stream);
int ppea_cv_ring_store_bf16(const void* src, void* dst, const int32_t* state, int B, int F, int C, int h, int w,
                            void* stream);
int ppea_cv_ring_advance(int32_t* state, int B, int F, void* stream);
int ppea_cost_volume_reduce_f32(const float* cost, const float* bins, float* cost_out,
                                float* confidence, int64_t* argmin, float* lowest,
                                int B, int D, int h, int w, void* stream);

/* ------------------------------------------------------------------------------------------
 * Depth errors of one validation batch (trainer.py:780-843, evaluate_depth.py:35-54): resize the predicted disparity to the
 * ground-truth size, 1 / x, scale factor, crop + validity mask, median scaling, clamp to [1e-3, 80], the 7 errors.
 *   pred_disp [B,h,w] fp32 = disp_to_depth-scaled disparity; gt = flat fp32 buffer of gt_len values holding ragged
 *   ground-truth maps; table [B][3] int64 = (offset into gt, H_gt, W_gt) of each image of the batch;
 *   mode 0: range test only, 1: eigen (Garg/Eigen crop), 2: cityscapes (first round(0.75 H) rows, window [256:, 192:1856]);
 *   mode 3: Trainer.val_ddad (trainer.py:583-623): the DEPTH is resized (the reciprocals of the four source disparities are
 *   interpolated with the same weights), the range test is 1e-3 < gt < 200, the clamp [1e-3, 200], the whole map is scored;
 *   any other mode: PPEA_ERR_UNSUPPORTED;
 *   max_region >= the largest scored rectangle (rows x columns after the crop) of the batch: the workspace stride.  An image
 *   whose table row does not fit gt_len / max_region, or with no valid pixel, gives NaN errors and count 0;
 *   workspace: ppea_depth_errors_workspace_bytes(B, max_region) bytes, contents free before and after the call;
 *   errors [B][7] fp64 (abs_rel, sq_rel, rmse, rmse_log, a1, a2, a3), ratio [B] fp32 = median(gt) / median(pred) (applied
 *   only if median_scaling), count [B] int32 = valid pixels.  One memset + 7 launches for any B; bitwise reproducible.
 * ppea_depth_errors_mean_f64: mean [7] = mean over n rows of errors [n][7] (the split's result).
 * ---------------------------------------------------------------------------------------- */
long ppea_depth_errors_workspace_bytes(int B, long max_region);
int ppea_depth_errors_f32(const float* pred_disp, const float* gt, long gt_len, const int64_t* table, void* workspace,
                          double* errors, float* ratio, int32_t* count, int B, int h, int w, long max_region, int mode,
                          int median_scaling, float scale, void* stream);
int ppea_depth_errors_mean_f64(const double* errors, double* mean, int n, void* stream);

/* ------------------------------------------------------------------------------------------
 * Prediction export (ABI 29), csrc/depth_export.hip: a predicted plane at the frame's own size, as metric depth (fp32, or the
 * KITTI depth benchmark's uint16 of depth * 256, eval_depth_ori.py:325-328) or as a colour picture (vis.colorize).
 *   The resize is the one of ppea_depth_errors_f32: cv2.resize(INTER_LINEAR) -- half-pixel centres, no antialiasing, source
 *   coordinate s = max((o + 0.5) * n_in / n_out - 0.5, 0) (in fp64; the weight s - i0 is rounded once to fp32 and the
 *   interpolation is fp32), the horizontal pair first, then the vertical; a target of the source's size reads the pixel itself.  table [B][3] int64 (device) = (offset, H, W) of image b in the flat output, counted in pixels
 *   (DeviceGroundTruth's table; dense [B,H,W] output: offsets b * H * W); out_len = pixels the output holds: a row that does
 *   not fit it writes nothing; max_pixels >= the largest H * W of the batch (it sizes the grid: pixels of an image past it
 *   are not written).  One launch for any B <= 65535 and any mix of sizes, on `stream`, no synchronisation, no workspace.
 * ppea_disp_export_f32 / _u16: pred [B][h][w] fp32 scaled disparity, scale [B] fp32 (device), fp32 throughout:
 *   mode 0 (Trainer.val, the benchmark writer): r = resize(pred),     depth = clamp(scale[b] / r, lo, hi);
 *   mode 1 (Trainer.val_ddad):                  r = resize(1 / pred), depth = clamp(scale[b] * r, lo, hi);
 *   any other mode: PPEA_ERR_UNSUPPORTED.  A NaN stays a NaN (np.clip).  _f32 writes depth; _u16 writes (uint16)(depth *
 *   256.0f), the truncation of exactly the value _f32 writes, and refuses lo < 0 or hi * 256 > 65535 with PPEA_ERR_ARG.
 * ppea_plane_range_f32: x [B][n] fp32 -> range [B][2] fp32 = (minimum, q-th percentile) of each plane's values that are
 *   not NaN; percentile = 100: the maximum.  np.percentile's default (linear) rule: the two neighbouring order statistics
 *   are exact (radix select on the order-mapped bit pattern, 8 bits per pass, LDS histograms, integer atomics: two calls
 *   agree bit for bit), their interpolation is done in fp64 and rounded once.  A plane of NaNs only gives (NaN, NaN).  One
 *   workgroup per plane.  percentile outside [0, 100]: PPEA_ERR_ARG.
 * ppea_colorize_u8: x [B][h][w] fp32, range [B][2] fp32 (device) = (vmin, vmax), lut [256][3] uint8 (device, 4-byte
 *   aligned) -> out uint8 HWC, image b at byte 3 * offset_b (out 4-byte aligned, 3 * out_len bytes).  Per pixel, v the
 *   resized value: x = (v - vmin) / (vmax - vmin) in fp32, or v * 0 when vmin == vmax (vis.colorize); then matplotlib's
 *   Colormap.__call__(bytes=True) for N = 256: row floor(x * 256), x < 0 row 0, x >= 1 row 255, NaN the bytes (0, 0, 0).
 *   Bytes between the images are left as they were.
 * ---------------------------------------------------------------------------------------- */
int ppea_disp_export_f32(const float* pred, const float* scale, const int64_t* table, float* out, long out_len, int B, int h,
                         int w, long max_pixels, float lo, float hi, int mode, void* stream);
int ppea_disp_export_u16(const float* pred, const float* scale, const int64_t* table, uint16_t* out, long out_len, int B,
                         int h, int w, long max_pixels, float lo, float hi, int mode, void* stream);
int ppea_plane_range_f32(const float* x, float* range, int B, long n, double percentile, void* stream);
int ppea_colorize_u8(const float* x, const float* range, const uint8_t* lut, const int64_t* table, uint8_t* out,
                     long out_len, int B, int h, int w, long max_pixels, void* stream);

/* ------------------------------------------------------------------------------------------
 * Point clouds (ABI 32), csrc/point_cloud.hip: 3D points from a predicted plane and the pose chain of a stream.
 * ppea_point_cloud_f32: pred, scale, table (offset, H, W), max_pixels and mode are ppea_disp_export_f32's; d(u, v) of target
 *   pixel (u, v) is the value that entry point computes BEFORE its clamp (same device function, csrc/export_sample.h), so a
 *   kept pixel's d is bit-equal to what ppea_disp_export_f32 writes for it.  inv_K, cam_to_world: [B][4][4] fp32 (device);
 *   inv_K belongs to the TARGET size of image b and only its upper-left 3x3 is read; cam_to_world NULL = identity (the
 *   camera point is written as it is).
 *   Candidates: pixels with u % stride == 0 && v % stride == 0.  A candidate is kept iff d > lo && d < hi (a NaN fails;
 *   pixels on the clamp are dropped) and (edge <= 0, or every 4-neighbour n inside the image, at distance 1 in the target
 *   plane whatever the stride, has |d_n - d| <= edge * d in fp32; a NaN neighbour does not drop the pixel).
 *   Point, fp32 in this order, no contraction, (u, v) the integer pixel (layers.BackprojectDepth):
 *     ray = ((k00 u + k01 v) + k02, (k10 u + k11 v) + k12, (k20 u + k21 v) + k22),  c = ray * d,
 *     p_i = ((r_i0 c_0 + r_i1 c_1) + r_i2 c_2) + t_i.
 *   colour_mode 0: none (colour, colour_off, rgb may be NULL); 1: uint8 HWC frames at the target sizes, image b at byte
 *   colour_off[b] of `colour` (a RaggedFrames buffer, ppea_colorize_u8's output); 2: fp32 planar [B][3][H][W] in [0, 1],
 *   every target (H, W) (the caller checks that: the launcher does not read the device table), byte = (uint8)rintf(c * 255)
 *   clamped to 0..255.
 *   Output: kept points in image order, raster order of (v, u) inside an image: a function of the inputs alone, bit for
 *   bit.  Point k: xyz[k][3] fp32, rgb[k][3] uint8, index[k] int64 = offset_b + v * W + u.  cursor [2] int64 (device):
 *   cursor[0] at entry = points the buffers already hold; the call appends behind them and never writes at or beyond
 *   `capacity`; at exit cursor[0] = min(capacity, start + total) and cursor[1] has grown by the points that did not fit.
 *   counts [B] int64 = kept pixels of image b, fitted or not.  Nothing is read on the host.
 *   Three launches on `stream`: validity bits (one 64-bit __ballot word per wave) and counts per chunk of 2048 candidates
 *   into the workspace; ONE workgroup scans the chunk counts, writes counts and cursor; the scatter takes a kept pixel's
 *   rank from the stored bits.  No workgroup waits for another one; no atomics.  workspace: 8-byte aligned,
 *   ppea_point_cloud_workspace_bytes(B, max_pixels, stride) bytes (a negative value for arguments the call refuses).
 *   PPEA_ERR_ARG: stride < 1, capacity < 0, B <= 0 or B > 65535, colour_mode outside 0..2, a NULL required array (with
 *   capacity 0 the three output arrays may be NULL);
 *   PPEA_ERR_UNSUPPORTED: any other mode, max_pixels >= 2^31.  A refused call writes nothing.
 * ppea_pose_accumulate_f32: world [B][4][4] fp32 in place, pose [B][F][4][4] fp32, present [B][F] uint8: where
 *   present[b][0] != 0, world[b] = world[b] @ pose[b][0], element ij = ((w_i0 p_0j + w_i1 p_1j) + w_i2 p_2j) + w_i3 p_3j in
 *   fp32; elsewhere world[b] = identity.  pose[b][0] is the stream's "0 -> -1" transform, so world stays the
 *   camera-to-world matrix of the newest frame with the clip's first frame as the world.  A plain product chain: no
 *   re-orthonormalisation.  One launch.
 * ---------------------------------------------------------------------------------------- */
long ppea_point_cloud_workspace_bytes(int B, long max_pixels, int stride);
int ppea_point_cloud_f32(const float* pred, const float* scale, const int64_t* table, int B, int h, int w, long max_pixels,
                         float lo, float hi, int mode, int stride, float edge, const float* inv_K,
                         const float* cam_to_world, const void* colour, const int64_t* colour_off, int colour_mode,
                         float* xyz, uint8_t* rgb, int64_t* index, long capacity, int64_t* cursor, int64_t* counts,
                         void* workspace, void* stream);
int ppea_pose_accumulate_f32(float* world, const float* pose, const uint8_t* present, int B, int F, void* stream);

/* ------------------------------------------------------------------------------------------
 * KITTI ground truth from raw LiDAR (kitti_utils.py:50-102 generate_depth_map, export_gt_depth.py), ABI 25: B velodyne scans
 * projected into B sparse depth maps, written into the flat layout ppea_depth_errors_f32 reads.  csrc/kitti_gt.hip.
 *   points [sum N][4] fp32 (device): the scans one after another, x forward; column 3 is ignored (the reference sets it to 1);
 *   point_offsets [B+1] int64, HOST: scan b is points[point_offsets[b] .. point_offsets[b+1]); ascending, an empty scan is fine;
 *   P [B][3][4] fp64 (device): P_rect @ R_cam2rect @ velo2cam of each scan's drive;
 *   table [B][3] int64, HOST: (offset, H, W) of each map in out_flat -- the values of DeviceGroundTruth's table.  The launcher
 *   reads both host arrays to refuse bad arguments and to size its grids without a device round trip; the scans' descriptors
 *   travel to the kernels as launch arguments;
 *   vel_depth != 0: the depth is the point's own fp32 x (export_gt_depth.py), else q2 = (P p)[2] rounded to fp32;
 *   out_flat (device): fp32, every pixel of every map is written (0 = no return); it must hold max(offset + H * W) values;
 *   workspace: ppea_velodyne_depth_workspace_bytes(sum H * W) bytes, cleared by the call itself on `stream`.
 * Per scan: points with x < 0 are dropped; u = rint(q0 / q2) - 1, v = rint(q1 / q2) - 1 in fp64; valid when 0 <= u < W and
 * 0 <= v < H (a NaN fails; q2 < 0 is not filtered); the last valid point in scan order on a pixel sets it; for every sub2ind
 * key v * (W - 1) + u - 1 held by more than one valid point, the pixel of the key's first point is set to the minimum depth of
 * the key's points (the key is shared by (v, W-1) and (v+1, 0): the reference's behaviour, kept); negative depths become 0.
 * One memset + 2 launches per 32 scans; integer atomics on ordered words only: bitwise reproducible.  No host synchronisation.
 * PPEA_ERR_ARG: B <= 0, a NULL array, offsets that do not ascend, a negative offset / H / W; PPEA_ERR_UNSUPPORTED: a scan of
 * more than 2^31 - 2 points or a map of more than 2^31 - 1 pixels.
 * ---------------------------------------------------------------------------------------- */
long ppea_velodyne_depth_workspace_bytes(long total_pixels);
int ppea_velodyne_depth_f32(const float* points, const int64_t* point_offsets, int B, const double* P, const int64_t* table,
                            int vel_depth, float* out_flat, void* workspace, void* stream);

/* ------------------------------------------------------------------------------------------
 * Input pipeline on uint8 frames (datasets/mono_dataset.py:89-112, 143-190 through PIL / torchvision), bit for bit:
 * Pillow's LANCZOS resize of 8-bit images (Resample.c) and torchvision's PIL-path ColorJitter (ImageEnhance blends,
 * Convert.c RGB <-> HSV).  ppeadepth/input_pipeline.py holds the readable restatement and builds the tables.
 *   taps [out][2 + kmax] int32: per output column / row (first input index, tap count n <= kmax, n 22-bit fixed-point
 *   coefficients).  Accumulator int32 from 1 << 21, >> 22 (arithmetic), clip to 0..255.
 * ppea_lanczos_h_u8 / ppea_lanczos_h_view_u8: rows, through one launcher and one strided kernel; the two entry points
 *   differ in how the sources are described.  Common: srcs = HOST array of nsrc <= 8 device pointers, the images of all
 *   sources numbered through; flip [images] int32 or NULL: non-zero = the image is read mirrored (the flipped frame is never
 *   written); nonzero [images] int32 or NULL: set to whether the image holds a non-zero byte (one memset); dst
 *   [images][C][H][Wout], planar.  A workgroup stages whole rows in LDS, each padded to 16 bytes, with 512 bytes of per-row
 *   bookkeeping behind them; a row that does not fit 60 KiB with it is PPEA_ERR_UNSUPPORTED.  One launch.
 * ppea_lanczos_h_u8: dense planar sources, each planes_per_src planes [H][Win]; planes_per_item consecutive planes form an
 *   image (C = planes_per_item): the views of pixel_stride 1, row_stride Win, channel_stride H * Win, item_stride
 *   C * H * Win.  The widest row is 60 928 bytes (61 440 before the entry points shared a launcher).  Every source holds
 *   whole images: planes_per_src that is no multiple of planes_per_item is PPEA_ERR_ARG (before, only the total of all
 *   sources was checked).
 * ppea_lanczos_h_view_u8 (ABI 24): VIEWS.  Image i of source k is C channels of [H][Win] pixels, the byte of (c, y, x) at
 *   srcs[k] + i * item_stride + c * channel_stride + y * row_stride + x * pixel_stride (all strides > 0; the window's x
 *   offset is folded into srcs[k]; a row's first to last byte must fit row_stride), items_per_src images per source.
 *   C = 3, pixel_stride = 3, channel_stride = 1 (a decoder's HWC) has a kernel of its own: one workgroup stages a row's
 *   window once, in 16-byte loads wherever its address allows and byte by byte at the ends, and writes the three channel
 *   rows.  No byte outside the windows is read.
 * ppea_lanczos_v_u8: columns of src [planes][Hin][W] -> dst [planes][Hout][W], planes <= 65535.  One launch.
 * ppea_lanczos_h_ragged_u8 / ppea_lanczos_v_ragged_u8 (ABI 28): the two passes over N interleaved-RGB (HWC) frames of
 *   DIFFERENT sizes (KITTI raw has one size per recording day and a training batch mixes them), packed back to back in one
 *   device buffer of buf_bytes < 2^31 bytes.  desc int32 [N][4] = (byte offset, H, W, size class), H = W = 0 an absent
 *   frame (a missing neighbour); it is given twice, on the host (desc_host: checked before anything is launched -- an
 *   extent outside the buffer, H > Hcap, a class >= K, only one of H and W zero: PPEA_ERR_ARG; a row that cannot be staged
 *   in 60 KiB less 1280 bytes of bookkeeping: PPEA_ERR_UNSUPPORTED) and on the device (desc: what the kernels read; they
 *   clamp it the same way, so a device copy that differs cannot make them read outside the buffer).  prefix: device int32
 *   [N + 1], prefix[n] = the rows of the images before n.  taps: device int32 [K][out][2 + kmax], the tables of the K size
 *   classes, rows zero-padded to the longest.  The horizontal pass writes rows [0, H_n) of dst [N][3][Hcap][Wout] (the
 *   rest is left as it was); flip / nonzero [N] as above.  The vertical pass reads only those rows and writes the dense
 *   [N][3][Hout][W]; an absent frame is written as zeros.  One launch each (and the memset of nonzero), N * 3 <= 65535.
 * ppea_color_jitter_u8: img [N][3][H][W] uint8 -> color = img / 255 and color_aug = jitter(img) / 255, both [N][3][H][W]
 *   fp32 (one correctly rounded division, as ToTensor).  params [N][10] int32: the order of the four operations
 *   (0 brightness, 1 contrast, 2 saturation, 3 hue), the brightness / contrast / saturation factors as fp32 bit patterns,
 *   trunc(hue * 255) & 255, apply, one unused word.  An image with apply == 0, or with nonzero[n] == 0 (nonzero may be
 *   NULL), gets color_aug = color.  workspace: ppea_color_jitter_workspace_bytes(N, H, W) bytes, contents free before and
 *   after the call.  Two launches for any N: the operations that precede contrast and an exact integer sum of Pillow's L
 *   per image, then the whole chain with int(mean(L) + 0.5) known.  H * W <= 2^32 / 255, N <= 65535.
 * ppea_repeat_rows_f32: dst [rows][reps][len] = src [rows][len] (the per-scale K / inv_K of a batch in one launch).
 * ---------------------------------------------------------------------------------------- */
int ppea_lanczos_h_u8(const void* const* srcs, int nsrc, long planes_per_src, const int32_t* taps, int kmax,
                      const int32_t* flip, int planes_per_item, int32_t* nonzero, uint8_t* dst, int H, int Win, int Wout,
                      void* stream);
int ppea_lanczos_h_view_u8(const void* const* srcs, int nsrc, int items_per_src, int C, long pixel_stride, long row_stride,
                           long channel_stride, long item_stride, const int32_t* taps, int kmax, const int32_t* flip,
                           int32_t* nonzero, uint8_t* dst, int H, int Win, int Wout, void* stream);
int ppea_lanczos_v_u8(const uint8_t* src, const int32_t* taps, int kmax, uint8_t* dst, long planes, int Hin, int Hout,
                      int W, void* stream);
int ppea_lanczos_h_ragged_u8(const uint8_t* buf, long buf_bytes, const int32_t* desc_host, const int32_t* desc,
                             const int32_t* prefix, int N, const int32_t* taps, int K, int kmax, const int32_t* flip,
                             int32_t* nonzero, uint8_t* dst, int Hcap, int Wout, void* stream);
int ppea_lanczos_v_ragged_u8(const uint8_t* src, const int32_t* desc_host, const int32_t* desc, int N, const int32_t* taps,
                             int K, int kmax, uint8_t* dst, int Hcap, int Hout, int W, void* stream);
long ppea_color_jitter_workspace_bytes(int N, int H, int W);
int ppea_color_jitter_u8(const uint8_t* img, const int32_t* params, const int32_t* nonzero, void* workspace, float* color,
                         float* color_aug, int N, int H, int W, void* stream);
int ppea_repeat_rows_f32(const float* src, float* dst, int rows, int reps, int len, void* stream);

/* ------------------------------------------------------------------------------------------
 * Training-mode BatchNorm (+ReLU, + residual added before the activation) on channels_last data: the ResNet-18 pose
 * trunk (networks/resnet_encoder.py:25-72).  The tensor is G consecutive sub-batches [G][P][C] (C contiguous,
 * C / 8 a power of two <= 256), each normalised with its own statistics (per-pair statistics of a 2B pose batch).
 *   forward : stats -> partial[G][slabs][2][C]; finalize -> stats[G][3][C] (mean | invstd | unbiased var),
 *             ab[G][2][C] (y = a x + b), running statistics updated once per sub-batch in order;
 *             apply -> y = act(a x + b + res), act 0 none / 1 ReLU
 *   backward: bwd_reduce -> partial; bwd_finalize -> k[G][2][C], dgamma_dbeta[2][C]; bwd_apply -> dx, dres
 * ---------------------------------------------------------------------------------------- */
int ppea_nhwc_bn_slabs(int P, int C);
int ppea_nhwc_bn_stats_f32(const void* x, float* partial, int P, int C, int G, void* stream);
int ppea_nhwc_bn_stats_bf16(const void* x, float* partial, int P, int C, int G, void* stream);
int ppea_nhwc_bn_finalize_f32(const float* partial, int P, int C, int G, const float* gamma, const float* beta,
                              float eps, float momentum, float* stats, float* ab, float* running_mean,
                              float* running_var, void* stream);
int ppea_nhwc_bn_apply_f32(const void* x, const void* res, const float* ab, void* y, int P, int C, int G, int act,
                           void* stream);
int ppea_nhwc_bn_apply_bf16(const void* x, const void* res, const float* ab, void* y, int P, int C, int G, int act,
                            void* stream);
int ppea_nhwc_bn_bwd_reduce_f32(const void* x, const void* dy, const void* res, const float* stats, const float* ab,
                                float* partial, int P, int C, int G, int act, void* stream);
int ppea_nhwc_bn_bwd_reduce_bf16(const void* x, const void* dy, const void* res, const float* stats, const float* ab,
                                 float* partial, int P, int C, int G, int act, void* stream);
int ppea_nhwc_bn_bwd_finalize_f32(const float* partial, int P, int C, int G, float* k, float* dgamma_dbeta,
                                  void* stream);
int ppea_nhwc_bn_bwd_apply_f32(const void* x, const void* dy, const void* res, const float* stats, const float* ab,
                               const float* k, void* dx, void* dres, int P, int C, int G, int act, void* stream);
int ppea_nhwc_bn_bwd_apply_bf16(const void* x, const void* dy, const void* res, const float* stats, const float* ab,
                                const float* k, void* dx, void* dres, int P, int C, int G, int act, void* stream);

/* ------------------------------------------------------------------------------------------
 * Bias + ELU of the decoders' ConvBlock (layers.py:103-116), NCHW: y = elu(z + bias[c]); backward dz = dy * elu'
 * (from the saved OUTPUT: elu' = 1 for y > 0 else y + 1) and partial[N*C][chunks] = per-plane-chunk sums of dz
 * (chunks = ppea_bias_elu_chunks(N, C, HW)); the bias gradient is their sum over N and chunks.
 * ---------------------------------------------------------------------------------------- */
int ppea_bias_elu_chunks(int N, int C, int HW);
int ppea_bias_elu_fwd_f32(const void* z, const void* bias, int bias_bf16, void* y, int N, int C, int HW, void* stream);
int ppea_bias_elu_fwd_bf16(const void* z, const void* bias, int bias_bf16, void* y, int N, int C, int HW, void* stream);
int ppea_bias_elu_bwd_f32(const void* dy, const void* y, void* dz, float* partial, int N, int C, int HW, void* stream);
int ppea_bias_elu_bwd_bf16(const void* dy, const void* y, void* dz, float* partial, int N, int C, int HW, void* stream);

/* Nearest 2x upsampling fused with the skip concatenation of the depth decoder (networks/depth_decoder_v2.py:231-236;
 * layers.py:204-207), channels-last: a [N][H/2][W/2][C1], b [N][H][W][C2] (NULL, C2 = 0: no skip) -> out [N][H][W][C1+C2];
 * backward: dout -> da (2x2 block sums accumulated in fp32), db.  H, W = OUTPUT size (even); C1, C2 % 8 == 0. */
int ppea_nhwc_up2cat_fwd_f32(const void* a, const void* b, void* out, int N, int H, int W, int C1, int C2, void* stream);
int ppea_nhwc_up2cat_fwd_bf16(const void* a, const void* b, void* out, int N, int H, int W, int C1, int C2, void* stream);
int ppea_nhwc_up2cat_bwd_f32(const void* dout, void* da, void* db, int N, int H, int W, int C1, int C2, void* stream);
int ppea_nhwc_up2cat_bwd_bf16(const void* dout, void* da, void* db, int N, int H, int W, int C1, int C2, void* stream);

/* channels_last versions of the decoder passes (x [B][H][W][C], C % 8 == 0; bias_elu: C / 8 a power of two <= 256):
 * the decoders hand the library's NHWC-native convolutions NHWC activations. */
int ppea_nhwc_reflect_pad1_fwd_f32(const void* x, void* out, int B, int H, int W, int C, void* stream);
int ppea_nhwc_reflect_pad1_fwd_bf16(const void* x, void* out, int B, int H, int W, int C, void* stream);
int ppea_nhwc_reflect_pad1_bwd_f32(const void* dout, void* dx, int B, int H, int W, int C, void* stream);
int ppea_nhwc_reflect_pad1_bwd_bf16(const void* dout, void* dx, int B, int H, int W, int C, void* stream);
int ppea_nhwc_bias_elu_slabs(int P, int C);
int ppea_nhwc_bias_elu_fwd_f32(const void* z, const void* bias, int bias_bf16, void* y, int P, int C, void* stream);
int ppea_nhwc_bias_elu_fwd_bf16(const void* z, const void* bias, int bias_bf16, void* y, int P, int C, void* stream);
int ppea_nhwc_bias_elu_bwd_f32(const void* dy, const void* y, void* dz, float* partial, int P, int C, void* stream);
int ppea_nhwc_bias_elu_bwd_bf16(const void* dy, const void* y, void* dz, float* partial, int P, int C, void* stream);

/* ------------------------------------------------------------------------------------------
 * Optimizer step (trainer.py:350, torch.optim.Adam with the reference's defaults) over ONE flat fp32 buffer
 * holding every trainable tensor: p, g, m, v fp32 [n]; w16 (may be NULL) = bf16 working copy of p[0, n_lo);
 * state = device float[2] {step t >= 1, learning rate}.
 * ---------------------------------------------------------------------------------------- */
int ppea_adam_flat_f32(float* p, const float* g, float* m, float* v, void* w16, long n, long n_lo,
                       const float* state, float beta1, float beta2, float eps, void* stream);
/* The same step on g * grad_scale (data-parallel mean of rank-summed gradients without a scaling pass of its own). */
int ppea_adam_flat_scaled_f32(float* p, const float* g, float* m, float* v, void* w16, long n, long n_lo,
                              const float* state, float beta1, float beta2, float eps, float grad_scale, void* stream);

/* ------------------------------------------------------------------------------------------
 * Scattered state <-> one contiguous buffer in ONE launch (checkpoints).  table: device int64 [nseg][4] =
 * {address of the segment, byte offset in the packed buffer, byte count, first work unit}; a work unit is
 * ppea_pack_unit_bytes() bytes of one segment (the last unit of a segment may be shorter, an empty segment owns none),
 * `first work unit` is the running sum of the units of the segments before, `units` their total (= the grid).  Packed
 * offsets are multiples of 16; a segment's address needs the alignment of its elements only (1, 2, 4 or 8 bytes): a unit
 * is copied with the widest access (<= 16 bytes) that both sides are aligned to, its last bytes one by one.  Byte-exact,
 * dtype-agnostic; exactly the listed bytes are read and written.  pack: segments -> packed; unpack: packed -> segments.
 * ---------------------------------------------------------------------------------------- */
long ppea_pack_unit_bytes(void);
int ppea_pack_segments(const void* table, int nseg, long units, void* packed, void* stream);
int ppea_unpack_segments(const void* table, int nseg, long units, const void* packed, void* stream);

/* ------------------------------------------------------------------------------------------
 * Run monitor (ABI 30), csrc/run_monitor.hip: one row per training step appended to a ring on the device, in TWO launches
 * (a scan that leaves one fp64 partial per block in `scratch`, and one block that adds the partials in a fixed order and
 * writes the row; stream order is the hand-off, there are no atomics: the same input gives the same bits).
 *   scalars  HOST array of 8 device pointers to fp32 scalars, NULL = absent; passed on as kernel arguments
 *   grads    fp32 [n] at any 4-byte aligned address; NULL or n == 0: the gradient columns are 0
 *   scratch  fp64 [scratch_blocks][3], scratch_blocks >= ppea_run_monitor_max_blocks()
 *   ring     32-bit words [capacity][ppea_run_monitor_row_words() = 16]:
 *            [0..7] the scalars' bits (0 where absent), [8] grad_l2 = grad_scale * sqrt(fp64 sum of squares of the finite
 *            elements) as fp32, [9] grad_max_abs = grad_scale * max |x| over the finite elements as fp32, [10] bit k set =
 *            scalar k present, [11] 0, [12,13] step (int64), [14,15] count of NaN / Inf elements (int64)
 *   state    int64 [2] = {rows appended so far, first_bad_step}; the caller initialises it to {0, -1}.  The row goes to
 *            slot (rows appended so far) % capacity and the counter is advanced; first_bad_step is set once, to `step` of
 *            the first row with a non-finite present scalar or a non-finite count > 0.
 * ---------------------------------------------------------------------------------------- */
int ppea_run_monitor_row_words(void);
int ppea_run_monitor_max_blocks(void);
int ppea_run_monitor_f32(const void* const* scalars, const float* grads, long n, long step, float grad_scale,
                         double* scratch, int scratch_blocks, void* ring, int capacity, void* state, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PPEA_DEPTH_H */
