/*
 * libmi355conv — C ABI of the MI355X (gfx950) conv-net hot path.
 *
 * The reference (bababyVN/medical-image-segmentation-and-classification) is pure
 * Python/PyTorch and has no FFI of its own: its boundary for this path is the
 * torch.nn leaf-op API called from models/ and utils/helpers.py::train.  Each
 * entry point below therefore cites the reference call site whose ATen/cuDNN
 * kernel it replaces (paths relative to the reference root).
 *
 * Conventions
 *   - all tensors are device pointers owned by the caller (PyTorch's caching
 *     allocator); the library never allocates, frees or synchronises;
 *   - activations are NHWC ("pixel rows"): element (n,h,w,c) of a tensor with
 *     channel stride `ld` lives at ((n*H+h)*W+w)*ld + c, so a channel slice of a
 *     wider (concatenated) tensor is addressed with the same pointer arithmetic;
 *   - `dtype` selects the storage/MFMA input type of activations and packed
 *     weights (MI355_F32: v_mfma_f32_32x32x2_f32, MI355_BF16 / MI355_F16:
 *     v_mfma_f32_{32x32x16,16x16x32}_{bf16,f16}); accumulation, statistics,
 *     parameters and parameter gradients are always fp32;
 *   - every launcher takes the hipStream_t to enqueue on and returns 0 or a
 *     negative MI355_ERR_* / positive hipError_t; mi355_last_error() gives text.
 */
#ifndef MI355CONV_H_
#define MI355CONV_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ihipStream_t* mi355_stream_t; /* == hipStream_t */

enum { MI355_F32 = 0, MI355_BF16 = 1, MI355_F16 = 2 };
enum { MI355_OK = 0, MI355_ERR_ARG = -1, MI355_ERR_UNSUPPORTED = -2, MI355_ERR_RUNTIME = -3 };

int mi355_version(void);
const char* mi355_last_error(void);

/* ---- layout staging ------------------------------------------------------------------ */

/* NCHW fp32 network input -> NHWC `dtype` (one rounding to nearest even) with channels padded with +0 to Cpad (any
 * multiple of 8 >= C; the plans use multiples of 32).  Replaces the implicit layout/precision change of
 * `x.to(device)` + autocast, utils/helpers.py:318-322. */
int mi355_pack_input_nchw(const float* x, void* y, int N, int C, int H, int W, int Cpad, int dtype,
                          mi355_stream_t s);
/* The same input as the 3 x 3 patches of a stride-1, pad-1 convolution: y[n][h][w][c * 9 + kh * 3 + kw] = x[n][c][h + kh - 1][w + kw - 1]
 * (+0 outside the image and for channels >= 9 C), 32 channels per pixel, C <= 3, any N * H below 2^31.  The stem Conv2d(3, Co, 3, 1, 1) (AttentionUNet.py:6,60) is then a
 * pointwise convolution over K = 27 -> 32 on the SAME parameter memory ([Co][3][3][3] read as [Co][27][1][1]). */
int mi355_pack_input_im2col3(const float* x, void* y, int N, int C, int H, int W, int dtype, mi355_stream_t s);
/* NHWC `dtype` (channel stride ld) -> NCHW fp32 (model outputs / logits). */
int mi355_unpack_output_nchw(const void* x, float* y, int N, int C, int H, int W, int ld, int dtype,
                             mi355_stream_t s);
/* NCHW fp32 -> NHWC `dtype` (channel stride ld >= C, C a multiple of the 16-byte chunk) without padding (incoming output
 * gradients). */
int mi355_pack_nchw(const float* x, void* y, int N, int C, int H, int W, int ld, int dtype, mi355_stream_t s);

/* fp32 parameter [Co][Ci][KH][KW] -> packed forward weights Wf[Co][KH*KW][Cip] and (if wb != NULL)
 * packed data-gradient weights Wb[Cip][KH*KW][Co] (any Cip >= Ci, the rows / columns ci >= Ci filled with +0; the plans
 * pad Ci up to a multiple of 32).  `transposed` != 0 reads a ConvTranspose2d parameter [Ci][Co][KH][KW] instead
 * (models/segmentation_models/ResnetUnet.py:21). */
int mi355_pack_conv_weight(const float* w, void* wf, void* wb, int Co, int Ci, int Cip, int KH, int KW,
                           int transposed, int dtype, mi355_stream_t s);

/* Every weight pack of a launch plan in ONE launch: `table` = n descriptors of 9 int64 in device memory
 * {w, wf, wb (0 = none), Co, Ci, Cip, KH*KW, transposed, scale (0 = none)}, same semantics as mi355_pack_conv_weight;
 * scale[Co] multiplies output channel co of both packs as one fp32 product before the rounding to `dtype` (eval-mode
 * BatchNorm folded into the weights); a transposed descriptor ignores its scale. */
int mi355_pack_conv_weights_batched(const int64_t* table, int n, int fields /* = 9: checked, the table is device memory */,
                                    int dtype, mi355_stream_t s);

/* ---- implicit-GEMM convolution on MFMA -------------------------------------------------
 * out[m][j] (+)= bias[j] + sum_{kh,kw,c} in[src(m,kh,kw)][c] * wk[j][kh*KW+kw][c]
 *   m = (n,ho,wo);  t = o*mul + k*kmul + off (per axis);  valid iff t % div == 0 and
 *   0 <= t/div < (up ? 2*Hi : Hi);  src row = t/div (>>1 when `up`: fused nearest x2).
 * forward conv stride s pad p : mul=s, kmul=+1, off=-p, div=1, wk = Wf      (nn.Conv2d forward,
 *   models/segmentation_models/AttentionUNet.py:6,9,20,32,36,40,84; ResNet.py:17-20,102)
 * data gradient stride s pad p: mul=1, kmul=-1, off=+p, div=s, wk = Wb     (convolution_backward
 *   input grad, reached from loss.backward(), utils/helpers.py:329)
 * ConvTranspose2d(k,s)        : data-gradient form with wk = Wf of the transposed parameter
 *   (ResnetUnet.py:21,51).
 * Ci % 32 == 0 (16 for fp32), Co % 32 == 0.  `accumulate` is a bit set: bit 0 adds the result into `out`,
 * bit 1 applies max(0, .) to conv + bias first (nn.ReLU fused into the epilogue: VGG.py:9-41, and eval-mode
 * Conv -> BN -> ReLU with the BN folded into weights and bias), bit 2 sums every 2x2 group of output pixels into a
 * half-resolution `out` [N][Ho/2][Wo/2] (the gradient of the nearest x2 up-sampling that the forward conv folds into
 * its gather, AttentionUNet.py:19; halo kernels only: mi355_conv2d_igemm_variant(...) in {2, 3, 5, 6, 7, 8}).
 * bf16 / fp16 dispatch: 3x3/s1/p1 with Co % 64 == 0 on images divisible by an 8x32 or 16x16 tile ->
 * conv3x3_halo_rw_kernel (halo patch in LDS by LDS-DMA, patch-row register window); 1x1/s1 with (Ci, Co) among
 * 32/64/128-channel pairs (the attention-gate projections, AttentionUNet.py:33-45) -> conv1x1_stream_kernel (weights in
 * registers, pixels streamed straight into MFMA fragments); everything else -> conv_igemm_dma_kernel (LDS-DMA ring);
 * fp32 -> register-staged conv_igemm_kernel. */
int mi355_conv2d_igemm(const void* in, const void* wk, const float* bias, void* out,
                       int N, int Hi, int Wi, int Ci, int ldi,
                       int Ho, int Wo, int Co, int ldo,
                       int KH, int KW, int mul, int kmul, int off, int div, int up,
                       int accumulate, float* stats, int dtype, mi355_stream_t s);
/* Which kernel serves a shape: 0 generic register-staged, 1 LDS-DMA ring, 2 / 3 halo kernel with 8x32 / 16x16 tiles,
 * 4 streaming pointwise kernel, 5 / 6 the 512-thread ping-pong halo kernels with 64 / 128 output channels per workgroup
 * (5: MI355_HALO_PP=1 only; 6: 3x3/s1/p1, Co % 128 == 0, Ci % 64 == 0 and Ci >= 256, image divisible by 16 x 32 — one workgroup
 * per CU, so the launcher falls back to variant 2 for a batch whose grid would leave more than a fifth of the last round of
 * workgroups empty; mi355_conv2d_igemm_stat_rows, which knows N, follows the launcher); 7 the weight-stationary persistent
 * kernel (3x3/s1/p1, Ci == 64, Co % 64 == 0, image divisible by 8 x 32: the 64-channel layers of every U-Net level,
 * AttentionUNet.py:62-63,82, R2AttU_Net.py:36-39; the launcher falls back to variant 2 below two tiles per workgroup); 8 its
 * Ci == 128 instantiation (4 x 32-pixel tiles: AttentionUNet.py:65-66,78-79,81); 9 the padding-free GEMM kernel (conv_gemm256_kernel:
 * 1x1 at stride 1 / 2, 2x2 / stride 2, ConvTranspose2d(2, 2) as four pointwise phases; Ci % 64 == 0, Co % 128 == 0, whole 256-row
 * tiles, at least 128 of them — the ResNet-50 encoder's 1x1 convolutions and ResnetUnet.py:21,51's transposed convolutions). */
int mi355_conv2d_igemm_variant(int Hi, int Wi, int Ci, int Ho, int Wo, int Co, int KH, int KW, int mul, int kmul, int off,
                               int div, int up, int dtype);
/* ... and the variant the launcher actually runs for a batch of N images (the batch-dependent fall-backs applied). */
int mi355_conv2d_igemm_variant_n(int N, int Hi, int Wi, int Ci, int Ho, int Wo, int Co, int KH, int KW, int mul, int kmul,
                                 int off, int div, int up, int dtype);
/* Fused BatchNorm statistics: when `stats` != NULL the epilogue also writes, per M tile b of the kernel
 * (per WORKGROUP for the streaming pointwise kernel) it dispatches to, stats[(b*2+0)*Co + c] = sum and stats[(b*2+1)*Co + c] = sum of squares of the
 * (rounded) outputs — the same partial layout mi355_bn_finalize consumes.  The number of tile rows is
 * mi355_conv2d_igemm_stat_rows(...) (0 = not available for this shape/dtype: use mi355_bn_stats; the launcher refuses a `stats`
 * buffer exactly there, and with the accumulate bit). */
/* Output-channel tile (128 / 64 / 32) of the LDS-DMA ring kernel (variant 1) for N x Ho x Wo output rows: the widest that divides
 * Co unless its grid would leave most of the chip idle (bench.py's kernel names). */
int mi355_conv2d_igemm_dma_tile(int N, int Ho, int Wo, int Ci, int Co);
int mi355_conv2d_igemm_generic_tile(int N, int Ho, int Wo, int Co);      /* ... and of the generic kernel (variant 0; fp32) */
int mi355_conv2d_igemm_stat_rows(int N, int Hi, int Wi, int Ci, int Ho, int Wo, int Co, int KH, int KW,
                                 int mul, int kmul, int off, int div, int up, int dtype);
/* Whether the kernel the launcher runs for this batch has the 2x2-sum epilogue (bit 2 of `accumulate`): the halo kernels only, so
 * 0 wherever mi355_conv2d_igemm_variant_n is not one of them, fp32 included. */
int mi355_conv2d_igemm_pool2_ok(int N, int Hi, int Wi, int Ci, int Ho, int Wo, int Co, int KH, int KW,
                                int mul, int kmul, int off, int div, int up, int dtype);
/* Name of the kernel instantiation the launcher runs for this batch, as bench.py's per-kernel table books it (NULL: unknown dtype).
 * The string lives in a thread-local buffer: valid until the calling thread's next call. */
const char* mi355_conv2d_igemm_kernel_name(int N, int Hi, int Wi, int Ci, int Ho, int Wo, int Co, int KH, int KW,
                                           int mul, int kmul, int off, int div, int up, int dtype);

/* Weight gradient: ws[split][Co][KH*KW][Ci] = sum over the split's pixel range of
 * dy[m][co] * x[src(m,kh,kw)][ci] (forward addressing as above), then
 * mi355_conv2d_wgrad_reduce sums the splits into the fp32 parameter-gradient layout
 * [Co][Ci_real][KH][KW] (or [Ci_real][Co][KH][KW] when transposed), beta in {0,1}.
 * (convolution_backward weight grad, utils/helpers.py:329.) */
int mi355_conv2d_wgrad_splits(int N, int Ho, int Wo, int Ci, int Co, int KH, int KW);
/* The kernel mi355_conv2d_wgrad runs for a 2-byte layer of this geometry: 0 = the generic per-tap split-K kernel; nine-tap kernels
 * (3x3 / stride 1 / pad 1, Ho % 8 == 0): 1 = four waves, rows of 32-pixel segments; 2 = four waves, 16-pixel-wide images two at a
 * time; 3 = eight waves, rows of 64-pixel segments (wgrad3x3_halo8_kernel); 4 = eight waves, 32-pixel-wide images two at a time. */
int mi355_conv2d_wgrad_variant(int N, int Ho, int Wo, int KH, int KW, int stride, int pad, int dtype);
/* Name of the kernel of that answer, as bench.py's per-kernel table books it (shape-level, like the variant query).  The string is
 * static or lives in a thread-local buffer: valid until the calling thread's next call. */
const char* mi355_conv2d_wgrad_kernel_name(int N, int Ho, int Wo, int Ci, int Co, int KH, int KW, int stride, int pad, int dtype);
int mi355_conv2d_wgrad(const void* x, const void* dy, float* ws, int splits,
                       int N, int Hi, int Wi, int Ci, int ldx,
                       int Ho, int Wo, int Co, int ldy,
                       int KH, int KW, int stride, int pad, int up, int dtype, mi355_stream_t s);
/* Weight gradient of ONE 3x3 / stride 1 / pad 1 convolution that was applied `napp` (<= 6) times to different inputs — the
 * shared convolution of a recurrent block (R2AttU_Net.py:29-45: conv(x), then five times conv(x + x1)): dW = sum over the
 * pairs (x_i, dy_i), computed by ONE launch of the nine-tap kernel (the pairs are more work items) into ONE set of partial
 * slabs, followed by ONE mi355_conv2d_wgrad_reduce.  All pairs share geometry and channel strides; unused pairs are NULL.
 * Served when mi355_conv2d_wgrad_multi_ok(N, Ho, Wo, dtype) != 0 (bf16 / fp16, images divisible into the kernel's row
 * segments); splits = mi355_conv2d_wgrad_splits(N * napp, ...), ws = splits * Co * 9 * Ci floats. */
int mi355_conv2d_wgrad_multi_ok(int N, int Ho, int Wo, int dtype);
int mi355_conv2d_wgrad_multi(const void* x0, const void* dy0, const void* x1, const void* dy1, const void* x2, const void* dy2,
                             const void* x3, const void* dy3, const void* x4, const void* dy4, const void* x5, const void* dy5,
                             int napp, float* ws, int splits, int N, int Hi, int Wi, int Ci, int ldx, int Ho, int Wo, int Co,
                             int ldy, int up, int dtype, mi355_stream_t s);
int mi355_conv2d_wgrad_reduce(const float* ws, int splits, float* dw, int Co, int Ci, int Ci_real,
                              int KH, int KW, int transposed, float beta, mi355_stream_t s);

/* ---- per-channel reductions / BatchNorm (nn.BatchNorm2d, AttentionUNet.py:7,10,21,34,38,42) -- */

/* partial[(b*2+0)*C + c] = sum over block b's rows of x[m][c]; [(b*2+1)*C+c] = sum of squares.
 * nblocks = mi355_rowreduce_blocks(M). */
int mi355_rowreduce_blocks(long long M);
int mi355_bn_stats(const void* x, float* partial, long long M, int C, int ld, int dtype, mi355_stream_t s);
/* Train-mode finalize: batch mean / biased var -> scale = gamma*invstd, shift = beta - mean*scale,
 * saves mean/invstd, updates running stats (momentum, unbiased var) and num_batches_tracked. */
int mi355_bn_finalize(const float* partial, int nblocks, long long M, int C, const float* gamma,
                      const float* beta, float* running_mean, float* running_var, int64_t* nbt,
                      float momentum, float eps, float* scale, float* shift, float* mean, float* invstd,
                      mi355_stream_t s);
/* out[j][c] = sum of partial rows [j*per, (j+1)*per) (per = ceil(rows / nsplit)), c < rowlen: pre-folds the one-row-per-tile
 * statistics a convolution epilogue leaves (thousands of rows) so that mi355_bn_finalize reads nsplit rows. */
int mi355_fold_rows(const float* partial, int rows, int rowlen, float* out, int nsplit, mi355_stream_t s);
/* Eval-mode scale/shift from running stats. */
/* out[c] = scale[c] * (bias ? bias[c] : 0) + shift[c]: the bias of a convolution with eval-mode BN folded in. */
int mi355_bn_fold_bias(const float* bias, const float* scale, const float* shift, float* out, int C, mi355_stream_t s);
int mi355_bn_eval_coeffs(const float* gamma, const float* beta, const float* running_mean,
                         const float* running_var, float eps, int C, float* scale, float* shift,
                         mi355_stream_t s);
/* y = act(x*scale[c]+shift[c] (+ x2*scale2[c]+shift2[c] | + r)) ; act bit0: ReLU, bit1: add `res` AFTER the
 * activation (y = relu(bn(x)) + r, the recurrent-block input of R2AttU_Net.py:44) instead of before it.
 * x2/scale2/shift2 optional second normalised operand (attention gate g1+x1,
 * AttentionUNet.py:51); `res` optional already-activated residual (ResNet.py:43). */
int mi355_bn_act(const void* x, int ldx, const float* scale, const float* shift,
                 const void* x2, int ldx2, const float* scale2, const float* shift2,
                 const void* res, int ldr, void* y, int ldy, long long M, int C, int act, int dtype,
                 mi355_stream_t s);
/* ... and with the MaxPool2d(2, 2) that follows it in every encoder level (AttentionUNet.py:61,89-95; R2AttU_Net.py:92,122-134)
 * in the same pass: y = act(x*scale+shift) as above (no second operand, no residual) AND p[n][h/2][w/2][c] = max of the 2 x 2
 * group of y (of the values as stored).  H and W even.  p == NULL: the activation only — the same kernel serves plain BatchNorm
 * apply passes on even images (a thread owns a 2 x 2 window: measured ≈8 % faster than the row-ordered mi355_bn_act). */
int mi355_bn_act_pool2(const void* x, int ldx, const float* scale, const float* shift, void* y, int ldy, void* p, int ldp,
                       int N, int H, int W, int C, int act, int dtype, mi355_stream_t s);
/* mi355_bn_act's forms WITHOUT a second normalised operand (plain, or with the residual `res` added before the activation — act
 * bit 1: after it, the recurrent block's x + relu(bn(.)), R2AttU_Net.py:44) in the window order of mi355_bn_act_pool2: the same
 * values, ≈8 % faster on even images. */
int mi355_bn_act_windows(const void* x, int ldx, const float* scale, const float* shift, const void* res, int ldr, void* y, int ldy,
                         int N, int H, int W, int C, int act, int dtype, mi355_stream_t s);
/* Backward reductions for y = act(bn(x) [+ other]) given dL/dy:
 * partial sums of g and g*xhat per channel, g = dy * (y > 0 if act).  When `y` is NULL the ReLU mask
 * is recomputed as x*mscale[c]+mshift[c] > 0 (the forward's own coefficients), which saves reading
 * the activated tensor; `y` is required when a residual / second operand was added before the ReLU. */
/* Partial rows mi355_bn_bwd_reduce can leave non-zero (= the workgroups it runs on, at most one per CU); rows from there up to
 * mi355_rowreduce_blocks(M) are written as zeros, so mi355_bn_bwd_finalize may fold this many rows only. */
int mi355_bn_bwd_reduce_rows(long long M);
int mi355_bn_bwd_reduce(const void* dy, int lddy, const void* y, int ldy, const void* x, int ldx,
                        const float* mean, const float* invstd, const float* mscale, const float* mshift,
                        float* partial, long long M, int C, int act, int dtype, mi355_stream_t s);
/* sums[0..C) = sum g (dbeta), sums[C..2C) = sum g*xhat (dgamma); beta-accumulate into dgamma/dbeta. */
int mi355_bn_bwd_finalize(const float* partial, int nblocks, int C, float* sums, float* dgamma, float* dbeta,
                          float acc, mi355_stream_t s);
/* The same fold over partial rows of nq quantities per channel: (sum g, sum g*xhat) = quantities (q0, q1) of each row. */
int mi355_bn_bwd_finalize_at(const float* partial, int nblocks, int nq, int q0, int q1, int C, float* sums, float* dgamma,
                             float* dbeta, float acc, mi355_stream_t s);
/* dx = gamma*invstd*(g - sum_g/M - xhat*sum_gx/M); optional dres = g (residual / second operand
 * gradient, pre-normalisation: the ReLU mask applied); optional dpost (+)= dy, the UNMASKED incoming gradient, for an
 * operand that was added AFTER the activation (x + relu(bn(.)), R2AttU_Net.py:44; post_acc != 0 accumulates) — the
 * pass reads dy anyway; optional bias-gradient partials (column sums of dx). */
int mi355_bn_bwd_apply(const void* dy, int lddy, const void* y, int ldy, const void* x, int ldx,
                       const float* gamma, const float* mean, const float* invstd, const float* mscale,
                       const float* mshift, const float* sums, void* dx, int lddx, void* dres, int lddres,
                       void* dpost, int lddpost, int post_acc, float* dbias_partial,
                       long long M, int C, int act, int dtype, mi355_stream_t s);
/* The same pass for the LAST of several applications whose incoming gradients all flow to the same post-activation operand (the
 * recurrent block's x in x + relu(bn(conv(.))), applied t times with shared weights: R2AttU_Net.py:41-44): dpost (+)= dy + ex0 +
 * ex1 + ex2 + ex3, the earlier applications' incoming gradients (ex1..ex3 may be NULL; row pitch ldex), summed in fp32 and rounded
 * once — the earlier applications' passes then carry no dpost at all (one pass over d x instead of t read-modify-writes). */
int mi355_bn_bwd_apply_post4(const void* dy, int lddy, const void* y, int ldy, const void* x, int ldx,
                             const float* gamma, const float* mean, const float* invstd, const float* mscale,
                             const float* mshift, const float* sums, void* dx, int lddx, void* dpost, int lddpost,
                             int post_acc, const void* ex0, const void* ex1, const void* ex2, const void* ex3, int ldex,
                             long long M, int C, int act, int dtype, mi355_stream_t s);
/* The same two passes for a BatchNorm + ReLU layer whose activation also feeds a MaxPool2d(2, 2) (mi355_bn_act_pool2;
 * AttentionUNet.py:61,89-95): dp, the gradient of the POOLED tensor [N][H/2][W/2][C], is added on the fly to the pixels that are
 * the first maximum of their window (torch's tie rule, the activation recomputed from x with mscale / mshift exactly as the
 * forward rounded it), so mi355_maxpool_bwd's pass over dy is not run: g = relu'(.) * (dy + [first max] * dp).  partial / sums /
 * dx as in mi355_bn_bwd_reduce / _apply with act = 1 and no y.  dy == NULL: the pooling is the activation's only consumer (VGG.py),
 * g = relu'(.) * [first max] * dp.  mi355_bn_bwd_pool2_ok: 1 when the window-ordered pass covers the
 * geometry (C / (16 / element size) a power of two <= 32, W a power-of-two multiple of 512 / that), else use the separate passes. */
int mi355_bn_bwd_pool2_ok(int H, int W, int C, int dtype);
int mi355_bn_bwd_reduce_pool2_rows(long long M);      /* partial rows mi355_bn_bwd_reduce_pool2 can leave non-zero (cf. mi355_bn_bwd_reduce_rows) */
int mi355_bn_bwd_reduce_pool2(const void* dy, int lddy, const void* dp, int lddp, const void* x, int ldx, const float* mean,
                              const float* invstd, const float* mscale, const float* mshift, float* partial,
                              int N, int H, int W, int C, int dtype, mi355_stream_t s);
int mi355_bn_bwd_apply_pool2(const void* dy, int lddy, const void* dp, int lddp, const void* x, int ldx, const float* gamma,
                             const float* mean, const float* invstd, const float* mscale, const float* mshift,
                             const float* sums, void* dx, int lddx, int N, int H, int W, int C, int dtype, mi355_stream_t s);
/* out[c] (+)= sum_b partial[b*stride*C + c]  (used for conv bias gradients). */
int mi355_colsum_finalize(const float* partial, int nblocks, int stride, int C, float* out, float acc,
                          mi355_stream_t s);
/* partial column sums of a plain tensor (bias gradient of convs without BN). */
int mi355_colsum(const void* x, int ld, float* partial, long long M, int C, int dtype, mi355_stream_t s);

/* ---- pooling / resampling / elementwise ------------------------------------------------- */
/* nn.MaxPool2d(k, s, p) forward and backward (AttentionUNet.py:61; ResNet.py:105); backward routes
 * to the first maximum in window scan order, accumulating into dx when accumulate != 0. */
int mi355_maxpool_fwd(const void* x, int ldx, void* y, int ldy, int N, int H, int W, int C,
                      int k, int stride, int pad, int dtype, mi355_stream_t s);
int mi355_maxpool_bwd(const void* x, int ldx, const void* dy, int lddy, void* dx, int lddx,
                      int N, int H, int W, int C, int k, int stride, int pad, int accumulate, int dtype,
                      mi355_stream_t s);
/* gradient of nn.Upsample(scale_factor=2) (nearest): dx[h][w] = sum of the 2x2 block of dy (+ dx when accumulate != 0),
 * summed in fp32 and rounded to `dtype` once; accumulate == 0 never reads dx. */
int mi355_upsample2_bwd(const void* dy, int lddy, void* dx, int lddx, int N, int H, int W, int C,
                        int accumulate, int dtype, mi355_stream_t s);
/* y = a + b (b == NULL: a strided copy of a's bits), one ld per operand; y may be a or b (in place). */
int mi355_add(const void* a, int lda, const void* b, int ldb, void* y, int ldy, long long M, int C, int dtype,
              mi355_stream_t s);
/* y = relu(x) forward; dx = y > 0 ? dy : +0 backward, a select: the bits of dy pass, an inf under y <= 0 gives 0 (VGG.py:10). */
int mi355_relu_fwd(const void* x, int ldx, void* y, int ldy, long long M, int C, int dtype, mi355_stream_t s);
int mi355_relu_bwd(const void* dy, int lddy, const void* y, int ldy, void* dx, int lddx, long long M, int C,
                   int dtype, mi355_stream_t s);

/* ---- attention gate / single-output 1x1 conv (AttentionUNet.py:29-54, 84) ------------------ */
/* z[m] = b + sum_c x[m][c]*w[c]  (ONE output channel of a Conv2d(C,K,1): the attention gate's psi, K = 1, and the logit
 * heads `out` / `conv_1x1` with out_channel = K, AttentionUNet.py:84, R2AttU_Net.py:117); optional per-block partial
 * (sum z, sum z^2).  K > 1: the launch produces channel plane k of an NCHW fp32 map [N][K][HW] — pass z + k*HW (and the
 * k-th weight row / bias); pixel m = n*HW + p lands at z[n*K*HW + p].  K == 1: HW is ignored. */
int mi355_rowdot_fwd(const void* x, int ldx, const float* w, const float* b, float* z, float* partial,
                     long long M, int C, int HW, int K, int dtype, mi355_stream_t s);
/* dx[m][c] = dz[m]*w[c] (masked by x>0 if relu_mask), added to dx when accumulate (the further planes of a K-channel
 * head); partial dw[c] = sum_m dz[m]*x[m][c], db.  dz is indexed like z above. */
int mi355_rowdot_bwd(const float* dz, const void* x, int ldx, const float* w, void* dx, int lddx,
                     float* partial, long long M, int C, int relu_mask, int HW, int K, int accumulate, int dtype,
                     mi355_stream_t s);
/* y[m][c] = x[m][c] * sigmoid(z[m]*scale[0]+shift[0]) */
int mi355_gate_mul_fwd(const void* x, int ldx, const float* z, const float* scale, const float* shift,
                       void* y, int ldy, long long M, int C, int dtype, mi355_stream_t s);
/* dx (+)= dy*psi ; dzn[m] = (sum_c dy*x) * psi*(1-psi); partial (sum dzn, sum dzn*zhat). */
int mi355_gate_mul_bwd(const void* dy, int lddy, const void* x, int ldx, const float* z, const float* scale,
                       const float* shift, const float* mean, const float* invstd, void* dx, int lddx,
                       int accumulate, float* dzn, float* partial, long long M, int C, int dtype,
                       mi355_stream_t s);
/* scalar-field BN backward: dz = gamma*invstd*(dzn - S0/M - zhat*S1/M). */
int mi355_bn1_bwd_apply(const float* dzn, const float* z, const float* gamma, const float* mean,
                        const float* invstd, const float* sums, float* dz, long long M, mi355_stream_t s);
/* psi_in = relu(BN_g(g1) + BN_x(x1)) and z = psi conv of it in ONE pass over the raw branch outputs (instead of mi355_bn_act with a
 * second operand + mi355_rowdot_fwd): psi_in is computed as mi355_bn_act would have stored it and is not stored — the backward
 * below recomputes it as well.  partial: per-block (sum z, sum z^2) or null.  _ok: C / (16 / element size) <= 64.
 * x1 == NULL (with scale_x / shift_x NULL): ONE normalised operand, z = w . relu(BN_g(g1)) + b — the logit head behind the last
 * decoder layer (AttentionUNet.py:84,119); the two backward entry points accept the same (the x-branch arguments NULL, quantity 2
 * of the partial rows zero, dx1 not written). */
int mi355_gate_psi_fwd_ok(int C, int dtype);
int mi355_gate_psi_fwd(const void* g1, int ldg, const void* x1, int ldx, const float* scale_g, const float* shift_g,
                       const float* scale_x, const float* shift_x, const float* w, const float* b, float* z,
                       float* partial, long long M, int C, int dtype, mi355_stream_t s);
/* Backward of the gate's two normalised branches in two passes instead of mi355_rowdot_bwd + 2 x (mi355_bn_bwd_reduce,
 * mi355_bn_bwd_apply) (AttentionUNet.py:32-38,48-52: psi_in = relu(BN_g(W_g g) + BN_x(W_x x)), z = psi conv).  g1 / x1 are the RAW
 * branch convolution outputs, scale / shift / mean / invstd the forward's coefficients of the two BatchNorms, w the psi
 * convolution's weight [C], dz the gradient of its output: the gradient of psi_in, dz[m] * w[c] where psi_in > 0, is recomputed
 * on the fly (psi_in exactly as mi355_bn_act rounded it) and never stored.  reduce leaves FIVE quantities per channel and partial
 * row — sum dp, sum dp * xhat_g, sum dp * xhat_x, sum dz * psi_in (the psi weight's gradient), sum dz (its bias's) — which
 * mi355_bn_bwd_finalize_at (quantities (0, 1) and (0, 2) of 5) and mi355_colsum_finalize (stride 5) fold; apply writes the input
 * gradients of both BatchNorms.  mi355_gate_bn_bwd_reduce_rows: the partial rows that can be non-zero. */
int mi355_gate_bn_bwd_reduce_rows(long long M);
int mi355_gate_bn_bwd_reduce(const float* dz, const void* g1, int ldg, const void* x1, int ldx, const float* scale_g,
                             const float* shift_g, const float* mean_g, const float* invstd_g, const float* scale_x,
                             const float* shift_x, const float* mean_x, const float* invstd_x, const float* w,
                             float* partial, long long M, int C, int dtype, mi355_stream_t s);
int mi355_gate_bn_bwd_apply(const float* dz, const void* g1, int ldg, const void* x1, int ldx, const float* scale_g,
                            const float* shift_g, const float* mean_g, const float* invstd_g, const float* scale_x,
                            const float* shift_x, const float* mean_x, const float* invstd_x, const float* w,
                            const float* gamma_g, const float* gamma_x, const float* sums_g, const float* sums_x,
                            void* dg1, int lddg, void* dx1, int lddx, long long M, int C, int dtype, mi355_stream_t s);

/* ---- heads (ResNet.py:112-115, VGG.py:109-119) --------------------------------------------- */
int mi355_global_pool_fwd(const void* x, int ldx, float* y, int32_t* argmax, int N, int HW, int C, int is_max,
                          int dtype, mi355_stream_t s);
int mi355_global_pool_bwd(const float* dy, const int32_t* argmax, void* dx, int lddx, int N, int HW, int C,
                          int is_max, int dtype, mi355_stream_t s);
/* y[b][o] = act(bias[o] + sum_i x[b][i]*w[o][i]) (fp32, tiny M); backward pieces. */
int mi355_linear_fwd(const float* x, const float* w, const float* bias, float* y, int B, int I, int O, int relu,
                     mi355_stream_t s);
int mi355_linear_bwd(const float* x, const float* w, const float* y, const float* dy, float* dx, float* dw,
                     float* db, int B, int I, int O, int relu, float beta, float* scratch, mi355_stream_t s);
/* fp32 elements of `scratch` mi355_linear_bwd needs to produce dx (0 for small layers; the wide layers of the torchvision
 * VGG head — 25088 x 4096 — stream W once per 16 batch rows and fold 16 deterministic output-range partials). */
int mi355_linear_bwd_scratch(int B, int I, int O);
/* inverted dropout with a counter hash (seed, counter[0], element index): mask byte kept for backward;
 * `counter` is a device word the host bumps per forward so a static launch plan draws fresh masks. */
int mi355_dropout_fwd(const float* x, float* y, uint8_t* mask, long long n, float p, uint64_t seed,
                      const int32_t* counter, mi355_stream_t s);
int mi355_dropout_bwd(const float* dy, const uint8_t* mask, float* dx, long long n, float p, mi355_stream_t s);

/* ---- losses (utils/helpers.py:244-246) ---------------------------------------------------- */
/* BCEWithLogitsLoss (mean): loss[0] and dz = (sigmoid(z)-t)/n * gscale[0] (NCHW fp32 with C==1 is
 * the same memory as NHWC, so logits/targets are taken as flat arrays). */
int mi355_bce_logits(const float* z, const float* t, float* loss, float* dz, const float* gscale, long long n,
                     mi355_stream_t s);
/* CrossEntropyLoss(label_smoothing): loss[0], dz[B][C]. */
int mi355_ce_smooth(const float* z, const int64_t* y, float* loss, float* dz, const float* gscale, int B,
                    int C, float smoothing, mi355_stream_t s);
/* Cross-entropy against a DISTRIBUTION: two labels with a weight per sample (mixup / CutMix, utils/mix.py), label smoothing and
 * optional per-class weights; mean reduction (nothing in the reference, which trains on hard labels).  z: [B][C] fp32 logits.
 *   t[b][c]  = (1 - smoothing) * (lam[b] * [c == ya[b]] + (1 - lam[b]) * [c == yb[b]]) + smoothing / C
 *   loss[0]  = (1 / B) * sum_b sum_c weight[c] * t[b][c] * (-log_softmax(z[b])[c])
 *   dz[b][c] = (gscale[0] / B) * (softmax(z[b])[c] * sum_k (weight[k] * t[b][k]) - weight[c] * t[b][c])
 * = torch.nn.functional.cross_entropy(z, t, weight=weight, label_smoothing=smoothing) with PROBABILITY targets: the sum is
 * divided by B.  (With class-index targets and a weight torch divides by the sum of the picked weights instead; that
 * normalisation is not built, so with a weight the hard-label case here differs from torch's class-index call by that factor.)
 * yb and lam NULL together: hard labels, t = the smoothed one-hot of ya.  weight ([C]) NULL: all ones.  dz NULL: loss only;
 * gscale NULL: 1.  Evaluated in double (inputs widened, exp / log in double, lam widened before 1 - lam) and rounded to float
 * once on store; one workgroup, thread b % 256 owns row b, then a block fold in a fixed order: bit-reproducible.  Labels outside
 * [0, C) are the caller's contract (they only select no class: nothing is indexed by them). */
int mi355_ce_mix(const float* z, const int64_t* ya, const int64_t* yb, const float* lam, const float* weight, float* loss,
                 float* dz, const float* gscale, int B, int C, float smoothing, mi355_stream_t s);
/* Dice / BCE + Dice on fp32 logits and targets [B][per] (the reference's DiceLoss / CombinedLoss,
 * utils/clip_seg_finetuner.py:40-74).  p = sigmoid(z), I = sum p t, P = sum p, T = sum t, D = P + T + smooth:
 *   loss[0] = bce_weight * mean(BCEWithLogits(z, t)) + dice_weight * (1 - (2 I + smooth) / D)
 * with the sums over the whole batch (per_sample = 0, the reference) or per image, the B Dice terms averaged
 * (per_sample = 1; the BCE term is the same).  Deterministic: no floating-point atomics, every fold in a fixed order.
 *   mi355_seg_loss_rows: rows of four floats `partial` must hold (16-byte aligned); a function of (B, per) alone.
 *   mi355_seg_loss_fwd:  one pass over z and t (16-byte accesses when per % 4 == 0 and z, t are 16-byte aligned), a
 *     one-workgroup finalize in double; leaves loss[0] and, in state[2 b], state[2 b + 1], the pair (a_b, c_b) of
 *     sample b: a = dice_weight 2 / D, c = dice_weight (2 I + smooth) / D^2 (per_sample: its own sums, both / B).
 *   mi355_seg_loss_bwd:  one pass, dz_i = gscale[0] * (bce_weight (p_i - t_i) / (B per) - (a_b t_i - c_b) p_i (1 - p_i))
 *     from the `state` the forward left (same B, per, bce_weight); gscale = upstream gradient x loss scale on the
 *     device, NULL = 1.  It does not recompute the loss.
 * B <= 65535; weights and smooth >= 0 (smooth = 0 with an all-zero target divides by sum p alone). */
int mi355_seg_loss_rows(int B, long long per);
int mi355_seg_loss_fwd(const float* z, const float* t, int B, long long per, float bce_weight, float dice_weight,
                       float smooth, int per_sample, float* partial, float* state, float* loss, mi355_stream_t s);
int mi355_seg_loss_bwd(const float* z, const float* t, int B, long long per, float bce_weight, const float* state,
                       const float* gscale, float* dz, mi355_stream_t s);
/* Focal + (focal-)Tversky on fp32 logits and targets [B][per] (nothing in the reference; Lin et al. 2017 with torchvision's
 * sigmoid_focal_loss convention, Salehi et al. 2017, Abraham & Khan 2019).  The target is binarised in the kernels, t = (target > 0.5).
 * p = sigmoid(z), I = sum p t, P = sum p, T = sum t, FP = P - I, FN = T - I, n = B per:
 *   focal_i = alpha_t (1 - p_t)^focal_gamma ce_i,  p_t = t p + (1 - t)(1 - p),  ce = BCEWithLogits(z, t),
 *             alpha_t = focal_alpha t + (1 - focal_alpha)(1 - t), focal_alpha < 0: alpha_t = 1
 *   TI      = Num / Den,  Num = I + smooth,  Den = I + tv_a FP + tv_b FN + smooth
 *   loss[0] = focal_weight * mean_i(focal_i) + tversky_weight * (1 - TI)^tv_exp
 * with TI over the whole batch (per_sample = 0) or per image, the B terms averaged (per_sample = 1; the focal term is the same).
 * tv_exp = 1: the Tversky loss; tv_a = tv_b = 0.5, tv_exp = 1, smooth = s: the Dice loss of mi355_seg_loss_fwd with smooth 2 s.
 * Deterministic: no floating-point atomics, every fold in a fixed order.
 *   mi355_ftv_loss_rows: rows of four floats `partial` must hold (16-byte aligned); a function of (B, per) alone.
 *   mi355_ftv_loss_fwd:  one pass over z and t (16-byte accesses when per % 4 == 0 and z, t are 16-byte aligned), a one-workgroup
 *     finalize in double; leaves loss[0] and, in state[2 b], state[2 b + 1], the pair (A_b, C_b) of sample b:
 *     A = tversky_weight tv_exp (1 - TI)^(tv_exp - 1) / Den, C = A Num / Den (per_sample: its own sums, both / B); with
 *     1 - TI <= 0 (a perfect, saturated prediction) A = C = 0: the sub-gradient 0, never NaN or inf.
 *   mi355_ftv_loss_bwd:  one pass, with s = 2 t - 1, u = 1 - p_t:
 *     dz_i = gscale[0] * (focal_weight / n * alpha_t u^focal_gamma s (-focal_gamma p_t ce - u)
 *                         - (A_b t - C_b (tv_a + (1 - tv_a - tv_b) t)) p (1 - p))
 *     from the `state` the forward left (same B, per and parameters); gscale = upstream gradient x loss scale on the device,
 *     NULL = 1.  It does not recompute the loss.
 * u and p (1 - p) come from e = exp(-|z|), without a 1 - p cancellation: every output is finite at |z| = 100.  focal_gamma = 0:
 * u^0 = 1 exactly, also at u = 0; u = 0 with focal_gamma > 0: the element's focal term and focal gradient are exactly 0.
 * B <= 65535; focal_weight, tversky_weight, focal_gamma, smooth >= 0; focal_alpha <= 1; tv_a, tv_b >= 0, tv_a + tv_b > 0; tv_exp > 0. */
int mi355_ftv_loss_rows(int B, long long per);
int mi355_ftv_loss_fwd(const float* z, const float* t, int B, long long per, float focal_weight, float focal_alpha,
                       float focal_gamma, float tversky_weight, float tv_a, float tv_b, float tv_exp, float smooth,
                       int per_sample, float* partial, float* state, float* loss, mi355_stream_t s);
int mi355_ftv_loss_bwd(const float* z, const float* t, int B, long long per, float focal_weight, float focal_alpha,
                       float focal_gamma, float tv_a, float tv_b, const float* state, const float* gscale, float* dz,
                       mi355_stream_t s);
/* Focal cross-entropy for classifiers (Lin et al. 2017, softmax form): z [B][C] fp32 logits, hard labels y, gamma >= 0, optional
 * per-class weight [C] (NULL: all ones).  With p = softmax(z[b]), py = p[y_b], u = sum_{c != y_b} p_c (summed, not 1 - py):
 *   loss[0]  = (1 / B) sum_b weight[y_b] u^gamma (-log py)
 *   dz[b][c] = (gscale[0] / B) weight[y_b] ([c == y_b] - p_c) (gamma py u^(gamma - 1) log py - u^gamma)
 * The sum is divided by B, as in mi355_ce_mix (not by the sum of the picked weights).  gamma = 0: mi355_ce_mix with hard labels and
 * smoothing 0.  A row with u = 0 and gamma > 0 contributes loss 0 and gradient 0; the gradient is formed without a division by u.
 * dz NULL: loss only; gscale NULL: 1.  Evaluated in double and rounded to float once on store; one workgroup, thread b % 256 owns
 * row b, then a block fold in a fixed order: bit-reproducible.  Labels in [0, C) are the caller's contract; a row with a label
 * outside contributes loss 0 and gradient 0 (z and weight are never indexed by it). */
int mi355_ce_focal(const float* z, const int64_t* y, const float* weight, float* loss, float* dz, const float* gscale, int B,
                   int C, float gamma, mi355_stream_t s);
/* Knowledge distillation (Hinton et al. 2015; nothing in the reference): the losses above with a third operand, the logits v of a
 * frozen teacher, and a temperature T > 0.
 * Binary segmentation, z, t, v fp32 [B][per], n = B per, a = z / T, b = v / T, p_T = sigmoid(a), q = sigmoid(b), p = sigmoid(z):
 *   KD      = T^2 (1 / n) sum_i (q_i log(q_i / p_T,i) + (1 - q_i) log((1 - q_i) / (1 - p_T,i))),
 *             each element formed as softplus(-a) - softplus(-b) + (1 - q)(a - b)
 *   loss[0] = bce_weight mean(BCEWithLogits(z, t)) + dice_weight Dice(z, t; smooth, per_sample) + kd_weight KD
 *   loss[1] = the two hard terms alone,  loss[2] = KD (unweighted)
 *   dz_i    = gscale[0] (bce_weight (p_i - t_i) / n - (a_b t_i - c_b) p_i (1 - p_i) + kd_weight T (p_T,i - q_i) / n)
 * The Dice term, its per_sample variant, the target (used as it is) and `state` are those of mi355_seg_loss_fwd / _bwd.  p_T and q
 * come from one device function: v == z gives loss[2] = 0 and loss[0], dz with the bits of the same call with kd_weight = 0.
 *   mi355_kd_seg_rows: rows of EIGHT floats `partial` must hold (16-byte aligned); a function of (B, per) alone.
 *   mi355_kd_seg_fwd:  one pass over z, t and v (16-byte accesses when per % 4 == 0 and all three are 16-byte aligned), a
 *     one-workgroup finalize in double; leaves loss[0 .. 2] and the pair (a_b, c_b) of sample b in state[2 b], state[2 b + 1].
 *   mi355_kd_seg_bwd:  one pass from the `state` the forward left (same B, per, weights and T); gscale NULL = 1.
 * kd_weight = 0: v may be NULL and is never read.  Deterministic: no floating-point atomics, every fold in a fixed order; nothing
 * is allocated and nothing synchronises.  B <= 65535; weights and smooth >= 0; T finite and > 0. */
int mi355_kd_seg_rows(int B, long long per);
int mi355_kd_seg_fwd(const float* z, const float* t, const float* v, int B, long long per, float bce_weight, float dice_weight,
                     float smooth, int per_sample, float kd_weight, float temperature, float* partial, float* state, float* loss,
                     mi355_stream_t s);
int mi355_kd_seg_bwd(const float* z, const float* t, const float* v, int B, long long per, float bce_weight, float kd_weight,
                     float temperature, const float* state, const float* gscale, float* dz, mi355_stream_t s);
/* Classifiers, z, v fp32 [B][C], hard labels y, t[b][c] = (1 - smoothing) [c == y_b] + smoothing / C:
 *   hard     = (1 / B) sum_b sum_c weight[c] t[b][c] (-log_softmax(z_b)[c])                 (mi355_ce_mix's hard-label case)
 *   KD       = T^2 (1 / B) sum_b KL(softmax(v_b / T) || softmax(z_b / T))
 *   loss[0]  = hard_weight hard + kd_weight KD,  loss[1] = hard,  loss[2] = KD
 *   dz[b][c] = (gscale[0] / B) (hard_weight (softmax(z_b)[c] sum_k weight[k] t[b][k] - weight[c] t[b][c])
 *                               + kd_weight T (softmax(z_b / T)[c] - softmax(v_b / T)[c]))
 * weight NULL: all ones; dz NULL: loss only; gscale NULL: 1; kd_weight = 0: v may be NULL and is never read.  v == z gives
 * loss[2] = 0.  Evaluated in double (inputs and T widened, exp / log in double) and rounded to float once on store; one workgroup,
 * thread b % 256 owns row b, then a block fold in a fixed order: bit-reproducible.  Labels only select a class, never index. */
int mi355_ce_distill(const float* z, const int64_t* y, const float* v, const float* weight, float* loss, float* dz,
                     const float* gscale, int B, int C, float smoothing, float hard_weight, float kd_weight, float temperature,
                     mi355_stream_t s);
/* Multi-class segmentation (nothing in the reference, whose losses and metrics are binary): per-pixel softmax cross-entropy +
 * per-class soft Dice, and the argmax / confusion-matrix pass of the metrics.  Logits z fp32 [N][C][HW] (the NCHW map of the
 * K-channel heads; a plan's dout has the same layout), labels y uint8 [N][HW], 2 <= C <= 16, N <= 65535, HW <= 2^30.
 * ignore_index is -1 (none) or in [C, 255]; a pixel is valid when its label is in [0, C), and EVERY label >= C is ignored, whether
 * or not it equals ignore_index: nothing is indexed by it.  weight fp32 [C] on the device or NULL (all ones); the weights must not
 * be negative (device memory: not checked).  With p = softmax_c(z) at each pixel, sums over the valid pixels:
 *   CE     = sum w[y] (logsumexp(z) - z_y) / sum w[y]: torch.nn.functional.cross_entropy(z, y, weight, ignore_index) with
 *            class-index targets and its weighted-mean normalisation, EXCEPT that with sum w[y] = 0 (no valid pixel) CE and
 *            its gradient are 0 where torch returns NaN.  No label smoothing.
 *   dice_c = (2 I_c + smooth) / (P_c + T_c + smooth),  I_c = sum p_c [y = c],  P_c = sum p_c,  T_c = sum [y = c], the sums
 *            over the whole batch (per_sample = 0) or per image (per_sample = 1)
 *   Dice   = 1 - mean_{c in S} dice_c (per_sample: the mean over images of that); S = every class, or c >= 1 with
 *            include_background = 0; a class absent from the targets stays in the mean (the reference DiceLoss rule per class)
 *   loss[0] = ce_weight CE + dice_weight Dice,  loss[1] = CE,  loss[2] = Dice
 *   dz_k   = gscale[0] (ce_weight w[y] (p_k - [y = k]) / sum w + dice_weight p_k (g_k - sum_c g_c p_c)) at valid pixels, exactly
 *            +0.f at ignored ones; g_c = -(a_c [y = c] - b_c) [c in S] / |S| (/ N with per_sample), a_c = 2 / den_c,
 *            b_c = (2 I_c + smooth) / den_c^2, den_c = P_c + T_c + smooth.
 * Inputs are widened to double, exp / log evaluated in double, every sum taken in double in a fixed order, results rounded to
 * float once on store; no floating-point atomics: the same input gives the same bytes.
 *   mi355_mcseg_rows:      rows of MI355_MCSEG_ROW doubles `partial` must hold (-1 + last_error when out of range); a function of
 *     (N, HW) alone.  A workgroup walks chunks of 1024 pixels of one image; rows = N * min(ceil(HW / 1024), max(1, 2048 / N)).
 *   mi355_mcseg_loss_fwd:  one pass over z and y (16-byte plane loads, four pixels per lane, when HW % 4 == 0, z is 16-byte and
 *     y 4-byte aligned; one pixel per lane otherwise), a fold of each image's rows (one workgroup per image) and a one-workgroup
 *     finalize, each in a fixed order; leaves loss[0..3) and `state`, 2 + 2 N C doubles:
 *     1 / sum w (0 when no pixel is valid), sum w, then per (n, c) the pair (a_c, b_c) [c in S] / |S| (/ N with per_sample).
 *   mi355_mcseg_loss_bwd:  one pass from the `state` the forward left (same arguments); gscale = upstream gradient x loss scale
 *     on the device, NULL = 1.  It does not recompute the loss.
 *   mi355_mcseg_confusion: pred = the first maximum of z over c (v > best in ascending c, starting from -inf and class 0: ties go
 *     to the lower class, a NaN never wins); conf int32 [N][C][C] is cleared and conf[n][y][pred] counts the valid pixels (integer
 *     atomics: exact, order-independent); pred uint8 [N][HW] or NULL is written for every pixel, ignored ones included. */
#define MI355_MCSEG_ROW 50
int mi355_mcseg_rows(int N, long long HW);
int mi355_mcseg_loss_fwd(const float* z, const uint8_t* y, int N, int C, long long HW, const float* weight, int ignore_index,
                         float ce_weight, float dice_weight, float smooth, int per_sample, int include_background,
                         double* partial, double* state, float* loss, mi355_stream_t s);
int mi355_mcseg_loss_bwd(const float* z, const uint8_t* y, int N, int C, long long HW, const float* weight, int ignore_index,
                         float ce_weight, float dice_weight, const double* state, const float* gscale, float* dz,
                         mi355_stream_t s);
int mi355_mcseg_confusion(const float* z, const uint8_t* y, int N, int C, long long HW, int ignore_index, int32_t* conf,
                          uint8_t* pred, mi355_stream_t s);
/* Boundary loss (Kervadec et al., MIDL 2019; nothing in the reference): the mean of sigmoid(z) * phi, phi the signed
 * Euclidean distance map of the ground truth, rebuilt on the device for every batch.
 *   mi355_signed_dist2: target [B][H][W] fp32, binarised as target > thr -> sd2 int32 [B][H][W]: +min(dy^2 + dx^2) over
 *     the sample's foreground pixels at an outside pixel (>= 1), -min(dy^2 + dx^2) over its background pixels at an
 *     inside pixel (<= -1), 0 everywhere for a sample without foreground or without background (no boundary).  Pixels
 *     outside the image are NOT background (unlike the border rule of mi355_surface_distances).  Integer arithmetic,
 *     exact.  1 <= H, W <= 1024, 0 < B <= 65535; `ws` = mi355_sdist_ws_ints(B, H, W) int32 elements of scratch (-1 +
 *     last_error when the shape is out of range); ws and sd2 must not overlap.  Two launches, no allocation, no sync.
 *   mi355_boundary_loss_rows: floats `partial` must hold; a function of (B, per) alone.
 *   mi355_boundary_loss_fwd: with phi = sqrt(sd2) (sd2 > 0), -(sqrt(-sd2) - 1) (sd2 < 0), 0 (sd2 = 0), on fp32 logits
 *     z [B][per]:  loss[0] = (base ? base[0] : 0) + weight / (B per) * sum_i sigmoid(z_i) phi_i.  `base` is a device
 *     scalar (the regional loss the term is added to) or NULL.  One pass (16-byte accesses when per % 4 == 0 and z, sd2
 *     are 16-byte aligned) and a one-workgroup fold in double; no floating-point atomics, bit-reproducible.
 *   mi355_boundary_loss_bwd: dz_i (+)= gscale[0] * weight / (B per) * phi_i p_i (1 - p_i); gscale NULL = 1;
 *     accumulate != 0 adds the rounded term to what dz holds (another criterion's gradient in the same buffer),
 *     accumulate = 0 overwrites.
 * weight >= 0, B <= 65535. */
int mi355_sdist_ws_ints(int B, int H, int W);
int mi355_signed_dist2(const float* target, int B, int H, int W, float thr, int32_t* ws, long long ws_ints,
                       int32_t* sd2, mi355_stream_t s);
int mi355_boundary_loss_rows(int B, long long per);
int mi355_boundary_loss_fwd(const float* z, const int32_t* sd2, int B, long long per, float weight, const float* base,
                            float* partial, float* loss, mi355_stream_t s);
int mi355_boundary_loss_bwd(const float* z, const int32_t* sd2, int B, long long per, float weight, const float* gscale,
                            int accumulate, float* dz, mi355_stream_t s);
/* Segmented stable argsort (nothing in the reference): keys [S][len] fp32 -> perm [S][len] int32, perm[s][k] = the index
 * within segment s (0 .. len - 1) of its k-th smallest key.  The order is that of np.argsort(keys[s], kind="stable"):
 * ascending as floats, -0.0 == +0.0 (canonicalised before the bit pattern is taken), equal keys in ascending index,
 * -inf and +inf in their natural places.  NaN keys are unsupported as an order: the call still terminates, perm is
 * still a permutation of every segment, nothing outside perm and ws is written.
 *   mi355_segsort_tile:    keys one workgroup handles per pass; several workgroups share a segment longer than that.
 *   mi355_segsort_ws_ints: int32 elements of scratch `ws` (-1 + last_error when the shape is out of range).
 *   mi355_segsort_f32:     a least-significant-digit radix sort, four 8-bit passes of per-tile digit counts, a scan and
 *     a scatter that is stable by construction (ballots, no returning atomic; integer LDS adds only for the counts).
 *     Grid sizes depend on (S, len) alone; no allocation, no sync, no host read-back; bit-reproducible.  keys, ws and
 *     perm must not overlap.
 * 1 <= S <= 65535, len >= 1, S * len <= 2^26. */
int mi355_segsort_tile(void);
int mi355_segsort_ws_ints(int S, long long len);
int mi355_segsort_f32(const float* keys, int S, long long len, int32_t* ws, long long ws_ints, int32_t* perm,
                      mi355_stream_t s);
/* Lovasz hinge (Berman, Triki, Blaschko, CVPR 2018, Algorithm 1; nothing in the reference): the convex surrogate of the
 * Jaccard index, on fp32 logits z and targets t [S][len]; a segment is one image, or the whole batch with S = 1.
 *   mi355_lovasz_ws_ints: int32 elements of scratch `ws` (-1 + last_error when the shape is out of range).
 *   mi355_lovasz_fwd: y_i = t_i > thr, margin m_i = y_i ? z_i : -z_i, ranked ascending per segment by the sort above.
 *     With P the segment's positives and c_k those among ranks 0 .. k: I_k = P - c_k, U_k = P + (k + 1) - c_k and
 *     w_k = 1 / U_k (positive), I_k / ((U_k - 1) U_k) (negative, U_k > 1), 1 (negative, U_k = 1) — the Jaccard increment
 *     in closed form from the integers.  L_s = sum_k max(1 - m_(k), 0) w_k;
 *       loss[0] = (base ? base[0] : 0) + weight / S * sum_s L_s,
 *       coef_i  = weight / S * (y_i ? -1 : +1) w_rank(i) where 1 - m_i > 0, else 0        (fp32 [S * len]).
 *     Every term and fold in double, folds in a fixed order, coef and loss rounded to fp32 once; a NaN logit gives a NaN
 *     loss.  `base` is a device scalar (the regional loss the term is added to) or NULL.  No floating-point atomics.
 *   mi355_lovasz_bwd: dz_i (+)= gscale[0] * coef_i over n = S * len elements; gscale NULL = 1; accumulate != 0 adds the
 *     rounded term to what dz holds, accumulate = 0 overwrites.  One pass, 16-byte accesses when coef and dz are 16-byte
 *     aligned, the remainder element-wise.
 * weight >= 0; shape limits as for the sort. */
int mi355_lovasz_ws_ints(int S, long long len);
int mi355_lovasz_fwd(const float* z, const float* t, int S, long long len, float thr, float weight, const float* base,
                     int32_t* ws, long long ws_ints, float* coef, float* loss, mi355_stream_t s);
int mi355_lovasz_bwd(const float* coef, long long n, const float* gscale, int accumulate, float* dz, mi355_stream_t s);
/* Threshold-free evaluation (nothing in the reference): ROC-AUC, average precision, the ROC / precision-recall operating
 * points and the calibration of a classifier.
 *   mi355_rank_ws_ints: int32 elements of scratch `ws` (-1 + last_error when the shape is out of range).
 *   mi355_rank_metrics: fp32 scores [S][len], ranked ascending per segment by the sort above.  The positives come from
 *     exactly one of `target` (fp32 [S][len], y = target > thr) and `labels` (int32 [len], shared by the segments,
 *     y = (labels[i] == s): one-vs-rest without a one-hot array; thr is ignored); the other is NULL.  A tie group g is a
 *     run of equal scores (-0.0 == +0.0); A_g, B_g = the negatives, positives up to and including group g, A_0 = B_0 = 0.
 *       counts int64 [S][4] = P, N, U2 = sum_g (B_g - B_{g-1}) (A_g + A_{g-1}), T
 *         U2 is twice the Mann-Whitney statistic with ties counted half, an exact integer (<= 2^51); T the number of
 *         distinct scores.  AUROC = U2 / (2 P N) is the caller's, NaN when P = 0 or N = 0.
 *       ap double [S] = sum_g (p_g / P) tp_g / (tp_g + fp_g), p_g = B_g - B_{g-1}, tp_g = P - B_{g-1}, fp_g = N - A_{g-1}:
 *         the step-wise average precision; NaN when P = 0.  Double partials per tile, folded in a fixed order.
 *       thresholds fp32 [S][len], tp, fp int32 [S][len], npoints int32 [S]: the T operating points (score_g, tp_g, fp_g) in
 *         DESCENDING threshold order; only the first npoints[s] = T entries of a row are written.  All four NULL: skipped.
 *     No floating-point atomics, no allocation, no sync, no host read-back; bit-reproducible.  NaN scores are not an
 *     order: that segment's outputs are unspecified, every write stays in bounds and P + N == len.
 *   mi355_cls_calibration_ws_ints: int32 elements of scratch `ws` (-1 + last_error when an argument is out of range).
 *   mi355_cls_calibration: x fp32 [N][C] logits (is_prob = 0) or probabilities (is_prob != 0), labels int32 [N].  The
 *     softmax is evaluated in double after subtracting the row maximum; conf = the largest probability, pred = the first
 *     argmax, bin = min(bins - 1, max(0, ceil(conf * bins) - 1)) — the bins (k / M, (k + 1) / M] of Guo et al. 2017.
 *       bin_count, bin_correct int64 [bins]; bin_conf double [bins] = the sum of the confidences, folded in a fixed order
 *       out double [3] = mean NLL (logits: log sum_j exp(x_j - max) - (x_y - max)), mean multi-class Brier score
 *         sum_j (p_j - 1[j = y])^2, ECE = sum_m |bin_correct_m - bin_conf_m| / N
 *       scores_t fp32 [C][N] = the probabilities rounded to fp32 once, transposed: one segment per class for
 *         mi355_rank_metrics(labels).
 * Shape limits of mi355_rank_metrics as for the sort; N >= 1, 1 <= C <= 4096, N * C <= 2^26, 1 <= bins <= 1024. */
int mi355_rank_ws_ints(int S, long long len);
int mi355_rank_metrics(const float* scores, const float* target, const int32_t* labels, int S, long long len, float thr,
                       int32_t* ws, long long ws_ints, int64_t* counts, double* ap, float* thresholds, int32_t* tp,
                       int32_t* fp, int32_t* npoints, mi355_stream_t s);
int mi355_cls_calibration_ws_ints(int N, int C, int bins);
int mi355_cls_calibration(const float* x, int N, int C, int is_prob, const int32_t* labels, int bins, int32_t* ws,
                          long long ws_ints, int64_t* bin_count, int64_t* bin_correct, double* bin_conf, double* out,
                          float* scores_t, mi355_stream_t s);
/* Resampling statistics (nothing in the reference): bootstrap weights, the evaluation figures on the resampled multiset,
 * percentile intervals over the replicates and DeLong's components.  A resample is a row of int32 weights, never a copy of
 * the data: counts int32 [R1][n], R1 = R + 1, counts[r][i] = how often replicate r drew sample i.  ROW 0 IS THE IDENTITY
 * (every weight 1), so row 0 of every output below is the point estimate, computed by the same code.  Weights a caller
 * supplies itself must be >= 0 with every row sum <= 2^26 (mi355_boot_counts' rows sum to n): the kernels add them in
 * int32 and in the halves of one int64, and the values live on the device, so the launchers cannot check them.
 *   mi355_boot_counts_lds_max: the longest row whose histogram is kept in LDS; longer rows use global integer adds.
 *   mi355_boot_counts: replicate r = 1 .. R makes n draws; draw k is word k & 3 of Philox4x32-10 (Salmon et al., SC 2011;
 *     multipliers 0xD2511F53, 0xCD9E8D57, Weyl constants 0x9E3779B9, 0xBB67AE85) with counter (k >> 2, r, 0, 0) and key
 *     (seed & 0xffffffff, seed >> 32); idx = (uint64(word) * n) >> 32 and counts[r][idx] += 1, so every row sums to n.  An
 *     index is hit by floor(2^32 / n) or that + 1 of the 2^32 words: the map's bias is at most n / 2^32 relative (< 1.6 %
 *     at the largest n, 1e-6 at n = 4096).  Integer adds only: the counts do not depend on the order of the adds.
 *   mi355_boot_rank: mi355_rank_metrics on the resampled multiset; scores / target / labels / thr as there.  The segments
 *     are sorted and their tie groups found once; per (replicate, segment) the weights are gathered in rank order and
 *     scanned.  With A_g, B_g the WEIGHTED negatives / positives up to and including group g:
 *       counts64 int64 [R1][S][3] = P, N, U2 = sum_g (B_g - B_{g-1}) (A_g + A_{g-1})   exact, U2 <= 2 n^2
 *       ap double [R1][S] = sum_g (p_g / P) tp_g / (tp_g + fp_g) over the groups with p_g > 0; NaN when P = 0.  Double
 *         partials per tile of the sort, folded in the order of mi355_rank_metrics: row 0 equals its ap to the bit.
 *     AUROC = U2 / (2 P N) is the caller's, NaN when P N = 0.  `ws` = mi355_boot_rank_ws_ints(S, len) int32 elements.
 *   mi355_boot_confusion: cm int64 [R1][C][C], cm[r][y][p] = the weight of the samples with labels = y and pred = p (rows
 *     the truth, columns the prediction); 1 <= C <= 64.  The class ids live on the device: a sample with pred or labels
 *     outside 0 .. C - 1 is skipped and its weight counted in bad int64 [R1].  With C = 2 and two models' 0 / 1
 *     correctness as (pred, labels), row 0 is their McNemar table.
 *   mi355_boot_sums: values double [M][n] -> sum double [R1][M] = sum_i counts[r][i] values[m][i] and weight int64 [R1][M]
 *     = sum_i counts[r][i], both over the samples whose value is not NaN.  Folded in a fixed order.
 *   mi355_boot_interval: reps double [R1][K] -> out double [K][6] = point (row 0), mean, se, lo, hi, valid over rows
 *     1 .. R, R <= 8192, NaN replicates counted out (valid = those left).  mean and se (ddof = 1) by the two-pass formula in
 *     a fixed order over the sorted replicates; lo, hi = the lo_q, hi_q quantiles by numpy's method="linear".  The
 *     percentile interval is the only kind.  valid = 0: NaN; valid = 1: se NaN, lo = hi.
 *   mi355_delong: scores fp32 [M][C][n] (model, class, sample), labels int32 [n]; the positives of segment (m, c) are
 *     labels == c.  DeLong, DeLong and Clarke-Pearson's (1988) structural components from the sort, after Sun and Xu (2014):
 *       v2 int64 [M][C][n]: a positive in tie group g: A_g + A_{g-1} (twice the negatives below it, ties half); a negative:
 *         2 (P - B_g) + (B_g - B_{g-1}) (twice the positives above it, ties half).  Exact.
 *       pnu int64 [M][C][3] = P, N, U2
 *       cov double [C][M][M] = cov(V10_a, V10_b) / P + cov(V01_a, V01_b) / N with V10 = v2 / (2 N) on the positives, V01 =
 *         v2 / (2 P) on the negatives, ddof = 1, two-pass, fixed order; var double [M][C] its diagonal.  NaN where P < 2
 *         or N < 2.
 *     `ws` = mi355_delong_ws_ints(M, C, n) int32 elements.
 * Every launcher validates before it touches the device (MI355_ERR_ARG + last_error; the *_ws_ints give -1 + last_error).
 * No floating-point atomics, no allocation, no sync, no host read-back; grids depend on the shapes alone; bit-reproducible.
 * R >= 1, n >= 1, R1 * n <= 2^26; segments as for the sort (S * n <= 2^26). */
int mi355_boot_counts_lds_max(void);
int mi355_boot_counts(uint64_t seed, int R, long long n, int32_t* counts, mi355_stream_t s);
int mi355_boot_rank_ws_ints(int S, long long len);
int mi355_boot_rank(const float* scores, const float* target, const int32_t* labels, int S, long long len, float thr,
                    const int32_t* counts, int R1, int32_t* ws, long long ws_ints, int64_t* counts64, double* ap,
                    mi355_stream_t s);
int mi355_boot_confusion(const int32_t* pred, const int32_t* labels, long long n, int C, const int32_t* counts, int R1,
                         int64_t* cm, int64_t* bad, mi355_stream_t s);
int mi355_boot_sums(const double* values, int M, long long n, const int32_t* counts, int R1, double* sum, int64_t* weight,
                    mi355_stream_t s);
int mi355_boot_interval(const double* reps, int R1, int K, double lo_q, double hi_q, double* out, mi355_stream_t s);
int mi355_delong_ws_ints(int M, int C, long long n);
int mi355_delong(const float* scores, const int32_t* labels, int M, int C, long long n, int32_t* ws, long long ws_ints,
                 int64_t* v2, int64_t* pnu, double* var, double* cov, mi355_stream_t s);

/* ---- post-hoc calibration (utils/calibrate.py; nothing in the reference): the temperature of a classifier fitted on held-out
 * logits (Guo et al. 2017) and the mask threshold of a segmenter with the best mean Dice over a list of candidates ---------- */
/* Temperature.  x fp32 [N][C] logits, labels int32 [N]; N >= 1, 2 <= C <= 4096, N * C <= 2^26.  With beta = 1 / T the mean NLL
 *     g(beta) = mean_i(log sum_j exp(beta x_ij - m_i) + m_i - beta x_iy),  m_i = max_j beta x_ij
 * is convex, g' = mean_i(E_p[x_i] - x_iy), g'' = mean_i Var_p[x_i], p = softmax(beta x_i): evaluated in double relative to the
 * row maximum, row partials folded in a fixed order.
 *   mi355_temperature_fit_ws_ints: int32 elements of scratch `ws` (-1 + last_error when the shape is out of range).
 *   mi355_temperature_fit: a safeguarded Newton iteration on g' over the bracket [2^-6, 2^6], all of it on the device: the host
 *     enqueues a fixed schedule of 64 (evaluate, update) kernel pairs and never reads beta; once the status is set the
 *     remaining kernels return at once.  Evaluation 1 is at beta = 1.  Evaluation 2 is at the end of the bracket that g'(1)
 *     points to (2^6 when g'(1) < 0), which either is the clamp or leaves a bracket with a sign change of g'.  From then on
 *     the bracket shrinks by the sign of g' and the next beta is beta - g' / g'', replaced by the bracket's geometric mean when
 *     g'' <= 0 or the step leaves the bracket.  It stops AT the evaluated beta when the step |dbeta| <= 2^-40 beta or
 *     g' = 0, or after 64 evaluations.
 *       state double [8] = beta, T = 1 / beta, mean NLL at beta = 1, mean NLL at beta, g'(beta), g''(beta), evaluations, status
 *       status 0: converged;  1: lower clamp (g' >= 0 at 2^-6), beta = 2^-6;  2: upper clamp (g' <= 0 at 2^6, e.g. separable
 *         data, where g' underflows to 0), beta = 2^6;  3: flat (g'' = 0 at beta = 1, e.g. every row constant), beta = 1;
 *         4: the evaluation cap, or g' is a NaN (NaN logits; a label outside 0 .. C - 1 reads nothing and counts as a NaN).
 *   mi355_temperature_eval: one evaluation at beta_dev[0] (device memory), by the kernels and in the fold order of the fit:
 *     out double [3] = g, g', g'' — at the fit's beta its state[3..5], bit for bit.  `ws` as for the fit.
 *   mi355_logits_scale: y[i] = (float)((double)x[i] * beta_dev[0]) over N * C elements (C >= 1), beta read from device memory —
 *     `state` of the fit — so nothing is read back between fit and apply.  16-byte accesses when x and y are 16-byte aligned.
 * Threshold sweep.  scores, target fp32 [B][len], thr fp32 [K] STRICTLY ASCENDING (the values live on the device: not checked);
 * 1 <= B <= 65535, 1 <= len <= 2^24, B * len <= 2^26, 1 <= K <= 1024.  v = scores[b][i], or with is_logit != 0
 * 1.f / (1.f + __expf(-v)) (mi355_seg_counts' expression); a pixel is positive where target > tthr; its bin is
 * #{k : v > thr[k]} — strict, as in mi355_seg_counts; a NaN is in bin 0.
 *   mi355_thr_sweep_chunk: pixels per workgroup; a longer image spans several, whose integer histograms are added.
 *   mi355_thr_sweep_ws_ints: int32 elements of scratch `ws` (-1 + last_error when the shape is out of range).
 *   mi355_thr_sweep: tp int32 [B][K], fp int32 [B][K], pos int32 [B]: tp[b][k] = #{positive pixels with v > thr[k]}, fp[b][k]
 *     the same over the negative pixels, pos[b] the positives.  tp[b][k] is mi355_seg_counts' counts[b][0] at thr[k] when
 *     tthr = thr[k], tp + fp its counts[b][1].  Exact integers.
 *   mi355_thr_sweep_fold: per candidate k and image b, in double, with pp = tp + fp and tt = pos:
 *       Dice = (2 tp + 1e-7) / (pp + tt + 1e-7),  IoU = (tp + 1e-7) / (pp + tt - tp + 1e-7)    (utils/tester.py, without x 100)
 *     acc double [2][K] (+)= the B images' Dice (row 0) and IoU (row 1) in image order, n_images int64 [1] += B.  The caller
 *     zeroes both before the first batch: a validation set of many batches accumulates in one fixed order.
 *   mi355_thr_sweep_pick: out_k int32 [1] = the lowest k with the largest mean Dice acc[0][k] / n_images (0 when nothing was
 *     folded); out_d double [4] = the mean Dice and mean IoU at out_k, then at k_ref — the candidate equal to the current
 *     operating point, -1 <= k_ref < K; NaN for -1.
 * No floating-point atomics (integer LDS atomics in the histogram), no allocation, no sync, no host read-back; bit-reproducible. */
int mi355_temperature_fit_ws_ints(int N, int C);
int mi355_temperature_fit(const float* x, int N, int C, const int32_t* labels, int32_t* ws, long long ws_ints, double* state,
                          mi355_stream_t s);
int mi355_temperature_eval(const float* x, int N, int C, const int32_t* labels, const double* beta_dev, int32_t* ws,
                           long long ws_ints, double* out, mi355_stream_t s);
int mi355_logits_scale(const float* x, int N, int C, const double* beta_dev, float* y, mi355_stream_t s);
int mi355_thr_sweep_chunk(void);
int mi355_thr_sweep_ws_ints(int B, long long len, int K);
int mi355_thr_sweep(const float* scores, const float* target, int B, long long len, const float* thr, int K, int is_logit,
                    float tthr, int32_t* ws, long long ws_ints, int32_t* tp, int32_t* fp, int32_t* pos, mi355_stream_t s);
int mi355_thr_sweep_fold(const int32_t* tp, const int32_t* fp, const int32_t* pos, int B, int K, double* acc, int64_t* n_images,
                         mi355_stream_t s);
int mi355_thr_sweep_pick(const double* acc, const int64_t* n_images, int K, int k_ref, double* out_d, int32_t* out_k,
                         mi355_stream_t s);

/* ---- optimiser on flat fp32 buffers (utils/helpers.py:251,304,332-336) ---------------------- */
/* sumsq partials of a flat gradient buffer; nblocks = mi355_rowreduce_blocks(n). */
int mi355_sumsq_partial(const float* g, float* partial, long long n, mi355_stream_t s);
/* norm[0] = sqrt(sum partial) * inv_scale * (dev_scale ? dev_scale[0] : 1); coef[0] = min(1, max_norm/(norm+1e-6))
 * (clip_grad_norm_); found_inf[0] = 1 if the norm is not finite; otherwise step[0] += 1 (the optimiser step counter).
 * dev_scale: optional device-side factor — the loss scaler's 1/scale (GradScaler.unscale_, helpers.py:329). */
int mi355_clip_coef(const float* partial, int nblocks, float max_norm, float inv_scale, const float* dev_scale,
                    float* norm, float* coef, float* found_inf, int32_t* step, mi355_stream_t s);
/* AdamW, decoupled decay; g is multiplied by coef[0]*inv_scale*(dev_scale ? dev_scale[0] : 1) first; skipped when
 * found_inf[0] != 0 (GradScaler.step).  step_count is read from device memory (graph-capturable). */
int mi355_adamw(float* p, const float* g, float* m, float* v, long long n, const float* lr, float beta1,
                float beta2, float eps, float wd, const float* coef, float inv_scale, const float* dev_scale,
                const float* found_inf, const int32_t* step, mi355_stream_t s);
/* step[0] += 1 unless found_inf[0] != 0 (found_inf may be NULL). */
int mi355_step_tick(int32_t* step, const float* found_inf, mi355_stream_t s);
/* torch.amp.GradScaler.update() (helpers.py:285,336) on device state: found_inf -> scale *= backoff, tracker = 0;
 * otherwise ++tracker == interval -> scale *= growth, tracker = 0;  inv_scale = 1/scale. */
int mi355_amp_update(float* scale, float* inv_scale, int32_t* growth_tracker, const float* found_inf, float growth,
                     float backoff, int interval, mi355_stream_t s);
int mi355_fill_f32(float* p, float v, long long n, mi355_stream_t s);

/* ---- weight averaging along the optimiser trajectory (mi355/averaging.py; nothing in the reference): EMA (Mean Teacher, timm's
 * ModelEmaV2) and the equal-weight average of SWA (Izmailov et al. 2018) over flat fp32 buffers.  With t = count[0], the number
 * of updates INCLUDING this one (the caller ticks it first with mi355_step_tick under the same found_inf):
 *   mode 0 (EMA):   d = warmup > 0 ? min(decay, (1 + t) / (warmup + t)) : decay;  a = 1 - d     (timm's warm-up of the decay)
 *   mode 1 (equal): a = 1 / t;  t == 1 COPIES p (avg + 1 * (p - avg) is not p in floating point)
 * a is formed in double (decay and warmup widened first) and rounded to float once.  Then, in fp32, every operation rounded on
 * its own (no FMA) and nothing atomic:
 *   diff = p[i] - avg[i];   avg[i] = diff == 0 ? avg[i] : avg[i] + a * diff
 * (the select keeps avg's bits where p equals it: -0 + a * +0 would be +0; padding and frozen parameters therefore never move).
 * Nothing is written when found_inf != NULL && found_inf[0] != 0 (AdamW skipped that step; mi355_step_tick did not count it), or
 * when t < 1.  tests/averaging_ref.py restates all of it in numpy float32; the same input gives the same bytes. ------------- */
/* One flat range of n floats.  16-byte accesses where avg and p share their offset within 16 bytes, between a scalar head up to
 * the first 16-byte boundary and a scalar tail; scalar throughout otherwise.  avg == p or disjoint ranges; n == 0: OK, no launch.
 * 12 bytes of traffic per element. */
int mi355_avg_update(float* avg, const float* p, long long n, int mode, float decay, float warmup, const int32_t* count,
                     const float* found_inf, mi355_stream_t s);
/* Elements one sweep of mi355_avg_update's grid covers on the 16-byte path (a longer range is strided): for tests of the stride. */
int mi355_avg_update_grid_elems(void);
/* The same arithmetic over `rows` rows {avg pointer, p pointer, n} of three int64 words each, held in DEVICE memory (the
 * BatchNorm running_mean / running_var buffers of a model: one launch for all of them).  Each row picks the 16-byte or the
 * scalar path from its own two pointers; a row with n <= 0 or a null pointer is skipped.  0 <= rows <= 65535; rows == 0: OK,
 * no launch.  Rows must not overlap one another. */
int mi355_avg_update_table(const int64_t* table, int rows, int mode, float decay, float warmup, const int32_t* count,
                           const float* found_inf, mi355_stream_t s);
/* dst[i] <-> src[i] for every row {dst pointer, src pointer, n} of such a table (fp32 words moved as they are: any bit pattern
 * survives); rows must not overlap one another or themselves (dst == src: skipped).  Swapping twice is the identity. */
int mi355_swap_table(const int64_t* table, int rows, mi355_stream_t s);
/* Bias correction of BatchNorm running statistics that were accumulated from ZERO with mi355_bn_finalize's recurrence
 * r = (1 - momentum) r + momentum b: rows {running pointer (fp32 [C]), nbt pointer (int64 [1]), C}; with k = *nbt,
 *   running[c] = (float)(running[c] / (1 - (1 - momentum)^k))     in double, momentum widened first
 * which makes running the exponentially weighted MEAN of the k batch statistics.  k == 0 leaves the row untouched (that
 * BatchNorm never ran).  0 < momentum <= 1. */
int mi355_bn_debias_table(const int64_t* table, int rows, float momentum, mi355_stream_t s);

/* AdaptiveAvgPool2d((OH,OW)) + Flatten of the torchvision VGG head (helpers.py:158-166 loads `vgg16_bn`):
 * NHWC `dtype` activations -> fp32 [N][C*OH*OW] in NCHW flatten order; backward writes (does not accumulate) dx. */
int mi355_adaptive_avgpool_fwd(const void* x, int ldx, float* y, int N, int H, int W, int C, int OH, int OW, int dtype,
                               mi355_stream_t s);
int mi355_adaptive_avgpool_bwd(const float* dy, void* dx, int lddx, int N, int H, int W, int C, int OH, int OW, int dtype,
                               mi355_stream_t s);

/* ---- input pipeline on the GPU (utils/trainer.py:52-115 Albumentations transforms; utils/dataset.py:100-134) ----------- */
/* dst[n][y][x][c] (uint8) = sample of src[n] ([Hs][Ws][C] uint8, C <= 4) at (sx, sy) = m[n] (2x3, row-major) applied to the dst
 * pixel (x, y): bilinear with cv2's rounding, or nearest; border = replicate (A.Resize) or reflect-101 (A.ShiftScaleRotate). */
int mi355_warp_u8(const uint8_t* src, int N, int Hs, int Ws, int C, const float* m, uint8_t* dst, int H, int W, int nearest,
                  int reflect, mi355_stream_t s);
/* out[n][c][y][x] (fp32 NCHW, what ToTensorV2 yields) = (clip(round(alpha_n*v + beta_n*255)) / 255 - mean[c]) / std[c];
 * bc = [N][2] (alpha, beta) or NULL (A.RandomBrightnessContrast off); mean == NULL: v / 255 (masks, dataset.py:126). */
int mi355_normalize_u8(const uint8_t* src, int N, int H, int W, int C, const float* bc, const float* mean, const float* stdv,
                       float* out, mi355_stream_t s);

/* ---- elastic deformation (Simard et al. 2003; A.ElasticTransform — not in the reference's pipelines, an optional stage of ours) ---- */
/* Separable 1-D correlation of `planes` fp32 planes [planes][H][W], along H then along W (scipy.ndimage's axis order):
 * per axis out[i] = sum_{k = 0 .. 2 radius} taps[k] * ext(in)[i + k - radius], ext = scipy's mode='reflect' (half-sample
 * symmetric, d c b a | a b c d | d c b a, period 2n: radius may exceed the extent many times).  taps: 2 radius + 1 fp32 values on
 * the device, any values (the kernel knows nothing about Gaussians); 0 <= radius <= 1024; tmp: scratch of planes H W floats (holds
 * the H pass); src, tmp and dst must differ.  fp32 FMA chain in ascending k per output, no atomics: bit-reproducible.  Two launches. */
int mi355_sepblur_reflect_f32(const float* src, int planes, int H, int W, const float* taps, int radius, float* tmp, float* dst,
                              mi355_stream_t s);
/* mi355_warp_u8 with a displacement field: field [N][2][H][W] fp32 at destination resolution (plane 0 dx, plane 1 dy), alpha [N]
 * fp32.  For destination pixel (x, y) of sample n, in fp32 without contraction and in this order,
 *   px = x + alpha[n] * dx(x, y);  py = y + alpha[n] * dy(x, y);  sx = m0 * px + m1 * py + m2;  sy = m3 * px + m4 * py + m5,
 * then mi355_warp_u8's sampling of (sx, sy) (the same device function): out(p) = src(M (p + alpha d(p))), the elastic displacement
 * applied after the affine map in ONE interpolation.  alpha[n] = 0 gives mi355_warp_u8's bytes.  src and dst must differ. */
int mi355_warp_field_u8(const uint8_t* src, int N, int Hs, int Ws, int C, const float* m, const float* field, const float* alpha,
                        uint8_t* dst, int H, int W, int nearest, int reflect, mi355_stream_t s);

/* ---- CLAHE (contrast-limited adaptive histogram equalisation; A.CLAHE / cv2.createCLAHE — not in the reference's pipelines, an
 * optional stage of ours).  The rules restate OpenCV's clahe.cpp; byte parity with cv2 itself has not been checked. --------------- */
/* src: [N][H][W][C] uint8 interleaved, C = 1 or 3; every channel plane of every sample is equalised on its own.
 * Padding: a plane with H % gy == 0 and W % gx == 0 is used as is; otherwise it is extended at the bottom by gy - H % gy rows AND on
 * the right by gx - W % gx columns (a side that divides evenly still gets a full gy or gx: OpenCV's quirk), mirrored without
 * repeating the edge pixel (BORDER_REFLECT_101: index i >= n reads 2 (n - 1) - i).  Tile th x tw = padded H / gy x padded W / gx,
 * area = th tw.  MI355_ERR_ARG: a pad above H - 1 or W - 1, area > 2^24, a grid side outside 1 .. 64.
 * Per tile, in integers: h = 256-bin histogram of the tile's pixels of the padded plane; with clip_count = lim > 0 (the caller's
 * max(int(clip area / 256), 1), in double; 0 = no clipping): excess = sum max(h - lim, 0), h = min(h, lim), h += excess / 256, and
 * with res = excess % 256 != 0 and step = max(256 / res, 1), bins 0, step, 2 step, ... get +1, stopping after res bins or at bin 255;
 * luts[n][c][ty][tx][v] = sat_u8(rint(float(sum_{u <= v} h[u]) * (255.f / float(area)))): one fp32 multiply, rounded half to even.
 * Integer LDS atomics and an integer scan: the order of the atomics cannot change a byte. */
int mi355_clahe_lut_u8(const uint8_t* src, int N, int H, int W, int C, int gy, int gx, int clip_count /* lim, 0 = no clipping */,
                       uint8_t* luts /* [N][C][gy][gx][256] */, mi355_stream_t s);
/* dst[n][y][x][c] = the bilinear blend of the four neighbouring tiles' LUTs at v = src[n][y][x][c] (tile geometry as above; only
 * the H x W pixels of the unpadded plane are written).  fp32, every operation rounded on its own, no FMA:
 *   inv_tw = 1.f / tw; txf = x * inv_tw - 0.5f; tx1 = floor(txf); xa = txf - tx1; xa1 = 1.f - xa; then tx1 = max(tx1, 0),
 *   tx2 = min(tx1 + 1, gx - 1) (tx1 + 1 taken before the clamp of tx1); the same in y;
 *   dst = sat_u8(rint((L[ty1][tx1][v] * xa1 + L[ty1][tx2][v] * xa) * ya1 + (L[ty2][tx1][v] * xa1 + L[ty2][tx2][v] * xa) * ya)).
 * luts: [N][C][gy][gx][256] as mi355_clahe_lut_u8 writes them (any bytes are accepted).  src and dst must differ. */
int mi355_clahe_apply_u8(const uint8_t* src, int N, int H, int W, int C, int gy, int gx, const uint8_t* luts,
                         uint8_t* dst, mi355_stream_t s);

/* ---- PNG files -> uint8 batch on the host (utils/dataset.py:55,101-102: PIL Image.open(path).convert("RGB" | "L")) ----------- */
/* Header fields of a PNG held in memory.  MI355_ERR_UNSUPPORTED (fields still filled) for an unknown interlace method or more
 * than 32768 pixels per side. */
int mi355_png_info(const uint8_t* file, long long nbytes, int* W, int* H, int* color_type, int* bit_depth);
/* out[H][W][channels] uint8 = what PIL yields for .convert("RGB") (channels = 3) or .convert("L") (channels = 1): gray replicated,
 * alpha dropped, palette looked up, 1/2/4-bit gray scaled to 0..255, RGB -> L by (19595 R + 38470 G + 7471 B + 0x8000) >> 16;
 * 16-bit RGB / RGBA / gray+alpha keep the high byte, 16-bit gray (PIL mode I;16) SATURATES at 255; Adam7-interlaced files too. */
int mi355_png_decode(const uint8_t* file, long long nbytes, int channels, uint8_t* out, long long out_bytes);
/* n files of one size W x H into out + i * stride (a pinned host batch), decoded by `threads` native threads. */
int mi355_png_decode_batch(const uint8_t* const* files, const long long* nbytes, int n, int channels, uint8_t* out,
                           long long stride, int W, int H, int threads);

/* ---- joint inference pipeline glue (utils/pipeline.py:324-357 classify, 359-418 process_image) ---------- */
/* pred[b] = argmax_c logits[b][c] (first maximum), conf[b] = 100 * max softmax; kept[0..n_kept) = the batch indices
 * with pred == keep_class, in order.  B <= 1024. */
int mi355_cls_decide(const float* logits, int B, int C, int keep_class, int32_t* pred, float* conf, int32_t* kept,
                     int32_t* n_kept, mi355_stream_t s);
/* y[i] = x[idx[i]], rows of `row` fp32 elements (row % 4 == 0): compacts the kept images. */
int mi355_gather_rows(const float* x, const int32_t* idx, int n, long long row, float* y, mi355_stream_t s);
/* out[idx[i]][p] = sigmoid(logit[i][p]) > thr ? 255 : 0 (pipeline.py:350-352); out is [B][per] uint8, zeroed by the caller. */
int mi355_mask_scatter(const float* logit, const int32_t* idx, int n, long long per, float thr, uint8_t* out,
                       mi355_stream_t s);

/* ---- test-time augmentation (utils/tta.py; nothing in the reference).  A view is (angle, scale, hflip) about the image centre; the
 * host forms d2s (view pixel -> the source location it shows) and s2d (source pixel -> its place in the view), 2x3 row-major.  In
 * all three kernels every fp32 operation is rounded on its own (no FMA), nothing is atomic and every sum runs in a fixed order:
 * outputs are bit-identical run to run (tests/tta_ref.py restates them in numpy float32). -------------------------------------- */
/* dst[n][c][y][x] (fp32 NCHW, like src) = bilinear sample of src[n][c] at sx = (m0 x + m1 y) + m2, sy = (m3 x + m4 y) + m5, x and y
 * converted to float, m = m[n] ([N][6]): fx = floor(sx), ax = sx - fx, taps at fx, fx + 1 (likewise y) under reflect-101, and
 * top = a00 (1 - ax) + a01 ax; bot = a10 (1 - ax) + a11 ax; out = top (1 - ay) + bot ay: mi355_warp_u8's reflect-mode sampling
 * without the rounding to bytes.  src and dst must differ. */
int mi355_warp_f32(const float* src, int N, int C, int H, int W, const float* m, float* dst, mi355_stream_t s);
/* z: fp32 [K][N][H][W], the one-channel logit maps of K <= 16 views; s2d: [K][6].  For pixel q = (x, y) of sample n, in order
 * k = 0 .. K - 1: p = s2d_k q (evaluated as above); view k is VALID at q iff 0 <= px <= W - 1 and 0 <= py <= H - 1; then v_k = the
 * bilinear sample of z[k][n] at p (formula above; the taps fx + 1 / fy + 1 clamped to the map, where their weight is 0), and with
 * prob != 0 v_k = sigmoid(v_k) (mi355_mask_scatter's expression).  Over the valid views, cnt of them:
 *   mean[n][q] = (0 + v_k summed in order k) / (float)cnt;  var[n][q] = (sum in order k of (v_k - mean)^2) / (float)cnt (population)
 *   votes[n][0][q] = #{valid k: v_k > thr (prob) or sigmoid(v_k) > thr (otherwise)}, votes[n][1][q] = cnt   (uint8 [N][2][H][W])
 *   mask[idx ? idx[n] : n][q] = 255 where mean > thr (prob) or sigmoid(mean) > thr (otherwise), else 0  (mi355_mask_scatter's rule:
 *   K = 1, the identity and prob = 0 give its bytes)
 * var, votes, mask, idx may be NULL (skipped; idx: rows in place).  A pixel with no valid view gets 0 / 0: pass the identity as one
 * view.  Known limit: within about 2 px of the border a valid view's taps may hold content the view got by reflection. */
int mi355_tta_fold(const float* z, int K, int N, int H, int W, const float* s2d, int prob, float thr, const int32_t* idx, float* mean,
                   float* var, uint8_t* votes, uint8_t* mask, mi355_stream_t s);
/* logits: [K][B][C], K <= 16, B <= 1024.  softmax_k = mi355_cls_decide's: e_c = expf(z_c - max z), den = sum_c e_c in ascending c.
 *   probs[b][c] = (0 + e_c / den summed in order k) / (float)K;  pred[b] = its first maximum;
 *   conf[b] = (0 + (100 e_pred) / den summed in order k) / (float)K  (= 100 probs[b][pred] up to rounding; formed this way so that
 *   K = 1 is mi355_cls_decide's 100 / den bit for bit);  agree[b] = #{k: first maximum of logits[k][b] == pred[b]};
 * kept / n_kept as in mi355_cls_decide (same order, same padding contract). */
int mi355_cls_tta_decide(const float* logits, int K, int B, int C, int keep_class, float* probs, int32_t* pred, float* conf,
                         int32_t* agree, int32_t* kept, int32_t* n_kept, mi355_stream_t s);

/* ---- sliding-window inference (utils/sliding.py; nothing in the reference).  A batch kept at a higher resolution is cut into
 * overlapping T x T tiles on a grid of Py row starts ys[] and Px column starts xs[]: tile p = iy * Px + ix of sample n has its
 * top-left corner at (ys[iy], xs[ix]).  ys and xs are HOST pointers (int32, 1 <= Py, Px <= 64): the launcher validates them
 * (strictly ascending, ys[0] == 0, ys[Py - 1] == H - T, every gap <= T so that no pixel is uncovered; likewise xs against W) and
 * passes them to the kernel by value; everything else is device memory.  In both kernels every fp32 operation is rounded on its
 * own (no FMA), nothing is atomic and every sum runs in a fixed order: outputs are bit-identical run to run (tests/sliding_ref.py
 * restates them in numpy float32).  T < 1, T > H, T > W, M < 1, N < 1, a NULL required pointer or invalid starts: an error from
 * the launcher, nothing is launched.  So is a grid on which more than 255 tiles cover one pixel (the most starts within T pixels
 * along y times the same along x; cover is a uint8 plane): utils/sliding.py's grids, overlap <= 0.75, stay at 7 x 7 = 49. ---- */
/* dst[i][c][ty][tx] = src[n][c][ys[iy] + ty][xs[ix] + tx], tiles[i] = (n * Py + iy) * Px + ix  (device int32 [M]; entries may repeat:
 * the caller pads the last chunk by repeating a tile; an entry outside [0, N Py Px) leaves dst[i] alone).  src fp32 [N][C][H][W],
 * dst fp32 [M][C][T][T], src != dst. */
int mi355_tile_gather_f32(const float* src, int N, int C, int H, int W, int T, const int32_t* ys, int Py, const int32_t* xs, int Px,
                          const int32_t* tiles, int M, float* dst, mi355_stream_t s);
/* z: fp32 [N * Py * Px][T][T], the one-channel logit maps of the tiles; wy, wx: device fp32 [T], all > 0 (caller's contract).
 * For pixel (y, x) of sample n, over the tiles that cover it, iy ascending and within iy ix ascending, from num = den = 0,
 * lo = +inf, hi = -inf, cnt = 0:
 *   v = z[(n Py + iy) Px + ix][y - ys[iy]][x - xs[ix]];  if (prob) v = sigmoid(v)   (mi355_mask_scatter's expression)
 *   w = wy[y - ys[iy]] * wx[x - xs[ix]];  num = num + (w * v);  den = den + w;  lo = min(lo, v);  hi = max(hi, v);  cnt++
 *   mean[n][y][x] = num / den;  spread[n][y][x] = hi - lo;  cover[y][x] = cnt (uint8 [H][W], the same for every n)
 *   mask[idx ? idx[n] : n][y][x] = 255 where mean > thr (prob) or sigmoid(mean) > thr (otherwise), else 0
 * spread, cover, mask, idx may be NULL (skipped; idx: rows in place).  One tile with wy = wx = 1 and prob = 0: mean has z's bits
 * — except that z = -0 comes out as +0 (num = 0 + (1 * -0) = +0) — and mask has mi355_mask_scatter's bytes.  N <= 65535. */
int mi355_tile_blend(const float* z, int N, int H, int W, int T, const int32_t* ys, int Py, const int32_t* xs, int Px,
                     const float* wy, const float* wx, int prob, float thr, const int32_t* idx, float* mean, float* spread,
                     uint8_t* cover, uint8_t* mask, mi355_stream_t s);

/* ---- batch mixing: mixup (Zhang et al. 2018) and CutMix (Yun et al. 2019) on the normalised batch (utils/mix.py; nothing in the
 * reference) ------------------------------------------------------------------------------------------------------------- */
/* x, out: fp32 [N][C][H][W], contiguous; perm: int32 [N], the partner of every sample; lam: fp32 [N]; box: int32 [N][4] =
 * (y0, x0, y1, x1), half-open, 0 <= y0 <= y1 <= H, 0 <= x0 <= x1 <= W (empty: y0 == y1 or x0 == x1).  With a = x[n][c][i][j] and
 * b = x[perm[n]][c][i][j]:
 *   out[n][c][i][j] = b                                                   if y0 <= i < y1 and x0 <= j < x1
 *                   = fl(fl(lam[n] * a) + fl(fl(1.0f - lam[n]) * b))      otherwise
 * every operation rounded on its own (no FMA), nothing atomic: the same input gives the same bytes (tests/mix_ref.py restates it
 * in numpy float32).  Mixup: an empty box.  CutMix: lam = 1, so outside the box out = fl(a + fl(0 * b)) = a for finite b (a = -0
 * comes out as +0 where 0 * b = +0).  An unmixed sample: perm[n] = n.
 * Out of place only (a sample is read as a by itself and as b by its partner): MI355_ERR_ARG, before the device is touched, for
 * a null pointer, a non-positive size, N > 65535, C H W >= 2^31, or [x, x + N C H W) overlapping [out, out + N C H W).  perm
 * entries in [0, N) and boxes within the image are the caller's contract (utils/mix.py checks both on the host, where they are
 * drawn; the kernel reads an entry outside [0, N) as n, so a bad entry cannot read out of bounds).  16-byte accesses along W when W % 4 == 0 and x, out are 16-byte aligned, a scalar path otherwise; the box test is per
 * element.  One pass: 2 N C H W floats read, N C H W written. */
int mi355_mix_batch_f32(const float* x, const int32_t* perm, const float* lam, const int32_t* box, float* out, int N, int C, int H,
                        int W, mi355_stream_t s);

/* ---- Grad-CAM and image overlays (utils/explain.py; utils/pipeline.py process_images, reference pipeline.py:399-407) ---------- */
/* dout[b][k] = (k == t_b) for the explained class t_b = target[b] when target is given (out of [0, K): a zero row, t_b = -1),
 * else the first maximum of logits[b][.]; target_out[b] = t_b (int32). */
int mi355_cam_seed(const float* logits, const int32_t* target, int B, int K, float* dout, int32_t* target_out, mi355_stream_t s);
/* Per image n of NHWC maps A, dA (compute dtype, channel strides ldA, lddA >= C): alpha[c] = mean_p dA[p][c],
 * raw[p] = relu(sum_c alpha[c] A[p][c]), cam_lowres[n][p] = (raw[p] - min raw) / (1e-7 + max raw - min raw), fp32 throughout.
 * MI355_ERR_UNSUPPORTED when 4 * (HW + C) exceeds the kernel's 48 KB of LDS. */
int mi355_gradcam(const void* A, int ldA, const void* dA, int lddA, int N, int HW, int C, int dtype, float* cam_lowres,
                  mi355_stream_t s);
/* dst[N][H][W] = F.interpolate(src[N][h][w], (H, W), mode="bilinear", align_corners=False) (fp32; any sizes). */
int mi355_resize_bilinear_f32(const float* src, int N, int h, int w, float* dst, int H, int W, mi355_stream_t s);
/* uint8 RGB [B][H][W][3]: where mask[b][(y h) / H][(x w) / W] == 255, R = sat(rint(R + 255 * opacity)); every other byte copied. */
int mi355_overlay_mask(const uint8_t* img, int B, int H, int W, const uint8_t* mask, int h, int w, float opacity, uint8_t* out,
                       mi355_stream_t s);
/* uint8 RGB [B][H][W][3], cam fp32 [B][H][W] in [0, 1]: out = sat(rint((1 - alpha) img + alpha 255 jet(cam))) per channel, jet =
 * matplotlib's 256-entry LUT indexed by min(int(256 cam), 255). */
int mi355_overlay_heatmap(const uint8_t* img, int B, int H, int W, const float* cam, float alpha, uint8_t* out, mi355_stream_t s);

/* ---- segmentation metrics counters (utils/tester.py:92-193; helpers.py:223-227) ------------- */
/* per sample b: counts[b*4+{0,1,2,3}] = tp, pred-positive, target-positive, equal   (p = prob > thr) */
int mi355_seg_counts(const float* prob_or_logit, const float* target, float* counts, int B, long long per,
                     int is_logit, float thr, mi355_stream_t s);

/* ---- surface-distance metrics (Hausdorff, HD95, ASSD, surface Dice; nothing in the reference, whose tester.py stops at the
 * overlap metrics above) ----------------------------------------------------------------------------------------------- */
/* Per sample b of [B][H][W] fp32 maps, binarised exactly as mi355_seg_counts does (P = prob > thr, T = target > thr): the border
 * of a mask is its pixels with a 4-neighbour outside it (outside the image counts as background), d2_PT(p) = min over the
 * border of T of |p - q|^2 for p on the border of P, d2_TP likewise: integers for unit pixel spacing.
 *   out_i[b][0..8) = n_P, n_T, max d2_PT, max d2_TP, lo2, hi2, #{d2_PT <= tol2}, #{d2_TP <= tol2}
 *   out_d[b][0..2) = sum sqrt(d2_PT), sum sqrt(d2_TP)       (fp64, added in a fixed order)
 * lo2 = d2[lo], hi2 = d2[lo + (r > 0)] of the ascending concatenation of both sets, lo = q (n - 1) div 100, r = q (n - 1) mod 100,
 * n = n_P + n_T (numpy.percentile's two neighbours).  n = 0: everything 0.  Exactly one border empty: the two counts, the rest 0.
 * 1 <= H, W <= 1024.  `ws` = mi355_surface_ws_ints(B, H, W) int32 elements of scratch (-1 + last_error when the shape is
 * unsupported); no floating-point atomics: the same input gives the same bytes. */
int mi355_surface_ws_ints(int B, int H, int W);
int mi355_surface_distances(const float* pred, const float* target, int B, int H, int W, int is_logit, float thr, int q,
                            int tol2, int32_t* ws, long long ws_ints, int32_t* out_i, double* out_d, mi355_stream_t s);

/* ---- connected components of a mask: clean-up and lesion statistics (nothing in the reference, which overlays the thresholded
 * mask as it is) --------------------------------------------------------------------------------------------------------- */
/* Per sample b of [B][H][W] fp32 maps, binarised exactly as mi355_seg_counts does (m = prob > thr), all in integers and equal to
 * scipy.ndimage:
 *   fill_holes (0 = off, 4 or 8): background components under that connectivity that do not touch the image frame become foreground
 *     (binary_fill_holes with generate_binary_structure(2, 1 or 2));
 *   the components of the filled mask under `connectivity` (4 or 8) are numbered 1..n by increasing `first`, the smallest linear
 *     index y W + x among a component's pixels (ndimage.label's numbering), and ranked by (area descending, first ascending);
 *   a component is kept iff area >= min_area and (keep_largest == 0 or its rank < keep_largest).
 *   mask_out[b][H][W]   uint8: 255 on kept components, 0 elsewhere
 *   labels_out[b][H][W] int32 or NULL: the numbering, whatever the filter keeps
 *   out_i[b][0..8)      foreground pixels after thresholding, pixels added by hole filling, components, kept components, foreground
 *                       pixels of mask_out, largest area of any component, rows reported = min(kept, max_report), status (0 = ok)
 *   out_c[b][max_report][8]  the kept components in rank order: area, first, y0, x0, y1, x1 (inclusive box), sum of y, sum of x;
 *                       unused rows zero
 * 1 <= H, W <= 1024, 0 <= max_report <= 16.  `ws` = mi355_components_ws_ints(B, H, W) int32 elements of scratch (-1 + last_error
 * when the shape is unsupported), 16-byte aligned.  Integer atomics only: the same input gives the same bytes.  No loop waits for
 * another workgroup, and every union-find loop is bounded: status != 0 reports a bound that was hit. */
int mi355_components_ws_ints(int B, int H, int W);
int mi355_components(const float* src, int B, int H, int W, int is_logit, float thr, int connectivity, int fill_holes, int min_area,
                     int keep_largest, int max_report, int32_t* ws, long long ws_ints, uint8_t* mask_out, int32_t* labels_out,
                     int32_t* out_i, int32_t* out_c, mi355_stream_t s);

/* ---- launch-plan replay: the per-batch host loop of utils/helpers.py:317-342 (model(x) ... loss.backward()) as ONE call ---- */
/* A plan is a table of pre-resolved launches of the entry points above: `name`, its arguments as 64-bit slots in prototype
 * order INCLUDING the trailing stream (pointers and integers by value, floats as their IEEE-754 bit pattern in the low 32
 * bits), flags bit 0 = "runs on the side stream" (weight-gradient launches).  mi355_plan_run issues launches [first, last) in
 * order; whenever a run of side-stream launches starts, the side stream first waits for everything issued on the main stream
 * so far (event fork).  mi355_plan_join makes the main stream wait for the side stream.  Nothing synchronises with the host.
 * mi355_plan_arity(name) = number of slots the entry point takes, or -1 if `name` is not a launcher of this header. */
int mi355_plan_arity(const char* name);
void* mi355_plan_create(int n);
int mi355_plan_set(void* plan, int i, const char* name, const uint64_t* args, int nargs, int flags);
int mi355_plan_patch(void* plan, int i, int arg, uint64_t value);
int mi355_plan_run(void* plan, int first, int last, mi355_stream_t main_stream, mi355_stream_t side_stream);
int mi355_plan_join(void* plan, mi355_stream_t main_stream, mi355_stream_t side_stream);
int mi355_plan_last_index(void* plan);
int mi355_plan_destroy(void* plan);

/* ---- data-parallel gradient exchange ----------------------------------------------------------------
 * The reference is single-device (no DDP / NCCL anywhere: utils/trainer.py:119-213); the data-parallel step of this path sums
 * the flat fp32 gradient buffer over the GPUs of a node in a few contiguous buckets.  One process per GPU, one communicator per
 * process, RCCL resolved at run time (the librccl.so already loaded by PyTorch when there is one).  mi355_comm_unique_id: rank 0
 * fills a 128-byte id (ncclUniqueId) that the host distributes; mi355_comm_init: collective over all ranks with that id;
 * mi355_allreduce_bucket: in-place sum of `count` elements at `ptr` over the ranks, enqueued on `s` (the caller orders `s` behind
 * the bucket's last writer); mi355_comm_world: ranks of the live communicator (0 = none); mi355_comm_destroy. */
int mi355_comm_unique_id(void* id128);
int mi355_comm_init(int rank, int world, const void* id128);
int mi355_comm_world(void);
int mi355_allreduce_bucket(void* ptr, long long count, int dtype, mi355_stream_t s);
int mi355_comm_destroy(void);
/* bf16 / fp16 buckets (SURVEY.md 8e "bf16 (perf) buckets"; the reference has no gradient exchange at all, utils/helpers.py:329-335):
 * wire[i] = round(g[i]) for a bucket of n gradients, and back (g[i] = wire[i]) behind the all-reduce of the staging buffer;
 * g 16-byte aligned, wire 8-byte aligned (a bucket starts on a multiple of four gradients), dtype = MI355_BF16 / MI355_F16. */
int mi355_grads_to_wire(const float* g, void* wire, long long n, int dtype, mi355_stream_t s);
int mi355_grads_from_wire(const void* wire, float* g, long long n, int dtype, mi355_stream_t s);

#ifdef __cplusplus
}
#endif
#endif /* MI355CONV_H_ */
