/*
 * tartangan_amd.h -- C ABI of libtartangan_amd.so (gfx950 / MI355X).
 *
 * The drop-in boundary for tartangan's SA-GAN / SA-GAN-IQN G+D training step
 * (SURVEY.md §8b).  The reference has no native code: every entry point below
 * replaces the ATen op(s) that the cited reference line dispatches through
 * torch.nn / torch.nn.functional.  Paths are relative to
 * /root/reference/tartangan.
 *
 * Conventions
 *   - all tensors fp32, contiguous, NCHW (the reference's layout); raw device
 *     pointers; the caller owns every byte including workspaces;
 *   - enqueue-only on `stream` (a hipStream_t passed as void*; NULL = default
 *     stream); no allocation, no synchronisation, graph-capture safe;
 *   - return 0 on success, a negative TG_E* code for a bad argument or an
 *     unsupported shape, a positive value = hipError_t from the launch;
 *   - re-entrant; no mutable global state.
 */
#ifndef TARTANGAN_AMD_H
#define TARTANGAN_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TG_OK 0
#define TG_EINVAL (-1)      /* null pointer / non-positive dimension */
#define TG_EUNSUPPORTED (-2) /* shape outside what the kernels implement */
#define TG_EWORKSPACE (-3)  /* workspace too small */

/* library / build identification */
int tg_version(void);
const char* tg_arch(void);

/* ---------------------------------------------------------------- convolution
 * nn.Conv2d(k=3,pad=1) / nn.Conv2d(k=1): models/blocks/generator.py:41,44,52,124
 * models/blocks/discriminator.py:17,63,66,78  models/blocks/attention.py:14-17
 * ks in {1,3}, stride 1, zero pad ks/2.  w is OIHW [Cout][Cin][ks][ks].        */
int tg_conv2d_fwd(const float* x, const float* w, const float* bias /*nullable*/,
                  const float* residual /*nullable: y = conv + bias + residual (x + h, generator.py:62)*/,
                  float* y, int B, int Cin, int Cout, int H, int W, int ks, void* stream);
/* The generator block's `h + up(project(x))` (generator.py:52-62: x = F.interpolate(x, scale_factor=2) first, then
 * convs(x) + project_input(x)): the 1x1 projection commutes with nearest-neighbour upsampling, so the shortcut stays at
 * HALF the resolution and the last 3x3 conv adds it upsampled on the fly: y = conv3x3(x) + bias + up2x(residual_lo),
 * residual_lo is (B, Cout, H/2, W/2); H, W even.  No high-resolution copy of the shortcut is ever written. */
int tg_conv2d_fwd_up2res(const float* x, const float* w, const float* bias /*nullable*/, const float* residual_lo,
                         float* y, int B, int Cin, int Cout, int H, int W, void* stream);
/* conv3x3(nearest_up2x(a)) + bias [+ residual] without the upsampled tensor (generator.py:52-58: the first 3x3
 * conv of every generator block reads an upsampled activation).  Output pixel (2i+dy, 2j+dx) only sees a 2x2 block
 * of source pixels, so the layer is four 2x2-tap convolutions at the LOW resolution with row/column-summed filters:
 *   tg_upconv3x3_weights  w [Cout][Cin][3][3] -> wp [4 phases (dy,dx)][Cout][Cin][2][2]
 *   tg_upconv3x3_fwd      a (B,Cin,H,W), wp -> y (B,Cout,2H,2W); residual (nullable) has y's shape
 * 2.25x fewer multiply-adds than the reference's formulation, same result up to fp32 rounding of the summed taps. */
int tg_upconv3x3_weights(const float* w, float* wp, int Cout, int Cin, void* stream);
int tg_upconv3x3_fwd(const float* a, const float* wp, const float* bias /*nullable*/, const float* residual /*nullable*/,
                     float* y, int B, int Cin, int Cout, int H, int W, void* stream);
/* gradient of tg_upconv3x3_fwd w.r.t. its low-resolution input (what autograd computes as pool2x2sum(dgrad3x3(gy))):
 * a 4x4-tap stride-2 convolution over gy (B,Cout,2H,2W) with w4t [Cin][Cout][4][4] from tg_upconv3x3_weights_t.
 * Only where the low-resolution plane gives >= 256 workgroups (tg_upconv3x3_dgrad_supported); callers fall back to
 * tg_conv2d_dgrad + tg_pool2 otherwise.                                                                    */
int tg_upconv3x3_weights_t(const float* w, float* w4t, int Cout, int Cin, void* stream);
/* both layouts in one launch (a training step needs both) */
int tg_upconv3x3_weights_pair(const float* w, float* wp, float* w4t, int Cout, int Cin, void* stream);
int tg_upconv3x3_dgrad_supported(int B, int Cin, int Cout, int H, int W);
int tg_upconv3x3_dgrad(const float* gy, const float* w4t, float* ga, int B, int Cin, int Cout, int H, int W, void* stream);
/* AvgPool2d(2)(conv3x3(x) + bias) [+ residual] as ONE 4x4-tap stride-2 convolution (discriminator.py:60-66: the second
 * 3x3 conv of every discriminator block is followed by the block's average pool): 16 products per OUTPUT pixel and
 * channel pair instead of 36, no full-resolution conv output, no pool pass.  The pair is 0.25 x the transpose of the
 * up-conv above with the flipped, transposed filter, so the same two kernels serve with their roles swapped:
 *   tg_poolconv3x3_weights  w [Cout][Cin][3][3] -> w4 [Cout][Cin][4][4] (forward) and wp [4][Cin][Cout][2][2] (dgrad)
 *   tg_poolconv3x3_fwd      x (B,Cin,2H,2W), w4 -> y (B,Cout,H,W); bias / residual (shape of y) nullable
 *   tg_poolconv3x3_dgrad    gy (B,Cout,H,W), wp -> gx (B,Cin,2H,2W)
 * Supported where H x W >= 16 x 16 gives both kernels >= 256 workgroups (tg_poolconv3x3_supported); the weight
 * gradient is tg_conv2d_wgrad(x, 0.25 * up2x(gy)).                                                          */
int tg_poolconv3x3_weights(const float* w, float* w4, float* wp, int Cout, int Cin, void* stream);
int tg_poolconv3x3_supported(int B, int Cin, int Cout, int H, int W);
int tg_poolconv3x3_fwd(const float* x, const float* w4, const float* bias /*nullable*/, const float* residual /*nullable*/,
                       float* y, int B, int Cin, int Cout, int H, int W, void* stream);
int tg_poolconv3x3_dgrad(const float* gy, const float* wp, float* gx, int B, int Cin, int Cout, int H, int W, void* stream);
/* Weight gradients of the two stride-2 forms (convolution_backward grad_weight of the 3x3 filter, deterministic):
 * both are T[o][i][u][v] = sum lo[o][r][c] * hi[i][2r-1+u][2c-1+v] folded back onto the 3x3 taps -- 16 products per
 * low-resolution pixel instead of 36 on the materialised high-resolution pair.  (B, ., H, W) is the LOW-resolution
 * plane; where the plane is smaller than 16 x 16 they return TG_EUNSUPPORTED and the caller uses tg_conv2d_wgrad.
 * gbias (nullable, Cout floats): the bias gradient sum_{b,h,w} gy, taken from the operands these kernels stage anyway
 * (convolution_backward's grad_bias; `accumulate` applies to it as to gw).                                          */
size_t tg_poolconv3x3_wgrad_workspace(int B, int Cin, int Cout, int H, int W);
int tg_poolconv3x3_wgrad(const float* x /*(B,Cin,2H,2W)*/, const float* gy /*(B,Cout,H,W)*/, float* gw, float* workspace,
                         size_t workspace_bytes, int B, int Cin, int Cout, int H, int W, int accumulate, float* gbias /*nullable*/,
                         void* stream);
size_t tg_upconv3x3_wgrad_workspace(int B, int Cin, int Cout, int H, int W);
int tg_upconv3x3_wgrad(const float* a /*(B,Cin,H,W)*/, const float* gy /*(B,Cout,2H,2W)*/, float* gw, float* workspace,
                       size_t workspace_bytes, int B, int Cin, int Cout, int H, int W, int accumulate, float* gbias /*nullable*/,
                       void* stream);
/* gx = d/dx: correlation of gy with the transposed, spatially flipped filter
 * (what autograd's convolution_backward computes for grad_input)              */
int tg_conv2d_dgrad(const float* gy, const float* w, float* gx,
                    int B, int Cin, int Cout, int H, int W, int ks, void* stream);
/* gw[co][ci][kh][kw] = sum_{b,h,w} gy[b,co,h,w] * x[b,ci,h+kh-p,w+kw-p]
 * (convolution_backward grad_weight) and, when gbias != NULL, gbias[co] = sum_{b,h,w} gy (grad_bias) from
 * the same pass; deterministic two-stage reduction.  accumulate != 0: add into gw / gbias instead of
 * overwriting (gradient accumulation straight into the flat .grad bucket).                              */
size_t tg_conv2d_wgrad_workspace(int B, int Cin, int Cout, int H, int W, int ks);
int tg_conv2d_wgrad(const float* x, const float* gy, float* gw, float* gbias /*nullable*/,
                    float* workspace, size_t workspace_bytes,
                    int B, int Cin, int Cout, int H, int W, int ks, int accumulate, void* stream);
/* SelfAttention2d's theta / phi / g projections (attention.py:15-17, 22-26: three bias-free 1x1 convolutions of the SAME input)
 * as ONE pass each way: x is read once for the three outputs, the three output gradients give the input gradient in one pass
 * (no three-way add) and the three filter gradients in one pass.  w / gw: the three filters back to back,
 * [c0 + c1 + c2][Cin] (they are adjacent in the parameter bucket); y_k / gy_k: (B, c_k, H, W) each.  Bandwidth-bound
 * streaming kernels (no LDS); need H*W % 16 == 0, at most 64 channels either side and EVERY pointer (filters and workspace included)
 * 16-byte aligned: TG_EUNSUPPORTED otherwise, nothing written. */
int tg_conv1x1_multi_supported(int c0, int c1, int c2, int B, int Cin, int H, int W);
int tg_conv1x1_multi_fwd(const float* x, const float* w, float* y0, float* y1, float* y2, int c0, int c1, int c2,
                         int B, int Cin, int H, int W, void* stream);
int tg_conv1x1_multi_dgrad(const float* gy0, const float* gy1, const float* gy2, const float* w, float* gx,
                           int c0, int c1, int c2, int B, int Cin, int H, int W, void* stream);
size_t tg_conv1x1_multi_wgrad_workspace(int c0, int c1, int c2, int B, int Cin, int H, int W);
int tg_conv1x1_multi_wgrad(const float* x, const float* gy0, const float* gy1, const float* gy2, float* gw,
                           float* workspace, size_t workspace_bytes, int c0, int c1, int c2, int B, int Cin, int H, int W,
                           int accumulate /* gw += */, void* stream);
/* The same in two steps, so that ONE launch can finish the reduction for many layers (a whole backward pass):
 *   tg_conv2d_wgrad_partials     stage 1 only: per-workgroup partial sums into `workspace` (which must then stay
 *                                untouched until the batch reduce has run);
 *   tg_conv2d_wgrad_reduce_batch stage 2 for n_items layers.  `items` is a HOST array of
 *                                n_items x TG_WGRAD_ITEM_FIELDS 64-bit words:
 *                                  [0] workspace (device address)   [1] gw (device address)
 *                                  [2] gbias (device address or 0; nonzero needs want_bias != 0 in stage 1)
 *                                  [3..8] B, Cin, Cout, H, W, ks     [9] accumulate
 * Results are bit-identical to tg_conv2d_wgrad (same partials, same summation order).  Within one call every
 * gw / gbias may appear at most once (items are reduced concurrently); further contributions to the same
 * gradient go into a later call.
 *
 * THE TABLE CONTRACT of the four entry points that take such a host table (tg_conv2d_wgrad_reduce_batch,
 * tg_conv1x1_wgrad_partials_batch, tg_poolconv3x3_weights_batch, tg_s2_wgrad_reduce_batch): `items` is read during the call only.
 * Every row is checked before anything is launched: the first bad row's code (TG_EINVAL / TG_EUNSUPPORTED / TG_EWORKSPACE) is
 * returned with nothing written.  More rows than one kernel argument block holds go into several launches; n_items == 0 is
 * TG_OK with no launch, n_items < 0 or a null `items` TG_EINVAL.                                                            */
typedef int64_t tg_host_i64;
#define TG_WGRAD_ITEM_FIELDS 10
int tg_conv2d_wgrad_partials(const float* x, const float* gy, float* workspace, size_t workspace_bytes,
                             int B, int Cin, int Cout, int H, int W, int ks, int want_bias, void* stream);
int tg_conv2d_wgrad_reduce_batch(const tg_host_i64* items /*host*/, int n_items, void* stream);
/* Stage 1 of MANY 1x1 weight gradients in one launch (a backward pass' shortcut, attention-output and theta / phi / g layers: each is a
 * few microseconds of traffic behind a launch, and nothing reads a weight gradient before the optimiser).  `items` is a HOST array of
 * n_items x TG_WGRAD1X1_ITEM_FIELDS 64-bit words:
 *   [0] x (B,Cin,H,W)     [1] gy0 (B,c0,H,W)     [2] gy1 (B,c1,H,W) or 0     [3] gy2 (B,c2,H,W) or 0      (device addresses)
 *   [4] workspace (device address)                [5] workspace bytes
 *   [6..8] c0, c1, c2: Cout = c0 + c1 + c2; a plain layer has c1 = c2 = 0 and [2] = [3] = 0, the theta / phi / g form all three
 *   [9..12] B, Cin, H, W   [13] ks (1: the only family so far)   [14] want_bias
 * Every row writes what tg_conv2d_wgrad_partials (tg_conv1x1_multi_wgrad's first half for three gy) writes for the same layer, bit for
 * bit, into a workspace of tg_conv2d_wgrad_workspace(B, Cin, Cout, H, W, 1) bytes: rows of tg_conv2d_wgrad_reduce_batch finish them.
 * Needs H*W % 16 == 0 (tg_conv1x1_wgrad_batch_supported: the shape part of the rule, host only) and [0]..[4] 16-byte aligned.
 * The table contract above holds.                                                                                              */
#define TG_WGRAD1X1_ITEM_FIELDS 15
int tg_conv1x1_wgrad_batch_supported(int B, int Cin, int Cout, int H, int W);
int tg_conv1x1_wgrad_partials_batch(const tg_host_i64* items /*host*/, int n_items, void* stream);
/* tg_poolconv3x3_weights for n_items layers in one launch (a discriminator's stride-2 layers all need their derived filters at
 * the start of a pass).  `items`: HOST array of n_items x TG_FORM_ITEM_FIELDS words: [0] w  [1] w4  [2] wp (device addresses)
 * [3] Cout  [4] Cin.  Same arithmetic per layer as the single call; the table contract above holds. */
#define TG_FORM_ITEM_FIELDS 5
int tg_poolconv3x3_weights_batch(const tg_host_i64* items /*host*/, int n_items, void* stream);
/* The stride-2 weight gradients in two steps, like tg_conv2d_wgrad_partials / _reduce_batch: stage 1 per layer into a workspace of its
 * own (tg_*_wgrad_workspace bytes, untouched until the reduce has run), then ONE launch that sums, folds onto the 3x3 taps and
 * finishes the bias gradients of all recorded layers.  Items as for tg_conv2d_wgrad_reduce_batch with [8] = 0 (pooled conv: stage 1
 * by tg_poolconv3x3_wgrad_partials) or 1 (up-conv: tg_upconv3x3_wgrad_partials) in the place of ks; (B, ., H, W) the LOW-resolution
 * plane; [2] gbias nonzero needs want_bias != 0 in stage 1.  Bit-identical to the one-call forms; the table contract above holds. */
/* The discriminator's from-RGB 1x1 convolution composed into the 3x3 convolution that follows it (discriminator.py:11-22 + :60-61,
 * nothing in between): wc [Cout][Cimg + 1][3][3] = sum_m [w1 | b1][m][c] * w3[co][m][tap] (the from-RGB bias on an all-ones input channel),
 * and its backward (gw1 [C][Cimg], gb1 [C], gw3 [Cout][C][3][3]; accumulate: += into all three).  One launch each.          */
int tg_rgb_compose_fwd(const float* w1, const float* b1, const float* w3, float* wc, int Cout, int C, int Cimg, void* stream);
int tg_rgb_compose_bwd(const float* gwc, const float* w1, const float* b1, const float* w3, float* gw1, float* gb1, float* gw3, int Cout,
                       int C, int Cimg, int accumulate, void* stream);
int tg_poolconv3x3_wgrad_partials(const float* x, const float* gy, float* workspace, size_t workspace_bytes, int B, int Cin, int Cout,
                                  int H, int W, int want_bias, void* stream);
int tg_upconv3x3_wgrad_partials(const float* a, const float* gy, float* workspace, size_t workspace_bytes, int B, int Cin, int Cout,
                                int H, int W, int want_bias, void* stream);
int tg_s2_wgrad_reduce_batch(const tg_host_i64* items /*host*/, int n_items, void* stream);
/* Which kernels would a call launch?  (tg_version 109; host only like the *_supported queries: no device, no HIP call, nothing
 * launched.)  The convolution entry points above choose among ~250 kernel instantiations by workgroup counts, channel
 * divisibility, plane size, pointer alignment and three process-wide switches.  This query makes the REAL call of entry point
 * `op` with made-up addresses under a thread-local probe: every launch site records instead of launching, so the answer comes
 * from the dispatch code itself.  -> one line per launch, in order (the four phases of an up-conv, stage 1 then the reduce):
 *     "<kernel as its demangled symbol reads, tile geometries by alias: conv_dma_kernel<GX, 32, 2, 8, false>>; <flag>=<value> ..."
 * the flags being the host-computed path arguments of that launch (vx / vw / vg / vh / vl: 16-byte staging of an operand;
 * swz / flags: swizzled tile order; prio: TG_DMA_PRIO; bias / res / res_up: epilogue operands present, residual at half
 * resolution; dgrad, mode, items, *segs), and a last line "rc=<code>" if the call returned one.  The string belongs to the
 * calling thread and lives until its next call.
 *   op            TG_OP_* below, one per launching entry point
 *   dims          as the entry point names them; tg_conv1x1_multi_* and _wgrad_partials_batch: c0 = Cout, c1, c2;
 *                 tg_rgb_compose_*: (Cout, C = Cin, Cimg = ks); tg_s2_wgrad_reduce_batch: ks is the row's mode; the batch
 *                 entries get a one-row table
 *   unaligned     bit k set: the k-th pointer parameter (the k-th address field of a table row) sits 4 bytes off a 16-byte
 *                 boundary; nullable pointers keep their bit
 *                 (4 bytes is the only offset modelled: a pointer 8 bytes off -- 8- but not 16-byte aligned, which some
 *                 stride-2 forms treat differently -- cannot be asked for, so the answers are not exhaustive over alignment)
 *   has_bias      bias / gbias / want_bias;  has_residual: residual (tg_conv2d_fwd_up2res always has one)
 *   wino, dma, prio   TG_CONV_WINO / TG_CONV_DMA / TG_DMA_PRIO for this call only; < 0: what the process read from its environment */
#define TG_OP_CONV2D_FWD 0
#define TG_OP_CONV2D_FWD_UP2RES 1
#define TG_OP_CONV2D_DGRAD 2
#define TG_OP_CONV2D_WGRAD 3
#define TG_OP_CONV2D_WGRAD_PARTIALS 4
#define TG_OP_CONV2D_WGRAD_REDUCE_BATCH 5
#define TG_OP_CONV1X1_WGRAD_PARTIALS_BATCH 6
#define TG_OP_UPCONV3X3_WEIGHTS 7
#define TG_OP_UPCONV3X3_WEIGHTS_T 8
#define TG_OP_UPCONV3X3_WEIGHTS_PAIR 9
#define TG_OP_UPCONV3X3_FWD 10
#define TG_OP_UPCONV3X3_DGRAD 11
#define TG_OP_UPCONV3X3_WGRAD 12
#define TG_OP_UPCONV3X3_WGRAD_PARTIALS 13
#define TG_OP_POOLCONV3X3_WEIGHTS 14
#define TG_OP_POOLCONV3X3_WEIGHTS_BATCH 15
#define TG_OP_POOLCONV3X3_FWD 16
#define TG_OP_POOLCONV3X3_DGRAD 17
#define TG_OP_POOLCONV3X3_WGRAD 18
#define TG_OP_POOLCONV3X3_WGRAD_PARTIALS 19
#define TG_OP_S2_WGRAD_REDUCE_BATCH 20
#define TG_OP_RGB_COMPOSE_FWD 21
#define TG_OP_RGB_COMPOSE_BWD 22
#define TG_OP_CONV1X1_MULTI_FWD 23
#define TG_OP_CONV1X1_MULTI_DGRAD 24
#define TG_OP_CONV1X1_MULTI_WGRAD 25
const char* tg_conv_dispatch(int op, int B, int Cin, int Cout, int H, int W, int ks, int c1, int c2, int unaligned, int has_bias,
                             int has_residual, int wino, int dma, int prio);
/* out[c] (+)= sum_{b,p} x[b][c][p]   (linear bias grad); workspace: tg_bn_workspace(B,C,HW) bytes */
int tg_channel_sum(const float* x, float* out, float* workspace, int B, int C, int HW, int accumulate,
                   void* stream);
/* out[b][c][p] = v[c] (transpose of tg_channel_sum) */
int tg_channel_bcast(const float* v, float* out, int B, int C, int HW, void* stream);

/* ---------------------------------------------------------------- GEMM
 * nn.Linear (generator.py:70-72, discriminator.py:137-139,158-160, iqn.py:33-35)
 * and torch.bmm (attention.py:32,34).  Row-major; C[b] = op(A[b]) op(B[b]) (+ bias[n]) + beta*C[b].
 * op(A) is MxK, op(B) is KxN; lda/ldb/ldc are row strides of the stored arrays.  The batch sits on a grid dimension:
 * batch > 65535 is TG_EUNSUPPORTED, nothing launched (the caller slices the batch). */
int tg_gemm(const float* A, const float* Bm, float* C, const float* bias_n /*nullable*/,
            int M, int N, int K, int lda, int ldb, int ldc, int transA, int transB,
            int batch, int64_t strideA, int64_t strideB, int64_t strideC, float beta, void* stream);

/* ---------------------------------------------------------------- BatchNorm2d (+LeakyReLU)
 * nn.BatchNorm2d train mode followed by nn.LeakyReLU(0.2): generator.py:38-44,
 * discriminator.py:60-66,133-136,153-156.  slope = 1 gives plain BatchNorm.
 * Workspace: tg_bn_workspace(B,C,HW) bytes.                                       */
size_t tg_bn_workspace(int B, int C, int HW);
/* batch mean / 1/sqrt(biased var + eps); optional running-stat update
 * (running_var uses the unbiased variance, momentum as nn.BatchNorm2d); *num_batches_tracked += 1.
 * replicate >= 1: x stands for a tensor in which every element occurs `replicate` times (the generator normalises
 * nearest-upsampled activations, generator.py:52-57: same mean and biased variance, so the statistics are taken at the
 * low resolution; only the unbiased correction n/(n-1) of running_var needs the true count n = replicate*B*HW).     */
int tg_bn_train_stats(const float* x, float* mean, float* invstd,
                      float* running_mean /*nullable*/, float* running_var /*nullable*/,
                      int64_t* num_batches_tracked /*nullable*/,
                      float momentum, float eps, float* workspace, int B, int C, int HW, int replicate, void* stream);
/* training forward in one call: tg_bn_train_stats followed by tg_bn_act_fwd (one kernel when a channel
 * has <= 16384 elements)                                                                              */
int tg_bn_train_fwd(const float* x, float* mean, float* invstd,
                    float* running_mean /*nullable*/, float* running_var /*nullable*/,
                    int64_t* num_batches_tracked /*nullable*/, const float* gamma, const float* beta,
                    float slope, float momentum, float eps, float* z, float* workspace,
                    int B, int C, int HW, int replicate, void* stream);
/* eval mode: mean = running_mean, invstd = 1/sqrt(running_var + eps) */
int tg_bn_eval_stats(const float* running_mean, const float* running_var, float* mean, float* invstd,
                     float eps, int C, void* stream);
/* z = lrelu(gamma * (x - mean) * invstd + beta, slope) */
int tg_bn_act_fwd(const float* x, const float* mean, const float* invstd, const float* gamma,
                  const float* beta, float slope, float* z, int B, int C, int HW, void* stream);
/* first backward (native_batch_norm_backward o leaky_relu_backward):
 * gyh = gz * lrelu'(y); ggamma = sum gyh*xhat; gbeta = sum gyh;
 * training: gx = gamma*invstd*(gyh - mean(gyh) - xhat*mean(gyh*xhat)); eval: gx = gamma*invstd*gyh */
int tg_bn_act_bwd(const float* gz, const float* x, const float* mean, const float* invstd,
                  const float* gamma, const float* beta, float slope, int training,
                  float* gx /*nullable*/, float* ggamma, float* gbeta, float* workspace,
                  int B, int C, int HW, int accumulate /* ggamma, gbeta += */,
                  const float* gx_add /*nullable: gx = ... + gx_add, a second gradient of x folded into the pass*/,
                  void* stream);
/* ---- grouped forms: ONE tensor of groups*B images normalised per (group, channel).  trainers/cnn.py:122-123 run the
 * discriminator on the real and on the fake batch as two forwards with the same weights; here both halves travel through
 * the network as one tensor of 2B images (convolutions are per image), and BatchNorm keeps the statistics of each half:
 * group g = images [g*B, (g+1)*B).  mean / invstd are [groups][C]; the running statistics are updated once per group, in
 * group order (exactly what the two forwards leave behind), *num_batches_tracked += groups; ggamma / gbeta are the sums
 * over all groups.  Workspace: tg_bn_workspace(B, groups*C, HW) bytes.  groups = 1 is tg_bn_train_fwd / tg_bn_act_bwd.
 * gx_add (nullable) holds the first add_groups*B images only (the R1 second-order gradient exists for the real half). */
int tg_bn_train_fwd_groups(const float* x, float* mean, float* invstd,
                           float* running_mean /*nullable*/, float* running_var /*nullable*/,
                           int64_t* num_batches_tracked /*nullable*/, const float* gamma, const float* beta,
                           float slope, float momentum, float eps, float* z, float* workspace,
                           int groups, int B, int C, int HW, int replicate, void* stream);
int tg_bn_act_bwd_groups(const float* gz, const float* x, const float* mean, const float* invstd,
                         const float* gamma, const float* beta, float slope, int training,
                         float* gx /*nullable*/, float* ggamma, float* gbeta, float* workspace,
                         int groups, int B, int C, int HW, int accumulate,
                         const float* gx_add /*nullable*/, int add_groups, void* stream);
/* second backward of the training-mode map (gz, x, gamma) -> (gx, ggamma, gbeta)
 * (NativeBatchNormBackwardBackward0; R1 penalty path, models/losses.py:23-26).
 * v = adjoint of gx, vgamma/vbeta = adjoints of ggamma/gbeta (nullable = 0).   */
int tg_bn_act_dbwd(const float* v, const float* vgamma /*nullable*/, const float* vbeta /*nullable*/,
                   const float* gz, const float* x, const float* mean, const float* invstd,
                   const float* gamma, const float* beta, float slope,
                   float* adj_gz, float* adj_x, float* adj_gamma, float* workspace,
                   int B, int C, int HW, int accumulate /* adj_gamma += */, void* stream);

/* ---- BatchNorm under data parallelism (SyncBN; SURVEY.md 8e collective 3).  The reference normalises over the whole
 * batch (trainers/cnn.py:122-123 evaluates D on all B images); when the batch is sharded over ranks the same numbers
 * need global statistics.  Each pass is split in three: *_local writes this rank's per-channel sums (float64,
 * [C][K] channel-major: K = 3 statistics (mean, mean^2, biased var), K = 2 first backward, K = 5 second backward), the
 * CALLER all-reduces them (SUM; torch.distributed -- RCCL on device buffers), *_finish completes the pass with the
 * global sums.  count_global = world * B * HW (equal shards).  Parameter gradients (ggamma, gbeta, adj_gamma) come out as
 * this rank's share, to be averaged by the gradient all-reduce like every other parameter gradient.
 * Workspace: tg_bn_workspace(B, C, HW) bytes; the *_finish call of the backward passes must get the same workspace
 * pointer contents-wise only in that it is scratch (nothing is carried from *_local).                              */
int tg_bn_sync_stats_local(const float* x, double* sums /*[C][3]*/, float* workspace, int B, int C, int HW,
                           void* stream);
int tg_bn_sync_stats_finish(const double* sums /*[C][3], all-reduced*/, int world, float* mean, float* invstd,
                            float* running_mean /*nullable*/, float* running_var /*nullable*/,
                            int64_t* num_batches_tracked /*nullable*/, float momentum, float eps,
                            int64_t count_global, int replicate, int C, void* stream);
int tg_bn_sync_bwd_local(const float* gz, const float* x, const float* mean, const float* invstd,
                         const float* gamma, const float* beta, float slope, double* sums /*[C][2]*/,
                         float* workspace, int B, int C, int HW, void* stream);
int tg_bn_sync_bwd_finish(const float* gz, const float* x, const float* mean, const float* invstd,
                          const float* gamma, const float* beta, float slope,
                          const double* local_sums /*[C][2]*/, const double* global_sums /*[C][2], all-reduced*/,
                          int64_t count_global, float* gx /*nullable*/, float* ggamma, float* gbeta,
                          float* workspace, int B, int C, int HW, int accumulate,
                          const float* gx_add /*nullable*/, void* stream);
int tg_bn_sync_dbwd_local(const float* v, const float* gz, const float* x, const float* mean,
                          const float* invstd, const float* gamma, const float* beta, float slope,
                          double* sums /*[C][5]*/, float* workspace, int B, int C, int HW, void* stream);
int tg_bn_sync_dbwd_finish(const float* v, const float* gz, const float* x, const float* mean,
                           const float* invstd, const float* gamma, const float* beta, float slope,
                           const double* global_sums /*[C][5], all-reduced*/, int64_t count_global, int world,
                           float* adj_gz, float* adj_x, float* adj_gamma, float* workspace,
                           int B, int C, int HW, int accumulate /* adj_gamma += */, void* stream);

/* ---------------------------------------------------------------- resampling
 * F.interpolate(scale_factor=2,'nearest') generator.py:58 and nn.AvgPool2d(2)
 * discriminator.py:67 are transposes of each other up to a factor:
 *   up2x : y[2h+i][2w+j] = alpha * x[h][w]       pool2: y[h][w] = alpha * sum_{i,j} x[2h+i][2w+j]
 * (nearest fwd = up2x(1), bwd = pool2(1); avgpool fwd = pool2(.25), bwd = up2x(.25)).
 * H, W are the dims of the SMALL side for up2x (output 2H x 2W) and of the LARGE
 * (input) side for pool2; both must be even for pool2.                          */
int tg_up2x(const float* x, float* y, float alpha, int BC, int H, int W, void* stream);
int tg_pool2(const float* x, const float* residual /*nullable: y = residual + pooled (discriminator.py:95)*/,
             float* y, float alpha, int BC, int H, int W, void* stream);
/* F.interpolate(scale_factor=0.5, mode='bilinear', align_corners=True) discriminator.py:55-57
 * input HxW -> output floor(H/2) x floor(W/2); _bwd is its transpose (scatter-free gather form), optionally
 * added to `residual` (the gradient that reached the same tensor through the block's main path) */
int tg_bilinear_half_fwd(const float* x, float* y, int BC, int H, int W, void* stream);
int tg_bilinear_half_bwd(const float* gy, const float* residual /*nullable, shape of gx*/, float* gx,
                         int BC, int H, int W, void* stream);
/* F.interpolate(scale_factor=2, mode='bilinear', align_corners=True) models/shared/blocks.py:64-67 (since version 102)
 * x (BC, H, W) -> y (BC, 2H, 2W) [+ residual, shape of y]; same fp32 source-index arithmetic as the half-size pair
 * (scale = (in - 1) / (out - 1), 0 for in = 1), so _bwd is the exact transpose of _fwd: gy (BC, 2H, 2W) -> gx (BC, H, W)
 * [+ residual, shape of gx], gather form, fixed summation order, no atomics: two runs are bit-identical.
 * H, W are the dims of the SMALL side for both; any H, W in 1 .. 16384 (TG_EUNSUPPORTED above), pointers at any multiple of
 * 4 bytes (16-byte rows are written where the alignment allows); no workspace.                                        */
int tg_bilinear_up2x_fwd(const float* x, const float* residual /*nullable*/, float* y, int BC, int H, int W, void* stream);
int tg_bilinear_up2x_bwd(const float* gy, const float* residual /*nullable*/, float* gx, int BC, int H, int W, void* stream);
/* Input side of the FID / Inception-score pipeline (8f-2).  out (B, C, OH, OW) = bilinear resize (align_corners=True;
 * F.interpolate(x, size=(299, 299), mode='bilinear', align_corners=True), inception_utils.py:49-50) of x (B, C, H, W) after
 * `stages` applications of  x <- ((x + 1) / 2 - mean[c]) / std[c]  -- one in WrapInception.forward (inception_utils.py:44-47), a
 * second, identical one in accumulate_inception_activations' transform (:254-258), which the reference applies to the
 * generator's samples before WrapInception sees them.  stages = 0: resize only; OH == H and OW == W: normalise only. */
int tg_inception_preprocess(const float* x, const float* mean /*[C]*/, const float* stdv /*[C]*/, float* out,
                            int B, int C, int H, int W, int OH, int OW, int stages, void* stream);

/* F.max_pool2d(x,[2,2]) attention.py:25-26; idx = argmax position 0..3 inside the window
 * (first maximum in row-major window order, like ATen)                          */
int tg_maxpool2_fwd(const float* x, float* y, uint8_t* idx, int BC, int H, int W, void* stream);
/* gx[window(o)[idx[o]]] = gy[o], zeros elsewhere (H,W = dims of gx) */
int tg_maxpool2_bwd(const float* gy, const uint8_t* idx, float* gx, int BC, int H, int W, void* stream);
/* y[o] = x[window(o)[idx[o]]] (transpose of _bwd; H,W = dims of x) */
int tg_maxpool2_gather(const float* x, const uint8_t* idx, float* y, int BC, int H, int W, void* stream);

/* ---------------------------------------------------------------- row ops
 * out[r] = alpha * sum_c x[r][c]  (torch.sum(feats,[2,3]) discriminator.py:143,165) */
int tg_row_sum(const float* x, float* out, float alpha, int rows, int cols, void* stream);
/* out[r][c] = alpha * v[r] */
int tg_row_bcast(const float* v, float* out, float alpha, int rows, int cols, void* stream);
/* x.repeat(reps,1) (iqn.py:93): out[q*rows + r][c] = alpha * x[r][c]            */
int tg_repeat_rows(const float* x, float* out, float alpha, int rows, int cols, int reps, void* stream);
/* out[r][c] = alpha * sum_q x[q*rows + r][c]  (p_target_tau.mean(0), discriminator.py:174-175) */
int tg_sum_reps(const float* x, float* out, float alpha, int rows, int cols, int reps, void* stream);
/* the same over `groups` independent row blocks back to back (x: groups x rows rows; the repeated side: groups x reps x rows): the
 * real and the fake batch of a discriminator step through the IQN head as one tensor, each half repeated / averaged on its own */
int tg_repeat_rows_groups(const float* x, float* out, float alpha, int rows, int cols, int reps, int groups, void* stream);
int tg_sum_reps_groups(const float* x, float* out, float alpha, int rows, int cols, int reps, int groups, void* stream);

/* ---------------------------------------------------------------- elementwise */
int tg_add(const float* a, const float* b, float* out, int64_t n, void* stream);
/* out = ((a + b) + c) + d, c / d nullable: the gradient fan-in of a tensor with several consumers (attention.py:22-35: x
 * feeds theta, phi, g and the residual) in one pass */
int tg_add4(const float* a, const float* b, const float* c /*nullable*/, const float* d /*nullable*/, float* out,
            int64_t n, void* stream);
int tg_mul(const float* a, const float* b, float* out, int64_t n, void* stream);
int tg_scale(const float* x, float alpha, float* out, int64_t n, void* stream);
/* out = (alpha * *s) * x, s a device scalar */
int tg_scale_dev(const float* s, float alpha, const float* x, float* out, int64_t n, void* stream);
/* out = *s * a + b  (gamma * o + x, attention.py:35) */
int tg_scale_add_dev(const float* s, const float* a, const float* b, float* out, int64_t n, void* stream);
/* *out = alpha * sum_i a[i]*b[i]  (deterministic two-stage; workspace tg_reduce_workspace(n)) */
size_t tg_reduce_workspace(int64_t n);
int tg_dot(const float* a, const float* b, float alpha, float* out, float* workspace, int64_t n,
           int accumulate, void* stream);
/* out = g * (x >= 0 ? 1 : slope)  (LeakyReLU fwd when g == x; leaky_relu_backward otherwise) */
int tg_lrelu_bwd(const float* g, const float* x, float slope, float* out, int64_t n, void* stream);
int tg_tanh_fwd(const float* x, float* y, int64_t n, void* stream);
/* out = g * (1 - y*y) */
int tg_tanh_bwd(const float* g, const float* y, float* out, int64_t n, void* stream);
/* nn.ELU / nn.SELU (trainers/cnn.py:42-44 --activation elu|selu): y = x > 0 ? scale*x : scale*alpha*(exp(x)-1) */
int tg_elu_fwd(const float* x, float alpha, float scale, float* y, int64_t n, void* stream);
/* order 1: out = g * f'(x) (elu_backward); order 2: out = g * f''(x) (elu_double_backward, the R1 real branch) */
int tg_elu_bwd(const float* g, const float* x, float alpha, float scale, int order, float* out, int64_t n,
               void* stream);
int tg_fill(float* x, float value, int64_t n, void* stream);
/* dst (B, Cd, HW) <- src (B, Cs, HW): channels [0, min(Cs, Cd)) copied, channels >= Cs set to `fill`.  Cd = Cs + 1, fill 1:
 * the all-ones channel that carries the from-RGB bias when discriminator.py:11-22 (1x1) is composed into the first 3x3
 * (blocks/discriminator.py forward_from_rgb; replaces torch.cat + ones); Cd < Cs: its transpose (drop the channel). */
int tg_copy_channels(const float* src, float* dst, int B, int Cs, int Cd, int HW, float fill, void* stream);
/* The shared filter bank (models/shared/blocks.py:124-127, since version 102): every 3x3 convolution of a network reads
 * filters.narrow(0, 0, O).narrow(1, 0, I) of ONE parameter bank [Omax][Imax][taps] (taps = kh * kw).
 *   tg_filter_narrow      view [O][I][taps] <- that corner of the bank, as the dense filter the convolution kernels take
 *   tg_filter_narrow_bwd  accumulate = 0: gbank is written completely -- the corner from gview, exact zeros elsewhere;
 *                         accumulate = 1: gbank's corner += gview, every other element is neither read nor written.
 * O <= Omax and I <= Imax, or TG_EINVAL.  Launches on one stream add in launch order: a deterministic sum.                */
int tg_filter_narrow(const float* bank, float* view, int O, int I, int Omax, int Imax, int taps, void* stream);
int tg_filter_narrow_bwd(const float* gview, float* gbank, int O, int I, int Omax, int Imax, int taps, int accumulate,
                         void* stream);

/* ---------------------------------------------------------------- softmax (attention.py:32) */
int tg_softmax_fwd(const float* s, float* y, int rows, int cols, void* stream);
/* gs = y * (gy - sum(gy*y)) */
int tg_softmax_bwd(const float* gy, const float* y, float* gs, int rows, int cols, void* stream);
/* adjoint of y in gs = softmax_bwd(gy, y) given v = adjoint of gs:
 * out = v*gy - v*sum(gy*y) - gy*sum(v*y)                                        */
int tg_softmax_dbwd(const float* v, const float* gy, const float* y, float* out, int rows, int cols, void* stream);

/* ---------------------------------------------------------------- fused attention core (attention.py:27-34)
 * o = g softmax_m(theta^T phi)^T without materialising the (N x M) map.
 * theta (B,D,N), phi (B,D,M), g (B,DV,M), o (B,DV,N), lse (B,N) = log sum_m exp(score).
 * Compiled for (D,DV) in {(1,4),(2,8),(4,16),(8,32),(16,64)} (C = 8..128); others: TG_EUNSUPPORTED
 * (the host then composes tg_gemm / tg_softmax_*).  The images sit on a grid dimension: B > 65535 is TG_EUNSUPPORTED for
 * tg_attn_fwd, tg_attn_bwd and tg_attn_dbwd alike, nothing launched or written (compose, in slices of the batch).
 * _bwd is the first-order backward;
 * workspace: tg_attn_bwd_workspace() bytes.  Second order (the R1 penalty differentiates _bwd): the
 * host forms the (N x M) maps with tg_gemm and calls tg_attn_dbwd_rows for everything row-wise.       */
int tg_attn_supported(int D, int DV);
size_t tg_attn_bwd_workspace(int B, int D, int DV, int N, int M);
int tg_attn_fwd(const float* theta, const float* phi, const float* g, float* o, float* lse,
                int B, int D, int DV, int N, int M, void* stream);
int tg_attn_bwd(const float* go, const float* theta, const float* phi, const float* g, const float* o,
                const float* lse, float* dtheta, float* dphi, float* dg, float* workspace,
                int B, int D, int DV, int N, int M, void* stream);
/* Row-wise middle of the derivative of tg_attn_bwd.  With a, b, c the adjoints of (dtheta, dphi, dg), on entry
 *   s = theta^T phi,  gp = go^T g,  u = a^T phi + theta^T b,  v = go^T c      (rows = B*N, cols = M, lse as tg_attn_fwd)
 * and on return, in place (P = exp(s - lse); delta, eps, zeta = row sums of P gp, P u, P dP):
 *   s <- P,  gp <- gS = P (gp - delta),  u <- dgP = P (u - eps),  v <- dS = P (dP - zeta),  dP = v + u (gp - delta) - gp eps
 * from which  d theta = phi dS^T + b gS^T,  d phi = theta dS + a gS,  d go = g dgP^T + c P^T,  d g = go dgP.          */
int tg_attn_dbwd_rows(float* s, const float* lse, float* gp, float* u, float* v, int rows, int cols, void* stream);
/* The same derivative in one kernel, no (N x M) map in memory, for key counts a wave can keep a whole row of in
 * registers (M <= 256 at D + DV = 20; fewer for the wider heads): a (B,D,N), b (B,D,M), c (B,DV,M) are the adjoints of
 * tg_attn_bwd's (dtheta, dphi, dg); d_go (B,DV,N), d_theta (B,D,N), d_phi (B,D,M), d_g (B,DV,M) the adjoints of its
 * (go, theta, phi, g).  workspace: tg_attn_dbwd_workspace() bytes.  Otherwise TG_EUNSUPPORTED (compose as above). */
int tg_attn_dbwd_supported(int D, int DV, int M);
size_t tg_attn_dbwd_workspace(int B, int D, int DV, int N, int M);
int tg_attn_dbwd(const float* go, const float* theta, const float* phi, const float* g, const float* lse,
                 const float* a, const float* b, const float* c, float* d_go, float* d_theta, float* d_phi, float* d_g,
                 float* workspace, int B, int D, int DV, int N, int M, void* stream);

/* ---------------------------------------------------------------- IQN head (models/iqn.py)
 * out[i][j] = cos((taus[i] * pi) * range[j])   iqn.py:41-45 (fp32, this evaluation order) */
int tg_iqn_cos_embed(const float* taus, const float* range, float* out, int n, int dims, void* stream);
/* iqn.py:111-130: preds (Q*B), row = q*B + b; target (B); taus (Q*B).
 * *loss = sum_q,b |tau - 1[err<0]| * huber_k(err) / B ; dpreds = d loss / d preds       */
int tg_iqn_loss(const float* preds, const float* target, const float* taus, float k,
                float* loss, float* dpreds, float* workspace, int Q, int B, void* stream);
/* `groups` evaluations back to back (preds / taus rows g*Q*B + q*B + b, target rows g*B + b): *loss = the SUM of their losses
 * (trainers/iqn.py:118-120: loss_real + loss_fake), dpreds per evaluation as above */
int tg_iqn_loss_groups(const float* preds, const float* target, const float* taus, float k,
                       float* loss, float* dpreds, float* workspace, int Q, int B, int groups, void* stream);
/* The head of IQNDiscriminatorOutput behind the pooled features (discriminator.py:149-178 after sum(x, [2, 3]); iqn.py:27-46,
 * 76-108 with mix = 'mult', 111-130), fused: cosine embedding -> Linear(D, C) -> tanh -> * features -> Linear(C, 1) -> quantile
 * mean and quantile Huber loss.  f (G*B, C): the pooled features of G in {1, 2} evaluations back to back; taus (G*Q*B), row
 * r = g*Q*B + q*B + b; target (G*B); W1 (C, D), b1 (C); w2 (C), b2 (1, nullable = 0); range (D).
 *   e[r][j] = cos((taus[r] * pi) * range[j])                     (tg_iqn_cos_embed's evaluation order)
 *   s[r][c] = tanh(b1[c] + sum_j e[r][j] W1[c][j])
 *   p[r]    = b2 + sum_c f[g*B + b][c] * s[r][c] * w2[c]
 *   pt[g*B + b] = (1/Q) sum_q p[r]
 *   *loss   = sum_g (1/B) sum_q,b |tau - 1[err<0]| * huber_k(err),  err = target - p   (the SUM over g, as tg_iqn_loss_groups)
 *   dpreds[r] = d loss / d p[r]
 * tg_iqn_head_fwd writes pt, and *loss and dpreds when `target` is given (then `loss`, `dpreds` and `workspace` of
 * tg_iqn_head_workspace(G, B) bytes are required; without `target` none of the three is touched).  Neither s nor the repeated
 * features are stored: tg_iqn_head_bwd recomputes s.  One workgroup per (g, b) sums its rows in a fixed order, a one-workgroup
 * second launch sums the G*B loss terms (none when G*B == 1; they cross in `workspace` as pairs of 32-bit words): no atomics,
 * bit-identical between runs.
 *
 * tg_iqn_head_bwd: the cotangent of the rows is delta[r] = gl[0] * dpreds[r] + gpt[g*B + b] / Q, each part nullable (`dpreds` is
 * required with `gl`).  Outputs, each nullable:
 *   df[g*B + b][c] = w2[c] * sum_q delta[r] s[r][c]
 *   dw2[c]   = sum_r delta[r] f[..][c] s[r][c]         db2[0]  = sum_r delta[r]
 *   da[r][c] = delta[r] f[..][c] w2[c] (1 - s[r][c]^2) dW1[c][j] = sum_r da[r][c] e[r][j]      db1[c] = sum_r da[r][c]
 * accumulate != 0: dW1, db1, dw2 and db2 are added to (df is always overwritten).  Every output is complete inside one
 * workgroup (a slab of channels walking all rows in a fixed order): no atomics, bit-identical between runs.
 * Every pointer may sit at any multiple of 4 bytes.  A null required pointer, G outside {1, 2}, B, Q, C or D < 1: TG_EINVAL;
 * D > 20: TG_EUNSUPPORTED; nothing launched or written.                                                                          */
size_t tg_iqn_head_workspace(int G, int B);
int tg_iqn_head_fwd(const float* f, const float* taus, const float* target /*nullable*/, const float* W1, const float* b1,
                    const float* w2, const float* b2 /*nullable*/, const float* range, float k, float* pt,
                    float* loss /*nullable*/, float* dpreds /*nullable*/, float* workspace /*nullable*/,
                    int G, int B, int Q, int C, int D, void* stream);
int tg_iqn_head_bwd(const float* gl /*nullable*/, const float* gpt /*nullable*/, const float* dpreds /*nullable*/,
                    const float* f, const float* taus, const float* W1, const float* b1, const float* w2, const float* range,
                    float* df /*nullable*/, float* dW1 /*nullable*/, float* db1 /*nullable*/, float* dw2 /*nullable*/,
                    float* db2 /*nullable*/, int G, int B, int Q, int C, int D, int accumulate, void* stream);

/* ---------------------------------------------------------------- losses
 * nn.BCEWithLogitsLoss (mean) trainers/cnn.py:88,131,147; dlogits = (sigmoid(x)-t)/n    */
int tg_bce_logits(const float* logits, const float* targets, float* loss, float* dlogits,
                  float* workspace, int n, void* stream);
/* InfoGAN code loss (trainers/info.py:139-151, 167-180), forward and gradient in ONE launch.  codes: (B, C + K) dense logits;
 * z: (B, ldz) latents, ldz >= C + K, whose first C + K columns are the targets, read in place.
 *   cat  = mean over B*C of  max(x,0) - x*t + log1p(exp(-|x|))     (absent when C == 0)
 *   cont = mean over B*K of  (x - t)^2                             (absent when K == 0)
 *   out[0] = cat + cont;   out[1] = (base ? *base : 0) + w * out[0]
 *   dcodes[b][c] = w (sigmoid(x) - t) / (B*C);   dcodes[b][C+k] = w 2 (x - t) / (B*K)
 * One workgroup sums everything in a fixed order: no atomics, bit-identical between runs; `workspace` is not used (nullable;
 * tg_reduce_workspace(B * (C + K)) is enough for any later version).  Every pointer may sit at any multiple of 4 bytes.
 * B < 1, C < 0, K < 0, C + K == 0, ldz < C + K or a null codes / z / out / dcodes: TG_EINVAL, nothing written.                 */
int tg_info_code_loss(const float* codes, const float* z, const float* base, float w, float* out, float* dcodes,
                      float* workspace, int B, int C, int K, int ldz, void* stream);
/* *out = alpha * sum x^2  (R1: grad.pow(2).view(B,-1).sum(1).mean(), losses.py:27-29)   */
int tg_sumsq(const float* x, float alpha, float* out, float* workspace, int64_t n, void* stream);

/* ---------------------------------------------------------------- spectral norm (north_star a15)
 * The reference never applies spectral norm (prep4web.py:24,33-51 only strips torch.nn.utils.spectral_norm
 * from a checkpoint); the hook is every block's conv_factory (discriminator.py:28,52, generator.py:34,117).
 * Semantics pinned against torch.nn.utils.spectral_norm:  n_iter x { v = normalize(W^T u, eps);
 * u = normalize(W v, eps) } in place, then *sigma = u^T W v (sigma nullable).  W: rows x cols row-major.    */
int tg_sn_power_iter(const float* W, float* u, float* v, float* sigma /*nullable*/,
                     int rows, int cols, int n_iter, float eps, void* stream);
/* out = 1 / x */
int tg_recip(const float* x, float* out, int64_t n, void* stream);
/* The same for every layer of a network at once (tg_version 107): ONE power iteration, sigma, the normalised weight and its
 * backward, in a number of launches that does not depend on the number of layers (4 forward with update, 2 without, 2 backward,
 * per group of 48 layers).  `items` is a HOST array of n_items x TG_SN_ITEM_FIELDS 64-bit words, read during the call only:
 *   [0] w_orig  [1] u  [2] v  [3] w_sn  [4] g_sn  [5] g_orig  (device addresses; [4], [5] may be 0 for the forward)
 *   [6] rows  [7] cols                                          (w_orig, w_sn, g_sn, g_orig: rows x cols row-major)
 * tg_sn_batch_fwd  update != 0: v = normalize(W^T u, eps), u = normalize(W v, eps) in place (x / max(|x|, eps), as torch);
 *                  update == 0: u, v are only read.  Either way sigma[i] = u^T W v and w_sn = w_orig / sigma[i].
 * tg_sn_batch_bwd  g_orig += (g_sn - <g_sn, w_sn> u v^T) / sigma[i]: the gradient of W / sigma(W) with u, v constant, from the
 *                  sigma a forward call left; clear != 0 leaves g_sn all zeros, clear == 0 leaves it untouched.
 * workspace: tg_sn_batch_workspace(items, n_items) bytes (0 for a table the calls below refuse), scratch within one call.
 * Stages are ordered by launch boundaries alone; every sum runs in one fixed order (two calls give the same bits).
 * Every device pointer may sit at any multiple of 4 bytes: float4 accesses are used where the pointers involved are 16-byte
 * aligned and cols % 4 == 0, a scalar path otherwise, and both give the same bits.  A layer may appear once per call.
 * n_items < 1, a null items / sigma / workspace, a zero address among [0..3] (backward: [0..5]), an address that is no multiple
 * of 4, rows or cols < 1: TG_EINVAL; rows * cols >= 2^31: TG_EUNSUPPORTED; a workspace below the query: TG_EWORKSPACE; nothing
 * launched or written in any of these cases.                                                                                  */
#define TG_SN_ITEM_FIELDS 8
size_t tg_sn_batch_workspace(const tg_host_i64* items /*host*/, int n_items);
int tg_sn_batch_fwd(const tg_host_i64* items /*host*/, int n_items, float* sigma /*device, n_items floats*/, float* workspace,
                    size_t workspace_bytes, int update, float eps, void* stream);
int tg_sn_batch_bwd(const tg_host_i64* items /*host*/, int n_items, const float* sigma, float* workspace, size_t workspace_bytes,
                    int clear, void* stream);

/* ---------------------------------------------------------------- optimiser / EMA
 * torch.optim.Adam (trainers/cnn.py:84-85), single flat tensor.
 * hyper (device, 6 floats): [lr/bias_correction1, sqrt(bias_correction2), beta1, beta2,
 * 1-beta1, 1-beta2] (host doubles rounded to fp32) so the captured graph is step-independent:
 *   m = lerp(m, g, 1-beta1); v = beta2*v + (1-beta2)*g*g;
 *   p -= hyper[0] * m / (sqrt(v)/hyper[1] + eps)                                        */
int tg_adam_step(float* p, const float* g, float* m, float* v, const float* hyper, float eps,
                 int64_t n, void* stream);
/* update_target_generator (trainers/cnn.py:158-165): t += (p - t) * lr */
int tg_ema(float* t, const float* p, float lr, int64_t n, void* stream);

/* ---------------------------------------------------------------- FID / Inception-score math
 * inception_utils.py:97-124 torch_cov, :129-144 sqrt_newton_schulz, :205-235 torch_calculate_frechet_distance,
 * :239-246 calculate_inception_score -- everything after the (network-less) pooled features / softmax outputs.   */
/* C (M x N) = alpha * op(A) B + diag * I on the fp32 matrix cores, row-major, 128 x 128 tiles staged by LDS-DMA.
 * transA: A is (K x M) and A^T is used (the covariance product X_c^T X_c).  The Newton-Schulz step
 * T = 0.5 (3 I - Z Y) is one call with alpha = -0.5, diag = 1.5.  Needs lda, ldb, K % 4 == 0 and 16-byte aligned
 * A, B (tg_gemm_big_supported); otherwise TG_EUNSUPPORTED (use tg_gemm).                                          */
int tg_gemm_big_supported(int M, int N, int K, int lda, int ldb, int transA);
int tg_gemm_big(const float* A, const float* Bm, float* C, int M, int N, int K, int lda, int ldb, int ldc,
                int transA, float alpha, float diag, void* stream);
/* X[n][d] -= mean[d]  (torch_cov centres its argument in place, inception_utils.py:120) */
int tg_center_rows(float* X, const float* mean, int N, int D, void* stream);
/* out[0] = trace(A), A (D x D) with leading dimension ld */
int tg_trace(const float* A, float* out, int D, int ld, void* stream);
/* rows[n] = sum_c p[n][c] * (log p[n][c] - log mean[c])  (the KL term of calculate_inception_score) */
int tg_is_kl_rows(const float* p, const float* mean, float* rows, int N, int Cn, void* stream);

/* ---------------------------------------------------------------- Inception-v3 forward (the network itself)
 * What torchvision's Inception3 runs in eval mode between the preprocess above and the FID math: BasicConv2d =
 * nn.Conv2d(bias=False) -> nn.BatchNorm2d(eps=0.001) -> F.relu, F.max_pool2d(3, stride=2), F.avg_pool2d(3, stride=1,
 * padding=1) and torch.cat over channels.  Forward only.
 *
 * tg_inception_conv_fwd: y[:, y_coff : y_coff + Cout] = act(conv2d(x[:, x_coff : x_coff + Cin], w, stride, (ph, pw)) + bias)
 * as an implicit GEMM on the fp32-input MFMA (M = Cout, N = B * OH * OW, K = Cin * KH * KW; exact fp32, no atomics,
 * bit-identical from run to run).  x is (B, x_ctot, H, W), y is (B, y_ctot, OH, OW) with OH = (H + 2 ph - KH) / stride + 1
 * (OW alike); channels outside the two slices are neither read nor written, so branches of a Mixed block write straight into
 * its concatenated output and stacked 1x1 branches are read back by slices.  Any KH x KW (1x1, 3x3, 5x5, 1x7, 7x1, 1x3, 3x1,
 * ...), stride 1 or 2, any zero padding per axis, any Cin / Cout.  bias (nullable, Cout floats) carries the folded BatchNorm;
 * relu != 0 applies max(., 0).
 * wp is the filter PACKED BY THE HOST, once per model: tg_inception_conv_weight_floats(Cin, Cout, KH, KW) floats, 16-byte
 * aligned, wp[k][co] with row length CoutP = Cout rounded up to 128 and Kp = K rounded up to 16 rows, k = (ci * KH + kh) * KW
 * + kw (the OIHW filter flattened and transposed), zero in the padding.                                               */
size_t tg_inception_conv_weight_floats(int Cin, int Cout, int KH, int KW);
int tg_inception_conv_supported(int B, int Cin, int Cout, int H, int W, int KH, int KW, int stride, int ph, int pw,
                                int x_ctot, int y_ctot);
int tg_inception_conv_fwd(const float* x, const float* wp, const float* bias /*nullable*/, float* y, int B, int Cin, int Cout,
                          int H, int W, int KH, int KW, int stride, int ph, int pw, int relu, int x_ctot, int x_coff,
                          int y_ctot, int y_coff, void* stream);
/* F.max_pool2d(x, 3, stride=2) (no padding: OH = (H - 3) / 2 + 1) and F.avg_pool2d(x, 3, stride=1, padding=1) (divides by 9
 * everywhere, count_include_pad=True) of channels [x_coff, x_coff + C) into channels [y_coff, y_coff + C). */
int tg_inception_maxpool3s2(const float* x, float* y, int B, int C, int H, int W, int x_ctot, int x_coff, int y_ctot,
                            int y_coff, void* stream);
int tg_inception_avgpool3(const float* x, float* y, int B, int C, int H, int W, int x_ctot, int x_coff, int y_ctot,
                          int y_coff, void* stream);

/* ---------------------------------------------------------------- scene structure stage (since version 101)
 * SceneStructureBlock.forward (models/blocks/scene.py:127-155): per patch p, F.affine_grid(theta[:, p], (B, 1, S, S),
 * align_corners=False) and F.grid_sample(m[:, p], grid, 'bilinear', 'zeros', align_corners=False), stacked to (B, P, S, S);
 * the sigmoid, the `1 -`, the noise multiply, the loop over the patches and the stack / permute are all inside one launch.
 *   theta        (B, P*6)            what the patch_transforms Linear writes: [b][p][row 0..1][col 0..2]
 *   mask_logits  (B, P*patch*patch)  raw output of the masks Linear; NULL = an opaque patch of ones (the full_masks branch)
 *   noise        (patch, patch)      shared by every b and p; NULL = no noise
 *   out          (B, P, S, S)        written completely
 * Texel m[b,p,v,u] = (mask_logits ? 1 - sigmoid(l) : 1) * (noise ? noise[v,u] : 1); base grid x_j = (2j+1)/S - 1, y_i alike;
 * gx = t00 x + t01 y + t02, gy = t10 x + t11 y + t12; sample at ix = ((gx+1) patch - 1)/2, iy alike; the four bilinear corners
 * contribute zero where they fall outside the patch.
 * tg_scene_patches_bwd: gtheta (B, P*6) and gmask_logits (B, P*patch*patch; NULL exactly when mask_logits is NULL) are written
 * completely (zeros for texels no sample touches); noise gets no gradient.  Every sum has a fixed order (no atomics): two runs
 * on the same inputs are bit-identical.
 * 1 <= patch <= 16 (TG_EUNSUPPORTED above), any S, B, P >= 1, pointers at any multiple of 4 bytes; no workspace.          */
int tg_scene_patches_fwd(const float* theta, const float* mask_logits /*nullable*/, const float* noise /*nullable*/, float* out,
                         int B, int P, int patch, int S, void* stream);
int tg_scene_patches_bwd(const float* gout, const float* theta, const float* mask_logits /*nullable*/,
                         const float* noise /*nullable*/, float* gtheta, float* gmask_logits /*nullable*/,
                         int B, int P, int patch, int S, void* stream);

/* ---------------------------------------------------------------- text trainer (since version 105)
 * nn.Conv1d(k=3, padding=1) / nn.Conv1d(k=1) over (B, C, L): the residual blocks of trainers/text_cnn.py:57-80 built with
 * conv_factory=nn.Conv1d, L = 4 .. 64 tokens.  ks in {1, 3}, stride 1, zero padding ks / 2; x (B, Cin, L), w (Cout, Cin, ks).
 * Implicit GEMMs on the fp32-input MFMA with the batch-flattened B * L token axis as the long side, so short sequences
 * still fill tiles; a tile may span several sequences, and every sequence is zero-padded at ITS OWN ends.  Exact fp32, no
 * atomics, bit-identical from run to run; pointers at any multiple of 4 bytes.  Other ks, or a shape whose 32-bit indexes
 * would overflow (tg_conv1d_supported == 0): TG_EUNSUPPORTED, nothing written.
 * tg_conv1d_wgrad: gw[co][ci][t] = sum_{b,l} gy[b][co][l] x[b][ci][l + t - ks/2] and, when gbias != NULL, gbias[co] =
 * sum_{b,l} gy from the same pass; two stages (per-workgroup partials over slices of B * L in `workspace`, then a
 * fixed-order sum); accumulate != 0 adds into gw / gbias; a workspace below tg_conv1d_wgrad_workspace(): TG_EWORKSPACE. */
int tg_conv1d_supported(int B, int Cin, int Cout, int L, int ks);
int tg_conv1d_fwd(const float* x, const float* w, const float* bias /*nullable*/, const float* residual /*nullable, shape of y*/,
                  float* y, int B, int Cin, int Cout, int L, int ks, void* stream);
int tg_conv1d_dgrad(const float* gy, const float* w, float* gx, int B, int Cin, int Cout, int L, int ks, void* stream);
size_t tg_conv1d_wgrad_workspace(int B, int Cin, int Cout, int L, int ks);
int tg_conv1d_wgrad(const float* x, const float* gy, float* gw, float* gbias /*nullable*/, float* workspace, size_t workspace_bytes,
                    int B, int Cin, int Cout, int L, int ks, int accumulate, void* stream);
/* F.interpolate(scale_factor=2) on (B, C, L) (generator.py:58) and nn.AvgPool1d(2) (discriminator.py:67), transposes of each
 * other up to a factor:  up2x1d: y[bc][2l + d] = alpha * x[bc][l];  pool2_1d: y[bc][l] = residual + 0.5 (x[bc][2l] + x[bc][2l+1]).
 * L is the length of the SHORT side for both (x of up2x1d, y of pool2_1d).  The discriminator block's
 * F.interpolate(scale_factor=0.5, mode='linear', align_corners=False) on an even length is tg_pool2_1d exactly. */
int tg_up2x1d(const float* x, float* y, float alpha, int BC, int L, void* stream);
int tg_pool2_1d(const float* x, const float* residual /*nullable*/, float* y, int BC, int L, void* stream);
/* One skip-gram step (models/text.py:42-55, its sparse backward + coalesce, torch.optim.SGD; trainers/text_cnn.py:162-182) in
 * two launches.  U, V (vocab, E) are updated IN PLACE; words (B), contexts (B, C2), negatives (B, C2) int64.
 *   loss_out[0] = -(1/B) sum_b sum_j [log sigmoid(V[ctx_bj] . U[w_b]) + log sigmoid(-V[neg_bj] . U[w_b])]
 * from the tables as they were on entry (log sigmoid in its stable form: scores of +-90 give finite values and saturated
 * gradients), then T[r] -= lr * g[r] for both tables, g from the pre-update values, all occurrences of a row summed in a
 * fixed order (words in batch order; contexts in (b, j) order, then negatives).  Rows equal to padding_idx (< 0: none) and
 * rows no index names stay bit-unchanged.  No atomics, bit-identical from run to run.
 * An index outside [0, vocab) is NOT refused (that would need a device-to-host read) and is never dereferenced: it reads as
 * a row of zeros and receives no update; callers that want the reference's IndexError check the indexes on the host.
 * E > 1024 or 2 * B * C2 > 65536: TG_EUNSUPPORTED; U == V or a null pointer: TG_EINVAL; nothing written either way. */
size_t tg_skipgram_workspace(int B, int C2, int E);
int tg_skipgram_step(float* U, float* V, const int64_t* words, const int64_t* contexts, const int64_t* negatives, float lr,
                     int padding_idx, float* loss_out, float* workspace, size_t workspace_bytes, int B, int C2, int E, int vocab,
                     void* stream);
/* embedding(idx).permute(0, 2, 1) (trainers/text_cnn.py:186): out[b][e][l] = U[idx[b][l]][e], copy-exact, rows read along e and
 * written along l through an LDS tile.  An index outside [0, vocab) writes zeros. */
int tg_embed_gather_t(const float* U, const int64_t* idx, float* out, int B, int L, int E, int vocab, void* stream);
/* SkipGram.lookup (models/text.py:57-69): out[b][l] = argmax_{i >= 1} (U[i] . z[b, :, l]) / |U[i]|, z (B, E, L), out (B, L)
 * int64.  The reference's quirk is kept: row 0 is skipped and the result counts from row 1 (0 means row 1).  First maximum
 * on exact ties, NaN (a zero row) counts as largest, like torch.argmax.  vocab < 2: TG_EINVAL; E > 1024: TG_EUNSUPPORTED. */
int tg_embed_lookup(const float* U, const float* z, int64_t* out, int B, int L, int E, int vocab, void* stream);

/* ---------------------------------------------------------------- input pipeline
 * ImageBytesDataset (image_bytes_dataset.py:12-49) + ToPILImage -> RandomCrop(size) -> ToTensor -> Normalize(.5, .5)
 * (trainers/trainer.py:69-78) for a whole batch: archive = device-resident uint8 (n_images, H, W, channels) exactly
 * as np.savez_compressed stores it, index[b] = image of batch row b (device int64), crop_y / crop_x = top-left corner
 * of the size x size crop per row (device int32, nullable = 0: image size == crop size, where RandomCrop draws nothing).
 * out (B, channels, size, size) fp32 = ((u8 / 255) - 0.5) / 0.5 in ToTensor's / Normalize's operation order.
 * The caller guarantees 0 <= index < n_images and crop + size <= H, W.  out must be 16-byte aligned (TG_EUNSUPPORTED
 * otherwise); archive, index and the crops may sit at any multiple of their element size.                         */
int tg_image_bytes_batch(const uint8_t* archive, const int64_t* index, const int* crop_y /*nullable*/,
                         const int* crop_x /*nullable*/, float* out, int B, int64_t n_images, int H, int W,
                         int channels, int size, void* stream);

/* ---------------------------------------------------------------- explore apps (tartangan_amd/explore/, csrc/explore.hip; tg_version 106)
 * All three: fp32, no atomics, sums in a fixed order (bit-identical between runs); every pointer may sit at any multiple of its
 * element size; a bad argument returns before anything is launched or written.
 *
 * find_image.py:59-68 without --vgg: the reconstruction loss of generator output against a normalised target and its image gradient.
 * imgs, target, grad_imgs: (B, 3, HW).  With mean = (0.485, 0.456, 0.406), std = (0.229, 0.224, 0.225) (find_image.py:99-100):
 *   d = ((x + 1) / 2 - mean_c) / std_c - t
 *   kind 0 (nn.MSELoss(reduction='sum')):       *loss_out = sum d^2,       rho'(d) = 2 d
 *   kind 1 (nn.SmoothL1Loss(reduction='sum')):  *loss_out = sum (|d| < 1 ? d^2 / 2 : |d| - 1/2),   rho'(d) = |d| < 1 ? d : sign(d)
 *   grad_imgs = rho'(d) / (2 std_c)             (nullable: the loss alone, e.g. an L-BFGS closure's re-evaluations)
 * At most two launches (one when B*3*HW <= 1024).  workspace: tg_recon_loss_workspace(B, C, HW) bytes, NaN-safe (written before
 * read); smaller: TG_EWORKSPACE.  C != 3, another kind, B or HW < 1, a null imgs / target / loss_out: TG_EINVAL.  The query
 * returns 0 for arguments tg_recon_loss refuses.                                                                             */
size_t tg_recon_loss_workspace(int B, int C, int HW);
int tg_recon_loss(const float* imgs, const float* target, float* grad_imgs /*nullable*/, float* loss_out, float* workspace,
                  size_t workspace_bytes, int B, int C, int HW, int kind, void* stream);
/* Everything a find-image step does to the latents after the backward pass (find_image.py:56-86), ONE launch of one workgroup over
 * n = num_samples * latent_dims elements.  In this order:
 *   1. stats[0] = *recon_loss + l2 * mean(z^2)                 the reported loss, from z before the update
 *   2. g = gz + 2 l2 z / n
 *   3. opt 0: torch.optim.Adam's default update of z (no weight decay, no amsgrad, bias correction from the counter *step, which
 *      lives on the device: this launch uses *step + 1 and stores it, so the launch replays from a graph unchanged);
 *      opt 1: z -= lr g                                        (m, v, step are not touched and may be null)
 *   4. stats[1], stats[2], stats[3] = min, mean, max of the updated z   (min and max are NaN when z holds one, as torch's)
 *   5. noise_next != null: z = noise_next where z > 3 or z < -3, strictly (find_image.py:77-81, the clip in front of the NEXT
 *      step); NaN is not clipped.
 * opt 2 does 5. alone (the clip in front of the first step): z and noise_next only, every other pointer may be null.
 * z, m, v and *step are updated in place.  n < 1, another opt, a beta outside [0, 1), a null pointer the opt needs: TG_EINVAL. */
int tg_latent_step(float* z, const float* gz, float* m, float* v, int64_t* step, const float* noise_next /*nullable*/,
                   float* stats, const float* recon_loss, int64_t n, int opt, double lr, double beta1, double beta2, double eps,
                   double l2, void* stream);
/* continuous_interp.py:36-52 as one gather.  imgs: (rows * cols, C, h, w), out: (C, S, S):
 *   out[c][y][x] = imgs[(y * rows) / S * cols + (x * cols) / S][c][(y * h) / S][(x * w) / S]        (integer division)
 * which equals the reference's int(a * b / S) for every index in range.  Copy-exact.  A non-positive dimension: TG_EINVAL.   */
int tg_mosaic_gather(const float* imgs, float* out, int rows, int cols, int C, int h, int w, int S, void* stream);

/* ---------------------------------------------------------------- dataset building (tartangan_amd/image_folder_dataset.py, csrc/dataset.hip; tg_version 110)
 * Pillow's two-pass separable resampler for 8-bit interleaved images (Resample.c, 8bpc) with host-supplied fixed-point taps: what
 * Image.resize((OW, OH), LANCZOS) computes, bit for bit, for a batch of same-shaped images.
 *   src (N, H, W, C), dst (N, OH, OW, C), C = 1 or 3 (otherwise TG_EUNSUPPORTED)
 *   kx (OW, ksx) int32 taps scaled by 2^22, bx (OW, 2) = (first input column, tap count) per output column; ky (OH, ksy), by (OH, 2)
 *   the same for rows.  kx null: no horizontal pass, W == OW required; ky null: no vertical pass, H == OH required; both null is
 *   TG_EINVAL (the caller copies).  With both passes tmp is (N, H, OW, C): HORIZONTAL FIRST, the intermediate clipped to uint8.
 * Per output sample: acc = 2^21 + sum_j pixel[first + j] * k[j] in 32 bits with unsigned wrap-around, out = clip((int32)acc >> 22,
 * 0, 255).  No atomics; integer sums are order-free.  The byte pointers may sit at any address, the int32 tables at any multiple
 * of 4; all indexing is 64-bit.
 * The bounds decide what is read, so they are copied to the host and checked before anything is launched (the call synchronises
 * the stream and does not replay from a graph): first < 0, count < 0, count > ks or first + count past the input is TG_EINVAL, as
 * are a null src / dst / bounds / missing tmp and a non-positive size; nothing is written then.  TG_EUNSUPPORTED: the input span
 * of 64 neighbouring output columns exceeds 64 KiB (about 21 000 RGB pixels): resize such an image on the host.              */
int tg_resample_u8(const uint8_t* src, uint8_t* dst, uint8_t* tmp /*nullable*/, const int32_t* kx /*nullable*/,
                   const int32_t* bx /*nullable*/, const int32_t* ky /*nullable*/, const int32_t* by /*nullable*/, int N, int H,
                   int W, int C, int OH, int OW, int ksx, int ksy, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TARTANGAN_AMD_H */
