/*
 * reidgan_hip.h — C ABI of libreidgan_hip.so, the MI355X (gfx950) kernel library behind the
 * ReID-GAN training step (joint FD-GAN + cluster-contrast).
 *
 * The reference (daemon-219/ReID-GAN) has no FFI: its hot path is torch.nn modules calling
 * cuDNN/cuBLAS/ATen.  Each entry point below replaces the ATen/cuDNN work behind one family of
 * reference call sites (cited per function as FD/ = FD-GAN-master/, CC/ = cluster-contrast-reid-main/).
 * The host side that binds them with ctypes lives in reid-gan_amd/rg_hip/lib.py; INTEGRATION.md
 * shows the stub a reference maintainer would add.
 *
 * Contract (every function):
 *   - returns 0 (RG_OK) or a negative status; rg_last_error() gives the message (thread local);
 *   - plain pointers to DEVICE memory and sizes; tensors are contiguous fp32 NCHW, labels int64;
 *   - asynchronous on `stream`; never allocates, frees or synchronises (rg_profile_collect excepted; the first call of a
 *     convolution geometry outside a stream capture waits once for a timing of its candidate kernels on `stream`: rg_conv_tune_stats);
 *   - scratch comes from the caller: `workspace`/`workspace_bytes`, sized by the *_workspace query;
 *   - pointers must be 16-byte aligned (torch allocations are).
 */
#ifndef REIDGAN_HIP_H
#define REIDGAN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ihipStream_t* rg_stream_t; /* == hipStream_t */

#define RG_OK 0
#define RG_ERR_INVALID (-1)
#define RG_ERR_LAUNCH (-2)
#define RG_ERR_WORKSPACE (-3)

/* activation codes of the fused epilogues */
#define RG_ACT_NONE 0
#define RG_ACT_RELU 1
#define RG_ACT_LEAKY 2
#define RG_ACT_TANH 3

const char* rg_last_error(void);
int rg_version(void);

/* ---- per-family launch profiler (HIP events on the launch stream; used by bench.py) ---------- */
#define RG_FAMILY_COUNT 11 /* conv_fwd, conv_dgrad, conv_wgrad, norm, eltwise, pool, loss, cm, optim, misc, conv_f8 */
int rg_family_count(void);
int rg_profile_enable(int on);
int rg_profile_reset(void);
int rg_profile_collect(double* ms, double* flops, double* bytes, long long* calls); /* synchronises events */

/* ---- convolution: implicit GEMM, fp32 tensors, split-bf16 arithmetic on v_mfma_f32_32x32x16_bf16 ----
 * (every fp32 operand is split exactly into three bf16 pieces and each product evaluated as the six partial products of weight
 * >= 2^-16 with fp32 accumulation: the error model of an fp32 FMA chain, csrc/conv_igemm.hip and conv_core.h).
 * Overflow is NOT fp32's: an operand that is +-Inf, or finite but above the
 * largest bf16 (|x| >= 3.3961e38: its leading piece rounds to Inf), makes its products NaN (Inf - Inf in the split) where an fp32
 * FMA chain would give +-Inf; nothing in the reference's training range comes within 30 orders of magnitude of that)
 * Replaces nn.Conv2d / nn.ConvTranspose2d of the ResNet-50 trunk (CC/clustercontrast/models/
 * resnet_ibn_a.py:70-159, FD/reid/models/resnet.py:65-75), CustomPoseGenerator
 * (FD/fdgan/networks.py:86-138) and NLayerDiscriminator (FD/fdgan/networks.py:206-232), and
 * nn.Linear / Tensor.mm (FD/reid/models/embedding.py:21-24, CC/clustercontrast/models/cm.py:16,26)
 * as 1x1 geometry.
 * Geometry: x[N][C][H][W], w[K][C][KH][KW], y[N][K][P][Q]; y = act(conv(x,w)*scale[k] + shift[k] + residual).
 * scale/shift/residual may be NULL. dgrad computes dx from dy (== ConvTranspose2d forward with
 * dy as its input and dx[N][C][H][W] as its output; epilogue indexed by c). Stride <= 2 for dgrad.
 */
size_t rg_conv2d_fwd_workspace(int N, int C, int K, int KH, int KW, int P, int Q);
/* w_krsc (optional, may be NULL): the weights re-laid out as [K][KH*KW][C] by rg_weights_to_krsc.  With it the
 * kernels walk the reduction (r,s)-major, so the padding test of the pixel gather happens once per 16-deep k-tile
 * (fwd, C % 16 == 0) and the weight operand of the data gradient is contiguous (float4 loads; K % 16 == 0,
 * C % 4 == 0); NULL selects the generic loaders.  Workspace: split-K scratch for layers too small to fill the chip
 * (dgrad: stride 1 only); a too-small workspace just disables the split.  Every tensor must be < 2 GiB. */
int rg_conv2d_fwd(const float* x, const float* w, const float* w_krsc, float* y, int N, int C, int H, int W, int K,
                  int KH, int KW, int SH, int SW, int PH, int PW, int P, int Q, const float* scale, const float* shift,
                  const float* residual, int act, float slope, void* workspace, size_t workspace_bytes,
                  rg_stream_t stream);
size_t rg_conv2d_dgrad_workspace(int N, int C, int H, int W, int K, int KH, int KW, int SH, int SW);
/* relu_mask (dgrad only, may be NULL): a tensor shaped like dx; after scale/shift/residual/act the result is zeroed where
 * relu_mask <= 0.  Passing the convolution's own forward INPUT (the ReLU output of the layer below) makes this the
 * ReLU backward of that layer, applied to the sum of this data gradient and `residual` (the skip gradient). */
int rg_conv2d_dgrad(const float* dy, const float* w, const float* w_krsc, float* dx, int N, int C, int H, int W, int K,
                    int KH, int KW, int SH, int SW, int PH, int PW, int P, int Q, const float* scale,
                    const float* shift, const float* residual, int act, float slope, const float* relu_mask,
                    float* rowsum, int rowsum_cols, void* workspace, size_t workspace_bytes, rg_stream_t stream);
/* rowsum (dgrad only, may be NULL): [C][rowsum_cols] — per input channel, the sums of the FINAL dx values over blocks of
 * pixels (one column per class, pixel tile and wave column; fixed summation order).  Their sum over the columns is the
 * per-channel sum of dx: exactly the `partials` rg_bn_fold_wgrad of the layer below needs (dbeta / dgamma), so that layer does
 * not read dx again.  rowsum_cols must equal rg_conv2d_dgrad_rowsum_cols(...), which is 0 when the launch would use split-K
 * or the small-C kernel (no fused row sums there). */
int rg_conv2d_dgrad_rowsum_cols(int N, int C, int H, int W, int K, int KH, int KW, int SH, int SW, int PH, int PW, int P,
                                int Q);
int rg_weights_to_krsc(const float* w, float* w_krsc, int K, int C, int KH, int KW, rg_stream_t stream);
/* the same re-layout for every filter of a network in ONE launch: `table` (device memory) holds `count` entries of 6 int64 words
 * {w, w_krsc, K, C, KH*KW, first block}, filters are cut into blocks of rg_krsc_chunk() elements, total_blocks = sum of the blocks */
int rg_krsc_chunk(void);
int rg_weights_to_krsc_multi(const void* table, int count, int total_blocks, rg_stream_t stream);
/* development knob: pin the fwd/dgrad planner's tile (0: 128x128, 1: 64x128, 2: 64x64, 3: 32x256) and split-K count;
 * (-1, -1) releases it (same effect as the RG_CONV_FORCE="tile,splits" environment variable) */
int rg_conv_set_force(int tile, int splits);
/* development knob: bit mask of the conv kernel families that run on the bf16-plane operand path of csrc/conv_planes.h (operands
 * split into their bf16 pieces once, on the way into LDS) instead of the default kernels: 1 forward, 2 data gradient, 4 weight
 * gradient, 8: with a family bit, the eight-wave form of the 128 x 128 tile; identical results up to fp32
 * summation order.  Returns the previous mask. */
int rg_conv_set_planes(int mask);
/* The generic fwd / dgrad / wgrad kernels exist in two implementations (default kernels and the plane path above); unless one is
 * forced (rg_conv_set_planes, RG_CONV_TUNE=0) the first call of a geometry outside a stream capture times both on the launch
 * stream and the faster serves that geometry from then on (the first call's output already comes from it); the tile / split-K plan
 * of a forward geometry and the tap-reuse-vs-generic path of a 3x3 layer are chosen the same way.  Returns the number of choices
 * measured so far; out[0] / out[1] (int[2], may be NULL): how many kernel choices went to the default kernels / the plane path. */
int rg_conv_tune_stats(int* out);
/* development knob (tests): pin one level of the measured choice above.  `kind` is the first field of the choice key as written to
 * RG_CONV_TUNE_CACHE: 1 / 2 / 4 kernel implementation (fwd / dgrad / wgrad), 16 / 32 tap-reuse vs generic path (fwd / dgrad),
 * 64 / 128 / 256 tile / split-K plan (fwd / dgrad / wgrad).  index >= 0 pins that kind: every choice of the kind runs candidate
 * min(index, ncand - 1) at once (before the plane-path mask and RG_CONV_TUNE are consulted), without measuring, synchronising or
 * recording anything (rg_conv_tune_stats and the cache file are untouched); -1 releases it.  It pins choices, it does not create
 * them: with RG_CONV_TUNE=0 a geometry has one plan and no path choice.  Returns the previous index (-1: not
 * pinned), or a value below -1 for an unknown kind / an index below -1 (rg_last_error).  Off by default. */
int rg_conv_set_pick(int kind, int index);
/* while any kind is pinned, every choice appends one record of 18 ints: the 16 key fields, its candidate count and the index that
 * ran.  Copies up to max_records records into buf (HOST memory, may be NULL), clears the log and returns how many it held. */
int rg_conv_pick_log(int* buf, int max_records);
/* Split-K without the finishing launch.  Registers (count > 0) or removes (counters == NULL) the arrival counters of `stream`:
 * `count` ZERO-INITIALISED 32-bit words of device memory that the caller keeps alive and never writes (the library does not
 * allocate; launches on one stream are ordered and every launch leaves its counters at zero, so one buffer per stream serves all of
 * them).  With counters registered, a split forward / unit-stride data-gradient launch on that stream with <= count output tiles
 * finishes inside the convolution kernel: the last split of a tile to arrive sums the tile's partials in split order and applies
 * the epilogue — the finishing kernel's values bit for bit, whichever split arrives last.  Without them, or inside a stream capture,
 * the finishing kernel follows as before.  (Measured equal to the finishing kernel within +-1 % on the FD-GAN step: rg_hip registers
 * counters only with RG_SPLITK_INKERNEL=1.) */
int rg_conv_splitk_arrivals(void* counters, int count, rg_stream_t stream);
/* test / development query: the number of split-K launches that finished inside the convolution kernel so far (this process) */
int rg_conv_splitk_inkernel_count(void);
size_t rg_conv2d_wgrad_workspace(int N, int C, int K, int KH, int KW, int P, int Q);
int rg_conv2d_wgrad(const float* x, const float* dy, float* dw, int N, int C, int H, int W, int K, int KH, int KW,
                    int SH, int SW, int PH, int PW, int P, int Q, void* workspace, size_t workspace_bytes,
                    rg_stream_t stream);

/* ---- BatchNorm 1d/2d on [N][C][HW] ------------------------------------------------------------
 * Replaces nn.BatchNorm2d/1d (FD/fdgan/networks.py:26-35; resnet_ibn_a.py:75-81; FD/reid/models/
 * embedding.py:16-19; CC/clustercontrast/models/resnet.py:58-66). `stat` is invstd (train, from
 * rg_bn_stats) or the running variance when stat_is_var != 0 (eval). The apply kernels fuse an
 * optional residual add and activation; the backward takes the forward OUTPUT for the mask. */
size_t rg_bn_workspace(int N, int C, int HW);
int rg_bn_stats(const float* x, float* mean, float* invstd, float* running_mean, float* running_var, int N, int C,
                int HW, float eps, float momentum, void* workspace, size_t workspace_bytes, rg_stream_t stream);
int rg_bn_apply_fwd(const float* x, const float* mean, const float* stat, const float* gamma, const float* beta,
                    const float* residual, float* y, int N, int C, int HW, int stat_is_var, float eps, int act,
                    float slope, rg_stream_t stream);
int rg_bn_bwd_reduce(const float* x, const float* dy, const float* y_act, const float* mean, const float* stat,
                     float* sum_dy, float* sum_dy_xhat, int N, int C, int HW, int stat_is_var, float eps, int act,
                     float slope, void* workspace, size_t workspace_bytes, rg_stream_t stream);
/* Train-mode torch.nn.BatchNorm2d / 1d (FD/fdgan/networks.py:28, CC/clustercontrast/models/resnet.py trunk) in one launch per
 * direction for small per-channel extents (rg_bn_train_fused_ok: N*HW <= 16384 and C >= 128): forward computes the batch statistics,
 * updates the running statistics, writes mean / invstd [C] and y = act(gamma*xhat + beta + residual); backward writes the channel sums
 * of g = dy*act'(y) and g*xhat (dbeta / dgamma) and dx / dres (either may be NULL). */
size_t rg_bn_train_fused_ok(int N, int C, int HW);
int rg_bn_train_fwd_fused(const float* x, const float* gamma, const float* beta, const float* residual, float* y, float* mean,
                          float* invstd, float* running_mean, float* running_var, int N, int C, int HW, float eps, float momentum,
                          int act, float slope, rg_stream_t stream);
int rg_bn_train_bwd_fused(const float* x, const float* dy, const float* y_act, const float* mean, const float* invstd,
                          const float* gamma, float* dx, float* dres, float* sum_dy, float* sum_dy_xhat, int N, int C, int HW,
                          int act, float slope, rg_stream_t stream);
/* torch.nn.InstanceNorm2d (affine or not; FD/fdgan/networks.py:30, CC/dual_gan/models/base_function.py:38-49) in one launch per
 * direction: forward writes y = act(gamma[c] * xhat + beta[c] + residual) and the per-instance mean / invstd [N*C]; backward
 * writes dx, dres (either may be NULL), the per-instance sums of g = dy*act'(y) and g*xhat [N*C] and, when sum_dx is given, the
 * per-instance sums of dx (the bias gradient of the convolution in front of the norm). */
int rg_instnorm_fwd(const float* x, const float* gamma, const float* beta, const float* residual, float* y, float* mean,
                    float* invstd, int N, int C, int HW, float eps, int act, float slope, rg_stream_t stream);
int rg_instnorm_bwd(const float* x, const float* dy, const float* y_act, const float* mean, const float* invstd,
                    const float* gamma, float* dx, float* dres, float* sum_dy, float* sum_dy_xhat, float* sum_dx, int N, int C,
                    int HW, int act, float slope, rg_stream_t stream);
/* out[c] = sum_{n, pixels} dy[n][c][.] in one launch (the bias gradient of torch's Conv2d / Linear backward, grad_output.sum over
 * every axis but the channel) when rg_channel_sum_ok says so — at most 32768 values per channel; larger maps use rg_bn_bwd_reduce */
size_t rg_channel_sum_ok(int N, int C, int HW);
int rg_channel_sum(const float* dy, float* out, int N, int C, int HW, rg_stream_t stream);
/* out_a[c] = sum_n a[n][c], out_b[c] = sum_n b[n][c]: dgamma / dbeta of an affine InstanceNorm2d (torch.nn.InstanceNorm2d
 * backward as used by CC/dual_gan/models/base_function.py:38-49) from the per-(n,c) sums of rg_bn_bwd_reduce. */
int rg_rows_sum_pair(const float* a, const float* b, float* out_a, float* out_b, int N, int C, rg_stream_t stream);
/* The IBN layer of the IBN-a ResNets (CC/clustercontrast/models/resnet_ibn_a.py:54-68: split -> InstanceNorm2d(half, affine) on
 * channels [0, half), BatchNorm2d(C - half) on [half, C) -> cat) on ONE x[N][C][HW] tensor, without the slice copies and the
 * concatenation: y / dx are the only tensors of the activation's size that are written.
 *   forward   y = act(affine(xhat)), act = none or ReLU; `residual` must be NULL (bn1 of a Bottleneck has none).  in_mean / in_invstd
 *             [N*half] are always written.  train != 0: batch statistics for the BN half (biased variance), bn_mean / bn_invstd
 *             [C-half] written, running_mean / running_var (may be NULL) updated with torch's rule; train == 0: the running statistics
 *             normalise and nothing is updated (bn_mean / bn_invstd unused).
 *   backward  dx [N][C][HW] and the four affine gradients; y_act is the forward output (needed when act != none).  bn_mean / bn_stat are
 *             the saved batch mean / invstd (train, with the batch-statistics correction terms) or the running mean / VARIANCE (eval).
 * Launches: eval 1 forward, 1 + 1 small backward; train with N*HW <= 16384 the same (one workgroup per BN channel next to the IN lane
 * groups in one grid); larger extents slice partial + finalize for the BN half, then one launch over all C channels.  Deterministic
 * (fixed summation order, no atomics).  workspace: rg_ibn_workspace bytes. */
int64_t rg_ibn_workspace(int N, int C, int HW, int half);
int rg_ibn_fwd(const float* x, const float* in_gamma, const float* in_beta, const float* bn_gamma, const float* bn_beta,
               const float* residual, float* y, float* in_mean, float* in_invstd, float* bn_mean, float* bn_invstd,
               float* running_mean, float* running_var, int N, int C, int HW, int half, int train, float in_eps, float bn_eps,
               float momentum, int act, void* workspace, size_t workspace_bytes, rg_stream_t stream);
int rg_ibn_bwd(const float* x, const float* dy, const float* y_act, const float* in_mean, const float* in_invstd,
               const float* bn_mean, const float* bn_stat, const float* in_gamma, const float* bn_gamma, float* dx,
               float* d_in_gamma, float* d_in_beta, float* d_bn_gamma, float* d_bn_beta, int N, int C, int HW, int half, int train,
               float bn_eps, int act, void* workspace, size_t workspace_bytes, rg_stream_t stream);
/* Domain-specific BatchNorm (CC/clustercontrast/models/dsbn.py:6-42), train mode, on x[N][C][HW] with N even: samples [0, N/2) are
 * normalised with their own batch statistics and the S parameter set, samples [N/2, N) with theirs and the T set — on the ONE
 * tensor, no slice copies and no concatenation.  Everything rg_bn_train_*_fused offers is kept per domain: residual add, activation
 * epilogue, running-statistics update (biased variance normalises, unbiased goes into running_var, count N/2*HW; any of the four
 * running tensors may be NULL), y_act-masked backward, dx / dres either NULL; the channel sums are written straight into the four
 * gradient outputs.  mean / invstd are [2][C] (S row, T row).
 * Launches: (N/2)*HW <= 16384 (rg_dsbn_one_launch), whatever C: one per direction, 2C workgroups; otherwise three per direction
 * as ONE BatchNorm — slice partial, finalize, apply over both domains, rg_dsbn_slices slices per domain, cut inside a domain and
 * never across sample N/2.  Deterministic (fixed summation order, no atomics).  An odd N is refused before anything is launched.
 * Eval mode is BatchNorm with the T set on the whole batch: use the rg_bn_* entry points.  workspace: rg_dsbn_workspace bytes. */
int64_t rg_dsbn_workspace(int N, int C, int HW);
int rg_dsbn_one_launch(int N, int C, int HW);
int rg_dsbn_slices(int N, int C, int HW);
/* float4 units per thread of the one-workgroup-per-channel train kernels for N samples (rg_bn_train_*_fused; rg_dsbn_* with N / 2):
 * 1, 2, 4, 8, 16 = register kernels, 0 = loop kernels (scalar rows, more than 16 units per thread, or RG_BN_REG=0). */
int rg_bn_reg_units(int N, int C, int HW);
int rg_dsbn_fwd(const float* x, const float* gamma_s, const float* beta_s, const float* gamma_t, const float* beta_t,
                const float* residual, float* y, float* mean, float* invstd, float* running_mean_s, float* running_var_s,
                float* running_mean_t, float* running_var_t, int N, int C, int HW, float eps_s, float eps_t, float momentum_s,
                float momentum_t, int act, float slope, void* workspace, size_t workspace_bytes, rg_stream_t stream);
int rg_dsbn_bwd(const float* x, const float* dy, const float* y_act, const float* mean, const float* invstd, const float* gamma_s,
                const float* gamma_t, float* dx, float* dres, float* d_gamma_s, float* d_beta_s, float* d_gamma_t, float* d_beta_t,
                int N, int C, int HW, int act, float slope, void* workspace, size_t workspace_bytes, rg_stream_t stream);
int rg_bn_bwd_apply(const float* x, const float* dy, const float* y_act, const float* mean, const float* stat,
                    const float* gamma, const float* sum_dy, const float* sum_dy_xhat, float* dx, float* dres, int N,
                    int C, int HW, int train, int stat_is_var, float eps, int act, float slope, rg_stream_t stream);

/* eval-mode backward in ONE pass (dx, dres and — when sum_dy / sum_dy_xhat are given — the affine-gradient sums) */
int rg_bn_eval_bwd(const float* x, const float* dy, const float* y_act, const float* running_mean,
                   const float* running_var, const float* gamma, float* dx, float* dres, float* sum_dy,
                   float* sum_dy_xhat, int N, int C, int HW, float eps, int act, float slope, void* workspace,
                   size_t workspace_bytes, rg_stream_t stream);

/* ---- element-wise --------------------------------------------------------------------------- */
int rg_act_fwd(const float* x, float* y, int64_t n, int act, float slope, rg_stream_t stream);
int rg_act_bwd(const float* dy, const float* y, float* dx, int64_t n, int act, float slope, rg_stream_t stream);
int rg_axpby(const float* a, const float* b, float* y, int64_t n, float alpha, float beta, rg_stream_t stream);
/* Pair batch of FDGANModel.set_input (FD/fdgan/model.py:127-150): out[0:B] = a, out[B:2B][i] = take_a[i] ? a[i] : b[i] — the
 * reference's `cat([x1, x1*mask + x2*(1-mask)])` with a 0/1 mask, and plain `cat([x1, x2])` for take_a == NULL.  per = floats
 * per sample. */
int rg_pair_cat(const float* a, const float* b, const int64_t* take_a, float* out, int B, int64_t per, rg_stream_t stream);
int rg_fill(float* y, int64_t n, float v, rg_stream_t stream);
/* one idle wave for `us` microseconds (1..100000) on `stream`: the probe rg_hip.ops.concurrent_stream uses to find streams that do
 * not share a hardware queue (no reference counterpart: the reference is single-stream) */
int rg_spin_us(int us, rg_stream_t stream);
/* (x1-x2)^2 of EltwiseSubEmbed, FD/reid/models/embedding.py:26-31 */
int rg_sub_square_fwd(const float* a, const float* b, float* y, int64_t n, rg_stream_t stream);
int rg_sub_square_bwd(const float* a, const float* b, const float* dy, float* da, float* db, int64_t n,
                      rg_stream_t stream);
/* nn.Dropout of the generator decoder, FD/fdgan/networks.py:105-109,149-156; counter-based mask */
int rg_dropout(const float* x, float* y, int64_t n, float p, unsigned long long seed, rg_stream_t stream);
int rg_dropout_clocked(const float* x, float* y, int64_t n, float p, unsigned long long seed, const unsigned long long* clock,
                       rg_stream_t stream);
/* F.normalize(x, dim=1) on [rows][D], CC/clustercontrast/models/cm.py:125, resnet.py:90-107 */
int rg_l2norm_rows_fwd(const float* x, float* y, float* norm, int rows, int D, float eps, rg_stream_t stream);
int rg_l2norm_rows_bwd(const float* y, const float* dy, const float* norm, float* dx, int rows, int D, float eps,
                       rg_stream_t stream);
/* F.normalize(x, dim=1) of a feature MAP [N][C][HW] (unit norm over the channels at every pixel; the `gan_x` output of the
 * cluster-contrast ResNet in train mode, CC/clustercontrast/models/resnet.py:100-107) and its backward; norm is [N][HW] */
int rg_l2norm_channels_fwd(const float* x, float* y, float* norm, int N, int C, int HW, float eps, rg_stream_t stream);
int rg_l2norm_channels_bwd(const float* y, const float* dy, const float* norm, float* dx, int N, int C, int HW, float eps,
                           rg_stream_t stream);
/* torch.cat along channels / its backward slices, FD/fdgan/model.py:160-161, networks.py:175 */
int rg_copy_channels(const float* src, float* dst, int N, int Cc, int HW, int Cs, int sc0, int Cd, int dc0,
                     int accumulate, rg_stream_t stream);

/* my_resize / my_normalize / my_transform, CC/clustercontrast/utils/data/diff_augs.py:6-16: bicubic (A = -0.75,
 * align_corners = False, clamped border taps) resize [N,C,H,W] -> [N,C,OH,OW] fused with (v - mean[c]) / std[c];
 * mean/std are device arrays of C floats or both NULL (resize only); OH == H and OW == W normalises only.
 * The backward is the exact adjoint, gathered per input pixel (deterministic). */
int rg_bicubic_normalize_fwd(const float* x, float* y, int N, int C, int H, int W, int OH, int OW, const float* mean,
                             const float* stdv, rg_stream_t stream);
int rg_bicubic_normalize_bwd(const float* dy, float* dx, int N, int C, int H, int W, int OH, int OW, const float* stdv,
                             rg_stream_t stream);

/* ClusterMemory_Gradient.update_clusters, CC/clustercontrast/models/cm.py:184-190: g[id][:] /= |g[id]| + eps for every id of
 * the int64 device list (each distinct id once) */
int rg_normalize_listed_rows(float* g, const void* ids, int n_ids, int rows, int D, float eps, rg_stream_t stream);

/* mean(f(a + b*x)), f = ReLU when clamp != 0 else identity: hinge / wgangp / generator branches of the dual_gan GANLoss,
 * CC/dual_gan/models/external_function.py:58-68; workspace as rg_loss_workspace() */
int rg_affine_relu_mean_fwd(const float* x, float* loss, int64_t n, float a, float b, int clamp, void* workspace,
                            size_t workspace_bytes, rg_stream_t stream);
int rg_affine_relu_mean_bwd(const float* x, const float* grad_out, float* dx, int64_t n, float a, float b, int clamp,
                            float grad_scale, rg_stream_t stream);

/* ---- FP8 convolution family (BASELINE config 5: "dual_gan two-generator path, fp8 MFMA convs") ------------------
 * Replaces, at reduced precision, the cuDNN work behind the nn.Conv2d / nn.ConvTranspose2d layers of the dual_gan
 * generators and discriminator (CC/dual_gan/models/base_function.py:236-443, networks.py:165-275,917-955), which the
 * reference runs in fp32.  OCP e4m3 for activations and filters, e5m2 for gradients, one scale per tensor, fp32
 * accumulation on v_mfma_f32_32x32x16_{fp8,bf8}_{fp8,bf8}; outputs are fp32 NCHW like every other entry point.
 *
 * Scaling state of one tensor: float[4] device memory {amax in use, amax being collected, dequantisation scale = amax in
 * use / format max, format max (448 e4m3 / 57344 e5m2; written once by the caller)}.  rg_f8_quantize scales by
 * format max / state[0], clamps, converts and collects max|x| into state[1]; rg_f8_roll_scales makes the collected
 * values current for `count` consecutive states (delayed scaling: once per step); rg_f8_amax followed by a roll gives
 * just-in-time scaling.  fmt: 0 = e4m3, 1 = e5m2. */
int rg_f8_amax(const float* x, int64_t n, float* state, rg_stream_t stream);
int rg_f8_roll_scales(float* states, int count, rg_stream_t stream);
/* out[b][l][r] (one byte each, r padded with zeros to a multiple of 16) = fp8(in[b*bs + r*rs + l]): the transposing
 * quantiser behind every operand layout; scale_out (one device float, may be NULL) receives the dequantisation scale this
 * call used, which is what the GEMMs below take as sx / sw / sdy (a layer's state may be re-scaled for another tensor
 * before the backward pass reads this one) —  activations [N][C][HW] -> [N][HW][Cp] (b = n, r = c) for the forward / data
 * gradient and -> [C][HW][Np] (b = c, r = n) for the weight gradient; filters [K][C][RS] -> [K][RS][Cp] and [C][RS][Kp] */
int rg_f8_quantize(const float* in, void* out, float* state, float* scale_out, int fmt, int B, int R, int L, int64_t bs,
                   int64_t rs, rg_stream_t stream);
/* both layouts of in[N][C][L] from ONE pass over the fp32 data: a [N][L][Cp] and b [C][L][Np] (either may be NULL) */
int rg_f8_quantize_dual(const float* in, void* a, void* b, float* state, float* scale_out, int fmt, int N, int C, int L,
                        rg_stream_t stream);
/* the output-gradient operand of a convolution backward in one pass over dy: g = dy * act'(yact) (act 0: g = dy, yact unused) is
 * quantised into a / b as rg_f8_quantize_dual does (either may be NULL) and its per-tile channel sums go to
 * part[rg_f8_grad_tiles(N, L)][C] (NULL: not wanted; the bias gradient is the column sum of `part`, rg_rows_sum_pair) — replaces
 * rg_act_bwd + rg_f8_quantize_dual + the channel-sum passes of the reference's autograd (torch Conv2d backward: grad_bias =
 * grad_output.sum((0, 2, 3))) on the fp8 path; g itself is never written */
int rg_f8_grad_tiles(int N, int L);
int rg_f8_quantize_grad(const float* dy, const float* yact, int act, float slope, void* a, void* b, float* part, float* state,
                        float* scale_out, int fmt, int N, int C, int L, rg_stream_t stream);
/* y = act(sx*sw * conv(xq, wq) + shift[k] + residual); xq [N][H*W][Cp], wq [K][KH*KW][Cp] (e4m3), sx / sw: the quantiser's scale_out of each operand */
int rg_conv2d_f8_fwd(const void* xq, const void* wq, const float* sx, const float* sw, int fmt_x, float* y, int N, int C,
                     int H, int W, int K, int KH, int KW, int SH, int SW, int PH, int PW, int P, int Q, const float* shift,
                     const float* residual, int act, float slope, rg_stream_t stream);
/* dx (or the forward of ConvTranspose2d) from dyq [N][P*Q][Kp] and the filters as [C][KH*KW][Kp]; stride <= 2 */
int rg_conv2d_f8_dgrad(const void* dyq, const void* wq_t, const float* sdy, const float* sw, int fmt_dy, float* dx, int N,
                       int C, int H, int W, int K, int KH, int KW, int SH, int SW, int PH, int PW, int P, int Q,
                       const float* shift, const float* residual, int act, float slope, rg_stream_t stream);
/* dw[K][C][KH][KW] from the batch-contiguous layouts xq [C][H*W][Np], dyq [K][P*Q][Np]; split over the pixels, partials in
 * the workspace, summed in fixed order */
size_t rg_conv2d_f8_wgrad_workspace(int N, int C, int K, int KH, int KW, int P, int Q);
int rg_conv2d_f8_wgrad(const void* xq, const void* dyq, const float* sx, const float* sdy, int fmt_x, int fmt_dy, float* dw,
                       int N, int C, int H, int W, int K, int KH, int KW, int SH, int SW, int PH, int PW, int P, int Q,
                       void* workspace, size_t workspace_bytes, rg_stream_t stream);

/* WGAN-GP penalty terms of cal_gradient_penalty, CC/dual_gan/models/external_function.py:100-101, per sample row r of
 * grads[rows][D] with g = grads[r] + 1e-16: pen[r] = scale * (|g|_2 - constant)^2, v[r][:] = d pen[r] / d grads[r] */
int rg_grad_penalty_rows(const float* grads, float* pen, float* v, int rows, int D, float constant, float scale,
                         rg_stream_t stream);

/* ---- pseudo-labelling front half / evaluation distances ------------------------------ */
/* faiss IndexFlatIP.search of CC/clustercontrast/utils/infomap_cluster.py:51-78 on a similarity block s[rows][cols]
 * (from the GEMM): the k best columns per row in (value descending, index ascending) order; idx int32 [rows][k] */
int rg_topk_rows(const float* s, int rows, int cols, int k, int* idx, float* val, rg_stream_t stream);
/* |x_r|^2 per row and m = alpha*m + a*rowv[r] + b*colv[c]: pairwise_distance, CC/clustercontrast/evaluators.py:71-88,
 * FD/reid/evaluators.py:76-98 (the -2 x.y^T term comes from the GEMM) */
int rg_row_sqsum(const float* x, float* out, int rows, int D, rg_stream_t stream);
int rg_add_outer_terms(float* m, const float* rowv, const float* colv, float alpha, float a, float b, int rows, int cols,
                       rg_stream_t stream);
/* generate_cluster_features, CC/examples/cluster_contrast_gan_train_usl_infomap.py:332-348: out[s] = mean of the rows
 * x[order[j]], j in [offsets[s], offsets[s+1]) (int64 device arrays; members in list order) */
int rg_segment_mean(const float* x, const void* order, const void* offsets, float* out, int segments, int D,
                    rg_stream_t stream);

/* ---- k-reciprocal re-ranking (Zhong et al., CVPR 2017) behind compute_jaccard_distance, CC/clustercontrast/utils/
 * faiss_rerank.py:31-127, and re_ranking, CC/clustercontrast/utils/rerank.py:32-99.  The encodings stay sparse: row lists
 * sets / w [N][cap] with counts [N] before the query expansion, CSR (rowptr [N + 1], cols, vals) and its column lists
 * (colptr [N + 1], crow, cval) after it; all index arrays int32, N <= 65536.  No floating-point atomics anywhere.
 *   rg_rerank_expand        rank [N][R] (ascending distance).  R(i, k) = { j in rank[i][:k] : i in rank[j][:k] }; sets[i] =
 *                           R(i, kf) united with every R(c, kh), c in R(i, kf), that has more than 2/3 of its members in
 *                           R(i, kf); sorted, unique; counts[i] is the full size (at most kf * (kh + 1); entries beyond cap
 *                           are dropped, so a count above cap asks for a second call)
 *   rg_rerank_weights_feat  w[i][e] = softmax_e(-(2 - 2 x_i . x_e)) over the first min(counts[i], cap) entries of the row's
 *                           set, x [N][D], the maximum subtracted (rows need not be normalised); w[i][min(counts[i], cap):]
 *                           is not written.  A set entry outside [0, N) gets the weight 0 exactly; a set of ONLY such
 *                           entries has no maximum and comes back NaN throughout (both forms)
 *   rg_rerank_weights_dist  w[i][e] = exp(-orig[i][e]) / sum_e, orig [N][N].  No maximum is subtracted: the domain is
 *                           exp(-orig[i][e]) normal in fp32 (orig below 87; rg_rerank_orig_dist gives [0, 1])
 *   rg_rerank_qe_count      local query expansion, row i = mean of the rows rank[i][:k2] (rank NULL: k2 == 1, the row
 *                           itself): rowcnt[i] = columns of the union, rowptr = their exclusive prefix sum
 *   rg_rerank_qe_fill       the CSR rows: columns ascending, terms added in rank order, divided by k2
 *   rg_rerank_columns       column lists of the CSR matrix (cursor: N ints of scratch; order inside a column unspecified)
 *   rg_rerank_jaccard       out[i][j - col_off] = 1 - m / (2 - m), m = sum_c min(V[i][c], V[j][c]) over row i's columns in
 *                           ascending order, rows i < rows, columns col_off <= j < N, out [rows][N - col_off]; orig != NULL:
 *                           (1 - lambda) * that + lambda * orig[i][j]; clamp != 0: negative results become 0.  chunk = columns
 *                           accumulated per workgroup (<= 16384; 0 = automatic), any value gives the same bits
 *   rg_rerank_orig_dist     orig = transpose(A^2 / max(A^2, axis 0)), A = [[q_q, q_g], [q_g^T, g_g]] (colmax: N floats of
 *                           scratch).  An all-zero column c of A gives 0 / 0: row c of orig is NaN, as the reference's numpy
 *                           expression gives it */
int rg_rerank_expand(const int* rank, int N, int R, int kf, int kh, int* sets, int* counts, int cap, rg_stream_t stream);
int rg_rerank_weights_feat(const float* x, int N, int D, const int* sets, const int* counts, int cap, float* w,
                           rg_stream_t stream);
int rg_rerank_weights_dist(const float* orig, int N, const int* sets, const int* counts, int cap, float* w, rg_stream_t stream);
int rg_rerank_qe_count(const int* rank, int R, int k2, int N, const int* sets, const int* counts, int cap, int* rowcnt,
                       int* rowptr, rg_stream_t stream);
int rg_rerank_qe_fill(const int* rank, int R, int k2, int N, const int* sets, const float* w, const int* counts, int cap,
                      const int* rowptr, int* cols, float* vals, rg_stream_t stream);
int rg_rerank_columns(const int* rowptr, const int* cols, const float* vals, int N, int64_t nnz, int* colptr, int* cursor,
                      int* crow, float* cval, rg_stream_t stream);
int rg_rerank_jaccard(const int* rowptr, const int* cols, const float* vals, const int* colptr, const int* crow,
                      const float* cval, int N, int rows, int col_off, const float* orig, float lambda_value, int clamp,
                      float* out, int chunk, rg_stream_t stream);
int rg_rerank_orig_dist(const float* q_g, const float* q_q, const float* g_g, int Q, int G, float* colmax, float* orig,
                        rg_stream_t stream);

/* ---- DBSCAN on a precomputed symmetric distance matrix d [N][ld] (fp32, or fp16 with is_half = 1), the pseudo-labelling step
 * between compute_jaccard_distance and generate_cluster_features (CC/examples/cluster_contrast_train_usl.py:146-200), with
 * the labels of scikit-learn's DBSCAN(metric='precomputed'): adj[i][j] = d[i][j] <= eps (entries widened to fp32, compared
 * with the fp32 eps; the diagonal counts like any other entry; a negative entry is simply <= eps), core[i] = |adj[i]| >=
 * min_samples, clusters = connected components of the core-core graph numbered by ascending lowest core index, a non-core
 * point gets the lowest cluster number among its core neighbours or -1.  An asymmetric matrix is not reproduced (scikit-learn's
 * search becomes directed).  All index arrays int32, N <= 65536; integer atomics only, results independent of their order.
 *   rg_dbscan_count        cnt[i] = entries of row i that are <= eps; rowptr [N + 1] = their exclusive prefix sum
 *   rg_dbscan_fill         nbr[rowptr[i] .. rowptr[i + 1]) = those columns, ascending; core[i] = cnt[i] >= min_samples
 *   rg_dbscan_components   parent[i] = lowest core index of i's component for a core point, -1 otherwise (lock-free
 *                          union-find: the higher root is hooked under the lower by compare-and-swap; every walk descends)
 *   rg_dbscan_labels       isroot[i] = parent[i] == i, rootnum [N + 1] = its exclusive prefix sum (rootnum[N] = number of
 *                          clusters), labels int64 [N] as above
 *   rg_dbscan_asymmetry    *count = entries above the diagonal whose bits differ from their mirror's */
int rg_dbscan_count(const void* d, int is_half, int N, int64_t ld, float eps, int* cnt, int* rowptr, rg_stream_t stream);
int rg_dbscan_fill(const void* d, int is_half, int N, int64_t ld, float eps, int min_samples, const int* rowptr, int* nbr, int* core,
                   rg_stream_t stream);
int rg_dbscan_components(const int* rowptr, const int* nbr, const int* core, int N, int* parent, rg_stream_t stream);
int rg_dbscan_labels(const int* rowptr, const int* nbr, const int* parent, int N, int* isroot, int* rootnum, int64_t* labels,
                     rg_stream_t stream);
int rg_dbscan_asymmetry(const void* d, int is_half, int N, int64_t ld, int* count, rg_stream_t stream);

/* ---- Two-level Infomap on a kNN table nbrs int32 / dists fp32 [N][k]: `cluster_by_infomap` of
 * CC/clustercontrast/utils/infomap_cluster.py:129-227 (the pseudo-labelling step of the infomap example scripts) as the
 * two-level directed map equation under a deterministic, host-driven search (not the labels of the seeded `infomap`
 * package).  All index arrays int32, all flows fp64, N <= 65536, k <= 128; every sum runs in a fixed order and only integer
 * atomics are used whose result does not depend on their order.  A unit graph is two CSR lists (out: orp / odst / oq, in:
 * irp / isrc / iq, in-lists in ascending source order) plus the unit flows pu; module totals live in slots [0, U).
 *   rg_infomap_links_count   cnt[i] = links of row i (left to right: self skipped, dist <= thr links, the first other entry or
 *                            an index outside [0, N) ends the row); rowptr [N + 1] = exclusive prefix sum
 *   rg_infomap_links_fill    src / dst / w (= double(1.0f - dist)) at rowptr[i] .., single[i] = the row gave no link,
 *                            incnt[j] = in-links of j, in_rowptr [N + 1] = its prefix sum
 *   rg_infomap_flow_start    wout / win = link weight out of / into every node, p = uniform over the nodes in a link,
 *                            tele = win / total, scal [16] = the iteration's fp64 scalars ([4] L1 change, [5] iterations,
 *                            [6] done, [7] sum_nodes plogp(flow) after rg_infomap_flow_finish)
 *   rg_infomap_flow_iterate  `iters` PageRank steps (alpha 0.15, teleportation to links, dangling nodes teleport with
 *                            probability 1); a step after the L1 change fell to 1e-13 or max_iters were run changes nothing
 *   rg_infomap_flow_finish   q[e] = p_src w_e / wout_src normalised to sum 1, iq = q in in-list order, flow[j] = in-flow
 *   rg_infomap_totals        xo / xi = flow of every unit's links that cross modules; per module (segments of `order`, a
 *                            stable sort of mod) exit / enter / flow / unit count into slot mod (zero the slots first)
 *   rg_infomap_codelength    out[0] = plogp(sum enter) - sum plogp(enter) - sum plogp(exit) + sum plogp(exit + flow) -
 *                            *nodeterm in bits, out[1] = sum enter
 *   rg_infomap_propose       per unit the best move to the module of a linked unit against the frozen totals (gain > 1e-10
 *                            bits, ties to the lower module): tgt (-1: none), key = (gain bits, unit), vals = the new exit /
 *                            enter of both modules; claim[m] / *best = highest key per module / overall
 *   rg_infomap_apply         single 0: every unit whose key holds both its modules moves and writes their totals; single 1:
 *                            only the unit holding *best; *nmoved = moves
 *   rg_infomap_segment_sum   out[s] = sum of q[eidx[t]], t in [segptr[s], segptr[s + 1]), front to back
 *   rg_infomap_labels        modules with more than cluster_num members numbered by ascending smallest member, -1 for the
 *                            rest; num[N] = number of kept modules */
int rg_infomap_links_count(const int* nbrs, const float* dists, int N, int k, float thr, int* cnt, int* rowptr, rg_stream_t stream);
int rg_infomap_links_fill(const int* nbrs, const float* dists, int N, int k, float thr, const int* rowptr, int* src, int* dst,
                          double* w, int* single, int* incnt, int* in_rowptr, rg_stream_t stream);
int rg_infomap_flow_start(const int* orp, const double* w, const int* irp, const int* ieid, int N, int E, double* wout, double* win,
                          double* p, double* tele, double* scal, rg_stream_t stream);
int rg_infomap_flow_iterate(const int* orp, const int* irp, const int* isrc, const int* ieid, const double* w, const double* wout,
                            const double* tele, int N, int E, int iters, int max_iters, double* p, double* raw, double* scal,
                            rg_stream_t stream);
int rg_infomap_flow_finish(const int* src, const int* irp, const int* ieid, const double* w, const double* wout, const double* p,
                           int N, int E, double* q, double* iq, double* flow, double* scal, rg_stream_t stream);
int rg_infomap_totals(const int* orp, const int* odst, const double* oq, const int* irp, const int* isrc, const double* iq,
                      const double* pu, const int* mod, const int* order, const int* segptr, int U, int S, double* xo, double* xi,
                      double* mexit, double* menter, double* mflow, int* nunits, rg_stream_t stream);
int rg_infomap_codelength(const double* mexit, const double* menter, const double* mflow, int M, const double* nodeterm, double* out,
                          rg_stream_t stream);
int rg_infomap_propose(const int* orp, const int* odst, const double* oq, const int* irp, const int* isrc, const double* iq,
                       const double* pu, const int* mod, const double* mexit, const double* menter, const double* mflow,
                       const int* nunits, int U, const double* cl, int* tgt, void* key, double* vals, void* claim, void* best,
                       int* nmoved, rg_stream_t stream);
int rg_infomap_apply(const int* tgt, const void* key, const double* vals, const void* claim, const void* best, const double* pu,
                     int U, int single, int* mod, double* mexit, double* menter, double* mflow, int* nunits, int* nmoved,
                     rg_stream_t stream);
int rg_infomap_segment_sum(const double* q, int E, const int* eidx, const int* segptr, int S, int T, double* out, rg_stream_t stream);
int rg_infomap_labels(const int* mod, int N, int cluster_num, int* size, int* minm, int* head, int* num, int64_t* labels,
                      rg_stream_t stream);

/* ---- k-means (Lloyd) on features x fp32 [N][D] with centroids c fp32 [K][D]: `label_generator_kmeans` of
 * CC/clustercontrast/models/kmeans.py (faiss.Kmeans, niter 300) as faiss's Clustering::train with spherical = false and
 * nredo = 1 under a deterministic split rule (faiss's objective and iteration, not its seeded labels).  One iteration
 * is assign, tally, update, split.  All index arrays int32; 1 <= K <= 8192, K <= N <= 1 048 576, 1 <= D <= 8192, anything else is
 * RG_ERR_INVALID.  No floating-point atomics; the integer atomics used give results independent of their order.
 *   rg_kmeans_assign   label[i] = argmin_j (csq[j] - 2 x_i . c_j), ties to the lowest j; score[i] = that minimum in fp32.  The
 *                      products are exact fp32 (v_mfma_f32_32x32x2_f32: one fma chain over d per score), the argmin is taken in
 *                      the kernel's epilogue and the [N][K] scores are never stored.  With more than one tile of 128 centroids
 *                      the tiles meet in N 64-bit keys (score bits, index) by integer atomicMin: rg_kmeans_assign_workspace
 *                      bytes (0 for K <= 128)
 *   rg_kmeans_tally    cnt[j] = members of cluster j, rowptr [K + 1] = their exclusive prefix sum, order [N] = the members of
 *                      cluster 0, then 1, ..., each in ascending row index, *changed = rows with label != prev, *obj =
 *                      sum_i (double(xsq[i]) + double(score[i])) in fp64 and a fixed order.  rg_kmeans_tally_workspace bytes.
 *                      A label outside [0, K) is left out of cnt / order
 *   rg_kmeans_update   c[j] = mean of the rows x[order[m]], m in [rowptr[j], rowptr[j + 1]): accumulated in FP64 in list order,
 *                      divided in fp64, rounded to fp32 once; csq[j] = float(sum_d double(c[j][d])^2).  A cluster without a
 *                      member keeps its row and its csq
 *   rg_kmeans_split    every cluster with cnt == 0, in ascending index, takes as donor the cluster with the currently largest cnt
 *                      (ties: lowest index): c[empty][d] = c[donor][d] * (1 + s_d), c[donor][d] *= (1 - s_d), s_d = +1/1024 for
 *                      even d and -1/1024 for odd d (fp32 products); cnt[empty] = cnt[donor] / 2, cnt[donor] -= cnt[empty]; csq of
 *                      both rows is refreshed; *nsplit += the number of splits.  One workgroup */
int64_t rg_kmeans_assign_workspace(int N, int K, int D);
int rg_kmeans_assign(const float* x, const float* c, const float* csq, int N, int K, int D, int* label, float* score,
                     void* workspace, size_t workspace_bytes, rg_stream_t stream);
int64_t rg_kmeans_tally_workspace(int N, int K);
int rg_kmeans_tally(const int* label, const int* prev, const float* xsq, const float* score, int N, int K, int* cnt, int* rowptr,
                    int* order, int* changed, double* obj, void* workspace, size_t workspace_bytes, rg_stream_t stream);
int rg_kmeans_update(const float* x, const int* order, const int* rowptr, int N, int K, int D, float* c, float* csq,
                     rg_stream_t stream);
int rg_kmeans_split(float* c, float* csq, int* cnt, int K, int D, int* nsplit, rg_stream_t stream);

/* ---- CMC / mAP scoring of a query x gallery distance matrix dist [Q][ld] (fp32, or fp64 with is_double = 1; compared in its
 * own type), CC/clustercontrast/evaluation_metrics/ranking.py `cmc` / `mean_ap`, without a sort.  All id / camera arrays int32.
 * Per query i: valid_j = (gid_j != qid_i) | (gcam_j != qcam_i) (and gcam_j != qcam_i with separate_camera_set), pos_j = valid_j
 * & (gid_j == qid_i);
 *   npos[i]            positives (0: the query is skipped)
 *   ap[i]     fp64     (1 / P) sum_p TP_le(p) / N_le(p): positives / valid entries with d <= d_p, ties by value (-0.0 == 0.0,
 *                      +-inf ordinary values) = scikit-learn's average_precision_score; the terms are added as 64.64 fixed point
 *   first[i]           valid non-matching entries before the first positive in stable (d, j) order (-1 without a positive)
 *   hits[i][0:topk]    hits[i][r] = positives with exactly r valid non-matching entries before them in stable order
 * and over the queries, in a fixed order: counts [topk + 2] = {status, valid queries, histogram of first}, sums [topk + 1] =
 * {sum_i ap[i], sum_i hits[i][k] / npos[i]}.  status != 0: a row holds a NaN (the results are then unspecified, nothing is
 * written out of bounds).  chunk = positives held in LDS per pass over a row (1 .. 1024; 0 = automatic); rows with more take
 * further passes, any value gives the same bits.  Integer atomics only. */
int rg_rank_eval(const void* dist, int is_double, int Q, int G, int64_t ld, const int* query_ids, const int* gallery_ids,
                 const int* query_cams, const int* gallery_cams, int separate_camera_set, int topk, int chunk, int* npos, double* ap,
                 int* first, int* hits, int* counts, double* sums, rg_stream_t stream);

/* ---- single-gallery-shot CMC (the reference's `cuhk03` protocol, `cmc(single_gallery_shot=True)` :53-75) on the same matrix
 * (csrc/cmc_shot.hip).  The gallery is grouped by identity by the caller: seg_ptr [nid + 1] and seg_perm [G] (identities
 * ascending, the entries of one in ascending j), query_seg [Q] = the segment of the query's identity or -1; 1 <= nid <= 4096.
 * Rows are ordered by the stable key (d, j), by value (-0.0 == 0.0).  valid_j as above.
 * rg_cmc_shot_order, per query i: n[i] = identities with a valid entry (0: no valid match, the query is skipped and draws
 *   nothing), slot[i][0:n) = their segment indices by smallest valid key = the order the reference draws for them,
 *   high[i][0:n) = their valid counts in that order; slot = -1 and high = 0 beyond n (both [Q][nid]).  status: bit 0 a NaN
 *   in the matrix, bit 1 a seg_perm entry outside [0, G) (results then unspecified, nothing is accessed out of bounds).
 * rg_cmc_shot_rank, queries [q0, q0 + nq) of the Q rows: draws + draw_off[i - q0] is query i's [repeat][n[i]] block of draws
 *   u[r][p] in [0, high[i][p]) (int32, position order; never read for a skipped query).  With t_r the u[r][own]-th valid
 *   entry of the own identity in key order and c_x(t) the valid entries of x with key < t:
 *   rank[i][r] = #{x != own : u[r][x] < c_x(t_r)} (the true rank, also when >= topk; -1 for a skipped query) and
 *   hist[rank] += 1 when rank < topk (hist [topk] is NOT zeroed here: launches over chunks of queries add up).
 *   1 <= repeat <= 64.  Finding t_r is quadratic in the own identity's valid entries.
 * rg_cmc_shot_regime: where the rank pass gathers a row's entries from (a value, not a status; -1 outside the limits):
 *   1 the row staged in LDS with 16-byte loads (G * element size <= 32 768 bytes), 0 global memory.
 * Integer atomics only: the same bits for any arrival order, stream or chunking. */
int64_t rg_cmc_shot_regime(int G, int nid, int is_double);
int rg_cmc_shot_order(const void* dist, int is_double, int Q, int G, int64_t ld, int nid, const int* seg_ptr, const int* seg_perm,
                      const int* gallery_cams, const int* query_seg, const int* query_cams, int separate_camera_set, int* n,
                      int* slot, int* high, int* status, rg_stream_t stream);
int rg_cmc_shot_rank(const void* dist, int is_double, int Q, int q0, int nq, int G, int64_t ld, int nid, const int* seg_ptr,
                     const int* seg_perm, const int* gallery_cams, const int* query_seg, const int* query_cams,
                     int separate_camera_set, const int* n, const int* slot, const int* draws, const int64_t* draw_off, int repeat,
                     int topk, int* rank, int* hist, rg_stream_t stream);

/* ---- conv + frozen-statistics BatchNorm fold (E / D_id of FD-GAN: set_bn_fix, FD/fdgan/networks.py:57-60 with
 * trainable affine parameters, model.py:72-85).  Forward: rg_conv2d_fwd with scale/shift from rg_bn_fold — the
 * pre-normalisation tensor is never written.  Backward without it:
 *   g = dy * act'(y), sum_g = channel sums (dbeta)                     rg_act_bwd_sum (g may be NULL for act none)
 *   G = rg_conv2d_wgrad(x, g);  dgamma = invstd * (sum_m W[k][m] G[k][m] - mean * sum_g);  G *= scale (in place -> dW)
 *                                                                      rg_bn_fold_wgrad (dgamma may be NULL)
 *   dx = rg_conv2d_dgrad(g, rows of W scaled by scale)                 rg_scale_rows */
int rg_bn_fold(const float* gamma, const float* beta, const float* running_mean, const float* running_var, float eps,
               float* scale, float* shift, float* invstd, int C, rg_stream_t stream);
int rg_act_bwd_sum(const float* dy, const float* y_act, float* g, float* sum_g, int N, int C, int HW, int act, float slope,
                   void* workspace, size_t workspace_bytes, rg_stream_t stream);
/* sums either as sum_g[K] (rg_act_bwd_sum) or as slice partials [K][n_slices] of rg_act_bwd_partial, which
 * rg_bn_fold_wgrad then adds up itself and also writes as dbeta (saves the finalize launch on the critical stream) */
int rg_bn_fold_wgrad(const float* w, float* g, const float* scale, const float* invstd, const float* running_mean,
                     const float* sum_g, const float* partials, int n_slices, float* dbeta, float* dgamma, int K, int M,
                     rg_stream_t stream);
/* rg_conv2d_wgrad + rg_bn_fold_wgrad in one call (same arguments): with split-K the fold finishes inside the reduction launch
 * (one launch, one pass over G less per folded layer) */
int rg_conv2d_wgrad_fold(const float* x, const float* dy, float* dw, int N, int C, int H, int W, int K, int KH, int KW,
                         int SH, int SW, int PH, int PW, int P, int Q, const float* w, const float* scale,
                         const float* invstd, const float* running_mean, const float* sum_g, const float* partials,
                         int n_slices, float* dbeta, float* dgamma, void* workspace, size_t workspace_bytes,
                         rg_stream_t stream);
int rg_bn_slices(int N, int C, int HW);
int rg_act_bwd_partial(const float* dy, const float* y_act, float* g, float* part, int N, int C, int HW, int act, float slope,
                       rg_stream_t stream);
int rg_scale_rows(const float* w, const float* scale, float* out, int K, int M, rg_stream_t stream);

/* All (conv, frozen BatchNorm) pairs of a network in ONE launch: `table` is a device array of 16 int64 words per pair
 * {w, gamma, beta, running_mean, running_var, w_scaled, w_scaled_krsc|0, scale, shift, invstd, K, C, KH*KW,
 *  eps (float bits), first workgroup of the pair, 0}; a pair takes ceil(K*C*KH*KW / rg_fold_chunk()) workgroups.
 * Writes scale/shift/invstd and the filters times scale[k] in [K][C][RS] and (optionally) [K][RS][C] layout, so that the
 * forward is conv(x, W*scale) + shift and the data gradient uses the same scaled filters. */
int rg_fold_filters_multi(const void* table, int n_pairs, int total_blocks, rg_stream_t stream);
int rg_fold_chunk(void);

/* ---- dual_gan blocks (CC/dual_gan/models/base_function.py, PTM.py) ---------------------------- */
/* nn.AvgPool2d(k, k) of the ResBlockEncoder shortcuts, base_function.py:372-420; P = H / k, Q = W / k */
int rg_avgpool2d_fwd(const float* x, float* y, int N, int C, int H, int W, int k, rg_stream_t stream);
int rg_avgpool2d_bwd(const float* dy, float* dx, int N, int C, int H, int W, int k, rg_stream_t stream);
/* nn.ReflectionPad2d(pad) of the Output block, base_function.py:423-443; y is [N,C,H+2pad,W+2pad] */
/* act (0 none, 1 relu, 2 leaky relu with slope > 0): the element-wise activation the Output block applies in front of the padding
 * (base_function.py:436-441 `nonlinearity, ReflectionPad2d, conv`), folded in: y = pad(act(x)), dx = act'(x_act) * pad^T(dy) with
 * x_act the tensor the forward padded (NULL when act == 0); the fused forms need W % 4 == 0, W >= 8, pad <= 3 */
int rg_reflection_pad2d_fwd(const float* x, float* y, int N, int C, int H, int W, int pad, int act, float slope, rg_stream_t stream);
int rg_reflection_pad2d_bwd(const float* dy, const float* x_act, float* dx, int N, int C, int H, int W, int pad, int act, float slope,
                            rg_stream_t stream);
/* torch.nn.utils.spectral_norm (base_function.py:121-126; every ResDiscriminator conv, networks.py:917-955) on the
 * filter viewed as W[K][M]: training != 0 runs one power iteration in place on u[K], v[M] (eps-clamped norms), then
 * sigma = u.(W v); writes w_sn = W / sigma and sigma[0] = sigma, sigma[1] = 1 / sigma (device, 2 floats); uv_saved (may be NULL,
 * K + M floats) receives the u, v this forward used — the constants of its backward, which the next forward overwrites.
 * K <= 1024, M <= 12288.  Backward: dw (+)= (dw_sn - (sum dw_sn * w_sn) u v^T) / sigma with the forward's u, v. */
int rg_spectral_norm_fwd(const float* w, float* u, float* v, float* w_sn, float* sigma, float* uv_saved, int K, int M,
                         int training, float eps, rg_stream_t stream);
/* The same for every spectral-normed filter of one network forward (ResDiscriminator: 13 filters) in two launches. */
#define RG_SN_MAX_BATCH 16
typedef struct rg_sn_desc {
    const float* w;
    float* u;
    float* v;
    float* w_sn;
    float* sigma;
    float* uv_saved;
    int K;
    int M;
} rg_sn_desc;
int rg_spectral_norm_fwd_multi(const rg_sn_desc* descs, int count, int training, float eps, rg_stream_t stream);
size_t rg_spectral_norm_bwd_workspace(int K, int M);
int rg_spectral_norm_bwd(const float* dw_sn, const float* w_sn, const float* u, const float* v, const float* sigma,
                         float* dw, int K, int M, int accumulate, void* workspace, size_t workspace_bytes,
                         rg_stream_t stream);
/* Batched strided fp32 GEMM (MFMA) for nn.MultiheadAttention inside CAB / TTB, PTM.py:162-247:
 * C[b0][b1][m][n] = alpha * sum_k A[b0][b1][m][k] B[b0][b1][k][n] + beta * C; all strides in elements, so Q^T K,
 * P V and the backward products run on [B][C][L] token maps without permutes. */
int rg_bgemm(const float* A, const float* B, float* C, int M, int N, int K, int64_t a_ms, int64_t a_ks, int64_t b_ks,
             int64_t b_ns, int64_t c_ms, int64_t c_ns, int batch0, int batch1, int64_t a_b0, int64_t a_b1, int64_t b_b0,
             int64_t b_b1, int64_t c_b0, int64_t c_b1, float alpha, float beta, rg_stream_t stream);
/* y[r][:] = softmax(scale * x[r][:]) and ds = scale * p * (dp - sum(dp * p)); in place allowed */
int rg_softmax_rows_fwd(const float* x, float* y, int rows, int cols, float scale, rg_stream_t stream);
int rg_softmax_rows_bwd(const float* p, const float* dp, float* ds, int rows, int cols, float scale, rg_stream_t stream);

/* AEModel.hard_mix, CC/dual_gan/models/AE_model.py:274-292: out[j] = lam * src[idx_a[j]] + (1 - lam) * src[idx_b[j]] over rows
 * of `len` floats; idx_* are int64 device arrays of rows_out entries.  Backward: dsrc[r] = sum over the rows that read r. */
int rg_mix_rows_fwd(const float* src, const void* idx_a, const void* idx_b, float lam, float* out, int rows_src,
                    int rows_out, int64_t len, rg_stream_t stream);
int rg_mix_rows_bwd(const float* g, const void* idx_a, const void* idx_b, float lam, float* dsrc, int rows_src, int rows_out,
                    int64_t len, rg_stream_t stream);

/* ---- pooling -------------------------------------------------------------------------------- */
int rg_maxpool2d_fwd(const float* x, float* y, unsigned char* argmax, int N, int C, int H, int W, int KH, int KW,
                     int SH, int SW, int PH, int PW, int P, int Q, rg_stream_t stream);
int rg_maxpool2d_bwd(const float* dy, const unsigned char* argmax, float* dx, int N, int C, int H, int W, int KH,
                     int KW, int SH, int SW, int PH, int PW, int P, int Q, rg_stream_t stream);
/* F.avg_pool2d(x, x.size()[2:]), FD/reid/models/resnet.py:71 */
int rg_global_avgpool_fwd(const float* x, float* y, int N, int C, int HW, rg_stream_t stream);
int rg_global_avgpool_bwd(const float* dy, float* dx, int N, int C, int HW, rg_stream_t stream);
/* GeneralizedMeanPoolingP, CC/clustercontrast/models/pooling.py:57-103 */
int rg_gem_pool_fwd(const float* x, const float* p, float* y, int N, int C, int HW, float eps, rg_stream_t stream);
int rg_gem_pool_bwd(const float* x, const float* p, const float* y, const float* dy, float* dx, float* dp, int N,
                    int C, int HW, float eps, void* workspace, size_t workspace_bytes, rg_stream_t stream);
/* part pooling of the multi-part encoder, CC/clustercontrast/models/resnet_mp.py:111-114: y / dy are [2][N][C]; part 0 pools
   rows [0, split_row) of every plane, part 1 rows [split_row, H) (0 < split_row < H), both read in one pass.  p NULL: average
   pooling, else GeM with the one-element device exponent.  bwd writes every element of dx once; GeM reads x and the forward's y,
   dp (1 element, may be NULL) is the exponent gradient of both parts, summed through workspace (N*C floats) in a fixed order;
   average pooling reads neither x nor y and takes dp NULL */
int rg_part_pool_fwd(const float* x, const float* p, float* y, int N, int C, int H, int W, int split_row, float eps,
                     rg_stream_t stream);
int rg_part_pool_bwd(const float* x, const float* p, const float* y, const float* dy, float* dx, float* dp, int N, int C,
                     int H, int W, int split_row, float eps, void* workspace, size_t workspace_bytes, rg_stream_t stream);

/* ---- fused [B][D] tail of the multi-part encoder, CC/clustercontrast/models/resnet_mp.py:118-143 ---------------------------
 * z_j = BatchNorm1d_j(x_j) for the three branches j = g, p1, p2 (each with its own gamma, beta, running statistics, momentum and
 * eps; train: biased batch statistics, running statistics updated with the unbiased variance; eval: running statistics),
 * z_gc = z_g + z_p1 + z_p2 (fusion 1) or z_g (fusion 0), out[k] = z_k / max(|z_k|, 1e-12) per row for k = g, p1, p2, gc.
 *   forward   out [4][B][D]; saved for the backward: xhat [3][B][D] (the normalised activations), mean / invstd [3][D] (the batch
 *             statistics, or the running mean and rsqrt(running_var + eps) in eval mode), norms [4][B].  Train: 2 launches and
 *             rg_mp_head_workspace bytes of workspace (B >= 2); eval: 1 launch, no workspace.
 *   backward  any of the four upstream gradients may be NULL (an unused output); dz_j (may be NULL) is a gradient arriving at z_j
 *             itself (the 'cat' fusion reads the BatchNorm outputs).  dx_j / dgamma_j / dbeta_j may be NULL; dx_j only
 *             when no given gradient reaches branch j (then the branch is skipped), a branch without dx takes no affine
 *             gradients.  dx_j doubles as scratch between the two launches.
 * Deterministic (fixed summation order, no atomics). */
int64_t rg_mp_head_workspace(int B, int D);
int rg_mp_head_fwd(const float* x_g, const float* x_p1, const float* x_p2, const float* gamma_g, const float* gamma_p1,
                   const float* gamma_p2, const float* beta_g, const float* beta_p1, const float* beta_p2, float* rm_g,
                   float* rm_p1, float* rm_p2, float* rv_g, float* rv_p1, float* rv_p2, float* out, float* xhat, float* mean,
                   float* invstd, float* norms, int B, int D, int train, int fusion, float eps_g, float eps_p1, float eps_p2,
                   float mom_g, float mom_p1, float mom_p2, void* workspace, size_t workspace_bytes, rg_stream_t stream);
int rg_mp_head_bwd(const float* dy_g, const float* dy_p1, const float* dy_p2, const float* dy_gc, const float* dz_g,
                   const float* dz_p1, const float* dz_p2, const float* xhat, const float* invstd, const float* norms,
                   const float* gamma_g, const float* gamma_p1, const float* gamma_p2, const float* beta_g,
                   const float* beta_p1, const float* beta_p2, float* dx_g, float* dx_p1, float* dx_p2,
                   float* dgamma_g, float* dgamma_p1, float* dgamma_p2, float* dbeta_g, float* dbeta_p1, float* dbeta_p2, int B,
                   int D, int train, int fusion, rg_stream_t stream);

/* ---- fused verification head of FD-GAN stage I, FD/reid/models/embedding.py:7-39 (use_batch_norm, use_classifier) under
 * nn.CrossEntropyLoss() and FD/reid/evaluation_metrics/classification.py -------------------------------------------------------
 * d = (x1 - x2)^2 [B][D], z = BatchNorm1d(d) (train: biased batch statistics, running statistics updated with the unbiased
 * variance; eval: running statistics), logits = z W^T + bias with W [C][D], 1 <= C <= 16 (bias may be NULL).  With labels
 * (int64 [B], may be NULL): loss_rows[b] = logsumexp(logits_b) - logits_b[label_b], out2 = {mean_b loss_rows, correct / B} where
 * correct counts the rows whose argmax is the label (a tie goes to the LOWEST class index), dlogits = (softmax - onehot) / B.
 * A label outside [0, C) gives its row loss 0 and a zero dlogits row, as rg_softmax_ce_fwd; the mean still divides by B.
 *   forward   logits [B][C]; saved for the backward: xhat [B][D] (the normalised d), mean / invstd [D] (the batch statistics, or
 *             the running mean and rsqrt(running_var + eps) in eval mode); with labels also loss_rows [B], out2 [2], dlogits
 *             [B][C] (all three required then, ignored otherwise).  Train: 2 launches and rg_verif_head_workspace bytes of
 *             workspace (B >= 2); eval: 1 launch, no workspace (workspace may be NULL), one more launch with labels.
 *   backward  the logit gradient is grad_loss[0] * dlogits + dlogits_up: grad_loss is a 1-element device tensor (NULL = 1),
 *             dlogits the forward's (NULL = the loss takes no part, grad_loss must be NULL too), dlogits_up [B][C] an upstream
 *             gradient of the logits themselves (may be NULL); one of the two is given.  x1 and x2 are read again; no [B][D]
 *             tensor besides xhat is kept.  dx1 / dx2 [B][D], dW [C][D], dbias [C], dgamma / dbeta [D]: each may be NULL.
 *             1 launch.
 * Deterministic (fixed summation order, no atomics). */
int64_t rg_verif_head_workspace(int B, int D, int C);
int rg_verif_head_fwd(const float* x1, const float* x2, const float* gamma, const float* beta, float* running_mean,
                      float* running_var, const float* W, const float* bias, const int64_t* labels, float* logits, float* xhat,
                      float* mean, float* invstd, float* loss_rows, float* out2, float* dlogits, int B, int D, int C, int train,
                      float eps, float momentum, void* workspace, size_t workspace_bytes, rg_stream_t stream);
int rg_verif_head_bwd(const float* grad_loss, const float* dlogits, const float* dlogits_up, const float* x1, const float* x2,
                      const float* xhat, const float* invstd, const float* gamma, const float* beta, const float* W, float* dx1,
                      float* dx2, float* dW, float* dbias, float* dgamma, float* dbeta, int B, int D, int C, int train,
                      rg_stream_t stream);

/* ---- second stage of the cascade evaluation, FD/reid/evaluators.py:19-43 and :198-227 (csrc/cascade.hip) -----------------------
 * rg_pair_score: the verification head above in eval mode on GATHERED pairs.  Pair (q, j) is probe row q against gallery row
 * idx[q][j]:  d = (probe_q - g)^2,  z = gamma (d - running_mean) rsqrt(running_var + eps) + beta,  logits[c] = sum_ch z[ch]
 * W[c][ch] + bias[c] (bias may be NULL),  score = softmax(logits)[0] = 1 / sum_c exp(l_c - l_0), computed with the maximum
 * subtracted first (no overflow; exactly 1 for C == 1).  logits [Q][k][C] and score [Q][k] may each be NULL, not both.
 * Limits: 1 <= C <= 16, 1 <= D <= 8192, 1 <= k <= G, 1 <= Q <= 65535, Q k C < 2^31.  The per-channel constants a = gamma
 * rsqrt(running_var + eps) and t_c = W_c a are folded once per D-chunk and shared by the rows in flight, K_c = sum_ch beta W_c +
 * bias_c once per workgroup (all read through the cache); running_mean is subtracted from d before the scaling.  No [Q k][D] or [Q][G] temporary and no workspace.  An index outside [0, G) is the
 * caller's error: nothing is read for that pair and NaN is written.  One wave sums a pair in an order that depends on D alone:
 * the same bits for any grid, stream or chunking of the queries.  No atomics.
 * rg_pair_score_regime: which launch regime the shape takes (a value, not a status; -1 outside the limits): bit 0 16-byte
 * loads (D a multiple of 4 and `aligned`, the 16-byte alignment of the arrays; else 4-byte loads), bit 1 k is split over several
 * workgroups per query (Q below the CU count).
 * rg_cascade_merge: the reference's "merge two-stage distances" in place on dist [Q][ld] (ld >= G).  The k indices of a row are
 * distinct (a top-k); with S the set of columns idx[q][:], in float32 and in this order: nxt = min_{j not in S} dist[q][j] on
 * the first-stage values, bar = max_j score[q][j], gap = max((bar + 1) - nxt, 0), dist[q][idx[q][j]] = score[q][j], dist[q][j]
 * += gap for j not in S when gap > 0.  k == G: the overwrite alone.  Membership comes from idx (a bitmap of G bits in LDS,
 * G <= 1 048 576), never from comparing distances.  A row that holds a NaN comes back unspecified; nothing is read or written
 * out of bounds.  Bit-reproducible (no float atomics). */
int64_t rg_pair_score_regime(int Q, int k, int D, int C, int aligned);
int rg_pair_score(const float* probe, const float* gallery, const int* idx, const float* gamma, const float* beta,
                  const float* running_mean, const float* running_var, const float* W, const float* bias, float* logits,
                  float* score, int Q, int G, int k, int D, int C, float eps, rg_stream_t stream);
int rg_cascade_merge(float* dist, int64_t ld, const int* idx, const float* score, int Q, int G, int k, rg_stream_t stream);

/* ---- losses (scalar outputs live in device memory; grad_out is a 1-element device tensor or NULL) */
size_t rg_loss_workspace(void);
/* GANLoss: sigmoid + BCE vs constant target, FD/fdgan/losses.py:29-32 */
int rg_sigmoid_bce_fwd(const float* x, float* loss, int64_t n, float target, void* workspace, size_t workspace_bytes,
                       rg_stream_t stream);
int rg_sigmoid_bce_bwd(const float* x, const float* grad_out, float* dx, int64_t n, float target, float grad_scale,
                       rg_stream_t stream);
/* lsgan: MSE vs constant label, CC/dual_gan/models/external_function.py:53-57 */
int rg_mse_const_fwd(const float* x, float* loss, int64_t n, float target, void* workspace, size_t workspace_bytes,
                     rg_stream_t stream);
int rg_mse_const_bwd(const float* x, const float* grad_out, float* dx, int64_t n, float target, float grad_scale,
                     rg_stream_t stream);
/* F.l1_loss, optionally over the rows with row_labels == 1 (same-identity pairs), FD/fdgan/model.py:190-194.
 * out2[0] = loss, out2[1] = 1/(number of selected elements). */
int rg_l1_fwd(const float* a, const float* b, const int64_t* row_labels, float* out2, int rows, int64_t inner,
              void* workspace, size_t workspace_bytes, rg_stream_t stream);
int rg_l1_bwd(const float* a, const float* b, const int64_t* row_labels, const float* grad_out, const float* out2,
              float* da, float* db, int rows, int64_t inner, float grad_scale, rg_stream_t stream);
/* per-sample form: out[r] = mean_i |a[r][i] - b[r][i]| — nn.L1Loss(reduction='none')(a, b).flatten(1).mean(-1), the `loss_rec` of
 * AEModel.get_loss_G(need_cm=True), CC/dual_gan/models/AE_model.py:366 — and its backward from the per-row cotangent */
int rg_l1_rows_fwd(const float* a, const float* b, float* out, int rows, int64_t inner, rg_stream_t stream);
int rg_l1_rows_bwd(const float* a, const float* b, const float* grad_rows, float* da, float* db, int rows, int64_t inner,
                   rg_stream_t stream);
/* out[r] = mean_i (x[r][i] - c)^2: GANLoss('lsgan')(D(fake), label)'s map averaged per sample, AE_model.py:378-384 get_L1_loss(with_dis) */
int rg_mse_const_rows_fwd(const float* x, float c, float* out, int rows, int64_t inner, rg_stream_t stream);
int rg_mse_const_rows_bwd(const float* x, float c, const float* grad_rows, float* dx, int rows, int64_t inner, rg_stream_t stream);
/* F.cross_entropy(scale*logits, labels, reduction='none'), FD/fdgan/model.py:189, CC/.../cm.py:134-135 */
int rg_softmax_ce_fwd(const float* logits, const int64_t* labels, float* loss_rows, float* lse, int B, int K,
                      float scale, rg_stream_t stream);
int rg_softmax_ce_bwd(const float* logits, const int64_t* labels, const float* lse, const float* grad_rows,
                      float* dlogits, int B, int K, float scale, float grad_scale, rg_stream_t stream);
/* The same cross entropy over two logit blocks la[n][m] | lb[n][t] read where the GEMMs left them, with a group-diagonal mask:
 * row i is the cross entropy of scale * la[i][j] followed by scale * (lb[i][j] + (j == i / group ? mask : 0)), the addition in
 * fp32 before the multiply (`outputs_ex += -10000 * eye(t).repeat_interleave(group, 0)`, then `/= temp`,
 * CC/clustercontrast/models/cm.py:165-177).  n == t * group.  A label lies in [0, m + t); outside it the row's loss and both
 * gradient rows are 0.  dla / dlb = grad_rows[i] (1 when NULL) * grad_scale * scale * (softmax - onehot). */
int rg_softmax_ce_ext_fwd(const float* la, const float* lb, const int64_t* labels, float* loss_rows, float* lse, int n, int m,
                          int t, int group, float mask, float scale, rg_stream_t stream);
int rg_softmax_ce_ext_bwd(const float* la, const float* lb, const int64_t* labels, const float* lse, const float* grad_rows,
                          float grad_scale, float* dla, float* dlb, int n, int m, int t, int group, float mask, float scale,
                          rg_stream_t stream);
/* out[0] = scale * sum_i x[i]*w[i] (w may be NULL): .mean() / conf_mask weighting of per-sample losses */
int rg_weighted_sum_fwd(const float* x, const float* w, float* out, int64_t n, float scale, rg_stream_t stream);
int rg_weighted_sum_bwd(const float* grad_out, const float* w, float* dx, int64_t n, float scale, rg_stream_t stream);

/* ---- ClusterMemory momentum update, CC/clustercontrast/models/cm.py:29-31 (CM), :57-70 (CM_Hard),
 * :100-104 (CM_gan second bank: normalize_eps = 1).  In place on features[K][D], batch order kept. */
int rg_cm_update(const float* inputs, const int64_t* targets, float* features, int B, int D, int K, float momentum,
                 int normalize_eps, rg_stream_t stream);
int rg_cm_update_hard(const float* inputs, const int64_t* targets, float* features, int B, int D, int K,
                      float momentum, rg_stream_t stream);

/* ---- fused optimizer steps on contiguous ranges (FD/fdgan/model.py:100-125; CC/examples/
 * cluster_contrast_gan_train_usl_infomap.py:281-284). grad_scale multiplies g first (1/world for DDP). */
int rg_adam_step(float* p, const float* g, float* exp_avg, float* exp_avg_sq, int64_t n, float lr, float beta1,
                 float beta2, float eps, float weight_decay, int step, float grad_scale, rg_stream_t stream);
int rg_sgd_step(float* p, const float* g, float* momentum_buf, int64_t n, float lr, float momentum,
                float weight_decay, int first_step, float grad_scale, rg_stream_t stream);
/* Device-side clocks for hipGraph replay (kernel arguments are frozen at capture, so per-step values live in device memory):
 * Adam state double[4] = {step, beta1^step, beta2^step, -} (initialise {0, 1, 1, 0}); rg_adam_advance once per optimizer step,
 * then rg_adam_step_dev per parameter range; rg_u64_add advances a step counter that rg_dropout_clocked mixes into its seed. */
int rg_adam_advance(double* state, float beta1, float beta2, rg_stream_t stream);
int rg_adam_step_dev(float* p, const float* g, float* exp_avg, float* exp_avg_sq, int64_t n, float lr, float beta1, float beta2,
                     float eps, float weight_decay, const double* state, float grad_scale, rg_stream_t stream);
int rg_u64_add(unsigned long long* p, unsigned long long v, rg_stream_t stream);

/* ---- on-device input synthesis: the reference's per-sample PIL / scipy steps as batch kernels ---- */
/* Pose heat maps out[N][J][H][W] from integer joint centres centers[N][J][2] = (row, col); a negative (or out-of-range)
 * coordinate marks a missing / erased joint -> zero map.  sigma[N]: one Gaussian width per sample.
 * mode 0: FD/reid/utils/data/preprocessor.py:114-131 (_generate_pose_map) — unit impulse -> scipy gaussian_filter(sigma,
 *         truncate 4, mode 'reflect') -> divided by the map maximum (float64 arithmetic, float32 result);
 * mode 1: CC/clustercontrast/utils/data/pose_utils.py:51-70 (cords_to_map) — exp(-((y-r)^2 + (x-c)^2) / (2 sigma^2)); centres
 *         outside the image are evaluated like any other (the reference does), only INT32_MIN marks a missing joint.
 * The random choices (erased joint, sigma) are drawn on the host in the reference's order and arrive as inputs. */
int rg_pose_maps(const int* centers, const float* sigma, float* out, int N, int J, int H, int W, int mode,
                 rg_stream_t stream);
/* out[n][c][y][x] = P[n][c][top + y][left + (flip ? W-1-x : x)] with P = x[N][C][Hs][Ws] padded by `pad` pixels of
 * pad_value[c] (NULL: 0) and params[N][3] = (flip, top, left): torchvision's Pad(pad) + RandomCrop((H, W)) +
 * RandomHorizontalFlip of CC/examples/cluster_contrast_gan_train_usl_infomap.py:110-119, and np.flip(maps, 2) of
 * FD/reid/utils/data/preprocessor.py:88-91 (pad 0, top = left = 0). */
int rg_flip_pad_crop(const float* x, const int* params, const float* pad_value, float* out, int N, int C, int Hs, int Ws,
                     int H, int W, int pad, rg_stream_t stream);
/* RandomErasing, CC/clustercontrast/utils/data/transforms.py:52-96: x[n][c][r0:r0+h][c0:c0+w] = fill[c] in place for
 * rects[N][4] = (r0, c0, h, w); h = 0 leaves sample n untouched; a NaN fill[c] leaves channel c untouched (the reference
 * erases only channel 0 of non-RGB inputs). */
int rg_erase_rects(float* x, const int* rects, const float* fill, int N, int C, int H, int W, rg_stream_t stream);

/* ---- device-resident image bank (csrc/databank.hip): finished fp32 NCHW batches gathered from uint8 planes in HBM ----
 * The reference's host pipeline (CC/examples/cluster_contrast_gan_train_usl_infomap.py:71-186, preprocessor.py:99-199) resizes
 * every image deterministically BEFORE any random draw, so the resized uint8 planes are built once and kept on the device:
 * Market-1501 (35 585 images) is 3.5 GB at 256x128 plus 0.9 GB at 128x64, MSMT17 (126 441 images) 12.4 + 3.1 GB, of 288 GB.
 * Each entry is ONE launch, uses no workspace, no atomic and no intermediate batch, and reads per sample n the bank row idx[n].
 * idx and the draws are made on the host; the Python wrappers (rg_hip/ops/databank.py) refuse every out-of-range value before
 * the launch.  The kernels additionally read nothing for an index outside [0, M) (such a sample is written as padding / zeros).
 *
 * rg_bank_reid_batch: bank_u8[M][Hs][Ws][3] interleaved RGB bytes; params[N][8] int32 = (flip, top, left, er0, ec0, eh, ew,
 * reserved); lut[3][256] = ToTensor + Normalize of every byte value per channel, ((b / 255) - mean[c]) / std[c] computed by
 * the caller in fp32; fill[3] = RandomErasing's per-channel value.  The reference's order is Pad(pad, black) ->
 * RandomCrop((H, W)) -> ToTensor -> Normalize -> RandomErasing -> torch.flip(img, [2]); for out[n][c][y][x]:
 *     xs = flip ? W-1-x : x                                   (the rectangle and the crop are in PRE-flip coordinates)
 *     eh > 0 and (y, xs) in [er0, er0+eh) x [ec0, ec0+ew)  -> fill[c]
 *     (r, q) = (top + y - pad, left + xs - pad) outside the stored plane -> lut[c][0]   (normalised black)
 *     otherwise                                            -> lut[c][bank_u8[idx[n]][r][q][c]]
 * No floating-point arithmetic happens on the device, so the batch equals the host pipeline's bit for bit.  The test-time
 * transform (Resize -> ToTensor -> Normalize) is pad = 0, (H, W) = (Hs, Ws) and all-zero params.  Output rows are written with
 * 16-byte stores where W % 4 == 0, element by element otherwise. */
int rg_bank_reid_batch(const unsigned char* bank_u8, int M, int Hs, int Ws, const int* idx, const int* params, const float* lut,
                       const float* fill, float* out, int N, int H, int W, int pad, rg_stream_t stream);
/* The GAN branch's image (preprocessor.py:145-175, `Xs`): out[n][c][y][x] = lut[c][bank_u8[idx[n]][y][flip ? Wg-1-x : x][c]] from
 * a second plane set [M][Hg][Wg][3] with its own table (Normalize((.5,.5,.5), (.5,.5,.5))).  The flip of sample n is
 * flip[n * flip_stride], so column 0 of the ReID entry's params serves with flip_stride = 8. */
int rg_bank_gan_batch(const unsigned char* bank_u8, int M, int Hg, int Wg, const int* idx, const int* flip, int flip_stride,
                      const float* lut, float* out, int N, rg_stream_t stream);
/* The GAN branch's pose maps (`obtain_bone` + torch.flip(Ps, [2])): out[N][J][Hg][Wg] = rg_pose_maps mode 1 of the centres
 * centres[idx[n]][J][2] = (row, col) (INT32_MIN: missing joint -> zero map), one sigma for all, read at (y, flip ? Wg-1-x : x);
 * bit-equal to rg_pose_maps(mode 1) on the gathered centres followed by the flip.  The centres are computed once per image
 * when the bank is built (the reference recomputes them from a pandas row per draw). */
int rg_bank_pose_batch(const int* centres, int M, int J, const int* idx, const int* flip, int flip_stride, float sigma, float* out,
                       int N, int Hg, int Wg, rg_stream_t stream);
/* FD-GAN stage II's images (FD/train.py:21-44, FD/reid/utils/data/preprocessor.py:63-98: RectScale -> RandomSizedEarser ->
 * RandomHorizontalFlip -> ToTensor -> Normalize for `origin`; RectScale -> flip -> ToTensor -> Normalize for `target`) from planes
 * bank_u8[M][H][W][3] that hold RectScale's result.  params[N][8] int32 = (flip, 0, 0, er0, ec0, eh, ew, rgb) with
 * rgb = R | G << 8 | B << 16; for out[n][c][y][x]:
 *     xs = flip ? W-1-x : x                                   (the eraser runs BEFORE the flip: pre-flip coordinates)
 *     eh > 0 and (y, xs) in [er0, er0+eh) x [ec0, ec0+ew)  -> lut[c][byte c of rgb]    (the patch is pasted on BYTES, before
 *                                                             ToTensor / Normalize, so it goes through the same table)
 *     otherwise                                            -> lut[c][bank_u8[idx[n]][y][xs][c]]
 * This is rg_bank_reid_batch's kernel with one more compile-time case: no floating-point arithmetic, 16-byte stores where
 * W % 4 == 0.  A target row is a row with eh = 0, so ONE launch writes origin and target of both items of every pair. */
int rg_bank_fd_image_batch(const unsigned char* bank_u8, int M, int H, int W, const int* idx, const int* params, const float* lut,
                           float* out, int N, rg_stream_t stream);
/* FD-GAN stage II's pose maps (preprocessor.py:84-91, 114-131): out[N][J][H][W] = rg_pose_maps mode 0 of the landmarks
 * landmarks[idx[n]][J][2] = (row, col) as `_load_landmark` gives them (computed once per image), with the sample's own draws
 * pose_params[N][4] int32 = (flip, sigma, erased joint or -1, 0), read at (y, flip ? W-1-x : x).  The erased joint and any
 * coordinate outside [0, H) x [0, W) (-1: not detected) give a zero map.  Same profile code as rg_pose_maps (csrc/pose_profiles.h):
 * bit-equal to rg_pose_maps(mode 0) on the gathered landmarks followed by the flip.  The closed form counts the first mirror
 * image only: the caller guarantees int(4 sigma + 0.5) <= min(H, W) (rg_hip/ops/databank.py refuses anything else).  One
 * workgroup per (sample, joint), 16-byte row stores where W % 4 == 0; N <= 65535, H, W <= 1024. */
int rg_bank_fd_pose_batch(const int* landmarks, int M, int J, const int* idx, const int* pose_params, float* out, int N, int H,
                          int W, rg_stream_t stream);
/* FD-GAN stage I's images (FD/baseline.py:39-45: RandomSizedRectCrop -> RandomSizedEarser -> RandomHorizontalFlip -> ToTensor ->
 * Normalize) from a RAW bank: every image at its own size, bank_u8 + offsets[m] = [H_m][W_m][3] interleaved RGB bytes with
 * sizes[m] = (H_m, W_m).  The crop is `img.crop(box).resize((W, H), BILINEAR)`: the resize FOLLOWS the draw, so the kernel
 * resamples the box itself, with PIL's integer rule — a horizontal pass over the box's rows to a uint8 intermediate, a vertical
 * pass over that, each  out = min(255, (2^21 + sum_x in[lo + x] * k_x) >> 22).  The resample box is always the whole crop, so
 * (lo, cnt, k) of an axis depend on (input length, output length) only; the host builds them once in float64
 * (clustercontrast/utils/data/device_bank.py pil_bilinear_table): table_x holds (nmax_x + 1) * W rows of stride_x ints
 * (lo, cnt, k_0 .. k_{stride_x - 3}), row (n, j) for input length n and output column j at (n * W + j) * stride_x; table_y likewise
 * (nmax_y + 1) * H rows for input length n and output row j.  draws[N][12] int32 = (bank row, x1, y1, w, h, flip, er0, ec0, eh, ew,
 * rgb, 0): the box's left / upper corner and size in the image, the eraser's patch in the H x W output BEFORE the flip and its
 * colour R | G << 8 | B << 16; for out[n][c][r][x]:
 *     xs = flip ? W-1-x : x
 *     eh > 0 and (r, xs) in [er0, er0+eh) x [ec0, ec0+ew)  -> lut[c][byte c of rgb]
 *     otherwise                                            -> lut[c][two-pass resample of the box at (r, xs), channel c]
 * No floating-point arithmetic, no atomic, ONE launch, no intermediate in global memory: a workgroup keeps the horizontally
 * resampled bytes of its output columns in LDS ([3][h][columns]).  hmax >= every draw's h sizes that tile: a workgroup takes a strip of
 * output columns, the largest multiple of 4 up to 32 whose hmax x columns x 3 bytes fit 60 KiB (a whole sample where W is no wider).  rg_bank_fd_crop_regime returns
 * the columns per workgroup (a value, not a status: W = whole samples, less = strips, -1 = W no multiple of 4 or no strip fits).
 * W % 4 == 0 (16-byte row stores), N <= 65535.  The wrapper (rg_hip/ops/databank.py) refuses every draw outside its image before
 * the launch; the kernel additionally reads nothing for such a sample (it comes out as normalised black under its patch). */
int64_t rg_bank_fd_crop_regime(int hmax, int W);
int rg_bank_fd_crop_batch(const unsigned char* bank_u8, const int64_t* offsets, const int* sizes, int M, const int* table_x,
                          int stride_x, int nmax_x, const int* table_y, int stride_y, int nmax_y, const int* draws, const float* lut,
                          float* out, int N, int H, int W, int hmax, rg_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* REIDGAN_HIP_H */
