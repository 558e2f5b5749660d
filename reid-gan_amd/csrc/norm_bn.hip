// BatchNorm (1d/2d, train and eval) for gfx950 — HBM-bound kernels: coalesced float4 streams,
// wave-shuffle (Chan) merges for the statistics, one read + one write per activation element.
//
// Replaces torch.nn.BatchNorm2d / BatchNorm1d as used by
//   ResNet-50 bottlenecks       CC/clustercontrast/models/resnet_ibn_a.py:70-109 (train mode in cluster-contrast,
//                               eval mode with trainable affine in FD-GAN: FD/fdgan/model.py:72-85, networks.py:57-60)
//   CustomPoseGenerator / NLayerDiscriminator norm layers   FD/fdgan/networks.py:26-35,141-156,218-229
//   EltwiseSubEmbed.bn, feat_bn                              FD/reid/models/embedding.py:16-19, CC/.../resnet.py:58-66
// Semantics follow torch: biased variance for normalisation, unbiased for running_var,
// running = (1-momentum)*running + momentum*batch.
//
// Tensor layout: [N][C][HW] contiguous (HW = 1 for BatchNorm1d on [N][C]).
//
// The kernels are in norm_bn.h (the two-domain layer of norm_dsbn.hip and the IBN layer of norm_ibn.hip run on them too); this unit
// holds the BatchNorm entry points and the eval-mode backward kernel.
#include "norm_bn.h"

namespace {

// Eval-mode backward in ONE pass (running statistics: dx does not depend on the channel sums):
//   g = dy * act'(y);  dx = gamma*invstd * g;  dres = g;  partial sums of g and g*xhat for dbeta / dgamma.
// Same (slice, channel) decomposition as the reduction kernel, so it reads x, dy, y once (12 B/element) and
// writes dx (+ dres) instead of the two-kernel reduce + apply sequence (28 B/element).
__global__ __launch_bounds__(256) void bn_eval_bwd_fused_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                                const float* __restrict__ yact,
                                                                const float* __restrict__ mean,
                                                                const float* __restrict__ var,
                                                                const float* __restrict__ gamma, float* __restrict__ dx,
                                                                float* __restrict__ dres, float* __restrict__ part,
                                                                int N, int C, int HW, int L, float eps, int act,
                                                                float slope, int want_sums) {
    const int c = blockIdx.y, s = blockIdx.x, S = gridDim.x;
    const int64_t total = (int64_t)N * HW;
    const int64_t beg = (int64_t)s * L;
    int64_t end = beg + L;
    if (end > total) end = total;
    const float mu = mean[c];
    const float is = rsqrtf(var[c] + eps);
    const float gs = (gamma ? gamma[c] : 1.f) * is;
    float s1 = 0.f, s2 = 0.f;
    if ((HW & 3) == 0) {
        for (int64_t e = beg + (int64_t)threadIdx.x * 4; e < end; e += 256 * 4) {
            const int n = (int)(e / HW);
            const int hw = (int)(e - (int64_t)n * HW);
            const int64_t o = ((int64_t)n * C + c) * HW + hw;
            float4 g = *reinterpret_cast<const float4*>(dy + o);
            if (act != RG_ACT_NONE) {
                const float4 yv = *reinterpret_cast<const float4*>(yact + o);
                g.x *= act_grad_from_out(yv.x, act, slope);
                g.y *= act_grad_from_out(yv.y, act, slope);
                g.z *= act_grad_from_out(yv.z, act, slope);
                g.w *= act_grad_from_out(yv.w, act, slope);
            }
            if (dres) *reinterpret_cast<float4*>(dres + o) = g;
            if (dx) *reinterpret_cast<float4*>(dx + o) = make_float4(gs * g.x, gs * g.y, gs * g.z, gs * g.w);
            if (want_sums) {
                const float4 xv = *reinterpret_cast<const float4*>(x + o);
                s1 += (g.x + g.y) + (g.z + g.w);
                s2 += (g.x * (xv.x - mu) + g.y * (xv.y - mu)) + (g.z * (xv.z - mu) + g.w * (xv.w - mu));
            }
        }
    } else {
        for (int64_t e = beg + threadIdx.x; e < end; e += 256) {
            const int n = (int)(e / HW);
            const int hw = (int)(e - (int64_t)n * HW);
            const int64_t o = ((int64_t)n * C + c) * HW + hw;
            float g = dy[o];
            if (act != RG_ACT_NONE) g *= act_grad_from_out(yact[o], act, slope);
            if (dres) dres[o] = g;
            if (dx) dx[o] = gs * g;
            if (want_sums) {
                s1 += g;
                s2 += g * (x[o] - mu);
            }
        }
    }
    if (!want_sums) return;
    s2 *= is;
    __shared__ float red[16];
    s1 = rg_block_sum(s1, red);
    s2 = rg_block_sum(s2, red);
    if (threadIdx.x == 0) {
        float* o = part + ((int64_t)c * S + s) * 2;
        o[0] = s1;
        o[1] = s2;
    }
}

}  // namespace

void rg::bn_launch_stats(const float* x, float* part, int N, int Cn, int C, int HW, int S, int L, float eps, float momentum,
                         float* mean, float* invstd, float* running_mean, float* running_var, hipStream_t stream) {
    hipLaunchKernelGGL(bn_stats_partial_kernel, dim3(S, Cn), dim3(256), 0, stream, x, part, N, C, HW, L);
    hipLaunchKernelGGL(bn_stats_finalize_kernel, dim3(rg::cdiv(Cn, 64)), dim3(64), 0, stream, part, Cn, S, eps, momentum,
                       mean, invstd, running_mean, running_var);
}

void rg::bn_launch_bwd_reduce(const float* x, const float* dy, const float* yact, const float* mean, const float* stat, float* part,
                              int N, int Cn, int C, int HW, int S, int L, int stat_is_var, float eps, int act, float slope,
                              float* sum_dy, float* sum_dy_xhat, hipStream_t stream) {
    hipLaunchKernelGGL(bn_bwd_reduce_partial_kernel, dim3(S, Cn), dim3(256), 0, stream, x, dy, yact, mean, stat, part, N,
                       C, HW, L, stat_is_var, eps, act, slope);
    hipLaunchKernelGGL(bn_bwd_reduce_finalize_kernel, dim3(rg::cdiv(Cn, 64)), dim3(64), 0, stream, part, Cn, S, sum_dy,
                       sum_dy_xhat);
}

extern "C" size_t rg_bn_workspace(int N, int C, int HW) {
    int L;
    const int S = pick_slices(N, C, HW, &L);
    return (size_t)C * S * 3 * sizeof(float);
}

// Batch statistics of x[N][C][HW]: mean[C], invstd[C] (=1/sqrt(biased var + eps)); updates the
// running statistics in place when they are given.
extern "C" int rg_bn_stats(const float* x, float* mean, float* invstd, float* running_mean, float* running_var, int N,
                           int C, int HW, float eps, float momentum, void* workspace, size_t workspace_bytes,
                           hipStream_t stream) {
    RG_REQUIRE(x && mean && invstd && N > 0 && C > 0 && HW > 0, "rg_bn_stats: bad arguments");
    RG_REQUIRE((int64_t)N * HW < (1ll << 31), "rg_bn_stats: N*HW exceeds 2^31");
    int L;
    const int S = pick_slices(N, C, HW, &L);
    if (!workspace || workspace_bytes < (size_t)C * S * 3 * sizeof(float)) {
        rg::set_error("rg_bn_stats: workspace too small");
        return RG_ERR_WORKSPACE;
    }
    float* part = static_cast<float*>(workspace);
    rg::ProfScope prof(rg::FAM_NORM, stream, 0.0, 4.0 * N * (double)C * HW);
    rg::bn_launch_stats(x, part, N, C, C, HW, S, L, eps, momentum, mean, invstd, running_mean, running_var, stream);
    return rg::check_launch("rg_bn_stats");
}

extern "C" int rg_bn_apply_fwd(const float* x, const float* mean, const float* stat, const float* gamma,
                               const float* beta, const float* residual, float* y, int N, int C, int HW,
                               int stat_is_var, float eps, int act, float slope, hipStream_t stream) {
    RG_REQUIRE(x && mean && stat && y && N > 0 && C > 0 && HW > 0, "rg_bn_apply_fwd: bad arguments");
    const int64_t total = (int64_t)N * C * HW;
    rg::ProfScope prof(rg::FAM_NORM, stream, 0.0, (residual ? 12.0 : 8.0) * total);
    hipLaunchKernelGGL(bn_apply_fwd_kernel, dim3(rg::grid_for((HW & 3) ? total : total / 4, NORM_GRID_CAP)), dim3(256), 0, stream, x, mean,
                       stat, gamma, beta, residual, y, total, C, HW, stat_is_var, eps, act, slope);
    return rg::check_launch("rg_bn_apply_fwd");
}

// Per-channel sums for the affine gradients: dbeta = sum(dy*act'(y)), dgamma = sum(dy*act'(y)*xhat).
extern "C" int rg_bn_bwd_reduce(const float* x, const float* dy, const float* y_act, const float* mean,
                                const float* stat, float* sum_dy, float* sum_dy_xhat, int N, int C, int HW,
                                int stat_is_var, float eps, int act, float slope, void* workspace,
                                size_t workspace_bytes, hipStream_t stream) {
    RG_REQUIRE(x && dy && mean && stat && sum_dy && sum_dy_xhat, "rg_bn_bwd_reduce: null tensor");
    RG_REQUIRE(act == RG_ACT_NONE || y_act, "rg_bn_bwd_reduce: fused activation needs the forward output");
    int L;
    const int S = pick_slices(N, C, HW, &L);
    if (!workspace || workspace_bytes < (size_t)C * S * 2 * sizeof(float)) {
        rg::set_error("rg_bn_bwd_reduce: workspace too small");
        return RG_ERR_WORKSPACE;
    }
    float* part = static_cast<float*>(workspace);
    rg::ProfScope prof(rg::FAM_NORM, stream, 0.0, (act ? 12.0 : 8.0) * N * (double)C * HW);
    rg::bn_launch_bwd_reduce(x, dy, y_act, mean, stat, part, N, C, C, HW, S, L, stat_is_var, eps, act, slope, sum_dy, sum_dy_xhat,
                             stream);
    return rg::check_launch("rg_bn_bwd_reduce");
}

// dx (may be NULL) and dres (may be NULL; the gradient of a fused residual input = dy*act'(y)).
extern "C" int rg_bn_bwd_apply(const float* x, const float* dy, const float* y_act, const float* mean,
                               const float* stat, const float* gamma, const float* sum_dy, const float* sum_dy_xhat,
                               float* dx, float* dres, int N, int C, int HW, int train, int stat_is_var, float eps,
                               int act, float slope, hipStream_t stream) {
    RG_REQUIRE(dy && mean && stat && (dx || dres), "rg_bn_bwd_apply: null tensor");
    RG_REQUIRE(!train || (x && sum_dy && sum_dy_xhat), "rg_bn_bwd_apply: train mode needs x and the channel sums");
    RG_REQUIRE(act == RG_ACT_NONE || y_act, "rg_bn_bwd_apply: fused activation needs the forward output");
    const int64_t total = (int64_t)N * C * HW;
    rg::ProfScope prof(rg::FAM_NORM, stream, 0.0, 16.0 * total);
    hipLaunchKernelGGL(bn_bwd_apply_kernel, dim3(rg::grid_for((HW & 3) ? total : total / 4, NORM_GRID_CAP)), dim3(256), 0, stream, x, dy,
                       y_act, mean, stat, gamma, sum_dy, sum_dy_xhat, dx, dres, total, C, HW,
                       1.f / (float)((int64_t)N * HW), train, stat_is_var, eps, act, slope);
    return rg::check_launch("rg_bn_bwd_apply");
}

// Eval-mode (running statistics) backward in one pass: dx (may be NULL), dres (may be NULL) and, when sum_dy /
// sum_dy_xhat are given, the channel sums for dbeta / dgamma (FD-GAN trains the affine parameters of E's and D_id's
// frozen BatchNorms: FD/fdgan/model.py:72-85).
extern "C" int rg_bn_eval_bwd(const float* x, const float* dy, const float* y_act, const float* running_mean,
                              const float* running_var, const float* gamma, float* dx, float* dres, float* sum_dy,
                              float* sum_dy_xhat, int N, int C, int HW, float eps, int act, float slope,
                              void* workspace, size_t workspace_bytes, hipStream_t stream) {
    RG_REQUIRE(dy && running_mean && running_var && (dx || dres || sum_dy), "rg_bn_eval_bwd: null tensor");
    RG_REQUIRE(act == RG_ACT_NONE || y_act, "rg_bn_eval_bwd: fused activation needs the forward output");
    const int want = (sum_dy && sum_dy_xhat) ? 1 : 0;
    RG_REQUIRE(!want || x, "rg_bn_eval_bwd: the channel sums need x");
    int L;
    const int S = pick_slices(N, C, HW, &L);
    if (want && (!workspace || workspace_bytes < (size_t)C * S * 2 * sizeof(float))) {
        rg::set_error("rg_bn_eval_bwd: workspace too small");
        return RG_ERR_WORKSPACE;
    }
    float* part = static_cast<float*>(workspace);
    rg::ProfScope prof(rg::FAM_NORM, stream, 0.0, (want ? 12.0 : 8.0) * N * (double)C * HW + (dx ? 4.0 : 0.0) * N * (double)C * HW +
                                                         (dres ? 4.0 : 0.0) * N * (double)C * HW);
    hipLaunchKernelGGL(bn_eval_bwd_fused_kernel, dim3(S, C), dim3(256), 0, stream, x, dy, y_act, running_mean,
                       running_var, gamma, dx, dres, part, N, C, HW, L, eps, act, slope, want);
    if (want)
        hipLaunchKernelGGL(bn_bwd_reduce_finalize_kernel, dim3(rg::cdiv(C, 64)), dim3(64), 0, stream, part, C, S, sum_dy,
                           sum_dy_xhat);
    return rg::check_launch("rg_bn_eval_bwd");
}

// slices per channel of the slice-parallel kernels for this geometry (the S of rg_bn_workspace and of rg_act_bwd_partial's part[C][S])
extern "C" int rg_bn_slices(int N, int C, int HW) {
    int L;
    return pick_slices(N, C, HW, &L);
}

// Train-mode BatchNorm, one launch per direction (see the kernels): rg_bn_train_fused_ok says whether the geometry qualifies;
// otherwise use rg_bn_stats + rg_bn_apply_fwd / rg_bn_bwd_reduce + rg_bn_bwd_apply.
extern "C" size_t rg_bn_train_fused_ok(int N, int C, int HW) {
    return (int64_t)N * HW <= 16384 && C >= 128 ? 1 : 0;
}

extern "C" int rg_bn_train_fwd_fused(const float* x, const float* gamma, const float* beta, const float* residual, float* y,
                                     float* mean, float* invstd, float* running_mean, float* running_var, int N, int C, int HW,
                                     float eps, float momentum, int act, float slope, hipStream_t stream) {
    RG_REQUIRE(x && y && mean && invstd && N > 0 && C > 0 && HW > 0, "rg_bn_train_fwd_fused: bad arguments");
    RG_REQUIRE((int64_t)N * HW < (1ll << 30), "rg_bn_train_fwd_fused: N*HW too large");
    rg::ProfScope prof(rg::FAM_NORM, stream, 0.0, (residual ? 12.0 : 8.0) * N * (double)C * HW);
    const unsigned bytes = (unsigned)((int64_t)N * C * HW * 4);
    if (!with_lanes_units(BnUnits{}, 256, g_bn_reg ? bn_reg_units(N, C, HW) : 0, [&](auto, auto U) {
            hipLaunchKernelGGL(bn_train_fwd_reg_kernel<U>, dim3(C), dim3(256), 0, stream, x, gamma, beta, residual, y, mean, invstd,
                               running_mean, running_var, N, C, HW, eps, momentum, act, slope, bytes);
        }))
        hipLaunchKernelGGL(bn_train_fwd_fused_kernel, dim3(C), dim3(256), 0, stream, x, gamma, beta, residual, y, mean, invstd,
                           running_mean, running_var, N, C, HW, eps, momentum, act, slope);
    return rg::check_launch("rg_bn_train_fwd_fused");
}

extern "C" int rg_bn_train_bwd_fused(const float* x, const float* dy, const float* y_act, const float* mean, const float* invstd,
                                     const float* gamma, float* dx, float* dres, float* sum_dy, float* sum_dy_xhat, int N, int C,
                                     int HW, int act, float slope, hipStream_t stream) {
    RG_REQUIRE(x && dy && mean && invstd && sum_dy && sum_dy_xhat && N > 0 && C > 0 && HW > 0, "rg_bn_train_bwd_fused: bad arguments");
    RG_REQUIRE(act == RG_ACT_NONE || y_act, "rg_bn_train_bwd_fused: fused activation needs the forward output");
    RG_REQUIRE((int64_t)N * HW < (1ll << 30), "rg_bn_train_bwd_fused: N*HW too large");
    rg::ProfScope prof(rg::FAM_NORM, stream, 0.0, ((act ? 12.0 : 8.0) + (dx ? 4.0 : 0.0) + (dres ? 4.0 : 0.0)) * N * (double)C * HW);
    const unsigned bytes = (unsigned)((int64_t)N * C * HW * 4);
    if (!with_lanes_units(BnUnits{}, 256, g_bn_reg ? bn_reg_units(N, C, HW) : 0, [&](auto, auto U) {
            hipLaunchKernelGGL(bn_train_bwd_reg_kernel<U>, dim3(C), dim3(256), 0, stream, x, dy, y_act, mean, invstd, gamma, dx, dres,
                               sum_dy, sum_dy_xhat, N, C, HW, act, slope, bytes);
        }))
        hipLaunchKernelGGL(bn_train_bwd_fused_kernel, dim3(C), dim3(256), 0, stream, x, dy, y_act, mean, invstd, gamma, dx, dres,
                           sum_dy, sum_dy_xhat, N, C, HW, act, slope);
    return rg::check_launch("rg_bn_train_bwd_fused");
}

// float4 units per thread the one-workgroup-per-channel kernels run with for N samples (what rg_bn_train_*_fused and, with N / 2,
// rg_dsbn_* launch): 1, 2, 4, 8, 16 = the register kernels, 0 = the loop kernels (scalar rows, more than 16 units, or RG_BN_REG=0)
extern "C" int rg_bn_reg_units(int N, int C, int HW) { return g_bn_reg && N > 0 && C > 0 && HW > 0 ? bn_reg_units(N, C, HW) : 0; }
