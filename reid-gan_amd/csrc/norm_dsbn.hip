// Domain-specific BatchNorm (DSBN): one [source half | target half] batch, every half with its own parameters and running
// statistics, on the BatchNorm kernels of norm_bn.h instantiated with the Dsbn* structs (see the comment on them there).
//
// Regime by the per-domain extent h*HW alone, h = N / 2: one launch per direction (2C workgroups) when h*HW <= 16384; otherwise slice
// partial + finalize + apply over both domains at once — three launches, as ONE BatchNorm.  No channel threshold as in
// rg_bn_train_fused_ok: the two-pass statistics of the one-launch kernels do not depend on how many values a thread is left with,
// while the slice kernels at a handful of values per thread merge single-value statistics and lose accuracy when |mean| >> std.
// (Whether three launches would be faster for few channels at the largest such extent, e.g. C = 64 on 128 workgroups, is not measured.)
#include "norm_bn.h"

static bool dsbn_one_launch(int h, int C, int HW) { return (int64_t)h * HW <= 16384; }

// slices of one domain's h*HW values: as many workgroups as a BatchNorm over 2C channels would start
static int dsbn_slices(int h, int C, int HW, int* L) { return pick_slices(h, 2 * C, HW, L); }

// bytes of workspace for rg_dsbn_fwd / rg_dsbn_bwd: the slice partials [2][C][S][3] (0 for an invalid geometry)
extern "C" int64_t rg_dsbn_workspace(int N, int C, int HW) {
    if (N <= 0 || (N & 1) || C <= 0 || HW <= 0) return 0;
    int L;
    const int S = dsbn_slices(N / 2, C, HW, &L);
    return (int64_t)((size_t)2 * C * S * 3 * sizeof(float));
}

// 1: one launch per direction, 0: the slice regime (rg_dsbn_slices slices per domain)
extern "C" int rg_dsbn_one_launch(int N, int C, int HW) { return N > 0 && !(N & 1) && dsbn_one_launch(N / 2, C, HW) ? 1 : 0; }

extern "C" int rg_dsbn_slices(int N, int C, int HW) {
    if (N <= 0 || (N & 1) || C <= 0 || HW <= 0) return 0;
    int L;
    return dsbn_slices(N / 2, C, HW, &L);
}

extern "C" int rg_dsbn_fwd(const float* x, const float* gamma_s, const float* beta_s, const float* gamma_t, const float* beta_t,
                           const float* residual, float* y, float* mean, float* invstd, float* running_mean_s, float* running_var_s,
                           float* running_mean_t, float* running_var_t, int N, int C, int HW, float eps_s, float eps_t,
                           float momentum_s, float momentum_t, int act, float slope, void* workspace, size_t workspace_bytes,
                           hipStream_t stream) {
    RG_REQUIRE(x && y && mean && invstd && N > 0 && C > 0 && HW > 0, "rg_dsbn_fwd: bad arguments");
    RG_REQUIRE((N & 1) == 0, "rg_dsbn_fwd: the batch of %d samples has no [source | target] halves", N);
    const int h = N / 2;
    RG_REQUIRE((int64_t)h * HW < (1ll << 30) && (int64_t)2 * C < (1ll << 16), "rg_dsbn_fwd: N*HW or C too large");
    const DsbnFwd a = {{{gamma_s, beta_s, running_mean_s, running_var_s, eps_s, momentum_s},
                        {gamma_t, beta_t, running_mean_t, running_var_t, eps_t, momentum_t}}};
    const float* no = nullptr;                           // per-domain arguments of the BatchNorm kernels: taken from `a` in the kernel
    float* non = nullptr;
    const int64_t half_total = (int64_t)h * C * HW;
    rg::ProfScope prof(rg::FAM_NORM, stream, 0.0, (residual ? 12.0 : 8.0) * 2.0 * (double)half_total);
    if (dsbn_one_launch(h, C, HW)) {                     // the BatchNorm kernels over h samples, grid (C, 2)
        const unsigned bytes = (unsigned)(half_total * 4);
        if (!with_lanes_units(BnUnits{}, 256, g_bn_reg ? bn_reg_units(h, C, HW) : 0, [&](auto, auto U) {
                hipLaunchKernelGGL(bn_train_fwd_reg_kernel<U>, dim3(C, 2), dim3(256), 0, stream, x, no, no, residual, y, mean, invstd, non,
                                   non, h, C, HW, 0.f, 0.f, act, slope, bytes, a);
            }))
            hipLaunchKernelGGL(bn_train_fwd_fused_kernel, dim3(C, 2), dim3(256), 0, stream, x, no, no, residual, y, mean, invstd, non, non,
                               h, C, HW, 0.f, 0.f, act, slope, a);
        return rg::check_launch("rg_dsbn_fwd");
    }
    int L;
    const int S = dsbn_slices(h, C, HW, &L);
    if (!workspace || workspace_bytes < (size_t)2 * C * S * 3 * sizeof(float)) {
        rg::set_error("rg_dsbn_fwd: workspace too small");
        return RG_ERR_WORKSPACE;
    }
    float* part = static_cast<float*>(workspace);
    hipLaunchKernelGGL(bn_stats_partial_kernel, dim3(S, C, 2), dim3(256), 0, stream, x, part, h, C, HW, L, DsbnPlane{});
    hipLaunchKernelGGL(bn_stats_finalize_kernel, dim3(rg::cdiv(C, 64), 2), dim3(64), 0, stream, (const float*)part, C, S, 0.f, 0.f, mean,
                       invstd, non, non, a);
    hipLaunchKernelGGL(bn_apply_fwd_kernel, dim3(rg::grid_for((HW & 3) ? half_total : half_total / 4, NORM_GRID_CAP), 2), dim3(256), 0, stream, x,
                       (const float*)mean, (const float*)invstd, no, no, residual, y, half_total, C, HW, 0, 0.f, act, slope, a);
    return rg::check_launch("rg_dsbn_fwd");
}

// dx, dres (either may be NULL) and the four affine gradients (outputs: the channel sums are written straight into them).
// mean / invstd [2][C] as rg_dsbn_fwd wrote them.
extern "C" int rg_dsbn_bwd(const float* x, const float* dy, const float* y_act, const float* mean, const float* invstd,
                           const float* gamma_s, const float* gamma_t, float* dx, float* dres, float* d_gamma_s, float* d_beta_s,
                           float* d_gamma_t, float* d_beta_t, int N, int C, int HW, int act, float slope, void* workspace,
                           size_t workspace_bytes, hipStream_t stream) {
    RG_REQUIRE(x && dy && mean && invstd && N > 0 && C > 0 && HW > 0, "rg_dsbn_bwd: bad arguments");
    RG_REQUIRE(d_gamma_s && d_beta_s && d_gamma_t && d_beta_t, "rg_dsbn_bwd: the four affine gradients are outputs");
    RG_REQUIRE((N & 1) == 0, "rg_dsbn_bwd: the batch of %d samples has no [source | target] halves", N);
    RG_REQUIRE(act == RG_ACT_NONE || y_act, "rg_dsbn_bwd: fused activation needs the forward output");
    const int h = N / 2;
    RG_REQUIRE((int64_t)h * HW < (1ll << 30) && (int64_t)2 * C < (1ll << 16), "rg_dsbn_bwd: N*HW or C too large");
    const DsbnBwd a = {{gamma_s, gamma_t}, {d_gamma_s, d_gamma_t}, {d_beta_s, d_beta_t}};
    const float* no = nullptr;                           // gamma and the sums: taken from `a` in the kernel
    float* non = nullptr;
    const int64_t half_total = (int64_t)h * C * HW;
    rg::ProfScope prof(rg::FAM_NORM, stream, 0.0,
                       ((act ? 12.0 : 8.0) + (dx ? 4.0 : 0.0) + (dres ? 4.0 : 0.0)) * 2.0 * (double)half_total);
    if (dsbn_one_launch(h, C, HW)) {
        const unsigned bytes = (unsigned)(half_total * 4);
        if (!with_lanes_units(BnUnits{}, 256, g_bn_reg ? bn_reg_units(h, C, HW) : 0, [&](auto, auto U) {
                hipLaunchKernelGGL(bn_train_bwd_reg_kernel<U>, dim3(C, 2), dim3(256), 0, stream, x, dy, y_act, mean, invstd, no, dx, dres,
                                   non, non, h, C, HW, act, slope, bytes, a);
            }))
            hipLaunchKernelGGL(bn_train_bwd_fused_kernel, dim3(C, 2), dim3(256), 0, stream, x, dy, y_act, mean, invstd, no, dx, dres, non,
                               non, h, C, HW, act, slope, a);
        return rg::check_launch("rg_dsbn_bwd");
    }
    int L;
    const int S = dsbn_slices(h, C, HW, &L);
    if (!workspace || workspace_bytes < (size_t)2 * C * S * 2 * sizeof(float)) {
        rg::set_error("rg_dsbn_bwd: workspace too small");
        return RG_ERR_WORKSPACE;
    }
    float* part = static_cast<float*>(workspace);
    hipLaunchKernelGGL(bn_bwd_reduce_partial_kernel, dim3(S, C, 2), dim3(256), 0, stream, x, dy, y_act, mean, invstd, part, h, C, HW, L,
                       0, 0.f, act, slope, DsbnPlane{});
    hipLaunchKernelGGL(bn_bwd_reduce_finalize_kernel, dim3(rg::cdiv(C, 64), 2), dim3(64), 0, stream, (const float*)part, C, S, non, non,
                       a);
    if (dx || dres)
        hipLaunchKernelGGL(bn_bwd_apply_kernel, dim3(rg::grid_for((HW & 3) ? half_total : half_total / 4, NORM_GRID_CAP), 2), dim3(256), 0, stream, x, dy,
                           y_act, mean, invstd, no, no, no, dx, dres, half_total, C, HW, 1.f / (float)((int64_t)h * HW), 1, 0, 0.f, act,
                           slope, a);
    return rg::check_launch("rg_dsbn_bwd");
}
