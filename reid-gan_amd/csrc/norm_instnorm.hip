// InstanceNorm2d (affine optional) for gfx950, one launch per direction on the row bodies of norm_rows.h: every lane group of
// 16 / 32 / 64 lanes, or a workgroup of 256, is one (n, c) instance and forms its own statistics / sums.
#include "norm_rows.h"

namespace {

// ---- InstanceNorm2d in one launch per direction: every lane group is one IBN_ROW_IN row (instance) -----------------------------------
template <int LANES>
__global__ __launch_bounds__(256) void instnorm_fwd_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                           const float* __restrict__ beta, const float* __restrict__ res,
                                                           float* __restrict__ y, float* __restrict__ mean_out,
                                                           float* __restrict__ invstd_out, int NC, int C, int HW, float eps,
                                                           int act, float slope) {
    __shared__ float red[4];
    const int inst = (int)blockIdx.x * (256 / LANES) + (int)threadIdx.x / LANES;
    if (inst >= NC) return;                                   // whole lane groups leave (LANES == 256: never taken, grid = NC)
    norm_row_fwd<LANES, 0>(x, res, y, 0u, (int64_t)inst * HW, HW, (int)threadIdx.x % LANES, red, true, 0.f, 0.f, eps, gamma, beta,
                           inst % C, act, slope, mean_out + inst, invstd_out + inst);
}

// sum_dy / sum_dy_xhat: per instance, for the affine gradients; sum_dx (may be NULL): the per-instance sums of dx
template <int LANES>
__global__ __launch_bounds__(256) void instnorm_bwd_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                           const float* __restrict__ yact, const float* __restrict__ mean,
                                                           const float* __restrict__ invstd, const float* __restrict__ gamma,
                                                           float* __restrict__ dx, float* __restrict__ dres,
                                                           float* __restrict__ sum_dy, float* __restrict__ sum_dy_xhat,
                                                           float* __restrict__ sum_dx, int NC, int C, int HW, int act,
                                                           float slope) {
    __shared__ float red[4];
    const int inst = (int)blockIdx.x * (256 / LANES) + (int)threadIdx.x / LANES;
    if (inst >= NC) return;
    norm_row_bwd<LANES, 0>(x, dy, yact, dx, dres, 0u, (int64_t)inst * HW, HW, (int)threadIdx.x % LANES, red, IBN_ROW_IN, mean[inst],
                           invstd[inst], 0.f, 0.f, gamma, inst % C, act, slope, sum_dy + inst, sum_dy_xhat + inst,
                           sum_dx ? sum_dx + inst : nullptr);
}

template <int LANES, int U>
__global__ __launch_bounds__(256) void instnorm_fwd_reg_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                               const float* __restrict__ beta, const float* __restrict__ res,
                                                               float* __restrict__ y, float* __restrict__ mean_out,
                                                               float* __restrict__ invstd_out, int NC, int C, int HW, float eps,
                                                               int act, float slope, unsigned bytes) {
    __shared__ float red[4];
    const int inst = (int)blockIdx.x * (256 / LANES) + (int)threadIdx.x / LANES;
    if (inst >= NC) return;
    norm_row_fwd<LANES, U>(x, res, y, bytes, (int64_t)inst * HW, HW, (int)threadIdx.x % LANES, red, true, 0.f, 0.f, eps, gamma, beta,
                           inst % C, act, slope, mean_out + inst, invstd_out + inst);
}

template <int LANES, int U>
__global__ __launch_bounds__(256) void instnorm_bwd_reg_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                               const float* __restrict__ yact, const float* __restrict__ mean,
                                                               const float* __restrict__ invstd, const float* __restrict__ gamma,
                                                               float* __restrict__ dx, float* __restrict__ dres,
                                                               float* __restrict__ sum_dy, float* __restrict__ sum_dy_xhat,
                                                               float* __restrict__ sum_dx, int NC, int C, int HW, int act,
                                                               float slope, unsigned bytes) {
    __shared__ float red[4];
    const int inst = (int)blockIdx.x * (256 / LANES) + (int)threadIdx.x / LANES;
    if (inst >= NC) return;
    norm_row_bwd<LANES, U>(x, dy, yact, dx, dres, bytes, (int64_t)inst * HW, HW, (int)threadIdx.x % LANES, red, IBN_ROW_IN, mean[inst],
                           invstd[inst], 0.f, 0.f, gamma, inst % C, act, slope, sum_dy + inst, sum_dy_xhat + inst,
                           sum_dx ? sum_dx + inst : nullptr);
}

using InPairs = LUList<LU<16, 0>, LU<16, 1>, LU<16, 2>, LU<32, 0>, LU<32, 1>, LU<32, 2>, LU<64, 0>, LU<64, 1>, LU<64, 2>, LU<64, 4>,
                       LU<64, 8>, LU<256, 0>, LU<256, 1>, LU<256, 2>, LU<256, 4>, LU<256, 8>>;

}  // namespace

// InstanceNorm2d forward: y = act(gamma[c] * (x - mean[n,c]) * invstd[n,c] + beta[c] + residual); mean / invstd [N*C] are kept for
// the backward.  One launch.
extern "C" int rg_instnorm_fwd(const float* x, const float* gamma, const float* beta, const float* residual, float* y,
                               float* mean, float* invstd, int N, int C, int HW, float eps, int act, float slope,
                               hipStream_t stream) {
    RG_REQUIRE(x && y && mean && invstd && N > 0 && C > 0 && HW > 0, "rg_instnorm_fwd: bad arguments");
    RG_REQUIRE((int64_t)N * C < (1ll << 31), "rg_instnorm_fwd: N*C exceeds 2^31");
    const int NC = N * C;
    rg::ProfScope prof(rg::FAM_NORM, stream, 0.0, (residual ? 12.0 : 8.0) * (double)NC * HW);
    const int lanes = in_lanes(HW), units = row_reg_units(HW, lanes, (int64_t)NC * HW);
    const unsigned bytes = units ? (unsigned)((int64_t)NC * HW * 4) : 0u;
    if (!with_lanes_units(InPairs{}, lanes, units, [&](auto L, auto U) {
            const dim3 grid(rg::cdiv(NC, 256 / L));
            if constexpr (U > 0)
                hipLaunchKernelGGL((instnorm_fwd_reg_kernel<L, U>), grid, dim3(256), 0, stream, x, gamma, beta, residual, y, mean,
                                   invstd, NC, C, HW, eps, act, slope, bytes);
            else
                hipLaunchKernelGGL(instnorm_fwd_kernel<L>, grid, dim3(256), 0, stream, x, gamma, beta, residual, y, mean, invstd, NC,
                                   C, HW, eps, act, slope);
        })) {
        rg::set_error("rg_instnorm_fwd: no kernel for %d lanes x %d units", lanes, units);
        return RG_ERR_INVALID;
    }
    return rg::check_launch("rg_instnorm_fwd");
}

// InstanceNorm2d backward in one launch: dx, dres (either may be NULL) and the per-instance sums [N*C] of g = dy*act'(y) and
// g*xhat (dbeta / dgamma = their sums over n: rg_rows_sum_pair); sum_dx (may be NULL) receives the per-instance sums of dx — the
// bias gradient of a convolution that feeds this layer, without another pass over dx.
extern "C" int rg_instnorm_bwd(const float* x, const float* dy, const float* y_act, const float* mean, const float* invstd,
                               const float* gamma, float* dx, float* dres, float* sum_dy, float* sum_dy_xhat, float* sum_dx, int N,
                               int C, int HW, int act, float slope, hipStream_t stream) {
    RG_REQUIRE(x && dy && mean && invstd && sum_dy && sum_dy_xhat && N > 0 && C > 0 && HW > 0, "rg_instnorm_bwd: bad arguments");
    RG_REQUIRE(act == RG_ACT_NONE || y_act, "rg_instnorm_bwd: fused activation needs the forward output");
    RG_REQUIRE((int64_t)N * C < (1ll << 31), "rg_instnorm_bwd: N*C exceeds 2^31");
    const int NC = N * C;
    rg::ProfScope prof(rg::FAM_NORM, stream, 0.0, ((act ? 12.0 : 8.0) + (dx ? 4.0 : 0.0) + (dres ? 4.0 : 0.0)) * (double)NC * HW);
    const int lanes = in_lanes(HW), units = row_reg_units(HW, lanes, (int64_t)NC * HW);
    const unsigned bytes = units ? (unsigned)((int64_t)NC * HW * 4) : 0u;
    if (!with_lanes_units(InPairs{}, lanes, units, [&](auto L, auto U) {
            const dim3 grid(rg::cdiv(NC, 256 / L));
            if constexpr (U > 0)
                hipLaunchKernelGGL((instnorm_bwd_reg_kernel<L, U>), grid, dim3(256), 0, stream, x, dy, y_act, mean, invstd, gamma, dx,
                                   dres, sum_dy, sum_dy_xhat, sum_dx, NC, C, HW, act, slope, bytes);
            else
                hipLaunchKernelGGL(instnorm_bwd_kernel<L>, grid, dim3(256), 0, stream, x, dy, y_act, mean, invstd, gamma, dx, dres,
                                   sum_dy, sum_dy_xhat, sum_dx, NC, C, HW, act, slope);
        })) {
        rg::set_error("rg_instnorm_bwd: no kernel for %d lanes x %d units", lanes, units);
        return RG_ERR_INVALID;
    }
    return rg::check_launch("rg_instnorm_bwd");
}
