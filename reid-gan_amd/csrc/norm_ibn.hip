// IBN-a for gfx950: InstanceNorm on channels [0, half), BatchNorm on [half, C) of ONE [N][C][HW] tensor.
// The reference writes the layer as split -> contiguous x 2 -> two norms -> cat (CC/clustercontrast/models/resnet_ibn_a.py:54-68):
// six extra passes over the activation per direction.  Here both halves are normalised in place of layout: the only tensors of
// the activation's size are x, y (forward) and x, dy, y, dx (backward).
//   row kernels     one lane group per row (n, c), on the row bodies of the InstanceNorm kernels (norm_row_fwd / norm_row_bwd: the
//                   same lane counts, the same register and loop forms; only the backward register row is the layer's own,
//                   ibn_row_bwd_reg).  An IN row forms its own statistics / sums; a BN row
//                   takes the channel's statistics (running ones in eval mode, the batch ones of the slice-parallel
//                   bn_stats_partial / bn_bwd_reduce_partial kernels, run over the channel sub-range with the full tensor's
//                   sample stride, in train mode).  A lane group is one kind of row, so the branches are group-uniform.
//   fused kernels   train mode with N*HW <= 16384: workgroups [0, C - half) each own one BN channel (bn_channel_fwd / _bwd, the
//                   one-workgroup-per-channel scheme), the rest of the grid are IN lane groups: one launch per direction.
// Backward sums: IN rows write sum g and sum g*xhat per instance, eval-mode BN rows per (n, channel) as well (their dx needs no
// channel sum, so the row is read once); rows_sum_pair_kernel adds them over n into the four affine gradients.  Train-mode BN
// channel sums come from the channel workgroups / the slice reduction and ARE dbeta / dgamma.  Fixed summation order, no atomics.
#include "norm_bn.h"
#include "norm_rows.h"

namespace {

// every row (n, c) of the tensor; BN rows use bn_mean / bn_stat [C - half] (stat_is_var: a variance, eps applied here)
template <int LANES, int U>
__global__ __launch_bounds__(256) void ibn_fwd_rows_kernel(const float* __restrict__ x, const float* __restrict__ in_gamma,
                                                           const float* __restrict__ in_beta, const float* __restrict__ bn_gamma,
                                                           const float* __restrict__ bn_beta, const float* __restrict__ bn_mean,
                                                           const float* __restrict__ bn_stat, float* __restrict__ y,
                                                           float* __restrict__ in_mean, float* __restrict__ in_invstd, int NC, int C,
                                                           int half, int HW, int stat_is_var, float in_eps, float bn_eps, int act,
                                                           unsigned bytes) {
    __shared__ float red[4];
    const int row = (int)blockIdx.x * (256 / LANES) + (int)threadIdx.x / LANES;
    if (row >= NC) return;                                       // whole lane groups leave (LANES == 256: grid = NC)
    const int n = row / C, c = row - n * C;
    const bool in_row = c < half;
    const int pc = in_row ? c : c - half;                        // index of the row's affine parameters (and BN statistics)
    const int inst = n * half + pc;                              // IN rows only
    float mu = 0.f, is = 0.f;
    if (!in_row) {
        mu = bn_mean[pc];
        is = bn_stat[pc];
        if (stat_is_var) is = rsqrtf(is + bn_eps);
    }
    norm_row_fwd<LANES, U>(x, nullptr, y, bytes, (int64_t)row * HW, HW, (int)threadIdx.x % LANES, red, in_row, mu, is, in_eps,
                           in_row ? in_gamma : bn_gamma, in_row ? in_beta : bn_beta, pc, act, 0.f, in_mean + inst, in_invstd + inst);
}

// grid = (C - half) BN channel workgroups, then the IN lane groups over the N * half instances
template <int LANES, int U>
__global__ __launch_bounds__(256) void ibn_train_fwd_fused_kernel(const float* __restrict__ x, const float* __restrict__ in_gamma,
                                                                  const float* __restrict__ in_beta, const float* __restrict__ bn_gamma,
                                                                  const float* __restrict__ bn_beta, float* __restrict__ y,
                                                                  float* __restrict__ in_mean, float* __restrict__ in_invstd,
                                                                  float* __restrict__ bn_mean, float* __restrict__ bn_invstd,
                                                                  float* __restrict__ running_mean, float* __restrict__ running_var,
                                                                  int N, int C, int half, int HW, float in_eps, float bn_eps,
                                                                  float momentum, int act, unsigned bytes) {
    __shared__ float red[4];
    const int cb = C - half;
    if ((int)blockIdx.x < cb) {                                   // workgroup-uniform
        bn_channel_fwd(x, bn_gamma, bn_beta, nullptr, y, bn_mean, bn_invstd, running_mean, running_var, N, C, HW, bn_eps, momentum,
                       act, 0.f, half + (int)blockIdx.x, (int)blockIdx.x, red);
        return;
    }
    const int inst = ((int)blockIdx.x - cb) * (256 / LANES) + (int)threadIdx.x / LANES;
    if (inst >= N * half) return;
    const int n = inst / half, c = inst - n * half;
    norm_row_fwd<LANES, U>(x, nullptr, y, bytes, ((int64_t)n * C + c) * HW, HW, (int)threadIdx.x % LANES, red, true, 0.f, 0.f, in_eps,
                           in_gamma, in_beta, c, act, 0.f, in_mean + inst, in_invstd + inst);
}

// The backward register rows of the IBN kernels keep guarded pointer loads: on norm_row_bwd's buffer loads (three operands x 8 units
// in flight) ibn_train_bwd_fused_kernel<64, 8> needs 113 VGPRs instead of 89 and drops from 5 waves per SIMD to 4.
template <int LANES, int U>
__device__ __forceinline__ void ibn_row_bwd_reg(const float* __restrict__ x, const float* __restrict__ dy, const float* __restrict__ yact,
                                                float* __restrict__ dx, int64_t row, int HW, int t, float* red, int kind, float mu,
                                                float is, float a, float b, const float* __restrict__ gamma, int c, int act,
                                                float* __restrict__ s1_out, float* __restrict__ s2_out) {
    const float* xp = x + row;
    const float* gp = dy + row;
    const float* yp = act != RG_ACT_NONE ? yact + row : nullptr;
    float* dxp = dx + row;
    const float gs = (gamma ? gamma[c] : 1.f) * is;
    const int nv = HW >> 2;
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 g[U], v[U];
#pragma unroll
    for (int j = 0; j < U; ++j) {
        const int i = t + LANES * j;
        g[j] = i < nv ? reinterpret_cast<const float4*>(gp)[i] : zero;
        v[j] = i < nv ? reinterpret_cast<const float4*>(xp)[i] : make_float4(mu, mu, mu, mu);
        if (yp) {
            const float4 yv = i < nv ? reinterpret_cast<const float4*>(yp)[i] : zero;
            g[j].x *= act_grad_from_out(yv.x, act, 0.f); g[j].y *= act_grad_from_out(yv.y, act, 0.f);
            g[j].z *= act_grad_from_out(yv.z, act, 0.f); g[j].w *= act_grad_from_out(yv.w, act, 0.f);
        }
        v[j].x -= mu; v[j].y -= mu; v[j].z -= mu; v[j].w -= mu;
    }
    if (kind != IBN_ROW_BN_TRAIN) {                              // lanes past the row hold g = 0, x - mu = 0
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int j = 0; j < U; ++j) {
            s1 += (g[j].x + g[j].y) + (g[j].z + g[j].w);
            s2 += (g[j].x * v[j].x + g[j].y * v[j].y) + (g[j].z * v[j].z + g[j].w * v[j].w);
        }
        s1 = in_reduce<LANES>(s1, red);
        s2 = in_reduce<LANES>(s2, red) * is;
        if (t == 0) {
            *s1_out = s1;
            *s2_out = s2;
        }
        if (kind == IBN_ROW_IN) {
            a = s1 / (float)HW;
            b = s2 / (float)HW * is;
        }
    }
#pragma unroll
    for (int j = 0; j < U; ++j) {
        const int i = t + LANES * j;
        float4 o;
        o.x = gs * (g[j].x - a - v[j].x * b); o.y = gs * (g[j].y - a - v[j].y * b);
        o.z = gs * (g[j].z - a - v[j].z * b); o.w = gs * (g[j].w - a - v[j].w * b);
        if (i < nv) reinterpret_cast<float4*>(dxp)[i] = o;
    }
}

// U = 0: the shared loop row; U > 0: the register row above
template <int LANES, int U>
__device__ __forceinline__ void ibn_bwd_row(const float* __restrict__ x, const float* __restrict__ dy, const float* __restrict__ yact,
                                            float* __restrict__ dx, int64_t row, int HW, int t, float* red, int kind, float mu, float is,
                                            float a, float b, const float* __restrict__ gamma, int c, int act,
                                            float* __restrict__ s1_out, float* __restrict__ s2_out) {
    if constexpr (U > 0) ibn_row_bwd_reg<LANES, U>(x, dy, yact, dx, row, HW, t, red, kind, mu, is, a, b, gamma, c, act, s1_out, s2_out);
    else norm_row_bwd<LANES, 0>(x, dy, yact, dx, nullptr, 0u, row, HW, t, red, kind, mu, is, a, b, gamma, c, act, 0.f, s1_out, s2_out, nullptr);
}

// every row of the tensor.  Row sums go to row_s1 / row_s2 [N][W]: W = half in train mode (IN rows only; the BN rows take the channel
// sums bn_s1 / bn_s2 [C - half]), W = C in eval mode (BN rows write theirs too).
template <int LANES, int U>
__global__ __launch_bounds__(256) void ibn_bwd_rows_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                           const float* __restrict__ yact, const float* __restrict__ in_mean,
                                                           const float* __restrict__ in_invstd, const float* __restrict__ in_gamma,
                                                           const float* __restrict__ bn_mean, const float* __restrict__ bn_stat,
                                                           const float* __restrict__ bn_gamma, const float* __restrict__ bn_s1,
                                                           const float* __restrict__ bn_s2, float* __restrict__ dx,
                                                           float* __restrict__ row_s1, float* __restrict__ row_s2, int NC, int C,
                                                           int half, int HW, int train, float bn_eps, float inv_count, int act) {
    __shared__ float red[4];
    const int row = (int)blockIdx.x * (256 / LANES) + (int)threadIdx.x / LANES;
    if (row >= NC) return;
    const int n = row / C, c = row - n * C;
    const bool in_row = c < half;
    const int pc = in_row ? c : c - half;
    const int kind = in_row ? IBN_ROW_IN : train ? IBN_ROW_BN_TRAIN : IBN_ROW_BN_EVAL;
    const int so = n * (train ? half : C) + c;                   // the row's place in row_s1 / row_s2 (not for train-mode BN rows)
    float mu, is, a = 0.f, b = 0.f;
    if (in_row) {
        mu = in_mean[n * half + c];
        is = in_invstd[n * half + c];
    } else {
        mu = bn_mean[pc];
        is = train ? bn_stat[pc] : rsqrtf(bn_stat[pc] + bn_eps);
        if (train) {
            a = bn_s1[pc] * inv_count;
            b = bn_s2[pc] * inv_count * is;
        }
    }
    auto body = [&](int k) {                                     // one copy per kind: the register rows drop what a kind does not need
        ibn_bwd_row<LANES, U>(x, dy, yact, dx, (int64_t)row * HW, HW, (int)threadIdx.x % LANES, red, k, mu, is, a, b,
                              in_row ? in_gamma : bn_gamma, pc, act, row_s1 + so, row_s2 + so);
    };
    if (kind == IBN_ROW_IN) body(IBN_ROW_IN);
    else if (kind == IBN_ROW_BN_TRAIN) body(IBN_ROW_BN_TRAIN);
    else body(IBN_ROW_BN_EVAL);
}

template <int LANES, int U>
__global__ __launch_bounds__(256) void ibn_train_bwd_fused_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                                  const float* __restrict__ yact, const float* __restrict__ in_mean,
                                                                  const float* __restrict__ in_invstd, const float* __restrict__ in_gamma,
                                                                  const float* __restrict__ bn_mean, const float* __restrict__ bn_invstd,
                                                                  const float* __restrict__ bn_gamma, float* __restrict__ dx,
                                                                  float* __restrict__ row_s1, float* __restrict__ row_s2,
                                                                  float* __restrict__ bn_s1, float* __restrict__ bn_s2, int N, int C,
                                                                  int half, int HW, int act) {
    __shared__ float red[4];
    const int cb = C - half;
    if ((int)blockIdx.x < cb) {
        bn_channel_bwd(x, dy, yact, bn_mean, bn_invstd, bn_gamma, dx, nullptr, bn_s1, bn_s2, N, C, HW, act, 0.f,
                       half + (int)blockIdx.x, (int)blockIdx.x, red);
        return;
    }
    const int inst = ((int)blockIdx.x - cb) * (256 / LANES) + (int)threadIdx.x / LANES;
    if (inst >= N * half) return;
    const int n = inst / half, c = inst - n * half;
    ibn_bwd_row<LANES, U>(x, dy, yact, dx, ((int64_t)n * C + c) * HW, HW, (int)threadIdx.x % LANES, red, IBN_ROW_IN, in_mean[inst],
                          in_invstd[inst], 0.f, 0.f, in_gamma, c, act, row_s1 + inst, row_s2 + inst);
}

using IbnPairs = LUList<LU<16, 0>, LU<16, 2>, LU<32, 0>, LU<32, 2>, LU<64, 0>, LU<64, 2>, LU<64, 8>, LU<256, 0>, LU<256, 8>>;

static bool ibn_train_fused(int N, int HW) { return (int64_t)N * HW <= 16384; }

// float4 per lane of the register rows for this tensor (2 or 8), 0 = the loop rows
static int ibn_reg_units(int N, int C, int HW) {
    const int units = row_reg_units(HW, in_lanes(HW), (int64_t)N * C * HW);
    return units == 0 ? 0 : units <= 2 ? 2 : 8;
}

}  // namespace

// bytes of workspace for rg_ibn_fwd / rg_ibn_bwd: the slice partials of the BN half, then the row sums [2][N][C]
extern "C" int64_t rg_ibn_workspace(int N, int C, int HW, int half) {
    if (N <= 0 || C <= 0 || HW <= 0 || half <= 0 || half >= C) return 0;
    int L;
    const int S = pick_slices(N, C - half, HW, &L);
    return (int64_t)(((size_t)(C - half) * S * 3 + (size_t)2 * N * C) * sizeof(float));
}

extern "C" int rg_ibn_fwd(const float* x, const float* in_gamma, const float* in_beta, const float* bn_gamma, const float* bn_beta,
                          const float* residual, float* y, float* in_mean, float* in_invstd, float* bn_mean, float* bn_invstd,
                          float* running_mean, float* running_var, int N, int C, int HW, int half, int train, float in_eps,
                          float bn_eps, float momentum, int act, void* workspace, size_t workspace_bytes, hipStream_t stream) {
    RG_REQUIRE(x && y && in_mean && in_invstd && N > 0 && C > 0 && HW > 0, "rg_ibn_fwd: bad arguments");
    RG_REQUIRE(half > 0 && half < C, "rg_ibn_fwd: the split point %d must lie inside the %d channels", half, C);
    RG_REQUIRE(!residual, "rg_ibn_fwd: the layer has no residual input (bn1 of a Bottleneck never has one)");
    RG_REQUIRE(act == RG_ACT_NONE || act == RG_ACT_RELU, "rg_ibn_fwd: activation %d (none or ReLU)", act);
    RG_REQUIRE((int64_t)N * C < (1ll << 31) && (int64_t)N * HW < (1ll << 30), "rg_ibn_fwd: N*C or N*HW too large");
    RG_REQUIRE(train ? (bn_mean && bn_invstd) : (running_mean && running_var),
               train ? "rg_ibn_fwd: train mode writes the batch statistics" : "rg_ibn_fwd: eval mode needs the running statistics");
    const int NC = N * C, cb = C - half;
    const bool fused = train && ibn_train_fused(N, HW);
    rg::ProfScope prof(rg::FAM_NORM, stream, 0.0, 8.0 * (double)NC * HW);
    if (train && !fused) {
        int L;
        const int S = pick_slices(N, cb, HW, &L);
        if (!workspace || workspace_bytes < (size_t)cb * S * 3 * sizeof(float)) {
            rg::set_error("rg_ibn_fwd: workspace too small");
            return RG_ERR_WORKSPACE;
        }
        float* part = static_cast<float*>(workspace);
        // the BN half's statistics: the slice kernels over channels [half, C) — same sample stride C*HW, channel 0 of the view = half
        rg::bn_launch_stats(x + (int64_t)half * HW, part, N, cb, C, HW, S, L, bn_eps, momentum, bn_mean, bn_invstd, running_mean,
                            running_var, stream);
    }
    const int lanes = in_lanes(HW), units = ibn_reg_units(N, C, HW);
    const unsigned bytes = units ? (unsigned)((int64_t)NC * HW * 4) : 0u;
    if (!with_lanes_units(IbnPairs{}, lanes, units, [&](auto L, auto U) {
            if (fused)
                hipLaunchKernelGGL((ibn_train_fwd_fused_kernel<L, U>), dim3(cb + rg::cdiv(N * half, 256 / L)), dim3(256), 0, stream, x,
                                   in_gamma, in_beta, bn_gamma, bn_beta, y, in_mean, in_invstd, bn_mean, bn_invstd, running_mean,
                                   running_var, N, C, half, HW, in_eps, bn_eps, momentum, act, bytes);
            else
                hipLaunchKernelGGL((ibn_fwd_rows_kernel<L, U>), dim3(rg::cdiv(NC, 256 / L)), dim3(256), 0, stream, x, in_gamma, in_beta,
                                   bn_gamma, bn_beta, train ? bn_mean : running_mean, train ? bn_invstd : running_var, y, in_mean,
                                   in_invstd, NC, C, half, HW, train ? 0 : 1, in_eps, bn_eps, act, bytes);
        })) {
        rg::set_error("rg_ibn_fwd: no kernel for %d lanes x %d units", lanes, units);
        return RG_ERR_INVALID;
    }
    return rg::check_launch("rg_ibn_fwd");
}

// dx and the four affine gradients.  bn_mean / bn_stat: the saved batch mean / invstd (train) or the running mean / variance (eval).
extern "C" int rg_ibn_bwd(const float* x, const float* dy, const float* y_act, const float* in_mean, const float* in_invstd,
                          const float* bn_mean, const float* bn_stat, const float* in_gamma, const float* bn_gamma, float* dx,
                          float* d_in_gamma, float* d_in_beta, float* d_bn_gamma, float* d_bn_beta, int N, int C, int HW, int half,
                          int train, float bn_eps, int act, void* workspace, size_t workspace_bytes, hipStream_t stream) {
    RG_REQUIRE(x && dy && in_mean && in_invstd && bn_mean && bn_stat && dx && N > 0 && C > 0 && HW > 0, "rg_ibn_bwd: bad arguments");
    RG_REQUIRE(d_in_gamma && d_in_beta && d_bn_gamma && d_bn_beta, "rg_ibn_bwd: the four affine gradients are outputs");
    RG_REQUIRE(half > 0 && half < C, "rg_ibn_bwd: the split point %d must lie inside the %d channels", half, C);
    RG_REQUIRE(act == RG_ACT_NONE || act == RG_ACT_RELU, "rg_ibn_bwd: activation %d (none or ReLU)", act);
    RG_REQUIRE(act == RG_ACT_NONE || y_act, "rg_ibn_bwd: fused activation needs the forward output");
    RG_REQUIRE((int64_t)N * C < (1ll << 31) && (int64_t)N * HW < (1ll << 30), "rg_ibn_bwd: N*C or N*HW too large");
    const int NC = N * C, cb = C - half;
    const bool fused = train && ibn_train_fused(N, HW);
    int L;
    const int S = pick_slices(N, cb, HW, &L);
    const size_t part_floats = (size_t)cb * S * 3;
    if (!workspace || workspace_bytes < (part_floats + (size_t)2 * NC) * sizeof(float)) {
        rg::set_error("rg_ibn_bwd: workspace too small");
        return RG_ERR_WORKSPACE;
    }
    float* part = static_cast<float*>(workspace);
    float* row_s1 = part + part_floats;
    float* row_s2 = row_s1 + NC;
    rg::ProfScope prof(rg::FAM_NORM, stream, 0.0, (act ? 16.0 : 12.0) * (double)NC * HW);
    if (train && !fused) {                                       // the BN half's channel sums ARE d_bn_beta / d_bn_gamma
        const int64_t off = (int64_t)half * HW;
        rg::bn_launch_bwd_reduce(x + off, dy + off, y_act ? y_act + off : nullptr, bn_mean, bn_stat, part, N, cb, C, HW, S, L, 0, bn_eps,
                                 act, 0.f, d_bn_beta, d_bn_gamma, stream);
    }
    const int lanes = in_lanes(HW), units = ibn_reg_units(N, C, HW);
    if (!with_lanes_units(IbnPairs{}, lanes, units, [&](auto L_, auto U) {
            if (fused)
                hipLaunchKernelGGL((ibn_train_bwd_fused_kernel<L_, U>), dim3(cb + rg::cdiv(N * half, 256 / L_)), dim3(256), 0, stream, x,
                                   dy, y_act, in_mean, in_invstd, in_gamma, bn_mean, bn_stat, bn_gamma, dx, row_s1, row_s2, d_bn_beta,
                                   d_bn_gamma, N, C, half, HW, act);
            else
                hipLaunchKernelGGL((ibn_bwd_rows_kernel<L_, U>), dim3(rg::cdiv(NC, 256 / L_)), dim3(256), 0, stream, x, dy, y_act, in_mean,
                                   in_invstd, in_gamma, bn_mean, bn_stat, bn_gamma, train ? d_bn_beta : nullptr,
                                   train ? d_bn_gamma : nullptr, dx, row_s1, row_s2, NC, C, half, HW, train ? 1 : 0, bn_eps,
                                   train ? 1.f / (float)((int64_t)N * HW) : 0.f, act);
        })) {
        rg::set_error("rg_ibn_bwd: no kernel for %d lanes x %d units", lanes, units);
        return RG_ERR_INVALID;
    }
    // the row sums over n: the IN gradients in train mode (row sums [N][half]), all four in eval mode ([N][C], split at half)
    if (train)
        rg::launch_rows_sum_pair(row_s1, row_s2, d_in_beta, d_in_gamma, N, half, half, nullptr, nullptr, stream);
    else
        rg::launch_rows_sum_pair(row_s1, row_s2, d_in_beta, d_in_gamma, N, C, half, d_bn_beta, d_bn_gamma, stream);
    return rg::check_launch("rg_ibn_bwd");
}
