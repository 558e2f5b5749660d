// Fused [B][D] tail of the multi-part encoder (CC/clustercontrast/models/resnet_mp.py:118-143):
//   z_j  = BatchNorm1d_j(x_j)            j = g, p1, p2: three independent layers
//   z_gc = z_g + z_p1 + z_p2 (fusion 1, 'sum') or z_g (fusion 0)
//   f_k  = z_k / max(|z_k|_2, 1e-12)     k = g, p1, p2, gc: F.normalize over the row
// Saved for the backward: xhat_j (the normalised activations), the batch mean / invstd and the four row norms; z and f are
// recomputed from xhat, so nothing else is kept.
//
// Two work shapes.  COLUMN phase: a workgroup owns kCG = 16 adjacent channels over all B rows as 16 row slices of 16 lanes: lane
// group `slice` takes the rows b = slice, slice + 16, ... (16 adjacent lanes read 64 contiguous bytes of a row); per-channel sums
// over the rows are added across the slices through LDS in a fixed order, per-row sums over the group's channels are a 16-lane
// butterfly.  D = 2048 gives 128 workgroups of 16 serial rows at B = 256 (64 channels x 4 slices left 32 workgroups of 64 serial
// rows: 3 x slower, latency bound).  ROW phase: a workgroup owns one row.
//   forward, train   column phase (two-pass, shift-corrected batch statistics, running statistics, xhat, per (k, channel group, row) partial sums
//                    of z^2 into the workspace), then row phase (adds the partials of a row in group order, norms, scales): 2 launches
//   forward, eval    everything is row-local: 1 launch
//   backward         row phase (F.normalize backward of the four outputs, added per branch), then column phase (BatchNorm
//                    backward, gamma / beta gradients): 2 launches
// No atomics, every sum has a fixed order: results are bit-reproducible.
#include "rg_common.h"

namespace {

constexpr int kCG = 16;             // channels per workgroup of the column phase
constexpr int kRS = 256 / kCG;      // row slices per workgroup
constexpr float kNormEps = 1e-12f;  // F.normalize's eps

struct HeadAffine {
    const float* gamma[3];
    const float* beta[3];
};

struct HeadFwd {
    const float* x[3];
    float* rm[3];
    float* rv[3];
    float eps[3];
    float mom[3];
};

struct HeadGrad {
    const float* dy[4];  // g, p1, p2, gc; NULL = no upstream gradient
    const float* dz[3];  // gradient arriving at z_j itself (the 'cat' fusion reads the BatchNorm outputs); NULL = none
    float* dx[3];        // NULL = the branch receives no gradient and is skipped
    float* dgamma[3];
    float* dbeta[3];
};

__device__ __forceinline__ float head_z(float gamma, float xhat, float beta) { return fmaf(gamma, xhat, beta); }

__device__ __forceinline__ float head_gc(float zg, float zp1, float zp2, int fusion) { return fusion ? (zg + zp1) + zp2 : zg; }

// sum over the kRS row slices of a per-channel value, the same order for every thread
__device__ __forceinline__ float head_cross_slices(float v, float (*red)[kCG], int slice, int lane) {
    __syncthreads();
    red[slice][lane] = v;
    __syncthreads();
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < kRS; ++i) s += red[i][lane];
    return s;
}

// sum over the kCG lanes of a slice (they are adjacent lanes of one slice and run the same trips)
__device__ __forceinline__ float head_group_sum(float v) {
#pragma unroll
    for (int off = kCG / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

__global__ __launch_bounds__(256) void mp_head_col_fwd_kernel(HeadFwd in, HeadAffine af, float* __restrict__ xhat,
                                                              float* __restrict__ mean_out, float* __restrict__ invstd_out,
                                                              float* __restrict__ part, int B, int D, int fusion) {
    __shared__ float red[kRS][kCG];
    const int lane = threadIdx.x % kCG, slice = threadIdx.x / kCG;              // channel of the group, row slice
    const int c = blockIdx.x * kCG + lane, G = gridDim.x;
    const bool ok = c < D;
    const int64_t BD = (int64_t)B * D;
    float mean[3], inv[3], ga[3], be[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const float* x = in.x[j];
        float s = 0.f;
        if (ok)
            for (int b = slice; b < B; b += kRS) s += x[(int64_t)b * D + c];
        mean[j] = head_cross_slices(s, red, slice, lane) / (float)B;
        // second pass around the ROUNDED mean: sum(d) / B is what the rounding took from the mean, and var = mean(d^2) - mean(d)^2
        // holds for any shift, so that rounding (u |mean|, which a channel with a small spread around a large mean feels) drops out
        s = 0.f;
        float sd = 0.f;
        if (ok)
            for (int b = slice; b < B; b += kRS) {
                const float d = x[(int64_t)b * D + c] - mean[j];
                sd += d;
                s = fmaf(d, d, s);
            }
        const float md = head_cross_slices(sd, red, slice, lane) / (float)B;
        const float var = fmaxf(head_cross_slices(s, red, slice, lane) / (float)B - md * md, 0.f);      // biased
        inv[j] = rsqrtf(var + in.eps[j]);
        ga[j] = ok ? af.gamma[j][c] : 0.f;
        be[j] = ok ? af.beta[j][c] : 0.f;
        if (ok && slice == 0) {
            mean_out[j * D + c] = mean[j];
            invstd_out[j * D + c] = inv[j];
            const float m = in.mom[j];
            in.rm[j][c] = (1.f - m) * in.rm[j][c] + m * mean[j];
            in.rv[j][c] = (1.f - m) * in.rv[j][c] + m * (var * ((float)B / (float)(B - 1)));
        }
    }
    for (int b = slice; b < B; b += kRS) {                                        // the same trips for the 16 lanes of a slice
        float z[4];
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            float xh = 0.f;
            if (ok) {
                xh = (in.x[j][(int64_t)b * D + c] - mean[j]) * inv[j];
                xhat[j * BD + (int64_t)b * D + c] = xh;
            }
            z[j] = ok ? head_z(ga[j], xh, be[j]) : 0.f;
        }
        z[3] = head_gc(z[0], z[1], z[2], fusion);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float q = head_group_sum(z[k] * z[k]);
            if (lane == 0) part[((int64_t)k * G + blockIdx.x) * B + b] = q;
        }
    }
}

// writes the four outputs of row b from xhat and the four norms
__device__ __forceinline__ void head_scale_row(const float* xhat, const HeadAffine& af, float* out,
                                               const float* inv, int b, int B, int D, int fusion) {
    const int64_t BD = (int64_t)B * D, row = (int64_t)b * D;
    for (int c = threadIdx.x; c < D; c += 256) {
        float z[4];
#pragma unroll
        for (int j = 0; j < 3; ++j) z[j] = head_z(af.gamma[j][c], xhat[j * BD + row + c], af.beta[j][c]);
        z[3] = head_gc(z[0], z[1], z[2], fusion);
#pragma unroll
        for (int k = 0; k < 4; ++k) out[k * BD + row + c] = z[k] * inv[k];
    }
}

__global__ __launch_bounds__(256) void mp_head_row_fwd_kernel(const float* __restrict__ xhat, HeadAffine af,
                                                              const float* __restrict__ part, float* __restrict__ out,
                                                              float* __restrict__ norms, int B, int D, int G, int fusion) {
    __shared__ float red[16];
    const int b = blockIdx.x;
    float inv[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        float s = 0.f;
        for (int g = threadIdx.x; g < G; g += 256) s += part[((int64_t)k * G + g) * B + b];
        const float nr = sqrtf(rg_block_sum(s, red));                            // a fixed order: the same bits every run
        inv[k] = 1.f / fmaxf(nr, kNormEps);
        if (threadIdx.x == 0) norms[k * B + b] = nr;
    }
    head_scale_row(xhat, af, out, inv, b, B, D, fusion);
}

__global__ __launch_bounds__(256) void mp_head_eval_fwd_kernel(HeadFwd in, HeadAffine af, float* xhat,
                                                               float* __restrict__ mean_out, float* __restrict__ invstd_out,
                                                               float* __restrict__ out, float* __restrict__ norms, int B, int D,
                                                               int fusion) {
    __shared__ float red[16];
    const int b = blockIdx.x;
    const int64_t BD = (int64_t)B * D, row = (int64_t)b * D;
    float q[4] = {0.f, 0.f, 0.f, 0.f};
    for (int c = threadIdx.x; c < D; c += 256) {
        float z[4];
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const float m = in.rm[j][c], iv = rsqrtf(in.rv[j][c] + in.eps[j]);
            const float xh = (in.x[j][row + c] - m) * iv;
            xhat[j * BD + row + c] = xh;                                         // read back below by this same thread
            if (b == 0) mean_out[j * D + c] = m, invstd_out[j * D + c] = iv;
            z[j] = head_z(af.gamma[j][c], xh, af.beta[j][c]);
        }
        z[3] = head_gc(z[0], z[1], z[2], fusion);
#pragma unroll
        for (int k = 0; k < 4; ++k) q[k] = fmaf(z[k], z[k], q[k]);
    }
    float inv[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float nr = sqrtf(rg_block_sum(q[k], red));
        inv[k] = 1.f / fmaxf(nr, kNormEps);
        if (threadIdx.x == 0) norms[k * B + b] = nr;
    }
    head_scale_row(xhat, af, out, inv, b, B, D, fusion);
}

// F.normalize backward of the four outputs of row b, dz_k = (dy_k - f_k <dy_k, f_k>) / max(norm_k, eps) (the inner product is
// dropped below the clamp, as rg_l2norm_rows_bwd), added per branch: dzt_g = dz_g + dz_gc, dzt_p = dz_p + [fusion] dz_gc, plus the
// gradient given for z_j itself.
// dzt_j is written into dx_j, which the column phase then rewrites in place.
__global__ __launch_bounds__(256) void mp_head_row_bwd_kernel(HeadGrad gr, const float* __restrict__ xhat, HeadAffine af,
                                                              const float* __restrict__ norms, int B, int D, int fusion) {
    __shared__ float red[16];
    const int b = blockIdx.x;
    const int64_t BD = (int64_t)B * D, row = (int64_t)b * D;
    float nr[4], inv[4], dot[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        nr[k] = norms[k * B + b];
        inv[k] = 1.f / fmaxf(nr[k], kNormEps);
    }
    for (int c = threadIdx.x; c < D; c += 256) {
        float z[4];
#pragma unroll
        for (int j = 0; j < 3; ++j) z[j] = head_z(af.gamma[j][c], xhat[j * BD + row + c], af.beta[j][c]);
        z[3] = head_gc(z[0], z[1], z[2], fusion);
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (gr.dy[k]) dot[k] = fmaf(gr.dy[k][row + c], z[k] * inv[k], dot[k]);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        dot[k] = gr.dy[k] ? rg_block_sum(dot[k], red) : 0.f;                     // gr.dy[k] is uniform over the grid
        if (!(nr[k] >= kNormEps)) dot[k] = 0.f;
    }
    for (int c = threadIdx.x; c < D; c += 256) {
        float z[4], dz[4];
#pragma unroll
        for (int j = 0; j < 3; ++j) z[j] = head_z(af.gamma[j][c], xhat[j * BD + row + c], af.beta[j][c]);
        z[3] = head_gc(z[0], z[1], z[2], fusion);
#pragma unroll
        for (int k = 0; k < 4; ++k) dz[k] = gr.dy[k] ? (gr.dy[k][row + c] - (z[k] * inv[k]) * dot[k]) * inv[k] : 0.f;
        dz[0] += dz[3];
        if (fusion) dz[1] += dz[3], dz[2] += dz[3];
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            if (gr.dz[j]) dz[j] += gr.dz[j][row + c];
            if (gr.dx[j]) gr.dx[j][row + c] = dz[j];
        }
    }
}

// BatchNorm backward per branch from dzt (in dx): dgamma = sum_b dzt xhat, dbeta = sum_b dzt,
// train: dx = gamma invstd (dzt - dbeta / B - xhat dgamma / B); eval (running statistics): dx = gamma invstd dzt
__global__ __launch_bounds__(256) void mp_head_col_bwd_kernel(HeadGrad gr, const float* __restrict__ xhat,
                                                              const float* __restrict__ invstd, HeadAffine af, int B, int D,
                                                              int train) {
    __shared__ float red[kRS][kCG];
    const int lane = threadIdx.x % kCG, slice = threadIdx.x / kCG;              // channel of the group, row slice
    const int c = blockIdx.x * kCG + lane;
    const bool ok = c < D;
    const int64_t BD = (int64_t)B * D;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        float* dx = gr.dx[j];
        if (!dx) continue;                                                       // uniform over the grid
        const float* xh = xhat + j * BD;
        float s1 = 0.f, s2 = 0.f;
        if (ok)
            for (int b = slice; b < B; b += kRS) {
                const float g = dx[(int64_t)b * D + c];
                s1 += g;
                s2 = fmaf(g, xh[(int64_t)b * D + c], s2);
            }
        s1 = head_cross_slices(s1, red, slice, lane);
        s2 = head_cross_slices(s2, red, slice, lane);
        if (!ok) continue;
        if (slice == 0) {
            if (gr.dgamma[j]) gr.dgamma[j][c] = s2;
            if (gr.dbeta[j]) gr.dbeta[j][c] = s1;
        }
        const float k = af.gamma[j][c] * invstd[j * D + c];
        const float m1 = train ? s1 / (float)B : 0.f, m2 = train ? s2 / (float)B : 0.f;
        for (int b = slice; b < B; b += kRS) {
            const int64_t i = (int64_t)b * D + c;
            dx[i] = k * ((dx[i] - m1) - xh[i] * m2);
        }
    }
}

}  // namespace

extern "C" int64_t rg_mp_head_workspace(int B, int D) {
    if (B <= 0 || D <= 0) return 0;
    return (int64_t)4 * rg::cdiv(D, kCG) * B * (int64_t)sizeof(float);
}

extern "C" int rg_mp_head_fwd(const float* x_g, const float* x_p1, const float* x_p2, const float* gamma_g,
                              const float* gamma_p1, const float* gamma_p2, const float* beta_g, const float* beta_p1,
                              const float* beta_p2, float* rm_g, float* rm_p1, float* rm_p2, float* rv_g, float* rv_p1,
                              float* rv_p2, float* out, float* xhat, float* mean, float* invstd, float* norms, int B, int D,
                              int train, int fusion, float eps_g, float eps_p1, float eps_p2, float mom_g, float mom_p1,
                              float mom_p2, void* workspace, size_t workspace_bytes, hipStream_t stream) {
    RG_REQUIRE(x_g && x_p1 && x_p2 && gamma_g && gamma_p1 && gamma_p2 && beta_g && beta_p1 && beta_p2 && rm_g && rm_p1 && rm_p2 &&
                   rv_g && rv_p1 && rv_p2 && out && xhat && mean && invstd && norms && B > 0 && D > 0,
               "rg_mp_head_fwd: bad arguments");
    RG_REQUIRE(fusion == 0 || fusion == 1, "rg_mp_head_fwd: fusion is 0 (f_gc from the global branch) or 1 (sum), got %d", fusion);
    RG_REQUIRE(!train || B >= 2, "rg_mp_head_fwd: batch statistics need more than 1 row");
    RG_REQUIRE(B <= 65535 * 32 && (int64_t)B * D < (1ll << 31), "rg_mp_head_fwd: extents too large");
    HeadFwd in = {{x_g, x_p1, x_p2}, {rm_g, rm_p1, rm_p2}, {rv_g, rv_p1, rv_p2}, {eps_g, eps_p1, eps_p2}, {mom_g, mom_p1, mom_p2}};
    HeadAffine af = {{gamma_g, gamma_p1, gamma_p2}, {beta_g, beta_p1, beta_p2}};
    const int G = rg::cdiv(D, kCG);
    rg::ProfScope prof(rg::FAM_NORM, stream, 0.0, 4.0 * B * (double)D * (train ? 13.0 : 10.0));
    if (!train) {
        hipLaunchKernelGGL(mp_head_eval_fwd_kernel, dim3(B), dim3(256), 0, stream, in, af, xhat, mean, invstd, out, norms, B, D,
                           fusion);
        return rg::check_launch("rg_mp_head_fwd");
    }
    if (!workspace || workspace_bytes < (size_t)rg_mp_head_workspace(B, D)) {
        rg::set_error("rg_mp_head_fwd: workspace too small");
        return RG_ERR_WORKSPACE;
    }
    float* part = static_cast<float*>(workspace);
    hipLaunchKernelGGL(mp_head_col_fwd_kernel, dim3(G), dim3(256), 0, stream, in, af, xhat, mean, invstd, part, B, D, fusion);
    hipLaunchKernelGGL(mp_head_row_fwd_kernel, dim3(B), dim3(256), 0, stream, xhat, af, part, out, norms, B, D, G, fusion);
    return rg::check_launch("rg_mp_head_fwd");
}

extern "C" int rg_mp_head_bwd(const float* dy_g, const float* dy_p1, const float* dy_p2, const float* dy_gc, const float* dz_g,
                              const float* dz_p1, const float* dz_p2, const float* xhat, const float* invstd, const float* norms, const float* gamma_g, const float* gamma_p1,
                              const float* gamma_p2, const float* beta_g, const float* beta_p1, const float* beta_p2, float* dx_g,
                              float* dx_p1, float* dx_p2, float* dgamma_g, float* dgamma_p1, float* dgamma_p2, float* dbeta_g,
                              float* dbeta_p1, float* dbeta_p2, int B, int D, int train, int fusion, hipStream_t stream) {
    RG_REQUIRE(xhat && invstd && norms && gamma_g && gamma_p1 && gamma_p2 && beta_g && beta_p1 && beta_p2 && B > 0 && D > 0,
               "rg_mp_head_bwd: bad arguments");
    RG_REQUIRE(fusion == 0 || fusion == 1, "rg_mp_head_bwd: fusion is 0 (f_gc from the global branch) or 1 (sum), got %d", fusion);
    RG_REQUIRE(dy_g || dy_p1 || dy_p2 || dy_gc || dz_g || dz_p1 || dz_p2, "rg_mp_head_bwd: no upstream gradient");
    // a branch is skipped (dx NULL) only when no given gradient reaches it
    RG_REQUIRE(dx_g || !(dy_g || dy_gc || dz_g), "rg_mp_head_bwd: dx_g is needed");
    RG_REQUIRE(dx_p1 || !(dy_p1 || dz_p1 || (fusion && dy_gc)), "rg_mp_head_bwd: dx_p1 is needed");
    RG_REQUIRE(dx_p2 || !(dy_p2 || dz_p2 || (fusion && dy_gc)), "rg_mp_head_bwd: dx_p2 is needed");
    RG_REQUIRE((dx_g || !(dgamma_g || dbeta_g)) && (dx_p1 || !(dgamma_p1 || dbeta_p1)) && (dx_p2 || !(dgamma_p2 || dbeta_p2)),
               "rg_mp_head_bwd: affine gradients of a branch without dx");
    RG_REQUIRE(B <= 65535 * 32 && (int64_t)B * D < (1ll << 31), "rg_mp_head_bwd: extents too large");
    HeadGrad gr = {{dy_g, dy_p1, dy_p2, dy_gc}, {dz_g, dz_p1, dz_p2}, {dx_g, dx_p1, dx_p2}, {dgamma_g, dgamma_p1, dgamma_p2}, {dbeta_g, dbeta_p1, dbeta_p2}};
    HeadAffine af = {{gamma_g, gamma_p1, gamma_p2}, {beta_g, beta_p1, beta_p2}};
    rg::ProfScope prof(rg::FAM_NORM, stream, 0.0, 4.0 * B * (double)D * 16.0);
    hipLaunchKernelGGL(mp_head_row_bwd_kernel, dim3(B), dim3(256), 0, stream, gr, xhat, af, norms, B, D, fusion);
    hipLaunchKernelGGL(mp_head_col_bwd_kernel, dim3(rg::cdiv(D, kCG)), dim3(256), 0, stream, gr, xhat, invstd, af, B, D, train);
    return rg::check_launch("rg_mp_head_bwd");
}
