// Fused verification head of FD-GAN stage I (FD/reid/models/embedding.py:7-39 with use_batch_norm and use_classifier, under
// nn.CrossEntropyLoss() and FD/reid/evaluation_metrics/classification.py):
//   d      = (x1 - x2)^2                                  [B][D]
//   z      = gamma * (d - mean) * invstd + beta           BatchNorm1d: batch statistics in train mode, running statistics in eval
//   logits = z W^T + bias                                 [B][C], W is [C][D], 1 <= C <= 16
//   loss_b = logsumexp(logits_b) - logits_b[label_b], loss = mean_b loss_b, correct = #{b : argmax_c logits_b == label_b}
// Ties of the argmax go to the lowest class index.  A label outside [0, C) gives its row loss 0 and gradient 0 (the rule of
// rg_softmax_ce_fwd); the mean still divides by B.
// Saved for the backward: xhat (the normalised d), mean / invstd and dlogits = (softmax - onehot) / B.  d, z and dz are never
// stored: z is recomputed from xhat, d from x1 and x2.
//
// COLUMN phase, the work shape of part_head.hip: a workgroup owns kCG = 16 adjacent channels over all B rows as 16 row slices of 16
// lanes; per-channel sums over the rows cross the slices through LDS in a fixed order, per-row sums over the group's channels are
// a 16-lane butterfly.
//   forward, train   column phase (two-pass shift-corrected batch statistics, running statistics, xhat, per (channel group, row,
//                    class) partial sums of W[c][ch] z[b][ch] into the workspace), then ONE workgroup adds each row's partials in
//                    group order, adds the bias and computes the cross entropy, its mean and the correct count: 2 launches
//   forward, eval    row-local, a workgroup per row: 1 launch, no workspace; with labels the finishing workgroup follows (the mean
//                    and the count need every row)
//   backward         everything is column-local: 1 launch
// No atomics, every sum has a fixed order: results are bit-reproducible.
#include "rg_common.h"

namespace {

constexpr int kCG = 16;             // channels per workgroup of the column phase
constexpr int kRS = 256 / kCG;      // row slices per workgroup
constexpr int kMaxC = 16;           // classes

// sum over the kRS row slices of a per-channel value, the same order for every thread
__device__ __forceinline__ float vh_cross_slices(float v, float (*red)[kCG], int slice, int lane) {
    __syncthreads();
    red[slice][lane] = v;
    __syncthreads();
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < kRS; ++i) s += red[i][lane];
    return s;
}

// sum over the kCG lanes of a slice (they are adjacent lanes of one slice and run the same trips)
__device__ __forceinline__ float vh_group_sum(float v) {
#pragma unroll
    for (int off = kCG / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

__device__ __forceinline__ float vh_sq(float a, float b) {
    const float t = a - b;
    return t * t;
}

__global__ __launch_bounds__(256) void verif_head_col_fwd_kernel(const float* __restrict__ x1, const float* __restrict__ x2,
                                                                 const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                 float* __restrict__ rm, float* __restrict__ rv,
                                                                 const float* __restrict__ W, float* __restrict__ xhat,
                                                                 float* __restrict__ mean_out, float* __restrict__ invstd_out,
                                                                 float* __restrict__ part, int B, int D, int C, float eps,
                                                                 float mom) {
    __shared__ float red[kRS][kCG];
    const int lane = threadIdx.x % kCG, slice = threadIdx.x / kCG;              // channel of the group, row slice
    const int c = blockIdx.x * kCG + lane;
    const bool ok = c < D;
    float s = 0.f;
    if (ok)
        for (int b = slice; b < B; b += kRS) s += vh_sq(x1[(int64_t)b * D + c], x2[(int64_t)b * D + c]);
    const float mean = vh_cross_slices(s, red, slice, lane) / (float)B;
    // second pass around the ROUNDED mean: var = mean(e^2) - mean(e)^2 holds for any shift, so the rounding of the mean drops out
    s = 0.f;
    float se = 0.f;
    if (ok)
        for (int b = slice; b < B; b += kRS) {
            const float e = vh_sq(x1[(int64_t)b * D + c], x2[(int64_t)b * D + c]) - mean;
            se += e;
            s = fmaf(e, e, s);
        }
    const float me = vh_cross_slices(se, red, slice, lane) / (float)B;
    const float var = fmaxf(vh_cross_slices(s, red, slice, lane) / (float)B - me * me, 0.f);            // biased
    const float inv = rsqrtf(var + eps);
    const float ga = ok ? gamma[c] : 0.f, be = ok ? beta[c] : 0.f;
    if (ok && slice == 0) {
        mean_out[c] = mean;
        invstd_out[c] = inv;
        rm[c] = (1.f - mom) * rm[c] + mom * mean;
        rv[c] = (1.f - mom) * rv[c] + mom * (var * ((float)B / (float)(B - 1)));
    }
    float w[kMaxC];
#pragma unroll
    for (int k = 0; k < kMaxC; ++k) w[k] = (ok && k < C) ? W[(int64_t)k * D + c] : 0.f;
    for (int b = slice; b < B; b += kRS) {                                        // the same trips for the 16 lanes of a slice
        float z = 0.f;
        if (ok) {
            const float xh = (vh_sq(x1[(int64_t)b * D + c], x2[(int64_t)b * D + c]) - mean) * inv;
            xhat[(int64_t)b * D + c] = xh;
            z = fmaf(ga, xh, be);
        }
        float mine = 0.f;
#pragma unroll
        for (int k = 0; k < kMaxC; ++k)
            if (k < C) {                                                          // uniform over the grid
                const float q = vh_group_sum(w[k] * z);
                if (lane == k) mine = q;
            }
        if (lane < C) part[((int64_t)blockIdx.x * B + b) * C + lane] = mine;      // lane k carries class k: one contiguous store
    }
}

// eval mode: a workgroup per row, running statistics
__global__ __launch_bounds__(256) void verif_head_eval_fwd_kernel(const float* __restrict__ x1, const float* __restrict__ x2,
                                                                  const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                  const float* __restrict__ rm, const float* __restrict__ rv,
                                                                  const float* __restrict__ W, const float* __restrict__ bias,
                                                                  float* __restrict__ xhat, float* __restrict__ mean_out,
                                                                  float* __restrict__ invstd_out, float* __restrict__ logits,
                                                                  int D, int C, float eps) {
    __shared__ float red[16];
    const int b = blockIdx.x;
    const int64_t row = (int64_t)b * D;
    float acc[kMaxC];
#pragma unroll
    for (int k = 0; k < kMaxC; ++k) acc[k] = 0.f;
    for (int c = threadIdx.x; c < D; c += 256) {
        const float m = rm[c], iv = rsqrtf(rv[c] + eps);
        const float xh = (vh_sq(x1[row + c], x2[row + c]) - m) * iv;
        xhat[row + c] = xh;
        if (b == 0) mean_out[c] = m, invstd_out[c] = iv;
        const float z = fmaf(gamma[c], xh, beta[c]);
#pragma unroll
        for (int k = 0; k < kMaxC; ++k)
            if (k < C) acc[k] = fmaf(W[(int64_t)k * D + c], z, acc[k]);
    }
#pragma unroll
    for (int k = 0; k < kMaxC; ++k)
        if (k < C) {                                                              // uniform over the grid
            const float s = rg_block_sum(acc[k], red);
            if (threadIdx.x == 0) logits[(int64_t)b * C + k] = s + (bias ? bias[k] : 0.f);
        }
}

// ONE workgroup.  part != NULL: logits[b][c] = sum over the G channel groups, in group order, + bias[c]; part NULL: logits are
// there already.  labels != NULL: per-row cross entropy, dlogits = (softmax - onehot) / B, out2 = {mean loss, correct / B}.
__global__ __launch_bounds__(256) void verif_head_row_kernel(const float* __restrict__ part, const float* __restrict__ bias,
                                                             const int64_t* __restrict__ labels, float* logits,
                                                             float* __restrict__ loss_rows, float* __restrict__ out2,
                                                             float* __restrict__ dlogits, int B, int C, int G) {
    __shared__ float red[16];
    const int64_t BC = (int64_t)B * C;
    if (part) {
        for (int64_t i = threadIdx.x; i < BC; i += 256) {
            float s = 0.f;
            for (int g = 0; g < G; ++g) s += part[(int64_t)g * BC + i];
            logits[i] = s + (bias ? bias[i % C] : 0.f);
        }
        __syncthreads();                                                          // the rows below read what other threads wrote
    }
    if (!labels) return;
    float lsum = 0.f, hits = 0.f;
    const float invB = 1.f / (float)B;
    for (int b = threadIdx.x; b < B; b += 256) {
        const float* lr = logits + (int64_t)b * C;
        float l[kMaxC];
        float mx = lr[0];
        int arg = 0;
#pragma unroll
        for (int k = 0; k < kMaxC; ++k) {
            l[k] = k < C ? lr[k] : -INFINITY;
            if (l[k] > mx) mx = l[k], arg = k;                                    // strict: a tie stays with the lowest index
        }
        float se = 0.f;
#pragma unroll
        for (int k = 0; k < kMaxC; ++k)
            if (k < C) se += expf(l[k] - mx);
        const float lse = mx + logf(se);
        const int64_t y = labels[b];
        const bool valid = y >= 0 && y < C;
        float ly = 0.f;
#pragma unroll
        for (int k = 0; k < kMaxC; ++k)
            if (k < C) {
                float p = expf(l[k] - lse);
                if (k == y) p -= 1.f, ly = l[k];
                dlogits[(int64_t)b * C + k] = valid ? p * invB : 0.f;
            }
        const float lb = valid ? lse - ly : 0.f;
        loss_rows[b] = lb;
        lsum += lb;
        hits += (valid && arg == (int)y) ? 1.f : 0.f;
    }
    lsum = rg_block_sum(lsum, red);
    hits = rg_block_sum(hits, red);                                               // whole numbers below 2^24: exact
    if (threadIdx.x == 0) {
        out2[0] = lsum * invB;
        out2[1] = hits * invB;
    }
}

// dl[b][k] = grad_loss * dlogits[b][k] + dlogits_up[b][k]; per channel: dz = dl W, dW[k] = sum_b dl[b][k] z[b], BatchNorm backward
// (train: dd = gamma invstd (dz - mean(dz) - xhat mean(dz xhat)); eval: dd = gamma invstd dz), dx1 = 2 (x1 - x2) dd, dx2 = -dx1.
// Workgroup 0 also writes dbias[k] = sum_b dl[b][k].
__global__ __launch_bounds__(256) void verif_head_col_bwd_kernel(const float* __restrict__ grad_loss, const float* __restrict__ dlogits,
                                                                 const float* __restrict__ dlogits_up, const float* __restrict__ x1,
                                                                 const float* __restrict__ x2, const float* __restrict__ xhat,
                                                                 const float* __restrict__ invstd, const float* __restrict__ gamma,
                                                                 const float* __restrict__ beta, const float* __restrict__ W,
                                                                 float* __restrict__ dx1, float* __restrict__ dx2,
                                                                 float* __restrict__ dW, float* __restrict__ dbias,
                                                                 float* __restrict__ dgamma, float* __restrict__ dbeta, int B, int D,
                                                                 int C, int train) {
    __shared__ float red[kRS][kCG];
    const int lane = threadIdx.x % kCG, slice = threadIdx.x / kCG;              // channel of the group, row slice
    const int c = blockIdx.x * kCG + lane;
    const bool ok = c < D;
    const float gl = dlogits ? (grad_loss ? grad_loss[0] : 1.f) : 0.f;
    const float ga = ok ? gamma[c] : 0.f, be = ok ? beta[c] : 0.f;
    float w[kMaxC], dw[kMaxC];
#pragma unroll
    for (int k = 0; k < kMaxC; ++k) {
        w[k] = (ok && k < C) ? W[(int64_t)k * D + c] : 0.f;
        dw[k] = 0.f;
    }
    float s1 = 0.f, s2 = 0.f;
    if (ok)
        for (int b = slice; b < B; b += kRS) {
            const float xh = xhat[(int64_t)b * D + c];
            const float z = fmaf(ga, xh, be);
            float dz = 0.f;
#pragma unroll
            for (int k = 0; k < kMaxC; ++k)
                if (k < C) {
                    const int64_t i = (int64_t)b * C + k;
                    const float dl = (dlogits ? gl * dlogits[i] : 0.f) + (dlogits_up ? dlogits_up[i] : 0.f);
                    dz = fmaf(dl, w[k], dz);
                    dw[k] = fmaf(dl, z, dw[k]);
                }
            s1 += dz;
            s2 = fmaf(dz, xh, s2);
        }
    s1 = vh_cross_slices(s1, red, slice, lane);
    s2 = vh_cross_slices(s2, red, slice, lane);
    if (dW) {                                                                     // uniform over the grid
#pragma unroll
        for (int k = 0; k < kMaxC; ++k)
            if (k < C) {
                const float t = vh_cross_slices(dw[k], red, slice, lane);
                if (ok && slice == 0) dW[(int64_t)k * D + c] = t;
            }
    }
    if (ok && slice == 0) {
        if (dgamma) dgamma[c] = s2;
        if (dbeta) dbeta[c] = s1;
    }
    if (ok && (dx1 || dx2)) {
        const float kk = ga * invstd[c];
        const float m1 = train ? s1 / (float)B : 0.f, m2 = train ? s2 / (float)B : 0.f;
        for (int b = slice; b < B; b += kRS) {
            const int64_t j = (int64_t)b * D + c;
            float dz = 0.f;                                                       // recomputed: the same operations as above
#pragma unroll
            for (int k = 0; k < kMaxC; ++k)
                if (k < C) {
                    const int64_t i = (int64_t)b * C + k;
                    const float dl = (dlogits ? gl * dlogits[i] : 0.f) + (dlogits_up ? dlogits_up[i] : 0.f);
                    dz = fmaf(dl, w[k], dz);
                }
            const float dd = kk * ((dz - m1) - xhat[j] * m2);
            const float g = 2.f * (x1[j] - x2[j]) * dd;
            if (dx1) dx1[j] = g;
            if (dx2) dx2[j] = -g;
        }
    }
    if (dbias && blockIdx.x == 0) {                                               // uniform over the workgroup
        float* r16 = &red[0][0];
        for (int k = 0; k < C; ++k) {
            float s = 0.f;
            for (int b = threadIdx.x; b < B; b += 256) {
                const int64_t i = (int64_t)b * C + k;
                s += (dlogits ? gl * dlogits[i] : 0.f) + (dlogits_up ? dlogits_up[i] : 0.f);
            }
            s = rg_block_sum(s, r16);
            if (threadIdx.x == 0) dbias[k] = s;
        }
    }
}

bool vh_extents_ok(int B, int D, int C) {
    return B <= 65535 * 32 && (int64_t)B * D < (1ll << 31) && (int64_t)rg::cdiv(D, kCG) * B * C < (1ll << 31);
}

}  // namespace

extern "C" int64_t rg_verif_head_workspace(int B, int D, int C) {
    if (B <= 0 || D <= 0 || C <= 0) return 0;
    return (int64_t)rg::cdiv(D, kCG) * B * C * (int64_t)sizeof(float);
}

extern "C" int rg_verif_head_fwd(const float* x1, const float* x2, const float* gamma, const float* beta, float* running_mean,
                                 float* running_var, const float* W, const float* bias, const int64_t* labels, float* logits,
                                 float* xhat, float* mean, float* invstd, float* loss_rows, float* out2, float* dlogits, int B,
                                 int D, int C, int train, float eps, float momentum, void* workspace, size_t workspace_bytes,
                                 hipStream_t stream) {
    RG_REQUIRE(x1 && x2 && gamma && beta && running_mean && running_var && W && logits && xhat && mean && invstd && B > 0 && D > 0,
               "rg_verif_head_fwd: bad arguments");
    RG_REQUIRE(C >= 1 && C <= kMaxC, "rg_verif_head_fwd: 1 to %d classes, got %d", kMaxC, C);
    RG_REQUIRE(!labels || (loss_rows && out2 && dlogits), "rg_verif_head_fwd: labels need loss_rows, out2 and dlogits");
    RG_REQUIRE(!train || B >= 2, "rg_verif_head_fwd: batch statistics need more than 1 row");
    RG_REQUIRE(vh_extents_ok(B, D, C), "rg_verif_head_fwd: extents too large");
    const int G = rg::cdiv(D, kCG);
    rg::ProfScope prof(rg::FAM_NORM, stream, 2.0 * B * (double)D * C, 4.0 * B * (double)D * (train ? 7.0 : 3.0));
    if (!train) {
        hipLaunchKernelGGL(verif_head_eval_fwd_kernel, dim3(B), dim3(256), 0, stream, x1, x2, gamma, beta, running_mean, running_var,
                           W, bias, xhat, mean, invstd, logits, D, C, eps);
        if (labels)
            hipLaunchKernelGGL(verif_head_row_kernel, dim3(1), dim3(256), 0, stream, (const float*)nullptr, bias, labels, logits,
                               loss_rows, out2, dlogits, B, C, 0);
        return rg::check_launch("rg_verif_head_fwd");
    }
    if (!workspace || workspace_bytes < (size_t)rg_verif_head_workspace(B, D, C)) {
        rg::set_error("rg_verif_head_fwd: workspace too small");
        return RG_ERR_WORKSPACE;
    }
    float* part = static_cast<float*>(workspace);
    hipLaunchKernelGGL(verif_head_col_fwd_kernel, dim3(G), dim3(256), 0, stream, x1, x2, gamma, beta, running_mean, running_var, W,
                       xhat, mean, invstd, part, B, D, C, eps, momentum);
    hipLaunchKernelGGL(verif_head_row_kernel, dim3(1), dim3(256), 0, stream, (const float*)part, bias, labels, logits, loss_rows,
                       out2, dlogits, B, C, G);
    return rg::check_launch("rg_verif_head_fwd");
}

extern "C" int rg_verif_head_bwd(const float* grad_loss, const float* dlogits, const float* dlogits_up, const float* x1,
                                 const float* x2, const float* xhat, const float* invstd, const float* gamma, const float* beta,
                                 const float* W, float* dx1, float* dx2, float* dW, float* dbias, float* dgamma, float* dbeta,
                                 int B, int D, int C, int train, hipStream_t stream) {
    RG_REQUIRE(x1 && x2 && xhat && invstd && gamma && beta && W && B > 0 && D > 0, "rg_verif_head_bwd: bad arguments");
    RG_REQUIRE(C >= 1 && C <= kMaxC, "rg_verif_head_bwd: 1 to %d classes, got %d", kMaxC, C);
    RG_REQUIRE(dlogits || dlogits_up, "rg_verif_head_bwd: no upstream gradient");
    RG_REQUIRE(dlogits || !grad_loss, "rg_verif_head_bwd: grad_loss scales dlogits, which is missing");
    RG_REQUIRE(vh_extents_ok(B, D, C), "rg_verif_head_bwd: extents too large");
    rg::ProfScope prof(rg::FAM_NORM, stream, 4.0 * B * (double)D * C, 4.0 * B * (double)D * 7.0);
    hipLaunchKernelGGL(verif_head_col_bwd_kernel, dim3(rg::cdiv(D, kCG)), dim3(256), 0, stream, grad_loss, dlogits, dlogits_up, x1,
                       x2, xhat, invstd, gamma, beta, W, dx1, dx2, dW, dbias, dgamma, dbeta, B, D, C, train);
    return rg::check_launch("rg_verif_head_bwd");
}
