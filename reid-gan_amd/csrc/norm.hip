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
#include "rg_common.h"
#include <type_traits>

namespace {

struct WStat {
    float n, mean, m2;
};

// ---- domain-specific BatchNorm (DSBN) on the BatchNorm kernels ---------------------------------------------------------------------
// A DSBN batch is [source half | target half] (h = N / 2 samples each) and every half has its own parameters and running statistics
// (CC/clustercontrast/models/dsbn.py:6-23).  The halves of an [N][C][HW] tensor are contiguous, so (domain, channel) are 2C virtual
// channels over h samples and a domain is a BatchNorm on a (sample base, sample count) view.  Every train-mode BatchNorm kernel below
// therefore ends in a parameter pack `DS... ds`: empty for a BatchNorm (the kernel is then exactly what it was), one of the structs
// here for the two-domain layer — the kernel is launched with h for N and one more grid plane, and its first lines move the
// tensors to sample d * h, the statistics to row d of [2][C] and pick parameter set d.  There is one copy of every kernel body.
struct DsbnSet {
    const float* gamma;
    const float* beta;
    float* running_mean;
    float* running_var;
    float eps, momentum;
};
struct DsbnFwd {                      // forward kernels that read parameters or update running statistics
    DsbnSet s[2];
};
struct DsbnBwd {                      // backward kernels
    const float* gamma[2];
    float* d_gamma[2];                // receive sum g * xhat
    float* d_beta[2];                 // receive sum g
};
struct DsbnPlane {};                  // kernels that only need the domain's offset
template <class T>
__device__ __forceinline__ const T& dsbn_arg(const T& t) {
    return t;
}

__device__ __forceinline__ WStat chan_merge(WStat a, WStat b) {
    WStat r;
    r.n = a.n + b.n;
    if (r.n == 0.f) {
        r.mean = 0.f;
        r.m2 = 0.f;
        return r;
    }
    const float d = b.mean - a.mean;
    const float f = b.n / r.n;
    r.mean = a.mean + d * f;
    r.m2 = a.m2 + b.m2 + d * d * a.n * f;
    return r;
}

__device__ __forceinline__ WStat wave_merge(WStat s) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        WStat o;
        o.n = __shfl_xor(s.n, off, 64);
        o.mean = __shfl_xor(s.mean, off, 64);
        o.m2 = __shfl_xor(s.m2, off, 64);
        s = chan_merge(s, o);
    }
    return s;
}

// grid (S, C): block (s, c) reduces elements [s*L, (s+1)*L) of channel c's N*HW values.
template <class... DS>
__global__ __launch_bounds__(256) void bn_stats_partial_kernel(const float* __restrict__ x, float* __restrict__ part,
                                                               int N, int C, int HW, int L, DS... ds) {
    if constexpr (sizeof...(DS) > 0) {                 // the two-domain layer: this plane's half, statistics row and parameter set
        const int d = blockIdx.z;
        x += (int64_t)d * N * C * HW;
        part += (int64_t)d * C * gridDim.x * 3;
    }
    const int c = blockIdx.y, s = blockIdx.x, S = gridDim.x;
    const int64_t total = (int64_t)N * HW;
    const int64_t beg = (int64_t)s * L;
    int64_t end = beg + L;
    if (end > total) end = total;
    float shift = 0.f, sum = 0.f, sq = 0.f, cnt = 0.f;
    bool first = true;
    if ((HW & 3) == 0) {
        for (int64_t e = beg + (int64_t)threadIdx.x * 4; e < end; e += 256 * 4) {
            const int n = (int)(e / HW);
            const int hw = (int)(e - (int64_t)n * HW);
            const float4 v = *reinterpret_cast<const float4*>(x + ((int64_t)n * C + c) * HW + hw);
            if (first) {
                shift = v.x;
                first = false;
            }
            const float a = v.x - shift, b = v.y - shift, cc = v.z - shift, d = v.w - shift;
            sum += (a + b) + (cc + d);
            sq += (a * a + b * b) + (cc * cc + d * d);
            cnt += 4.f;
        }
    } else {
        for (int64_t e = beg + threadIdx.x; e < end; e += 256) {
            const int n = (int)(e / HW);
            const int hw = (int)(e - (int64_t)n * HW);
            const float v = x[((int64_t)n * C + c) * HW + hw];
            if (first) {
                shift = v;
                first = false;
            }
            const float a = v - shift;
            sum += a;
            sq += a * a;
            cnt += 1.f;
        }
    }
    WStat st;
    st.n = cnt;
    st.mean = cnt > 0.f ? shift + sum / cnt : 0.f;
    st.m2 = cnt > 0.f ? fmaxf(sq - sum * sum / cnt, 0.f) : 0.f;
    st = wave_merge(st);
    __shared__ WStat red[4];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    if (lane == 0) red[wid] = st;
    __syncthreads();
    if (threadIdx.x == 0) {
        WStat t = red[0];
        for (int i = 1; i < 4; ++i) t = chan_merge(t, red[i]);
        float* o = part + ((int64_t)c * S + s) * 3;
        o[0] = t.n;
        o[1] = t.mean;
        o[2] = t.m2;
    }
}

template <class... DS>
__global__ void bn_stats_finalize_kernel(const float* __restrict__ part, int C, int S, float eps, float momentum,
                                         float* __restrict__ mean, float* __restrict__ invstd,
                                         float* __restrict__ running_mean, float* __restrict__ running_var, DS... ds) {
    if constexpr (sizeof...(DS) > 0) {                 // the two-domain layer: this plane's half, statistics row and parameter set
        const int d = blockIdx.y;
        const auto& a = dsbn_arg(ds...);
        const DsbnSet p = d ? a.s[1] : a.s[0];
        part += (int64_t)d * C * S * 3;
        mean += d * C, invstd += d * C;
        running_mean = p.running_mean, running_var = p.running_var, eps = p.eps, momentum = p.momentum;
    }
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    WStat t;
    t.n = 0.f;
    t.mean = 0.f;
    t.m2 = 0.f;
    for (int s = 0; s < S; ++s) {
        const float* o = part + ((int64_t)c * S + s) * 3;
        WStat b;
        b.n = o[0];
        b.mean = o[1];
        b.m2 = o[2];
        t = chan_merge(t, b);
    }
    const float var = t.n > 0.f ? t.m2 / t.n : 0.f;
    mean[c] = t.mean;
    invstd[c] = rsqrtf(var + eps);
    if (running_mean) running_mean[c] = (1.f - momentum) * running_mean[c] + momentum * t.mean;
    if (running_var) {
        const float unb = t.n > 1.f ? t.m2 / (t.n - 1.f) : var;
        running_var[c] = (1.f - momentum) * running_var[c] + momentum * unb;
    }
}

// y = act((x - mean[c]) * invstd[c] * gamma[c] + beta[c] + res)
// stat_is_var: `invstd` holds a variance (eval mode: running_var) and eps is applied here.
template <class... DS>
__global__ __launch_bounds__(256) void bn_apply_fwd_kernel(const float* __restrict__ x, const float* __restrict__ mean,
                                                           const float* __restrict__ invstd,
                                                           const float* __restrict__ gamma,
                                                           const float* __restrict__ beta, const float* __restrict__ res,
                                                           float* __restrict__ y, int64_t total, int C, int HW,
                                                           int stat_is_var, float eps, int act, float slope, DS... ds) {
    if constexpr (sizeof...(DS) > 0) {                 // the two-domain layer: this plane's half, statistics row and parameter set
        const int d = blockIdx.y;
        const auto& a = dsbn_arg(ds...);
        const DsbnSet p = d ? a.s[1] : a.s[0];
        const int64_t o = d * total;
        x += o, y += o, mean += d * C, invstd += d * C;
        if (res) res += o;
        gamma = p.gamma, beta = p.beta;
    }
    if ((HW & 3) == 0) {
        const int64_t nv = total >> 2;
        for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nv; i += (int64_t)gridDim.x * blockDim.x) {
            const int64_t e = i << 2;
            const int c = (int)((e / HW) % C);
            float is = invstd[c];
            if (stat_is_var) is = rsqrtf(is + eps);
            const float sc = is * (gamma ? gamma[c] : 1.f);
            const float sh = (beta ? beta[c] : 0.f) - mean[c] * sc;
            float4 v = *reinterpret_cast<const float4*>(x + e);
            v.x = v.x * sc + sh;
            v.y = v.y * sc + sh;
            v.z = v.z * sc + sh;
            v.w = v.w * sc + sh;
            if (res) {
                const float4 r = *reinterpret_cast<const float4*>(res + e);
                v.x += r.x;
                v.y += r.y;
                v.z += r.z;
                v.w += r.w;
            }
            v.x = rg_apply_act(v.x, act, slope);
            v.y = rg_apply_act(v.y, act, slope);
            v.z = rg_apply_act(v.z, act, slope);
            v.w = rg_apply_act(v.w, act, slope);
            *reinterpret_cast<float4*>(y + e) = v;
        }
    } else {
        for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
            const int c = (int)((e / HW) % C);
            float is = invstd[c];
            if (stat_is_var) is = rsqrtf(is + eps);
            const float sc = is * (gamma ? gamma[c] : 1.f);
            const float sh = (beta ? beta[c] : 0.f) - mean[c] * sc;
            float v = x[e] * sc + sh;
            if (res) v += res[e];
            y[e] = rg_apply_act(v, act, slope);
        }
    }
}

__device__ __forceinline__ float act_grad_from_out(float yv, int act, float slope) {
    switch (act) {
        case RG_ACT_RELU: return yv > 0.f ? 1.f : 0.f;
        case RG_ACT_LEAKY: return yv > 0.f ? 1.f : slope;
        case RG_ACT_TANH: return 1.f - yv * yv;
        default: return 1.f;
    }
}

// partial sums over a slice: sum(dy_eff), sum(dy_eff * xhat); dy_eff = dy * act'(y)
template <class... DS>
__global__ __launch_bounds__(256) void bn_bwd_reduce_partial_kernel(const float* __restrict__ x,
                                                                    const float* __restrict__ dy,
                                                                    const float* __restrict__ yact,
                                                                    const float* __restrict__ mean,
                                                                    const float* __restrict__ invstd,
                                                                    float* __restrict__ part, int N, int C, int HW,
                                                                    int L, int stat_is_var, float eps, int act,
                                                                    float slope, DS... ds) {
    if constexpr (sizeof...(DS) > 0) {                 // the two-domain layer: this plane's half, statistics row and parameter set
        const int d = blockIdx.z;
        const int64_t o = (int64_t)d * N * C * HW;
        x += o, dy += o, mean += d * C, invstd += d * C;
        if (yact) yact += o;
        part += (int64_t)d * C * gridDim.x * 2;
    }
    const int c = blockIdx.y, s = blockIdx.x, S = gridDim.x;
    const int64_t total = (int64_t)N * HW;
    const int64_t beg = (int64_t)s * L;
    int64_t end = beg + L;
    if (end > total) end = total;
    const float mu = mean[c];
    float is = invstd[c];
    if (stat_is_var) is = rsqrtf(is + eps);
    float s1 = 0.f, s2 = 0.f;
    if ((HW & 3) == 0) {
        for (int64_t e = beg + (int64_t)threadIdx.x * 4; e < end; e += 256 * 4) {
            const int n = (int)(e / HW);
            const int hw = (int)(e - (int64_t)n * HW);
            const int64_t o = ((int64_t)n * C + c) * HW + hw;
            const float4 xv = *reinterpret_cast<const float4*>(x + o);
            float4 g = *reinterpret_cast<const float4*>(dy + o);
            if (act != RG_ACT_NONE) {
                const float4 yv = *reinterpret_cast<const float4*>(yact + o);
                g.x *= act_grad_from_out(yv.x, act, slope);
                g.y *= act_grad_from_out(yv.y, act, slope);
                g.z *= act_grad_from_out(yv.z, act, slope);
                g.w *= act_grad_from_out(yv.w, act, slope);
            }
            s1 += (g.x + g.y) + (g.z + g.w);
            s2 += (g.x * (xv.x - mu) + g.y * (xv.y - mu)) + (g.z * (xv.z - mu) + g.w * (xv.w - mu));
        }
    } else {
        for (int64_t e = beg + threadIdx.x; e < end; e += 256) {
            const int n = (int)(e / HW);
            const int hw = (int)(e - (int64_t)n * HW);
            const int64_t o = ((int64_t)n * C + c) * HW + hw;
            float g = dy[o];
            if (act != RG_ACT_NONE) g *= act_grad_from_out(yact[o], act, slope);
            s1 += g;
            s2 += g * (x[o] - mu);
        }
    }
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

template <class... DS>
__global__ void bn_bwd_reduce_finalize_kernel(const float* __restrict__ part, int C, int S, float* __restrict__ sum_dy,
                                              float* __restrict__ sum_dy_xhat, DS... ds) {
    if constexpr (sizeof...(DS) > 0) {                 // the two-domain layer: this plane's half, statistics row and parameter set
        const int d = blockIdx.y;
        const auto& a = dsbn_arg(ds...);
        part += (int64_t)d * C * S * 2;
        sum_dy = d ? a.d_beta[1] : a.d_beta[0], sum_dy_xhat = d ? a.d_gamma[1] : a.d_gamma[0];
    }
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    float a = 0.f, b = 0.f;
    for (int s = 0; s < S; ++s) {
        a += part[((int64_t)c * S + s) * 2 + 0];
        b += part[((int64_t)c * S + s) * 2 + 1];
    }
    sum_dy[c] = a;
    sum_dy_xhat[c] = b;
}

// dx = gamma*invstd * (g - train*(sum_dy/cnt + xhat*sum_dy_xhat/cnt)),  g = dy*act'(y);  dres = g
template <class... DS>
__global__ __launch_bounds__(256) void bn_bwd_apply_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                           const float* __restrict__ yact,
                                                           const float* __restrict__ mean,
                                                           const float* __restrict__ invstd,
                                                           const float* __restrict__ gamma,
                                                           const float* __restrict__ sum_dy,
                                                           const float* __restrict__ sum_dy_xhat,
                                                           float* __restrict__ dx, float* __restrict__ dres,
                                                           int64_t total, int C, int HW, float inv_count, int train,
                                                           int stat_is_var, float eps, int act, float slope, DS... ds) {
    if constexpr (sizeof...(DS) > 0) {                 // the two-domain layer: this plane's half, statistics row and parameter set
        const int d = blockIdx.y;
        const auto& a = dsbn_arg(ds...);
        const int64_t o = d * total;
        x += o, dy += o, mean += d * C, invstd += d * C;
        if (yact) yact += o;
        if (dx) dx += o;
        if (dres) dres += o;
        gamma = d ? a.gamma[1] : a.gamma[0];
        sum_dy = d ? a.d_beta[1] : a.d_beta[0], sum_dy_xhat = d ? a.d_gamma[1] : a.d_gamma[0];
    }
    const bool vec = (HW & 3) == 0;
    const int64_t nitems = vec ? (total >> 2) : total;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nitems; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t e = vec ? (i << 2) : i;
        const int c = (int)((e / HW) % C);
        const float mu = mean[c];
        float is = invstd[c];
        if (stat_is_var) is = rsqrtf(is + eps);
        const float gs = (gamma ? gamma[c] : 1.f) * is;
        const float a = train ? sum_dy[c] * inv_count : 0.f;
        const float b = train ? sum_dy_xhat[c] * inv_count : 0.f;
        if (vec) {
            float4 g = *reinterpret_cast<const float4*>(dy + e);
            if (act != RG_ACT_NONE) {
                const float4 yv = *reinterpret_cast<const float4*>(yact + e);
                g.x *= act_grad_from_out(yv.x, act, slope);
                g.y *= act_grad_from_out(yv.y, act, slope);
                g.z *= act_grad_from_out(yv.z, act, slope);
                g.w *= act_grad_from_out(yv.w, act, slope);
            }
            if (dres) *reinterpret_cast<float4*>(dres + e) = g;
            if (dx) {
                float4 o;
                if (train) {
                    const float4 xv = *reinterpret_cast<const float4*>(x + e);
                    o.x = gs * (g.x - a - (xv.x - mu) * is * b);
                    o.y = gs * (g.y - a - (xv.y - mu) * is * b);
                    o.z = gs * (g.z - a - (xv.z - mu) * is * b);
                    o.w = gs * (g.w - a - (xv.w - mu) * is * b);
                } else {
                    o.x = gs * g.x;
                    o.y = gs * g.y;
                    o.z = gs * g.z;
                    o.w = gs * g.w;
                }
                *reinterpret_cast<float4*>(dx + e) = o;
            }
        } else {
            float g = dy[e];
            if (act != RG_ACT_NONE) g *= act_grad_from_out(yact[e], act, slope);
            if (dres) dres[e] = g;
            if (dx) dx[e] = train ? gs * (g - a - (x[e] - mu) * is * b) : gs * g;
        }
    }
}

// ---- conv + frozen-statistics BatchNorm folded into the convolution ---------------------------------------------
// y = act(conv(x, W) * scale + shift [+ residual]) runs in the conv epilogue (scale = gamma * invstd,
// shift = beta - mean * scale), so the pre-normalisation tensor z is never written.  Backward without z:
//   g      = dy * act'(y)                         (this kernel; + per-channel sum of g = dbeta)
//   G      = wgrad(x, g)                          (conv kernel)        because sum_{n,p,q} g z = sum_{c,r,s} W G
//   dgamma = invstd * (sum W.G - mean * sum g);  dW = scale * G        (bn_fold_wgrad_kernel, one workgroup per filter)
//   dx     = dgrad(g, scale * W)                  (conv kernel on row-scaled filters, scale_rows_kernel)
__global__ __launch_bounds__(256) void act_bwd_sum_kernel(const float* __restrict__ dy, const float* __restrict__ yact,
                                                          float* __restrict__ g_out, float* __restrict__ part, int N, int C,
                                                          int HW, int L, int act, float slope, int want_sum) {
    const int c = blockIdx.y, s = blockIdx.x, S = gridDim.x;
    const int64_t total = (int64_t)N * HW;
    const int64_t beg = (int64_t)s * L;
    int64_t end = beg + L;
    if (end > total) end = total;
    float s1 = 0.f;
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
            if (g_out) *reinterpret_cast<float4*>(g_out + o) = g;
            s1 += (g.x + g.y) + (g.z + g.w);
        }
    } else {
        for (int64_t e = beg + threadIdx.x; e < end; e += 256) {
            const int n = (int)(e / HW);
            const int hw = (int)(e - (int64_t)n * HW);
            const int64_t o = ((int64_t)n * C + c) * HW + hw;
            float g = dy[o];
            if (act != RG_ACT_NONE) g *= act_grad_from_out(yact[o], act, slope);
            if (g_out) g_out[o] = g;
            s1 += g;
        }
    }
    if (!want_sum) return;
    __shared__ float red[16];
    s1 = rg_block_sum(s1, red);
    if (threadIdx.x == 0) part[(int64_t)c * S + s] = s1;
}

__global__ void sum_slices_kernel(const float* __restrict__ part, int C, int S, float* __restrict__ out) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    float a = 0.f;
    for (int s = 0; s < S; ++s) a += part[(int64_t)c * S + s];
    out[c] = a;
}

__global__ void bn_fold_kernel(const float* __restrict__ gamma, const float* __restrict__ beta, const float* __restrict__ mean,
                               const float* __restrict__ var, float eps, float* __restrict__ scale, float* __restrict__ shift,
                               float* __restrict__ invstd, int C) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    const float is = rsqrtf(var[c] + eps);
    const float sc = (gamma ? gamma[c] : 1.f) * is;
    scale[c] = sc;
    shift[c] = (beta ? beta[c] : 0.f) - mean[c] * sc;
    invstd[c] = is;
}

__global__ __launch_bounds__(256) void bn_fold_wgrad_kernel(const float* __restrict__ w, float* __restrict__ g,
                                                            const float* __restrict__ scale, const float* __restrict__ invstd,
                                                            const float* __restrict__ mean, const float* __restrict__ sum_g,
                                                            const float* __restrict__ part, int S, float* __restrict__ dbeta,
                                                            float* __restrict__ dgamma, int M) {
    __shared__ float red[16];
    const int k = blockIdx.x;
    const float* wr = w + (int64_t)k * M;
    float* gr = g + (int64_t)k * M;
    float sg = 0.f;
    if (part) {                       // channel sum of g from slice / tile partials (fixed tree: deterministic)
        float t = 0.f;
        for (int s = threadIdx.x; s < S; s += 256) t += part[(int64_t)k * S + s];
        sg = rg_block_sum(t, red);
        if (dbeta && threadIdx.x == 0) dbeta[k] = sg;
    } else if (sum_g) {
        sg = sum_g[k];
    }
    if (dgamma) {
        float t = 0.f;
        for (int m = threadIdx.x; m < M; m += 256) t += wr[m] * gr[m];
        t = rg_block_sum(t, red);
        if (threadIdx.x == 0) dgamma[k] = invstd[k] * (t - mean[k] * sg);
    }
    const float sc = scale[k];
    for (int m = threadIdx.x; m < M; m += 256) gr[m] *= sc;
}

__global__ void scale_rows_kernel(const float* __restrict__ w, const float* __restrict__ scale, float* __restrict__ out, int M,
                                  int64_t total) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x)
        out[i] = w[i] * scale[i / M];
}

// One launch folds EVERY (conv, frozen BatchNorm) pair of a network: per pair scale / shift / invstd and the filters
// multiplied by scale[k] in the checkpoint layout [K][C][RS] and, when requested, in [K][RS][C] for the (r,s)-major
// loaders.  The table lives in device memory, 16 int64 words per pair:
//   0 w  1 gamma  2 beta  3 running_mean  4 running_var  5 w_scaled  6 w_scaled_krsc (0 = none)  7 scale  8 shift  9 invstd
//   10 K  11 C  12 RS  13 eps (float bits)  14 first block of the pair  15 unused
constexpr int FOLD_WORDS = 16;
constexpr int FOLD_CHUNK = 2048;          // filter elements per workgroup

__global__ __launch_bounds__(256) void fold_filters_multi_kernel(const long long* __restrict__ tab, int n_pairs) {
    // binary search of the pair this block belongs to
    int lo = 0, hi = n_pairs - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (tab[(int64_t)mid * FOLD_WORDS + 14] <= (long long)blockIdx.x) lo = mid; else hi = mid - 1;
    }
    const long long* e = tab + (int64_t)lo * FOLD_WORDS;
    const float* w = reinterpret_cast<const float*>(e[0]);
    const float* gamma = reinterpret_cast<const float*>(e[1]);
    const float* beta = reinterpret_cast<const float*>(e[2]);
    const float* mean = reinterpret_cast<const float*>(e[3]);
    const float* var = reinterpret_cast<const float*>(e[4]);
    float* ws = reinterpret_cast<float*>(e[5]);
    float* wk = reinterpret_cast<float*>(e[6]);
    float* scale = reinterpret_cast<float*>(e[7]);
    float* shift = reinterpret_cast<float*>(e[8]);
    float* invstd = reinterpret_cast<float*>(e[9]);
    const int K = (int)e[10], C = (int)e[11], RS = (int)e[12];
    const float eps = __int_as_float((int)e[13]);
    const int blk = (int)((long long)blockIdx.x - e[14]);
    const int64_t total = (int64_t)K * C * RS;
    const int64_t crs = (int64_t)C * RS;
    const int64_t beg = (int64_t)blk * FOLD_CHUNK;
    for (int64_t i = beg + threadIdx.x; i < beg + FOLD_CHUNK && i < total; i += 256) {
        const int k = (int)(i / crs);
        const int rem = (int)(i - (int64_t)k * crs);
        const float is = rsqrtf(var[k] + eps);
        const float sc = gamma[k] * is;
        const float v = w[i] * sc;
        ws[i] = v;
        if (wk) {
            const int c = rem / RS, rs = rem - c * RS;
            wk[((int64_t)k * RS + rs) * C + c] = v;
        }
        if (rem == 0) {
            scale[k] = sc;
            shift[k] = beta[k] - mean[k] * sc;
            invstd[k] = is;
        }
    }
}

static int pick_slices(int N, int C, int HW, int* L) {
    const int64_t total = (int64_t)N * HW;
    int64_t S = rg::cdiv(2048, C);
    const int64_t maxS = rg::cdiv64(total, 4096);
    if (S > maxS) S = maxS;
    if (S < 1) S = 1;
    int64_t l = rg::cdiv64(total, S);
    l = (l + 3) & ~3ll;
    *L = (int)l;
    return (int)rg::cdiv64(total, l);
}

static unsigned grid_for(int64_t items) {
    int64_t g = rg::cdiv64(items, 256);
    if (g > 4096) g = 4096;
    if (g < 1) g = 1;
    return (unsigned)g;
}

}  // namespace

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
    hipLaunchKernelGGL(bn_stats_partial_kernel, dim3(S, C), dim3(256), 0, stream, x, part, N, C, HW, L);
    hipLaunchKernelGGL(bn_stats_finalize_kernel, dim3(rg::cdiv(C, 64)), dim3(64), 0, stream, part, C, S, eps, momentum,
                       mean, invstd, running_mean, running_var);
    return rg::check_launch("rg_bn_stats");
}

extern "C" int rg_bn_apply_fwd(const float* x, const float* mean, const float* stat, const float* gamma,
                               const float* beta, const float* residual, float* y, int N, int C, int HW,
                               int stat_is_var, float eps, int act, float slope, hipStream_t stream) {
    RG_REQUIRE(x && mean && stat && y && N > 0 && C > 0 && HW > 0, "rg_bn_apply_fwd: bad arguments");
    const int64_t total = (int64_t)N * C * HW;
    rg::ProfScope prof(rg::FAM_NORM, stream, 0.0, (residual ? 12.0 : 8.0) * total);
    hipLaunchKernelGGL(bn_apply_fwd_kernel, dim3(grid_for((HW & 3) ? total : total / 4)), dim3(256), 0, stream, x, mean,
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
    hipLaunchKernelGGL(bn_bwd_reduce_partial_kernel, dim3(S, C), dim3(256), 0, stream, x, dy, y_act, mean, stat, part, N,
                       C, HW, L, stat_is_var, eps, act, slope);
    hipLaunchKernelGGL(bn_bwd_reduce_finalize_kernel, dim3(rg::cdiv(C, 64)), dim3(64), 0, stream, part, C, S, sum_dy,
                       sum_dy_xhat);
    return rg::check_launch("rg_bn_bwd_reduce");
}

// ---- train-mode BatchNorm in one launch per direction, small per-channel extents ----------------------------------------------
// One workgroup per channel: its N rows of HW floats (stride C*HW) are <= 64 KB, so passes two and three hit L1 / L2.  Used when
// N*HW <= 16384 and the channel count alone fills the chip (layer3 / layer4 of the ResNets, the inner generator layers); the
// slice-parallel kernels above stay for the large maps.  Statistics as bn_stats (biased variance for the normalisation, unbiased
// for running_var), two-pass.
__device__ __forceinline__ float bn_block_sum(float v, float* red) {
    v = rg_wave_sum(v);
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) red[wid] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

// `c` is the channel of the tensor, `sc` the index of its statistics / affine parameters (the same number for a BatchNorm; the
// channel-split IBN layer below normalises channels [half, C) with parameters [0, C - half))
__device__ __forceinline__ void bn_channel_fwd(const float* __restrict__ x, const float* __restrict__ gamma,
                                               const float* __restrict__ beta, const float* __restrict__ res,
                                               float* __restrict__ y, float* __restrict__ mean_out,
                                               float* __restrict__ invstd_out, float* __restrict__ running_mean,
                                               float* __restrict__ running_var, int N, int C, int HW, float eps,
                                               float momentum, int act, float slope, int c, int sc, float* red) {
    const int t = threadIdx.x;
    const bool vec = (HW & 3) == 0;
    const int rl = vec ? HW >> 2 : HW;                   // units (float4 or float) per row
    const int total = N * rl;
    const int64_t cs = (int64_t)C * HW;
    const float cnt = (float)N * (float)HW;
    float s = 0.f;
    for (int i = t; i < total; i += 256) {
        const int n = i / rl, v = i - n * rl;
        const float* p = x + (int64_t)n * cs + (int64_t)c * HW;
        if (vec) {
            const float4 a = reinterpret_cast<const float4*>(p)[v];
            s += (a.x + a.y) + (a.z + a.w);
        } else {
            s += p[v];
        }
    }
    const float mu = bn_block_sum(s, red) / cnt;
    float q = 0.f;
    for (int i = t; i < total; i += 256) {
        const int n = i / rl, v = i - n * rl;
        const float* p = x + (int64_t)n * cs + (int64_t)c * HW;
        if (vec) {
            const float4 a = reinterpret_cast<const float4*>(p)[v];
            const float d0 = a.x - mu, d1 = a.y - mu, d2 = a.z - mu, d3 = a.w - mu;
            q += (d0 * d0 + d1 * d1) + (d2 * d2 + d3 * d3);
        } else {
            const float d = p[v] - mu;
            q += d * d;
        }
    }
    const float m2 = bn_block_sum(q, red);
    const float var = m2 / cnt;
    const float is = rsqrtf(var + eps);
    if (t == 0) {
        mean_out[sc] = mu;
        invstd_out[sc] = is;
        if (running_mean) running_mean[sc] = (1.f - momentum) * running_mean[sc] + momentum * mu;
        if (running_var) running_var[sc] = (1.f - momentum) * running_var[sc] + momentum * (cnt > 1.f ? m2 / (cnt - 1.f) : var);
    }
    const float gs = (gamma ? gamma[sc] : 1.f) * is;
    const float sh = (beta ? beta[sc] : 0.f) - mu * gs;
    for (int i = t; i < total; i += 256) {
        const int n = i / rl, v = i - n * rl;
        const int64_t off = (int64_t)n * cs + (int64_t)c * HW;
        if (vec) {
            const float4 a = reinterpret_cast<const float4*>(x + off)[v];
            float4 o;
            o.x = a.x * gs + sh; o.y = a.y * gs + sh; o.z = a.z * gs + sh; o.w = a.w * gs + sh;
            if (res) {
                const float4 r = reinterpret_cast<const float4*>(res + off)[v];
                o.x += r.x; o.y += r.y; o.z += r.z; o.w += r.w;
            }
            o.x = rg_apply_act(o.x, act, slope); o.y = rg_apply_act(o.y, act, slope);
            o.z = rg_apply_act(o.z, act, slope); o.w = rg_apply_act(o.w, act, slope);
            reinterpret_cast<float4*>(y + off)[v] = o;
        } else {
            float o = x[off + v] * gs + sh;
            if (res) o += res[off + v];
            y[off + v] = rg_apply_act(o, act, slope);
        }
    }
}

template <class... DS>
__global__ __launch_bounds__(256) void bn_train_fwd_fused_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                                 const float* __restrict__ beta, const float* __restrict__ res,
                                                                 float* __restrict__ y, float* __restrict__ mean_out,
                                                                 float* __restrict__ invstd_out, float* __restrict__ running_mean,
                                                                 float* __restrict__ running_var, int N, int C, int HW, float eps,
                                                                 float momentum, int act, float slope, DS... ds) {
    if constexpr (sizeof...(DS) > 0) {                 // the two-domain layer: this plane's half, statistics row and parameter set
        const int d = blockIdx.y;
        const auto& a = dsbn_arg(ds...);
        const DsbnSet p = d ? a.s[1] : a.s[0];
        const int64_t o = (int64_t)d * N * C * HW;
        x += o, y += o, mean_out += d * C, invstd_out += d * C;
        if (res) res += o;
        gamma = p.gamma, beta = p.beta, running_mean = p.running_mean, running_var = p.running_var, eps = p.eps, momentum = p.momentum;
    }
    __shared__ float red[4];
    bn_channel_fwd(x, gamma, beta, res, y, mean_out, invstd_out, running_mean, running_var, N, C, HW, eps, momentum, act, slope,
                   (int)blockIdx.x, (int)blockIdx.x, red);
}

// ---- the same two kernels for maps whose rows are float4 multiples, with the loads taken out of the loops ---------------------------
// One workgroup per channel holds N*HW <= 16384 values = at most 16 float4 per thread.  The loops above issue one load per
// iteration behind an integer division and wait for it: with two workgroups per CU nothing hides that latency (a [32, 512, 16 x 8]
// layer: 15 us forward, 1 TB/s).  Here every thread computes its U offsets once (buffer resource over the tensor: offsets past
// the end return zeros / drop the store, so there are no bounds branches) and issues its loads together:
//   forward   x (and the residual) are loaded ONCE into registers; mean, centred sum of squares and the output come from them;
//   backward  two sweeps (the sums, then dx / dres) of U float4 per operand, eight units in flight per sweep.
// Same per-thread summation order and block reduction as the loop kernels: same statistics.
typedef __amdgpu_buffer_rsrc_t nrsrc_t;
constexpr unsigned NOOB = 0x80000000u;                  // tensors are < 2^31 bytes here (host check)
__device__ __forceinline__ nrsrc_t n_rsrc(const void* p, unsigned bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), 0, bytes, 0x00020000);
}
__device__ __forceinline__ float4 n_load4(nrsrc_t r, unsigned off) {
    typedef float f4v __attribute__((ext_vector_type(4)));
    const f4v v = __builtin_bit_cast(f4v, __builtin_amdgcn_raw_buffer_load_b128(r, off, 0, 0));
    return make_float4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ void n_store4(nrsrc_t r, unsigned off, float4 v) {
    typedef float f4v __attribute__((ext_vector_type(4)));
    const f4v w = {v.x, v.y, v.z, v.w};
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(__attribute__((__vector_size__(4 * sizeof(unsigned)))) unsigned, w), r, off, 0, 0);
}

template <int U>
__device__ __forceinline__ void bn_unit_offsets(unsigned (&off)[U], int t, int total, int rl, int C, int c, int HW) {
#pragma unroll
    for (int j = 0; j < U; ++j) {
        const int i = t + 256 * j;
        const int n = i / rl, v = i - n * rl;            // U divisions per thread, once
        off[j] = i < total ? (unsigned)((n * C + c) * HW + 4 * v) * 4u : NOOB;
    }
}

template <int U, class... DS>
__global__ __launch_bounds__(256) void bn_train_fwd_reg_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                               const float* __restrict__ beta, const float* __restrict__ res,
                                                               float* __restrict__ y, float* __restrict__ mean_out,
                                                               float* __restrict__ invstd_out, float* __restrict__ running_mean,
                                                               float* __restrict__ running_var, int N, int C, int HW, float eps,
                                                               float momentum, int act, float slope, unsigned bytes, DS... ds) {
    if constexpr (sizeof...(DS) > 0) {                 // the two-domain layer: this plane's half, statistics row and parameter set
        const int d = blockIdx.y;
        const auto& a = dsbn_arg(ds...);
        const DsbnSet p = d ? a.s[1] : a.s[0];
        const int64_t o = (int64_t)d * N * C * HW;
        x += o, y += o, mean_out += d * C, invstd_out += d * C;
        if (res) res += o;
        gamma = p.gamma, beta = p.beta, running_mean = p.running_mean, running_var = p.running_var, eps = p.eps, momentum = p.momentum;
    }
    __shared__ float red[4];
    const int c = blockIdx.x, t = threadIdx.x;
    const int rl = HW >> 2;
    const int total = N * rl;
    const float cnt = (float)N * (float)HW;
    const nrsrc_t rx = n_rsrc(x, bytes), ry = n_rsrc(y, bytes);
    const nrsrc_t rr = n_rsrc(res ? res : x, res ? bytes : 0u);
    unsigned off[U];
    bn_unit_offsets<U>(off, t, total, rl, C, c, HW);
    float4 a[U], r[U];
#pragma unroll
    for (int j = 0; j < U; ++j) a[j] = n_load4(rx, off[j]);
    if (res) {                                           // uniform; in flight behind x while the statistics are formed
#pragma unroll
        for (int j = 0; j < U; ++j) r[j] = n_load4(rr, off[j]);
    }
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < U; ++j) s += (a[j].x + a[j].y) + (a[j].z + a[j].w);
    const float mu = bn_block_sum(s, red) / cnt;
    float q = 0.f;
#pragma unroll
    for (int j = 0; j < U; ++j) {
        const float d0 = a[j].x - mu, d1 = a[j].y - mu, d2 = a[j].z - mu, d3 = a[j].w - mu;
        const float e = (d0 * d0 + d1 * d1) + (d2 * d2 + d3 * d3);
        q += off[j] != NOOB ? e : 0.f;
    }
    const float m2 = bn_block_sum(q, red);
    const float var = m2 / cnt;
    const float is = rsqrtf(var + eps);
    if (t == 0) {
        mean_out[c] = mu;
        invstd_out[c] = is;
        if (running_mean) running_mean[c] = (1.f - momentum) * running_mean[c] + momentum * mu;
        if (running_var) running_var[c] = (1.f - momentum) * running_var[c] + momentum * (cnt > 1.f ? m2 / (cnt - 1.f) : var);
    }
    const float gs = (gamma ? gamma[c] : 1.f) * is;
    const float sh = (beta ? beta[c] : 0.f) - mu * gs;
#pragma unroll
    for (int j = 0; j < U; ++j) {
        float4 o;
        o.x = a[j].x * gs + sh; o.y = a[j].y * gs + sh; o.z = a[j].z * gs + sh; o.w = a[j].w * gs + sh;
        if (res) { o.x += r[j].x; o.y += r[j].y; o.z += r[j].z; o.w += r[j].w; }
        o.x = rg_apply_act(o.x, act, slope); o.y = rg_apply_act(o.y, act, slope);
        o.z = rg_apply_act(o.z, act, slope); o.w = rg_apply_act(o.w, act, slope);
        n_store4(ry, off[j], o);
    }
}

template <int U, class... DS>
__global__ __launch_bounds__(256) void bn_train_bwd_reg_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                               const float* __restrict__ yact, const float* __restrict__ mean,
                                                               const float* __restrict__ invstd, const float* __restrict__ gamma,
                                                               float* __restrict__ dx, float* __restrict__ dres,
                                                               float* __restrict__ sum_dy, float* __restrict__ sum_dy_xhat, int N,
                                                               int C, int HW, int act, float slope, unsigned bytes, DS... ds) {
    if constexpr (sizeof...(DS) > 0) {                 // the two-domain layer: this plane's half, statistics row and parameter set
        const int d = blockIdx.y;
        const auto& a = dsbn_arg(ds...);
        const int64_t o = (int64_t)d * N * C * HW;
        x += o, dy += o, mean += d * C, invstd += d * C;
        if (yact) yact += o;
        if (dx) dx += o;
        if (dres) dres += o;
        gamma = d ? a.gamma[1] : a.gamma[0];
        sum_dy = d ? a.d_beta[1] : a.d_beta[0], sum_dy_xhat = d ? a.d_gamma[1] : a.d_gamma[0];
    }
    __shared__ float red[4];
    const int c = blockIdx.x, t = threadIdx.x;
    const int rl = HW >> 2;
    const int total = N * rl;
    const float cnt = (float)N * (float)HW;
    const float mu = mean[c], is = invstd[c];
    const bool has_act = act != RG_ACT_NONE;
    const nrsrc_t rx = n_rsrc(x, bytes), rg = n_rsrc(dy, bytes), ry = n_rsrc(has_act ? yact : dy, has_act ? bytes : 0u);
    const nrsrc_t rdx = n_rsrc(dx ? dx : dres, dx ? bytes : 0u), rdr = n_rsrc(dres ? dres : dx, dres ? bytes : 0u);
    unsigned off[U];
    bn_unit_offsets<U>(off, t, total, rl, C, c, HW);
    constexpr int B = U < 8 ? U : 8;                     // units in flight per operand
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int j0 = 0; j0 < U; j0 += B) {
        float4 g[B], a[B], yv[B];
#pragma unroll
        for (int j = 0; j < B; ++j) {
            g[j] = n_load4(rg, off[j0 + j]);
            a[j] = n_load4(rx, off[j0 + j]);
            if (has_act) yv[j] = n_load4(ry, off[j0 + j]);
        }
#pragma unroll
        for (int j = 0; j < B; ++j) {
            if (has_act) {
                g[j].x *= act_grad_from_out(yv[j].x, act, slope); g[j].y *= act_grad_from_out(yv[j].y, act, slope);
                g[j].z *= act_grad_from_out(yv[j].z, act, slope); g[j].w *= act_grad_from_out(yv[j].w, act, slope);
            }
            s1 += (g[j].x + g[j].y) + (g[j].z + g[j].w);
            s2 += (g[j].x * (a[j].x - mu) + g[j].y * (a[j].y - mu)) + (g[j].z * (a[j].z - mu) + g[j].w * (a[j].w - mu));
        }
    }
    s1 = bn_block_sum(s1, red);
    s2 = bn_block_sum(s2, red) * is;
    if (t == 0) {
        sum_dy[c] = s1;
        sum_dy_xhat[c] = s2;
    }
    if (!dx && !dres) return;
    const float gs = (gamma ? gamma[c] : 1.f) * is;
    const float a0 = s1 / cnt, b0 = s2 / cnt * is;
#pragma unroll
    for (int j0 = 0; j0 < U; j0 += B) {
        float4 g[B], a[B], yv[B];
#pragma unroll
        for (int j = 0; j < B; ++j) {
            g[j] = n_load4(rg, off[j0 + j]);
            if (dx) a[j] = n_load4(rx, off[j0 + j]);
            if (has_act) yv[j] = n_load4(ry, off[j0 + j]);
        }
#pragma unroll
        for (int j = 0; j < B; ++j) {
            if (has_act) {
                g[j].x *= act_grad_from_out(yv[j].x, act, slope); g[j].y *= act_grad_from_out(yv[j].y, act, slope);
                g[j].z *= act_grad_from_out(yv[j].z, act, slope); g[j].w *= act_grad_from_out(yv[j].w, act, slope);
            }
            if (dres) n_store4(rdr, off[j0 + j], g[j]);
            if (dx) {
                float4 o;
                o.x = gs * (g[j].x - a0 - (a[j].x - mu) * b0); o.y = gs * (g[j].y - a0 - (a[j].y - mu) * b0);
                o.z = gs * (g[j].z - a0 - (a[j].z - mu) * b0); o.w = gs * (g[j].w - a0 - (a[j].w - mu) * b0);
                n_store4(rdx, off[j0 + j], o);
            }
        }
    }
}

// ---- one row of HW contiguous floats: InstanceNorm2d and both halves of the IBN layer ----------------------------------------------
// A row (n, c) is <= 32 KB for every map of the networks here.  LANES = 16 / 32 / 64 lanes per row (several rows per wave for the
// small maps, shuffles only), 256: one workgroup per row.  Two forms of each direction, the same per-lane summation order and the
// same reduction in both, so the same values:
//   U == 0  loops: the row is walked three times (twice in the backward), passes two and three hit L1 / L2;
//   U  > 0  registers (HW % 4 == 0, at most U <= 8 float4 per lane): each lane loads its U units of every operand together, forms
//           the statistics / sums from registers and writes the results — one memory round trip instead of 3 * U.  One buffer
//           resource per operand over the WHOLE tensor (a wave may hold several rows, a resource must be wave-uniform); lanes
//           past the row carry the offset NOOB: their loads return zeros, their stores are dropped.
// Statistics: mean, then the centred sum of squares (two-pass, biased variance).
// A row either forms its own statistics / sums (an InstanceNorm instance) or takes its channel's (a BatchNorm row of the IBN layer):
enum { IBN_ROW_IN = 0, IBN_ROW_BN_TRAIN = 1, IBN_ROW_BN_EVAL = 2 };

template <int LANES>
__device__ __forceinline__ float in_reduce(float v, float* red) {
    // LANES <= 64: butterfly inside the aligned lane group (several rows share a wave); 256: the whole workgroup
#pragma unroll
    for (int off = (LANES < 64 ? LANES : 64) / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    if (LANES <= 64) return v;
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) red[wid] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

// byte offsets of lane t's U float4 units of the row that starts at element `row`
template <int LANES, int U>
__device__ __forceinline__ void row_unit_offsets(unsigned (&off)[U], int64_t row, int t, int HW) {
#pragma unroll
    for (int j = 0; j < U; ++j) off[j] = t + LANES * j < (HW >> 2) ? ((unsigned)row + 4u * (unsigned)(t + LANES * j)) * 4u : NOOB;
}

// y = act(gamma[c] * (x - mu) * is + beta[c] + res).  own_stats: mu / is are formed here and written to mean_out / invstd_out;
// otherwise they are given.  own_stats is uniform over the lane group (LANES == 256: the workgroup).
template <int LANES, int U>
__device__ __forceinline__ void norm_row_fwd(const float* __restrict__ x, const float* __restrict__ res, float* __restrict__ y,
                                             unsigned bytes, int64_t row, int HW, int t, float* red, bool own_stats, float mu,
                                             float is, float eps, const float* __restrict__ gamma, const float* __restrict__ beta,
                                             int c, int act, float slope, float* __restrict__ mean_out,
                                             float* __restrict__ invstd_out) {
    if constexpr (U > 0) {
        const nrsrc_t rx = n_rsrc(x, bytes), ry = n_rsrc(y, bytes), rr = n_rsrc(res ? res : x, res ? bytes : 0u);
        unsigned off[U];
        row_unit_offsets<LANES, U>(off, row, t, HW);
        float4 a[U], r[U];
#pragma unroll
        for (int j = 0; j < U; ++j) a[j] = n_load4(rx, off[j]);
        if (res) {                                               // uniform; in flight behind x while the statistics are formed
#pragma unroll
            for (int j = 0; j < U; ++j) r[j] = n_load4(rr, off[j]);
        }
        if (own_stats) {
            float s = 0.f;
#pragma unroll
            for (int j = 0; j < U; ++j) s += (a[j].x + a[j].y) + (a[j].z + a[j].w);
            mu = in_reduce<LANES>(s, red) / (float)HW;
            float q = 0.f;
#pragma unroll
            for (int j = 0; j < U; ++j) {
                const float d0 = a[j].x - mu, d1 = a[j].y - mu, d2 = a[j].z - mu, d3 = a[j].w - mu;
                const float e = (d0 * d0 + d1 * d1) + (d2 * d2 + d3 * d3);
                q += off[j] != NOOB ? e : 0.f;
            }
            is = rsqrtf(in_reduce<LANES>(q, red) / (float)HW + eps);
            if (t == 0) {
                *mean_out = mu;
                *invstd_out = is;
            }
        }
        const float gs = (gamma ? gamma[c] : 1.f) * is;
        const float sh = (beta ? beta[c] : 0.f) - mu * gs;
#pragma unroll
        for (int j = 0; j < U; ++j) {
            float4 o;
            o.x = a[j].x * gs + sh; o.y = a[j].y * gs + sh; o.z = a[j].z * gs + sh; o.w = a[j].w * gs + sh;
            if (res) { o.x += r[j].x; o.y += r[j].y; o.z += r[j].z; o.w += r[j].w; }
            o.x = rg_apply_act(o.x, act, slope); o.y = rg_apply_act(o.y, act, slope);
            o.z = rg_apply_act(o.z, act, slope); o.w = rg_apply_act(o.w, act, slope);
            n_store4(ry, off[j], o);
        }
    } else {
        constexpr int T = LANES;
        const float* xp = x + row;
        const bool vec = (HW & 3) == 0;
        const int nv = HW >> 2;
        if (own_stats) {
            float s = 0.f;
            if (vec) {
                for (int i = t; i < nv; i += T) {
                    const float4 v = reinterpret_cast<const float4*>(xp)[i];
                    s += (v.x + v.y) + (v.z + v.w);
                }
            } else {
                for (int i = t; i < HW; i += T) s += xp[i];
            }
            mu = in_reduce<LANES>(s, red) / (float)HW;
            float q = 0.f;
            if (vec) {
                for (int i = t; i < nv; i += T) {
                    const float4 v = reinterpret_cast<const float4*>(xp)[i];
                    const float d0 = v.x - mu, d1 = v.y - mu, d2 = v.z - mu, d3 = v.w - mu;
                    q += (d0 * d0 + d1 * d1) + (d2 * d2 + d3 * d3);
                }
            } else {
                for (int i = t; i < HW; i += T) {
                    const float d = xp[i] - mu;
                    q += d * d;
                }
            }
            is = rsqrtf(in_reduce<LANES>(q, red) / (float)HW + eps);
            if (t == 0) {
                *mean_out = mu;
                *invstd_out = is;
            }
        }
        const float gs = (gamma ? gamma[c] : 1.f) * is;
        const float sh = (beta ? beta[c] : 0.f) - mu * gs;
        float* yp = y + row;
        const float* rp = res ? res + row : nullptr;
        if (vec) {
            for (int i = t; i < nv; i += T) {
                const float4 v = reinterpret_cast<const float4*>(xp)[i];
                float4 o;
                o.x = v.x * gs + sh; o.y = v.y * gs + sh; o.z = v.z * gs + sh; o.w = v.w * gs + sh;
                if (rp) {
                    const float4 r = reinterpret_cast<const float4*>(rp)[i];
                    o.x += r.x; o.y += r.y; o.z += r.z; o.w += r.w;
                }
                o.x = rg_apply_act(o.x, act, slope); o.y = rg_apply_act(o.y, act, slope);
                o.z = rg_apply_act(o.z, act, slope); o.w = rg_apply_act(o.w, act, slope);
                reinterpret_cast<float4*>(yp)[i] = o;
            }
        } else {
            for (int i = t; i < HW; i += T) {
                float o = xp[i] * gs + sh;
                if (rp) o += rp[i];
                yp[i] = rg_apply_act(o, act, slope);
            }
        }
    }
}

// g = dy * act'(y); s1 = sum g, s2 = sum g * xhat; dx = gamma[c] * is * (g - a - (x - mu) * b); dres = g.  `kind` (uniform over the
// lane group) says where a and b come from and whether s1 / s2 are written:
//   IBN_ROW_IN        a = s1 / HW, b = s2 / HW * is from the row's own sums; s1 / s2 written (per instance, for the affine gradients)
//   IBN_ROW_BN_TRAIN  a, b given (the channel sums); nothing written
//   IBN_ROW_BN_EVAL   a = b = 0 given (running statistics: dx needs no sum); s1 / s2 written, gathered in the same pass as dx
// dx, dres and sdx_out (the sum of dx: the bias gradient of a convolution in front) may be NULL.
template <int LANES, int U>
__device__ __forceinline__ void norm_row_bwd(const float* __restrict__ x, const float* __restrict__ dy, const float* __restrict__ yact,
                                             float* __restrict__ dx, float* __restrict__ dres, unsigned bytes, int64_t row, int HW,
                                             int t, float* red, int kind, float mu, float is, float a, float b,
                                             const float* __restrict__ gamma, int c, int act, float slope,
                                             float* __restrict__ s1_out, float* __restrict__ s2_out, float* __restrict__ sdx_out) {
    const bool has_act = act != RG_ACT_NONE;
    float s1 = 0.f, s2 = 0.f, sdx = 0.f;
    if constexpr (U > 0) {
        const nrsrc_t rx = n_rsrc(x, bytes), rg = n_rsrc(dy, bytes), ry = n_rsrc(has_act ? yact : dy, has_act ? bytes : 0u);
        const nrsrc_t rdx = n_rsrc(dx ? dx : dres, dx ? bytes : 0u), rdr = n_rsrc(dres ? dres : dx, dres ? bytes : 0u);
        unsigned off[U];
        row_unit_offsets<LANES, U>(off, row, t, HW);
        float4 g[U], v[U], yv[U];
#pragma unroll
        for (int j = 0; j < U; ++j) {
            g[j] = n_load4(rg, off[j]);
            v[j] = n_load4(rx, off[j]);
            if (has_act) yv[j] = n_load4(ry, off[j]);
        }
#pragma unroll
        for (int j = 0; j < U; ++j) {                            // as the units arrive
            if (has_act) {
                g[j].x *= act_grad_from_out(yv[j].x, act, slope); g[j].y *= act_grad_from_out(yv[j].y, act, slope);
                g[j].z *= act_grad_from_out(yv[j].z, act, slope); g[j].w *= act_grad_from_out(yv[j].w, act, slope);
            }
            if (kind != IBN_ROW_BN_TRAIN) {                      // lanes past the row hold g = 0
                s1 += (g[j].x + g[j].y) + (g[j].z + g[j].w);
                s2 += (g[j].x * (v[j].x - mu) + g[j].y * (v[j].y - mu)) + (g[j].z * (v[j].z - mu) + g[j].w * (v[j].w - mu));
            }
        }
        if (kind != IBN_ROW_BN_TRAIN) {
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
        const float gs = (gamma ? gamma[c] : 1.f) * is;
#pragma unroll
        for (int j = 0; j < U; ++j) {
            if (dres) n_store4(rdr, off[j], g[j]);
            if (dx) {
                float4 o;
                o.x = gs * (g[j].x - a - (v[j].x - mu) * b); o.y = gs * (g[j].y - a - (v[j].y - mu) * b);
                o.z = gs * (g[j].z - a - (v[j].z - mu) * b); o.w = gs * (g[j].w - a - (v[j].w - mu) * b);
                n_store4(rdx, off[j], o);
                sdx += off[j] != NOOB ? (o.x + o.y) + (o.z + o.w) : 0.f;
            }
        }
    } else {
        constexpr int T = LANES;
        const float* xp = x + row;
        const float* gp = dy + row;
        const float* yp = has_act ? yact + row : nullptr;
        float* dxp = dx ? dx + row : nullptr;
        float* drp = dres ? dres + row : nullptr;
        const bool vec = (HW & 3) == 0;
        const int nv = HW >> 2;
        auto grad4 = [&](int i) {
            float4 g = reinterpret_cast<const float4*>(gp)[i];
            if (yp) {
                const float4 yv = reinterpret_cast<const float4*>(yp)[i];
                g.x *= act_grad_from_out(yv.x, act, slope); g.y *= act_grad_from_out(yv.y, act, slope);
                g.z *= act_grad_from_out(yv.z, act, slope); g.w *= act_grad_from_out(yv.w, act, slope);
            }
            return g;
        };
        auto grad1 = [&](int i) { return yp ? gp[i] * act_grad_from_out(yp[i], act, slope) : gp[i]; };
        auto sums4 = [&](int i, const float4& g) {
            const float4 v = reinterpret_cast<const float4*>(xp)[i];
            s1 += (g.x + g.y) + (g.z + g.w);
            s2 += (g.x * (v.x - mu) + g.y * (v.y - mu)) + (g.z * (v.z - mu) + g.w * (v.w - mu));
        };
        auto sums1 = [&](int i, float g) {
            s1 += g;
            s2 += g * (xp[i] - mu);
        };
        auto reduce_sums = [&] {
            s1 = in_reduce<LANES>(s1, red);
            s2 = in_reduce<LANES>(s2, red) * is;
            if (t == 0) {
                *s1_out = s1;
                *s2_out = s2;
            }
        };
        if (kind == IBN_ROW_IN) {
            if (vec) {
                for (int i = t; i < nv; i += T) sums4(i, grad4(i));
            } else {
                for (int i = t; i < HW; i += T) sums1(i, grad1(i));
            }
            reduce_sums();
            a = s1 / (float)HW;
            b = s2 / (float)HW * is;
        }
        const float gs = (gamma ? gamma[c] : 1.f) * is;
        if (vec) {
            for (int i = t; i < nv; i += T) {
                const float4 g = grad4(i);
                if (drp) reinterpret_cast<float4*>(drp)[i] = g;
                if (dxp) {
                    const float4 v = reinterpret_cast<const float4*>(xp)[i];
                    float4 o;
                    o.x = gs * (g.x - a - (v.x - mu) * b); o.y = gs * (g.y - a - (v.y - mu) * b);
                    o.z = gs * (g.z - a - (v.z - mu) * b); o.w = gs * (g.w - a - (v.w - mu) * b);
                    reinterpret_cast<float4*>(dxp)[i] = o;
                    sdx += (o.x + o.y) + (o.z + o.w);
                }
                if (kind == IBN_ROW_BN_EVAL) sums4(i, g);
            }
        } else {
            for (int i = t; i < HW; i += T) {
                const float g = grad1(i);
                if (drp) drp[i] = g;
                if (dxp) {
                    const float o = gs * (g - a - (xp[i] - mu) * b);
                    dxp[i] = o;
                    sdx += o;
                }
                if (kind == IBN_ROW_BN_EVAL) sums1(i, g);
            }
        }
        if (kind == IBN_ROW_BN_EVAL) reduce_sums();
    }
    if (sdx_out) {                                               // uniform
        sdx = in_reduce<LANES>(sdx, red);
        if (t == 0) *sdx_out = sdx;
    }
}

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

// out[c] = sum over n and the pixels of dy[n][c][.] — the bias gradient of a convolution / linear layer — in ONE launch when a
// channel holds at most 32768 values (one workgroup per channel; eight loads in flight per thread; fixed order).  The two-stage
// slice reduction (rg_bn_bwd_reduce on unit statistics) stays for the large maps.
template <bool VEC>
__global__ __launch_bounds__(256) void channel_sum_small_kernel(const float* __restrict__ dy, float* __restrict__ out, int N, int C,
                                                                int HW, unsigned bytes) {
    __shared__ float red[4];
    const int c = blockIdx.x, t = threadIdx.x;
    const int rl = VEC ? HW >> 2 : HW;
    const int total = N * rl;
    const nrsrc_t rg = n_rsrc(dy, bytes);
    float s = 0.f;
    for (int i0 = t; i0 < total; i0 += 256 * 8) {
        unsigned off[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int i = i0 + 256 * j;
            const int n = i / rl, v = i - n * rl;
            off[j] = i < total ? (unsigned)((n * C + c) * HW + (VEC ? 4 * v : v)) * 4u : NOOB;
        }
        if (VEC) {
            float4 a[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) a[j] = n_load4(rg, off[j]);
#pragma unroll
            for (int j = 0; j < 8; ++j) s += (a[j].x + a[j].y) + (a[j].z + a[j].w);
        } else {
            float a[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) a[j] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rg, off[j], 0, 0));
#pragma unroll
            for (int j = 0; j < 8; ++j) s += a[j];
        }
    }
    s = bn_block_sum(s, red);
    if (t == 0) out[c] = s;
}

// units (float4) per thread of the register kernels for this geometry, 0 = use the loop kernels
static int bn_reg_units(int N, int C, int HW) {
    if ((HW & 3) || (int64_t)N * C * HW * 4 >= (1ll << 31)) return 0;
    const int total = N * (HW >> 2);
    const int per = (total + 255) / 256;
    if (per > 16) return 0;
    return per <= 1 ? 1 : per <= 2 ? 2 : per <= 4 ? 4 : per <= 8 ? 8 : 16;
}

// g = dy * act'(y); sum_dy[c] = sum g, sum_dy_xhat[c] = sum g * xhat; dx = gamma * invstd * (g - mean(g) - xhat * mean(g xhat)); dres = g
__device__ __forceinline__ void bn_channel_bwd(const float* __restrict__ x, const float* __restrict__ dy,
                                               const float* __restrict__ yact, const float* __restrict__ mean,
                                               const float* __restrict__ invstd, const float* __restrict__ gamma,
                                               float* __restrict__ dx, float* __restrict__ dres,
                                               float* __restrict__ sum_dy, float* __restrict__ sum_dy_xhat, int N,
                                               int C, int HW, int act, float slope, int c, int sc, float* red) {
    const int t = threadIdx.x;
    const bool vec = (HW & 3) == 0;
    const int rl = vec ? HW >> 2 : HW;
    const int total = N * rl;
    const int64_t cs = (int64_t)C * HW;
    const float cnt = (float)N * (float)HW;
    const float mu = mean[sc], is = invstd[sc];
    const bool has_act = act != RG_ACT_NONE;
    float s1 = 0.f, s2 = 0.f;
    for (int i = t; i < total; i += 256) {
        const int n = i / rl, v = i - n * rl;
        const int64_t off = (int64_t)n * cs + (int64_t)c * HW;
        if (vec) {
            float4 g = reinterpret_cast<const float4*>(dy + off)[v];
            if (has_act) {
                const float4 yv = reinterpret_cast<const float4*>(yact + off)[v];
                g.x *= act_grad_from_out(yv.x, act, slope); g.y *= act_grad_from_out(yv.y, act, slope);
                g.z *= act_grad_from_out(yv.z, act, slope); g.w *= act_grad_from_out(yv.w, act, slope);
            }
            const float4 a = reinterpret_cast<const float4*>(x + off)[v];
            s1 += (g.x + g.y) + (g.z + g.w);
            s2 += (g.x * (a.x - mu) + g.y * (a.y - mu)) + (g.z * (a.z - mu) + g.w * (a.w - mu));
        } else {
            float g = dy[off + v];
            if (has_act) g *= act_grad_from_out(yact[off + v], act, slope);
            s1 += g;
            s2 += g * (x[off + v] - mu);
        }
    }
    s1 = bn_block_sum(s1, red);
    s2 = bn_block_sum(s2, red) * is;
    if (t == 0) {
        sum_dy[sc] = s1;
        sum_dy_xhat[sc] = s2;
    }
    if (!dx && !dres) return;
    const float gs = (gamma ? gamma[sc] : 1.f) * is;
    const float a0 = s1 / cnt, b0 = s2 / cnt * is;
    for (int i = t; i < total; i += 256) {
        const int n = i / rl, v = i - n * rl;
        const int64_t off = (int64_t)n * cs + (int64_t)c * HW;
        if (vec) {
            float4 g = reinterpret_cast<const float4*>(dy + off)[v];
            if (has_act) {
                const float4 yv = reinterpret_cast<const float4*>(yact + off)[v];
                g.x *= act_grad_from_out(yv.x, act, slope); g.y *= act_grad_from_out(yv.y, act, slope);
                g.z *= act_grad_from_out(yv.z, act, slope); g.w *= act_grad_from_out(yv.w, act, slope);
            }
            if (dres) reinterpret_cast<float4*>(dres + off)[v] = g;
            if (dx) {
                const float4 a = reinterpret_cast<const float4*>(x + off)[v];
                float4 o;
                o.x = gs * (g.x - a0 - (a.x - mu) * b0); o.y = gs * (g.y - a0 - (a.y - mu) * b0);
                o.z = gs * (g.z - a0 - (a.z - mu) * b0); o.w = gs * (g.w - a0 - (a.w - mu) * b0);
                reinterpret_cast<float4*>(dx + off)[v] = o;
            }
        } else {
            float g = dy[off + v];
            if (has_act) g *= act_grad_from_out(yact[off + v], act, slope);
            if (dres) dres[off + v] = g;
            if (dx) dx[off + v] = gs * (g - a0 - (x[off + v] - mu) * b0);
        }
    }
}

template <class... DS>
__global__ __launch_bounds__(256) void bn_train_bwd_fused_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                                 const float* __restrict__ yact, const float* __restrict__ mean,
                                                                 const float* __restrict__ invstd, const float* __restrict__ gamma,
                                                                 float* __restrict__ dx, float* __restrict__ dres,
                                                                 float* __restrict__ sum_dy, float* __restrict__ sum_dy_xhat, int N,
                                                                 int C, int HW, int act, float slope, DS... ds) {
    if constexpr (sizeof...(DS) > 0) {                 // the two-domain layer: this plane's half, statistics row and parameter set
        const int d = blockIdx.y;
        const auto& a = dsbn_arg(ds...);
        const int64_t o = (int64_t)d * N * C * HW;
        x += o, dy += o, mean += d * C, invstd += d * C;
        if (yact) yact += o;
        if (dx) dx += o;
        if (dres) dres += o;
        gamma = d ? a.gamma[1] : a.gamma[0];
        sum_dy = d ? a.d_beta[1] : a.d_beta[0], sum_dy_xhat = d ? a.d_gamma[1] : a.d_gamma[0];
    }
    __shared__ float red[4];
    bn_channel_bwd(x, dy, yact, mean, invstd, gamma, dx, dres, sum_dy, sum_dy_xhat, N, C, HW, act, slope, (int)blockIdx.x,
                   (int)blockIdx.x, red);
}

// out_a[c] = sum_n a[n][c], out_b[c] = sum_n b[n][c] (fixed summation order): the affine gradients of an InstanceNorm from the per-(n,c) sums
// its backward reduction already produced.  Either pair may be NULL.
// Columns [split, C) go to oa2 / ob2 (the BatchNorm half of an IBN layer); split = C: one output pair.
__global__ __launch_bounds__(256) void rows_sum_pair_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                            float* __restrict__ oa, float* __restrict__ ob, int N, int C,
                                                            int split, float* __restrict__ oa2, float* __restrict__ ob2) {
    // 16 channels x 16 row lanes per workgroup: lane ny sums rows ny, ny + 16, ...; the 16 lane sums are added in lane order
    __shared__ float sa[16][17], sb[16][17];
    const int cx = threadIdx.x & 15, ny = threadIdx.x >> 4;
    const int c = blockIdx.x * 16 + cx;
    float x = 0.f, y = 0.f;
    if (c < C) {
        for (int n = ny; n < N; n += 16) {
            if (a) x += a[(int64_t)n * C + c];
            if (b) y += b[(int64_t)n * C + c];
        }
    }
    sa[ny][cx] = x;
    sb[ny][cx] = y;
    __syncthreads();
    if (ny == 0 && c < C) {
        float ta = 0.f, tb = 0.f;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            ta += sa[i][cx];
            tb += sb[i][cx];
        }
        if (c < split) {
            if (a) oa[c] = ta;
            if (b) ob[c] = tb;
        } else {
            if (a) oa2[c - split] = ta;
            if (b) ob2[c - split] = tb;
        }
    }
}

// 1 when rg_channel_sum runs as one launch for this geometry (else use rg_bn_bwd_reduce on unit statistics)
extern "C" size_t rg_channel_sum_ok(int N, int C, int HW) {
    return (int64_t)N * HW <= 32768 && (int64_t)N * C * HW * 4 < (1ll << 31) ? 1 : 0;
}

extern "C" int rg_channel_sum(const float* dy, float* out, int N, int C, int HW, hipStream_t stream) {
    RG_REQUIRE(dy && out && N > 0 && C > 0 && HW > 0, "rg_channel_sum: bad arguments");
    RG_REQUIRE(rg_channel_sum_ok(N, C, HW), "rg_channel_sum: %d x %d values per channel need the two-stage reduction", N, HW);
    rg::ProfScope prof(rg::FAM_NORM, stream, 0.0, 4.0 * N * (double)C * HW);
    const unsigned bytes = (unsigned)((int64_t)N * C * HW * 4);
    if ((HW & 3) == 0)
        hipLaunchKernelGGL(channel_sum_small_kernel<true>, dim3(C), dim3(256), 0, stream, dy, out, N, C, HW, bytes);
    else
        hipLaunchKernelGGL(channel_sum_small_kernel<false>, dim3(C), dim3(256), 0, stream, dy, out, N, C, HW, bytes);
    return rg::check_launch("rg_channel_sum");
}

extern "C" int rg_rows_sum_pair(const float* a, const float* b, float* out_a, float* out_b, int N, int C,
                                hipStream_t stream) {
    RG_REQUIRE((a || b) && (!a || out_a) && (!b || out_b) && N > 0 && C > 0, "rg_rows_sum_pair: bad arguments");
    rg::ProfScope prof(rg::FAM_NORM, stream, 0.0, 4.0 * ((a ? 1 : 0) + (b ? 1 : 0)) * (double)(N + 1) * C);
    hipLaunchKernelGGL(rows_sum_pair_kernel, dim3(rg::cdiv(C, 16)), dim3(256), 0, stream, a, b, out_a, out_b, N, C,
                       C, nullptr, nullptr);
    return rg::check_launch("rg_rows_sum_pair");
}

// Train-mode BatchNorm, one launch per direction (see the kernels): rg_bn_train_fused_ok says whether the geometry qualifies;
// otherwise use rg_bn_stats + rg_bn_apply_fwd / rg_bn_bwd_reduce + rg_bn_bwd_apply.
// development switch: RG_BN_REG=0 keeps the loop kernels (A/B timing)
static const bool g_bn_reg = rg::env_int("RG_BN_REG", 1) != 0;

// The templated kernels exist for fixed lists of (lanes per row, float4 per lane) pairs; units = 0 are the loop kernels.
// with_lanes_units finds the runtime pair in a list and calls f with it as two std::integral_constant; false: not in the list.
template <int L, int U>
struct LU {};
template <class... P>
struct LUList {};
using BnUnits = LUList<LU<256, 1>, LU<256, 2>, LU<256, 4>, LU<256, 8>, LU<256, 16>>;      // one workgroup per channel
using InPairs = LUList<LU<16, 0>, LU<16, 1>, LU<16, 2>, LU<32, 0>, LU<32, 1>, LU<32, 2>, LU<64, 0>, LU<64, 1>, LU<64, 2>, LU<64, 4>,
                       LU<64, 8>, LU<256, 0>, LU<256, 1>, LU<256, 2>, LU<256, 4>, LU<256, 8>>;
using IbnPairs = LUList<LU<16, 0>, LU<16, 2>, LU<32, 0>, LU<32, 2>, LU<64, 0>, LU<64, 2>, LU<64, 8>, LU<256, 0>, LU<256, 8>>;

template <class F, int... L, int... U>
static bool with_lanes_units(LUList<LU<L, U>...>, int lanes, int units, F&& f) {
    return ((lanes == L && units == U && (f(std::integral_constant<int, L>{}, std::integral_constant<int, U>{}), true)) || ...);
}

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

// lanes per instance: at least ~2 load units (float4 when HW % 4 == 0) per lane, one workgroup above 2048 elements
static int in_lanes(int HW) {
    if (HW > 2048) return 256;
    const int units = (HW & 3) ? HW : HW >> 2;
    if (units <= 32) return 16;
    if (units <= 64) return 32;
    return 64;
}

// float4 per lane (1, 2, 4, 8) of the register rows for a tensor of `elems` floats, 0 = the loop rows
static int row_reg_units(int HW, int lanes, int64_t elems) {
    if (!g_bn_reg || (HW & 3) || elems * 4 >= (1ll << 31)) return 0;
    const int per = ((HW >> 2) + lanes - 1) / lanes;
    return per <= 1 ? 1 : per <= 2 ? 2 : per <= 4 ? 4 : per <= 8 ? 8 : 0;
}

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
    hipLaunchKernelGGL(bn_bwd_apply_kernel, dim3(grid_for((HW & 3) ? total : total / 4)), dim3(256), 0, stream, x, dy,
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

// ---- entry points of the conv + frozen-BatchNorm fold (see the kernel comments above) ------------------------
extern "C" int rg_bn_fold(const float* gamma, const float* beta, const float* running_mean, const float* running_var,
                          float eps, float* scale, float* shift, float* invstd, int C, hipStream_t stream) {
    RG_REQUIRE(running_mean && running_var && scale && shift && invstd && C > 0, "rg_bn_fold: bad arguments");
    hipLaunchKernelGGL(bn_fold_kernel, dim3(rg::cdiv(C, 256)), dim3(256), 0, stream, gamma, beta, running_mean, running_var,
                       eps, scale, shift, invstd, C);
    return rg::check_launch("rg_bn_fold");
}

extern "C" int rg_act_bwd_sum(const float* dy, const float* y_act, float* g, float* sum_g, int N, int C, int HW, int act,
                              float slope, void* workspace, size_t workspace_bytes, hipStream_t stream) {
    RG_REQUIRE(dy && (g || sum_g) && N > 0 && C > 0 && HW > 0, "rg_act_bwd_sum: bad arguments");
    RG_REQUIRE(act == RG_ACT_NONE || y_act, "rg_act_bwd_sum: the activation gradient needs the forward output");
    int L;
    const int S = pick_slices(N, C, HW, &L);
    if (sum_g && (!workspace || workspace_bytes < (size_t)C * S * sizeof(float))) {
        rg::set_error("rg_act_bwd_sum: workspace too small");
        return RG_ERR_WORKSPACE;
    }
    const double el = (double)N * C * HW;
    rg::ProfScope prof(rg::FAM_NORM, stream, 0.0, 4.0 * el * (1.0 + (act != RG_ACT_NONE ? 1.0 : 0.0) + (g ? 1.0 : 0.0)));
    float* part = static_cast<float*>(workspace);
    hipLaunchKernelGGL(act_bwd_sum_kernel, dim3(S, C), dim3(256), 0, stream, dy, y_act, g, part, N, C, HW, L, act, slope,
                       sum_g ? 1 : 0);
    if (sum_g) hipLaunchKernelGGL(sum_slices_kernel, dim3(rg::cdiv(C, 64)), dim3(64), 0, stream, part, C, S, sum_g);
    return rg::check_launch("rg_act_bwd_sum");
}

extern "C" int rg_bn_fold_wgrad(const float* w, float* g, const float* scale, const float* invstd, const float* running_mean,
                                const float* sum_g, const float* partials, int n_slices, float* dbeta, float* dgamma, int K,
                                int M, hipStream_t stream) {
    RG_REQUIRE(w && g && scale && K > 0 && M > 0, "rg_bn_fold_wgrad: bad arguments");
    RG_REQUIRE(!dgamma || (invstd && running_mean && (sum_g || partials)), "rg_bn_fold_wgrad: dgamma needs invstd, mean and the sums");
    RG_REQUIRE(!partials || n_slices > 0, "rg_bn_fold_wgrad: partials need their slice count");
    rg::ProfScope prof(rg::FAM_NORM, stream, 0.0, 12.0 * K * (double)M);
    hipLaunchKernelGGL(bn_fold_wgrad_kernel, dim3(K), dim3(256), 0, stream, w, g, scale, invstd, running_mean, sum_g, partials,
                       n_slices, dbeta, dgamma, M);
    return rg::check_launch("rg_bn_fold_wgrad");
}

// slice partials only (no finalize launch): part[C][rg_bn_slices(N, C, HW)], consumed by rg_bn_fold_wgrad
extern "C" int rg_bn_slices(int N, int C, int HW) {
    int L;
    return pick_slices(N, C, HW, &L);
}

extern "C" int rg_act_bwd_partial(const float* dy, const float* y_act, float* g, float* part, int N, int C, int HW, int act,
                                  float slope, hipStream_t stream) {
    RG_REQUIRE(dy && part && N > 0 && C > 0 && HW > 0, "rg_act_bwd_partial: bad arguments");
    RG_REQUIRE(act == RG_ACT_NONE || y_act, "rg_act_bwd_partial: the activation gradient needs the forward output");
    int L;
    const int S = pick_slices(N, C, HW, &L);
    const double el = (double)N * C * HW;
    rg::ProfScope prof(rg::FAM_NORM, stream, 0.0, 4.0 * el * (1.0 + (act != RG_ACT_NONE ? 1.0 : 0.0) + (g ? 1.0 : 0.0)));
    hipLaunchKernelGGL(act_bwd_sum_kernel, dim3(S, C), dim3(256), 0, stream, dy, y_act, g, part, N, C, HW, L, act, slope, 1);
    return rg::check_launch("rg_act_bwd_partial");
}

extern "C" int rg_scale_rows(const float* w, const float* scale, float* out, int K, int M, hipStream_t stream) {
    RG_REQUIRE(w && scale && out && K > 0 && M > 0, "rg_scale_rows: bad arguments");
    const int64_t total = (int64_t)K * M;
    rg::ProfScope prof(rg::FAM_MISC, stream, 0.0, 8.0 * total);
    hipLaunchKernelGGL(scale_rows_kernel, dim3(grid_for(total)), dim3(256), 0, stream, w, scale, out, M, total);
    return rg::check_launch("rg_scale_rows");
}

extern "C" int rg_fold_filters_multi(const void* table, int n_pairs, int total_blocks, hipStream_t stream) {
    RG_REQUIRE(table && n_pairs > 0 && total_blocks > 0, "rg_fold_filters_multi: bad arguments");
    rg::ProfScope prof(rg::FAM_MISC, stream, 0.0, 12.0 * (double)total_blocks * FOLD_CHUNK);
    hipLaunchKernelGGL(fold_filters_multi_kernel, dim3(total_blocks), dim3(256), 0, stream,
                       static_cast<const long long*>(table), n_pairs);
    return rg::check_launch("rg_fold_filters_multi");
}

extern "C" int rg_fold_chunk(void) { return FOLD_CHUNK; }

// ---- IBN-a: InstanceNorm on channels [0, half), BatchNorm on [half, C) of ONE [N][C][HW] tensor -------------------------------
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

static bool ibn_train_fused(int N, int HW) { return (int64_t)N * HW <= 16384; }

// float4 per lane of the register rows for this tensor (2 or 8), 0 = the loop rows
static int ibn_reg_units(int N, int C, int HW) {
    const int units = row_reg_units(HW, in_lanes(HW), (int64_t)N * C * HW);
    return units == 0 ? 0 : units <= 2 ? 2 : 8;
}

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
        hipLaunchKernelGGL(bn_stats_partial_kernel, dim3(S, cb), dim3(256), 0, stream, x + (int64_t)half * HW, part, N, C, HW, L);
        hipLaunchKernelGGL(bn_stats_finalize_kernel, dim3(rg::cdiv(cb, 64)), dim3(64), 0, stream, part, cb, S, bn_eps, momentum, bn_mean,
                           bn_invstd, running_mean, running_var);
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
        hipLaunchKernelGGL(bn_bwd_reduce_partial_kernel, dim3(S, cb), dim3(256), 0, stream, x + off, dy + off,
                           y_act ? y_act + off : nullptr, bn_mean, bn_stat, part, N, C, HW, L, 0, bn_eps, act, 0.f);
        hipLaunchKernelGGL(bn_bwd_reduce_finalize_kernel, dim3(rg::cdiv(cb, 64)), dim3(64), 0, stream, part, cb, S, d_bn_beta,
                           d_bn_gamma);
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
        hipLaunchKernelGGL(rows_sum_pair_kernel, dim3(rg::cdiv(half, 16)), dim3(256), 0, stream, row_s1, row_s2, d_in_beta, d_in_gamma, N,
                           half, half, nullptr, nullptr);
    else
        hipLaunchKernelGGL(rows_sum_pair_kernel, dim3(rg::cdiv(C, 16)), dim3(256), 0, stream, row_s1, row_s2, d_in_beta, d_in_gamma, N,
                           C, half, d_bn_beta, d_bn_gamma);
    return rg::check_launch("rg_ibn_bwd");
}

// ---- domain-specific BatchNorm: entry points ----------------------------------------------------------------------------------------
// Regime by the per-domain extent h*HW alone, h = N / 2: one launch per direction (2C workgroups) when h*HW <= 16384; otherwise slice
// partial + finalize + apply over both domains at once — three launches, as ONE BatchNorm.  No channel threshold as in
// rg_bn_train_fused_ok: the two-pass statistics of the one-launch kernels do not depend on how many values a thread is left with,
// while the slice kernels at a handful of values per thread merge single-value statistics and lose accuracy when |mean| >> std.
// (Whether three launches would be faster for few channels at the largest such extent, e.g. C = 64 on 128 workgroups, is not measured.)

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

// float4 units per thread the one-workgroup-per-channel kernels run with for N samples (what rg_bn_train_*_fused and, with N / 2,
// rg_dsbn_* launch): 1, 2, 4, 8, 16 = the register kernels, 0 = the loop kernels (scalar rows, more than 16 units, or RG_BN_REG=0)
extern "C" int rg_bn_reg_units(int N, int C, int HW) { return g_bn_reg && N > 0 && C > 0 && HW > 0 ? bn_reg_units(N, C, HW) : 0; }

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
    hipLaunchKernelGGL(bn_apply_fwd_kernel, dim3(grid_for((HW & 3) ? half_total : half_total / 4), 2), dim3(256), 0, stream, x,
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
        hipLaunchKernelGGL(bn_bwd_apply_kernel, dim3(grid_for((HW & 3) ? half_total : half_total / 4), 2), dim3(256), 0, stream, x, dy,
                           y_act, mean, invstd, no, no, no, dx, dres, half_total, C, HW, 1.f / (float)((int64_t)h * HW), 1, 0, 0.f, act,
                           slope, a);
    return rg::check_launch("rg_dsbn_bwd");
}
