// The BatchNorm kernels: slice-parallel (partial + finalize + apply), one launch per direction in a loop form and a register
// form.  Every train-mode kernel ends in the parameter pack `DS... ds`, so this header serves the BatchNorm (norm_bn.hip), the
// two-domain layer (norm_dsbn.hip) and, through bn_channel_fwd / bn_channel_bwd, the IBN layer (norm_ibn.hip).  A unit compiles
// the instantiations it launches; the plain-BatchNorm slice instantiations that norm_ibn.hip needs as well are compiled in
// norm_bn.hip alone and reached through the rg::bn_launch_* functions at the end.
#pragma once
#include "norm_core.h"

namespace {

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

// ---- train-mode BatchNorm in one launch per direction, small per-channel extents ----------------------------------------------
// One workgroup per channel: its N rows of HW floats (stride C*HW) are <= 64 KB, so passes two and three hit L1 / L2.  Used when
// N*HW <= 16384 and the channel count alone fills the chip (layer3 / layer4 of the ResNets, the inner generator layers); the
// slice-parallel kernels above stay for the large maps.  Statistics as bn_stats (biased variance for the normalisation, unbiased
// for running_var), two-pass.

// `c` is the channel of the tensor, `sc` the index of its statistics / affine parameters (the same number for a BatchNorm; the
// channel-split IBN layer of norm_ibn.hip normalises channels [half, C) with parameters [0, C - half))
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

// ---- the same two kernels for maps whose rows are float4 multiples, with the loads taken out of the loops ---------------------------
// One workgroup per channel holds N*HW <= 16384 values = at most 16 float4 per thread.  The loops above issue one load per
// iteration behind an integer division and wait for it: with two workgroups per CU nothing hides that latency (a [32, 512, 16 x 8]
// layer: 15 us forward, 1 TB/s).  Here every thread computes its U offsets once (buffer resource over the tensor: offsets past
// the end return zeros / drop the store, so there are no bounds branches) and issues its loads together:
//   forward   x (and the residual) are loaded ONCE into registers; mean, centred sum of squares and the output come from them;
//   backward  two sweeps (the sums, then dx / dres) of U float4 per operand, eight units in flight per sweep.
// Same per-thread summation order and block reduction as the loop kernels: same statistics.
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

// units (float4) per thread of the register kernels for this geometry, 0 = use the loop kernels
static int bn_reg_units(int N, int C, int HW) {
    if ((HW & 3) || (int64_t)N * C * HW * 4 >= (1ll << 31)) return 0;
    const int total = N * (HW >> 2);
    const int per = (total + 255) / 256;
    if (per > 16) return 0;
    return per <= 1 ? 1 : per <= 2 ? 2 : per <= 4 ? 4 : per <= 8 ? 8 : 16;
}

using BnUnits = LUList<LU<256, 1>, LU<256, 2>, LU<256, 4>, LU<256, 8>, LU<256, 16>>;      // one workgroup per channel

}  // namespace

namespace rg {

// The slice kernels of a plain BatchNorm (empty DS pack), compiled in norm_bn.hip only.  `Cn` channels are reduced, `C` is the
// channel stride of a sample (Cn = C for a BatchNorm; the IBN layer runs them over the channel sub-range [half, C) of its tensor);
// S, L from pick_slices(N, Cn, HW).  bn_launch_stats: partial + finalize; bn_launch_bwd_reduce: partial + finalize.
void bn_launch_stats(const float* x, float* part, int N, int Cn, int C, int HW, int S, int L, float eps, float momentum, float* mean,
                     float* invstd, float* running_mean, float* running_var, hipStream_t stream);
void bn_launch_bwd_reduce(const float* x, const float* dy, const float* yact, const float* mean, const float* stat, float* part,
                          int N, int Cn, int C, int HW, int S, int L, int stat_is_var, float eps, int act, float slope,
                          float* sum_dy, float* sum_dy_xhat, hipStream_t stream);

}  // namespace rg
