// The row bodies: one row of HW contiguous floats normalised by a lane group.  norm_instnorm.hip and norm_ibn.hip build their
// kernels on them.
#pragma once
#include "norm_core.h"

namespace {

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
    if constexpr (LANES > 64) {
        return bn_block_sum(v, red);
    } else {
#pragma unroll
        for (int off = LANES / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
        return v;
    }
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

}  // namespace
