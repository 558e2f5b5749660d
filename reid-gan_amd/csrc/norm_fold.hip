// The conv + frozen-statistics BatchNorm fold and the generic per-channel sums for gfx950: what the convolution library and the
// bias gradients take from the normalisation family (booked under FAM_NORM / FAM_MISC as before).
#include "norm_core.h"

namespace {

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

}  // namespace

void rg::launch_rows_sum_pair(const float* a, const float* b, float* oa, float* ob, int N, int C, int split, float* oa2, float* ob2,
                              hipStream_t stream) {
    hipLaunchKernelGGL(rows_sum_pair_kernel, dim3(rg::cdiv(C, 16)), dim3(256), 0, stream, a, b, oa, ob, N, C, split, oa2, ob2);
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
    rg::launch_rows_sum_pair(a, b, out_a, out_b, N, C, C, nullptr, nullptr, stream);
    return rg::check_launch("rg_rows_sum_pair");
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
    hipLaunchKernelGGL(scale_rows_kernel, dim3(rg::grid_for(total, NORM_GRID_CAP)), dim3(256), 0, stream, w, scale, out, M, total);
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
