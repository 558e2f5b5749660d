// Second stage of FD-GAN's cascade evaluation (FD/reid/evaluators.py:19-43 and :198-227) on the device:
//   rg_pair_score      the eval-mode verification head (FD/reid/models/embedding.py:7-39) of every query against the k gallery rows
//                      its first-stage ranking lists, gathered by index: no [Q * k][D] operand exists
//   rg_cascade_merge   "merge two-stage distances" (:218-226) in place on the [Q][G] matrix
//
// rg_pair_score, pair (q, j) with g = gallery[idx[q][j]]:
//   d = (probe_q - g)^2,  z = gamma (d - running_mean) rsqrt(running_var + eps) + beta,  logits[c] = sum_ch z[ch] W[c][ch] + bias[c]
// evaluated as  logits[c] = sum_ch t_c[ch] (d[ch] - running_mean[ch]) + K_c  with the per-channel constants folded:
// a = gamma rsqrt(running_var + eps) and t_c = W_c a once per D-chunk (shared by the rows in flight), K_c = sum_ch beta[ch] W[c][ch]
// + bias[c] once per workgroup.  The mean is subtracted from d BEFORE the scaling (the expanded form A d + b cancels on a channel
// whose mean is large against its spread), and the square is never expanded into GEMM terms.
//
// Work shape (a gather of whole rows): a workgroup of 4 waves serves one query and a slice of its k pairs; a wave owns kRows = 4
// gallery rows at a time and walks D in chunks of 64 lanes x 16 bytes, so 4 row loads per lane are in flight beside the probe
// chunk, which is loaded once per chunk and reused by the 4 rows, as are the coefficients.  Per pair and class the lanes' sums
// meet in one butterfly and lane 0 writes.  A pair's sum is made by ONE wave in an order that depends on D alone (lane-serial over
// the chunks, then the butterfly), so the bits do not depend on the grid, on the slice a pair falls in or on how the caller chunks
// the queries.  No atomics.
// The per-channel vectors (running_mean, gamma, running_var, W) come through the cache: staging running_mean and t_c in LDS once
// per workgroup was built and measured 6 % SLOWER at Market-1501 size (504 against 475 us at k = 100, D 2048, 2 classes: 24 KB of
// LDS per workgroup cost more occupancy than the L2 hits cost time), so that regime was removed.
// Regimes (rg_pair_score_regime):
//   vector / scalar 16-byte loads when D is a multiple of 4 and probe / gallery are 16-byte aligned, else 4-byte loads
//   split          Q below the CU count: k is split over several workgroups per query so that the chip is not idle
//
// rg_cascade_merge, row q with S = the columns idx[q][:], float32 operations in this order:
//   nxt = min_{j not in S} dist[q][j] (first-stage values), bar = max_j score[q][j], gap = max((bar + 1) - nxt, 0),
//   dist[q][idx[q][j]] = score[q][j],  dist[q][j] += gap for j not in S when gap > 0;  k == G: the overwrite alone.
// One workgroup per row; membership in S is a bitmap of G bits in LDS built from idx (integer LDS atomics only).
#include "rg_common.h"

namespace {

constexpr int kMaxC = 16;               // classes
constexpr int kMaxD = 8192;
constexpr int kRows = 4;                // gallery rows a wave keeps in flight
constexpr int kWaves = 4;               // waves per workgroup
constexpr int kSlicePairs = kRows * kWaves;
constexpr int kNumCU = 256;
constexpr int kMaxG = 1 << 20;          // bitmap of the merge: 128 KB of LDS

// V consecutive floats of a row (V = 4: one 16-byte load); zero beyond D or for a row that is not read
template <int V>
__device__ __forceinline__ void ps_load(const float* __restrict__ p, int ch, int D, bool on, float (&v)[V]) {
    if constexpr (V == 4) {
        float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
        if (on && ch < D) t = *reinterpret_cast<const float4*>(p + ch);              // D % 4 == 0: the vector lies inside the row
        v[0] = t.x, v[1] = t.y, v[2] = t.z, v[3] = t.w;
    } else {
#pragma unroll
        for (int i = 0; i < V; ++i) v[i] = (on && ch + i < D) ? p[ch + i] : 0.f;
    }
}

__device__ __forceinline__ float ps_coef_a(float gamma, float rv, float eps) { return gamma * rsqrtf(rv + eps); }

// CT: compile-time bound of the classes (C <= CT); V: floats per lane and chunk
template <int CT, int V>
__global__ __launch_bounds__(256) void pair_score_kernel(const float* __restrict__ probe, const float* __restrict__ gallery,
                                                         const int* __restrict__ idx, const float* __restrict__ gamma,
                                                         const float* __restrict__ beta, const float* __restrict__ rm,
                                                         const float* __restrict__ rv, const float* __restrict__ W,
                                                         const float* __restrict__ bias, float* __restrict__ logits,
                                                         float* __restrict__ score, int G, int k, int D, int C, float eps,
                                                         int pairs_per_wg) {
    __shared__ float red[16];
    __shared__ float kc[kMaxC];
    constexpr int kChunk = 64 * V;
    const int Dp = (D + kChunk - 1) / kChunk * kChunk;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int q = blockIdx.y;
    // ---- prologue: the per-class constants, the same values in every workgroup
    for (int c = 0; c < C; ++c) {
        float s = 0.f;
        for (int ch = tid; ch < D; ch += 256) s = fmaf(beta[ch], W[(int64_t)c * D + ch], s);
        s = rg_block_sum(s, red);
        if (tid == 0) kc[c] = s + (bias ? bias[c] : 0.f);
    }
    __syncthreads();
    const int j0 = blockIdx.x * pairs_per_wg, j1 = min(k, j0 + pairs_per_wg);
    const float* pq = probe + (int64_t)q * D;
    for (int jb = j0 + wave * kRows; jb < j1; jb += kSlicePairs) {                  // wave-uniform
        int gi[kRows];
        bool on[kRows];
        const float* gp[kRows];
#pragma unroll
        for (int r = 0; r < kRows; ++r) {
            const int j = jb + r;
            gi[r] = j < j1 ? idx[(int64_t)q * k + j] : -1;
            on[r] = gi[r] >= 0 && gi[r] < G;                                        // an index outside [0, G): nothing is read
            gp[r] = gallery + (int64_t)(on[r] ? gi[r] : 0) * D;
        }
        float acc[kRows][CT];
#pragma unroll
        for (int r = 0; r < kRows; ++r)
#pragma unroll
            for (int c = 0; c < CT; ++c) acc[r][c] = 0.f;
        for (int c0 = 0; c0 < Dp; c0 += kChunk) {
            const int ch = c0 + lane * V;
            float p[V], m[V], a[V], g4[V], v4[V], e[kRows][V];
            ps_load<V>(pq, ch, D, true, p);
#pragma unroll
            for (int r = 0; r < kRows; ++r) ps_load<V>(gp[r], ch, D, on[r], e[r]);
            ps_load<V>(rm, ch, D, true, m);
            ps_load<V>(gamma, ch, D, true, g4);
            ps_load<V>(rv, ch, D, true, v4);
#pragma unroll
            for (int i = 0; i < V; ++i) a[i] = ch + i < D ? ps_coef_a(g4[i], v4[i], eps) : 0.f;      // beyond D: t = 0, nothing is added
#pragma unroll
            for (int r = 0; r < kRows; ++r)
#pragma unroll
                for (int i = 0; i < V; ++i) {
                    const float t = p[i] - e[r][i];
                    e[r][i] = t * t - m[i];                                         // the mean leaves d before any scaling
                }
#pragma unroll
            for (int c = 0; c < CT; ++c)
                if (c < C) {                                                        // uniform over the grid
                    float t[V];
                    ps_load<V>(W + (int64_t)c * D, ch, D, true, t);
#pragma unroll
                    for (int i = 0; i < V; ++i) t[i] *= a[i];
#pragma unroll
                    for (int r = 0; r < kRows; ++r)
#pragma unroll
                        for (int i = 0; i < V; ++i) acc[r][c] = fmaf(t[i], e[r][i], acc[r][c]);
                }
        }
#pragma unroll
        for (int r = 0; r < kRows; ++r) {
            float l[CT];
#pragma unroll
            for (int c = 0; c < CT; ++c) l[c] = c < C ? rg_wave_sum(acc[r][c]) + kc[c] : -INFINITY;
            const int j = jb + r;
            if (lane == 0 && j < j1) {
                const int64_t o = (int64_t)q * k + j;
                const float bad = __builtin_nanf("");
                if (logits) {
#pragma unroll
                    for (int c = 0; c < CT; ++c)
                        if (c < C) logits[o * C + c] = on[r] ? l[c] : bad;
                }
                if (score) {
                    float mx = l[0];
#pragma unroll
                    for (int c = 1; c < CT; ++c) mx = fmaxf(mx, l[c]);
                    float se = 0.f;
#pragma unroll
                    for (int c = 0; c < CT; ++c)
                        if (c < C) se += expf(l[c] - mx);
                    score[o] = on[r] ? expf(l[0] - mx) / se : bad;                 // softmax(logits)[0]; exactly 1 for C == 1
                }
            }
        }
    }
}

struct PairPlan {
    int vec, split, wgs_x, pairs_per_wg;
};

PairPlan pair_plan(int Q, int k, int D, int C, int aligned) {
    PairPlan p;
    p.vec = (D % 4 == 0 && aligned) ? 1 : 0;
    // Q below the CU count: slices of k, whole groups of the 4 rows a wave holds, until about two workgroups per CU exist
    int s = 1;
    if (Q < kNumCU) s = min(rg::cdiv(k, kRows), rg::cdiv(2 * kNumCU, Q));
    p.pairs_per_wg = rg::cdiv(rg::cdiv(k, s), kRows) * kRows;
    p.wgs_x = rg::cdiv(k, p.pairs_per_wg);
    p.split = p.wgs_x > 1 ? 1 : 0;
    return p;
}

template <int CT>
void pair_launch(const PairPlan& p, dim3 grid, hipStream_t stream, const float* probe, const float* gallery, const int* idx,
                 const float* gamma, const float* beta, const float* rm, const float* rv, const float* W, const float* bias,
                 float* logits, float* score, int G, int k, int D, int C, float eps) {
    if (p.vec)
        hipLaunchKernelGGL((pair_score_kernel<CT, 4>), grid, dim3(256), 0, stream, probe, gallery, idx, gamma, beta, rm, rv, W, bias,
                           logits, score, G, k, D, C, eps, p.pairs_per_wg);
    else
        hipLaunchKernelGGL((pair_score_kernel<CT, 1>), grid, dim3(256), 0, stream, probe, gallery, idx, gamma, beta, rm, rv, W, bias,
                           logits, score, G, k, D, C, eps, p.pairs_per_wg);
}

__device__ __forceinline__ float cm_block_min(float v, float* red) { return -rg_block_max(-v, red); }

__global__ __launch_bounds__(256) void cascade_merge_kernel(float* __restrict__ dist, int64_t ld, const int* __restrict__ idx,
                                                            const float* __restrict__ score, int G, int k) {
    extern __shared__ unsigned bits[];              // G bits: column j is in S
    __shared__ float red[16];
    const int q = blockIdx.x, tid = threadIdx.x;
    float* row = dist + (int64_t)q * ld;
    const int* iq = idx + (int64_t)q * k;
    const float* sq = score + (int64_t)q * k;
    if (k >= G) {                                                                   // uniform: the overwrite alone
        for (int j = tid; j < k; j += 256) {
            const int c = iq[j];
            if (c >= 0 && c < G) row[c] = sq[j];
        }
        return;
    }
    const int words = (G + 31) >> 5;
    for (int w = tid; w < words; w += 256) bits[w] = 0u;
    __syncthreads();
    float bar = -INFINITY;
    for (int j = tid; j < k; j += 256) {
        const int c = iq[j];
        if (c >= 0 && c < G) atomicOr(&bits[c >> 5], 1u << (c & 31));
        bar = fmaxf(bar, sq[j]);
    }
    bar = rg_block_max(bar, red);                                                   // its barriers also publish the bitmap
    float nxt = INFINITY;
    for (int j = tid; j < G; j += 256)
        if (!((bits[j >> 5] >> (j & 31)) & 1u)) nxt = fminf(nxt, row[j]);
    nxt = cm_block_min(nxt, red);                                                   // every first-stage value is read before any write
    const float gap = fmaxf((bar + 1.f) - nxt, 0.f);
    if (gap > 0.f)
        for (int j = tid; j < G; j += 256)
            if (!((bits[j >> 5] >> (j & 31)) & 1u)) row[j] += gap;
    for (int j = tid; j < k; j += 256) {
        const int c = iq[j];
        if (c >= 0 && c < G) row[c] = sq[j];
    }
}

}  // namespace

extern "C" int64_t rg_pair_score_regime(int Q, int k, int D, int C, int aligned) {
    if (Q < 1 || k < 1 || D < 1 || D > kMaxD || C < 1 || C > kMaxC) return -1;
    const PairPlan p = pair_plan(Q, k, D, C, aligned);
    return (int64_t)(p.vec | (p.split << 1));
}

extern "C" int rg_pair_score(const float* probe, const float* gallery, const int* idx, const float* gamma, const float* beta,
                             const float* running_mean, const float* running_var, const float* W, const float* bias, float* logits,
                             float* score, int Q, int G, int k, int D, int C, float eps, hipStream_t stream) {
    RG_REQUIRE(probe && gallery && idx && gamma && beta && running_mean && running_var && W, "rg_pair_score: bad arguments");
    RG_REQUIRE(logits || score, "rg_pair_score: one of logits and score must be given");
    RG_REQUIRE(C >= 1 && C <= kMaxC, "rg_pair_score: 1 to %d classes, got %d", kMaxC, C);
    RG_REQUIRE(D >= 1 && D <= kMaxD, "rg_pair_score: 1 to %d features, got %d", kMaxD, D);
    RG_REQUIRE(Q >= 1 && Q <= 65535 && G >= 1 && k >= 1 && k <= G, "rg_pair_score: needs 1 <= Q <= 65535 and 1 <= k <= G, got Q=%d G=%d k=%d",
               Q, G, k);
    RG_REQUIRE((int64_t)Q * k * C < (1ll << 31), "rg_pair_score: Q * k * C must stay below 2^31");
    const int aligned = (((uintptr_t)probe | (uintptr_t)gallery | (uintptr_t)gamma | (uintptr_t)running_mean | (uintptr_t)running_var |
                          (uintptr_t)W) & 15) == 0;
    const PairPlan p = pair_plan(Q, k, D, C, aligned);
    rg::ProfScope prof(rg::FAM_CM, stream, 2.0 * Q * (double)k * D * (C + 1), 4.0 * Q * (double)(k + 1) * D);
    const dim3 grid(p.wgs_x, Q);
    if (C <= 2)
        pair_launch<2>(p, grid, stream, probe, gallery, idx, gamma, beta, running_mean, running_var, W, bias, logits, score, G, k, D, C, eps);
    else if (C <= 4)
        pair_launch<4>(p, grid, stream, probe, gallery, idx, gamma, beta, running_mean, running_var, W, bias, logits, score, G, k, D, C, eps);
    else
        pair_launch<kMaxC>(p, grid, stream, probe, gallery, idx, gamma, beta, running_mean, running_var, W, bias, logits, score, G, k, D, C, eps);
    return rg::check_launch("rg_pair_score");
}

extern "C" int rg_cascade_merge(float* dist, int64_t ld, const int* idx, const float* score, int Q, int G, int k, hipStream_t stream) {
    RG_REQUIRE(dist && idx && score && Q >= 1 && G >= 1 && k >= 1 && k <= G && ld >= G, "rg_cascade_merge: bad arguments (1 <= k <= G <= ld)");
    RG_REQUIRE(G <= kMaxG, "rg_cascade_merge: at most %d gallery columns (the bitmap of a row lives in LDS), got %d", kMaxG, G);
    const size_t lds = k < G ? (size_t)((G + 31) / 32) * sizeof(unsigned) : 0;
    if (lds > 48 * 1024) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(cascade_merge_kernel),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        RG_REQUIRE(e == hipSuccess, "rg_cascade_merge: %zu bytes of LDS refused (%s)", lds, hipGetErrorString(e));
    }
    rg::ProfScope prof(rg::FAM_CM, stream, 0.0, 12.0 * Q * (double)G);
    hipLaunchKernelGGL(cascade_merge_kernel, dim3(Q), dim3(256), lds, stream, dist, ld, idx, score, G, k);
    return rg::check_launch("rg_cascade_merge");
}
