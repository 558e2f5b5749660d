// CMC and mAP of a query x gallery distance matrix d [Q][ld] without a sort, entirely on the device: the scoring step of
// CC/clustercontrast/evaluation_metrics/ranking.py (`cmc`, `mean_ap`) behind Evaluator.evaluate.
//   valid_j = (gid_j != qid_i) | (gcam_j != qcam_i)          (& gcam_j != qcam_i with separate_camera_set)
//   pos_j   = valid_j & (gid_j == qid_i)
// Both metrics need, per positive p of a row, three counts over the row's valid entries: the non-matching entries a stable
// sort by (d, j) puts before p (its CMC rank), and the positives / all entries with d <= d_p (scikit-learn's tie-grouped
// average precision = (1/P) sum_p TP_le(p) / N_le(p)).  One workgroup per row: the positives are compacted into LDS (at most
// `cap` per pass, ascending j), sorted there by (d, j), and every valid entry of the row binary-searches them and bumps an
// integer LDS histogram; a prefix sum over the bins gives the counts.  Rows with more positives take further passes.
// Every sum is an integer one (the AP terms are accumulated as 64.64 fixed point), so the outputs do not depend on the
// order the atomics land in, on the stream or on `cap`: two runs give the same bits.  No floating-point atomics.
#include "rg_common.h"
#include <limits.h>

namespace {

constexpr int kThreads = 256;
constexpr int kMaxCap = 1024;             // positives per pass: kMaxCap / kThreads bins per thread in the prefix sums
constexpr int kAutoCap = 512;
constexpr int kScanPer = 4;               // consecutive gallery entries per thread and step of the compaction

template <typename T>
__device__ __forceinline__ bool key_less(T da, int ja, T db, int jb) {
    return da < db || (da == db && ja < jb);          // by value: -0.0 == 0.0, +-inf are ordinary
}

// floor(tp * 2^64 / n) for 0 < tp < n < 2^31, by two steps of long division
__device__ __forceinline__ unsigned long long frac64(unsigned tp, unsigned n) {
    const unsigned long long a = (unsigned long long)tp << 32;
    const unsigned long long q1 = a / n, r1 = a % n;
    const unsigned long long q2 = (r1 << 32) / n;
    return (q1 << 32) | q2;
}

struct Acc {                              // 64.64 fixed point: hi whole units, lo / 2^64
    unsigned long long hi, lo;
};
__device__ __forceinline__ void acc_add(Acc& a, unsigned long long hi, unsigned long long lo) {
    const unsigned long long s = a.lo + lo;
    a.hi += hi + (s < a.lo ? 1ull : 0ull);
    a.lo = s;
}

// LDS layout (dynamic), cap2 = cap rounded up to a power of two (the bitonic sort pads the pass to one):
// T sd[cap2] | int sj[cap2] | int h_before[cap2 + 1] | int h_negle[cap2 + 1] | int h_posle[cap2 + 1]
template <typename T>
__global__ __launch_bounds__(kThreads) void rank_eval_row_kernel(const T* __restrict__ dist, int G, int64_t ld,
                                                                const int* __restrict__ qid, const int* __restrict__ gid,
                                                                const int* __restrict__ qcam, const int* __restrict__ gcam,
                                                                int separate, int topk, int cap, int* __restrict__ npos_out,
                                                                double* __restrict__ ap_out, int* __restrict__ first_out,
                                                                int* __restrict__ hits, int* __restrict__ status) {
    constexpr int VEC = 16 / (int)sizeof(T);
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ int red[17];
    __shared__ unsigned long long red64[2 * (kThreads / 64)];
    int cap2 = 1;
    while (cap2 < cap) cap2 <<= 1;
    T* sd = reinterpret_cast<T*>(smem);
    int* sj = reinterpret_cast<int*>(sd + cap2);
    int* h_before = sj + cap2;
    int* h_negle = h_before + cap2 + 1;
    int* h_posle = h_negle + cap2 + 1;

    const int tid = threadIdx.x, i = blockIdx.x;
    const T* row = dist + (int64_t)i * ld;
    const int my_id = qid[i], my_cam = qcam[i];
    const T inf = (T)__builtin_huge_val();

    auto is_valid = [&](int g, int c) { return (g != my_id || c != my_cam) && !(separate && c == my_cam); };

    Acc acc = {0ull, 0ull};
    int first = INT_MAX, npos = 0, has_nan = 0;

    for (int ord0 = 0; ord0 == 0 || ord0 < npos; ord0 += cap) {
        // ---- 1. the positives with ordinal [ord0, ord0 + cap) in ascending j -> sd / sj; pass 0 walks the whole row for npos
        int seen = 0;
        for (int j0 = 0; j0 < G && (ord0 == 0 || seen < ord0 + cap); j0 += kThreads * kScanPer) {
            const int jb = j0 + tid * kScanPer;
            bool p[kScanPer];
            int c = 0;
#pragma unroll
            for (int k = 0; k < kScanPer; ++k) {
                const int j = jb + k;
                p[k] = false;
                if (j < G) {
                    const int g = gid[j];
                    p[k] = g == my_id && is_valid(g, gcam[j]);
                }
                c += p[k];
            }
            int total;
            int o = seen + block_excl_scan(c, red, &total) - ord0;
#pragma unroll
            for (int k = 0; k < kScanPer; ++k)
                if (p[k]) {
                    if (o >= 0 && o < cap) {
                        sd[o] = row[jb + k];
                        sj[o] = jb + k;
                    }
                    ++o;
                }
            seen += total;
        }
        if (ord0 == 0) npos = seen;
        if (npos == 0) {                            // uniform: every thread holds the same count; only the NaN check is left
            for (int j = tid; j < G; j += kThreads) has_nan |= row[j] != row[j];
            break;
        }
        const int n = min(cap, npos - ord0);
        int n2 = 1;
        while (n2 < n) n2 <<= 1;
        for (int t = n + tid; t < n2; t += kThreads) {
            sd[t] = inf;
            sj[t] = INT_MAX;
        }
        for (int t = tid; t <= n; t += kThreads) h_before[t] = h_negle[t] = h_posle[t] = 0;
        __syncthreads();

        // ---- 2. bitonic sort of sd / sj [0, n2) by (d, j)
        for (int k = 2; k <= n2; k <<= 1)
            for (int s = k >> 1; s > 0; s >>= 1) {
                for (int t = tid; t < n2; t += kThreads) {
                    const int u = t ^ s;
                    if (u > t) {
                        const T dt = sd[t], du = sd[u];
                        const int jt = sj[t], ju = sj[u];
                        const bool up = (t & k) == 0;
                        if (key_less(du, ju, dt, jt) == up) {
                            sd[t] = du;
                            sd[u] = dt;
                            sj[t] = ju;
                            sj[u] = jt;
                        }
                    }
                }
                __syncthreads();
            }

        // ---- 3. every valid entry of the row finds its place among the n sorted positives
        const T dmax = sd[n - 1];
        auto visit = [&](T d, int j) {
            has_nan |= d != d;
            const int g = gid[j];
            if (!is_valid(g, gcam[j])) return;
            if (!(d <= dmax)) return;               // counts for no positive of this pass (the common case)
            int lo = 0, hi = n;                     // lo = positives of the pass with d_c < d
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (sd[mid] < d) lo = mid + 1; else hi = mid;
            }
            if (lo >= n) return;
            if (g == my_id) {
                atomicAdd(&h_posle[lo], 1);
                return;
            }
            atomicAdd(&h_negle[lo], 1);
            hi = n;                                 // lo = positives of the pass before (d, j) in stable order
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (key_less(sd[mid], sj[mid], d, j)) lo = mid + 1; else hi = mid;
            }
            if (lo < n) atomicAdd(&h_before[lo], 1);
        };
        const int head = min(G, (int)(((16u - (unsigned)((uintptr_t)row & 15u)) & 15u) / sizeof(T)));
        for (int j = tid; j < head; j += kThreads) visit(row[j], j);
        const int nvec = (G - head) / VEC;
        for (int v = tid; v < nvec; v += kThreads) {
            const uint4 raw = *reinterpret_cast<const uint4*>(row + head + (int64_t)v * VEC);
            T e[VEC];
            __builtin_memcpy(e, &raw, 16);
#pragma unroll
            for (int k = 0; k < VEC; ++k) visit(e[k], head + v * VEC + k);
        }
        for (int j = head + nvec * VEC + tid; j < G; j += kThreads) visit(row[j], j);
        __syncthreads();

        // ---- 4. inclusive prefix sums over the bins: thread t owns bins [t * per, t * per + per)
        const int per = (n + kThreads - 1) / kThreads, b0 = min(n, tid * per), b1 = min(n, b0 + per);
        int sb = 0, sn = 0, sp = 0, total;
        for (int b = b0; b < b1; ++b) {
            sb += h_before[b];
            sn += h_negle[b];
            sp += h_posle[b];
        }
        int rb = block_excl_scan(sb, red, &total);
        int rn = block_excl_scan(sn, red, &total);
        int rp = block_excl_scan(sp, red, &total);
        for (int b = b0; b < b1; ++b) {
            rb += h_before[b];
            rn += h_negle[b];
            rp += h_posle[b];
            // positive b of the pass: rank rb among the non-matching entries, rp positives and rn others with d <= its own
            if (rb < topk) atomicAdd(&hits[(int64_t)i * topk + rb], 1);
            first = min(first, rb);
            if (rn == 0) acc_add(acc, 1ull, 0ull);
            else acc_add(acc, 0ull, frac64((unsigned)rp, (unsigned)(rp + rn)));
        }
        __syncthreads();                            // the next pass overwrites sd / sj and clears the bins
    }

    if (has_nan) atomicOr(status, 1);
    __syncthreads();                                // a row without positives comes here straight from a scan that reads `red`
    // ---- block reduction: integer sums and a minimum, the same for every order
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long ohi = __shfl_xor(acc.hi, off, 64), olo = __shfl_xor(acc.lo, off, 64);
        acc_add(acc, ohi, olo);
        first = min(first, __shfl_xor(first, off, 64));
    }
    const int lane = tid & 63, wid = tid >> 6;
    if (lane == 0) {
        red64[2 * wid] = acc.hi;
        red64[2 * wid + 1] = acc.lo;
        red[wid] = first;
    }
    __syncthreads();
    if (tid == 0) {
        Acc t = {0ull, 0ull};
        int f = INT_MAX;
        for (int w = 0; w < kThreads / 64; ++w) {
            acc_add(t, red64[2 * w], red64[2 * w + 1]);
            f = min(f, red[w]);
        }
        npos_out[i] = npos;
        first_out[i] = npos ? f : -1;
        ap_out[i] = npos ? ((double)t.hi + (double)t.lo * 0x1p-64) / (double)npos : 0.0;
    }
}

// Sums over the queries in a fixed order.  Block k < topk: counts[2 + k] = valid queries with first == k, sums[1 + k] =
// sum_i hits[i][k] / npos[i]; block topk: counts[1] = valid queries, sums[0] = sum_i ap[i].  counts[0] is the status word.
__global__ __launch_bounds__(kThreads) void rank_eval_reduce_kernel(const int* __restrict__ npos, const double* __restrict__ ap,
                                                                   const int* __restrict__ first, const int* __restrict__ hits,
                                                                   int Q, int topk, int* __restrict__ counts, double* __restrict__ sums) {
    __shared__ double sred[kThreads / 64];
    __shared__ int cred[kThreads / 64];
    const int k = blockIdx.x, tid = threadIdx.x;
    double s = 0.0;
    int c = 0;
    for (int i = tid; i < Q; i += kThreads) {
        const int np = npos[i];
        if (np <= 0) continue;
        if (k == topk) {
            s += ap[i];
            ++c;
        } else {
            const int h = hits[(int64_t)i * topk + k];
            if (h) s += (double)h / (double)np;
            c += first[i] == k;
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        s += __shfl_xor(s, off, 64);
        c += __shfl_xor(c, off, 64);
    }
    if ((tid & 63) == 0) {
        sred[tid >> 6] = s;
        cred[tid >> 6] = c;
    }
    __syncthreads();
    if (tid == 0) {
        double ts = 0.0;
        int tc = 0;
        for (int w = 0; w < kThreads / 64; ++w) {
            ts += sred[w];
            tc += cred[w];
        }
        if (k == topk) {
            sums[0] = ts;
            counts[1] = tc;
        } else {
            sums[1 + k] = ts;
            counts[2 + k] = tc;
        }
    }
}

}  // namespace

extern "C" int rg_rank_eval(const void* dist, int is_double, int Q, int G, int64_t ld, const int* query_ids, const int* gallery_ids,
                            const int* query_cams, const int* gallery_cams, int separate_camera_set, int topk, int chunk, int* npos,
                            double* ap, int* first, int* hits, int* counts, double* sums, hipStream_t stream) {
    RG_REQUIRE(dist && (is_double == 0 || is_double == 1) && Q > 0 && G > 0 && G <= (1 << 30) && ld >= G && ((uintptr_t)dist & (is_double ? 7u : 3u)) == 0,
               "rg_rank_eval: bad matrix (Q=%d, G=%d, ld=%lld; fp32 or fp64, aligned to its element)", Q, G, (long long)ld);
    RG_REQUIRE(query_ids && gallery_ids && query_cams && gallery_cams && npos && ap && first && hits && counts && sums,
               "rg_rank_eval: null id / camera / output array");
    RG_REQUIRE(topk >= 1 && (int64_t)Q * topk < ((int64_t)1 << 31), "rg_rank_eval: need topk >= 1 and Q * topk < 2^31, got Q=%d topk=%d", Q, topk);
    RG_REQUIRE(chunk == 0 || (chunk >= 1 && chunk <= kMaxCap), "rg_rank_eval: chunk must be 0 (automatic) or 1 .. %d, got %d", kMaxCap, chunk);
    RG_REQUIRE(separate_camera_set == 0 || separate_camera_set == 1, "rg_rank_eval: separate_camera_set must be 0 or 1");
    const int cap = chunk ? chunk : kAutoCap;
    const size_t esz = is_double ? 8 : 4;
    size_t cap2 = 1;
    while (cap2 < (size_t)cap) cap2 <<= 1;
    const size_t lds = cap2 * esz + cap2 * 4 + 3 * (cap2 + 1) * 4;
    rg::ProfScope prof(rg::FAM_MISC, stream, 0.0, (double)esz * Q * (double)G);
    if (hipMemsetAsync(hits, 0, (size_t)Q * topk * sizeof(int), stream) != hipSuccess ||
        hipMemsetAsync(counts, 0, sizeof(int), stream) != hipSuccess) {
        rg::set_error("rg_rank_eval: hipMemsetAsync failed");
        return RG_ERR_LAUNCH;
    }
    if (is_double)
        hipLaunchKernelGGL(rank_eval_row_kernel<double>, dim3(Q), dim3(kThreads), lds, stream, (const double*)dist, G, ld, query_ids,
                           gallery_ids, query_cams, gallery_cams, separate_camera_set, topk, cap, npos, ap, first, hits, counts);
    else
        hipLaunchKernelGGL(rank_eval_row_kernel<float>, dim3(Q), dim3(kThreads), lds, stream, (const float*)dist, G, ld, query_ids,
                           gallery_ids, query_cams, gallery_cams, separate_camera_set, topk, cap, npos, ap, first, hits, counts);
    hipLaunchKernelGGL(rank_eval_reduce_kernel, dim3(topk + 1), dim3(kThreads), 0, stream, npos, ap, first, hits, Q, topk, counts, sums);
    return rg::check_launch("rg_rank_eval");
}
