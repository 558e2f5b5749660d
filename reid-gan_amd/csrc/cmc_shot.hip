// Single-gallery-shot CMC (the reference's `cuhk03` protocol: cmc(single_gallery_shot=True) of
// FD/reid/evaluation_metrics/ranking.py :53-75) of a query x gallery distance matrix d [Q][ld] without a sort and without a
// per-repeat gather.  The reference keeps, per query and `repeat` times, ONE randomly drawn valid gallery entry of every
// identity and asks where the query's own identity lands among them.  With every row ordered by the stable key (d, j):
//   * the identities, in the order the reference draws for them (first appearance among the row's valid entries), are the
//     identities sorted by their smallest valid key                                                        -> rg_cmc_shot_order
//   * a draw u in [0, cnt_x) selects the u-th valid entry of identity x in key order.  With t_r the entry drawn for the own
//     identity in repeat r, the entry drawn for x precedes t_r iff u[r][x] < c_x(t_r) = #{valid entries of x with key < t_r},
//     so the rank the reference adds to is k_r = #{x != own : u[r][x] < c_x(t_r)}                          -> rg_cmc_shot_rank
// The draws themselves are made on the host (numpy's generator defines the result); only the per-position counts go down and
// only the draws come up.
//
// The gallery is grouped by identity once per call (host, O(G)): seg_ptr [nid + 1], seg_perm [G], identities ascending and the
// entries of one identity in ascending j.  valid_j = (gid_j != qid_i) | (gcam_j != qcam_i), and gcam_j != qcam_i with
// separate_camera_set; inside the segment x it reads (x != own_i | gcam_j != qcam_i) with own_i the segment of the query's id.
//
// Order pass, one workgroup per row: a wave per segment reduces (valid count, smallest valid key), the at most nid keys are
// sorted in LDS (bitonic, segments without a valid entry carry j = INT_MAX and end up behind the others).
// Rank pass, one workgroup per row: t_r is found by counting inside the own segment (quadratic in its valid entries, which
// are few), then a wave per segment sweeps its entries once, one ballot + popcount per threshold, lane r holding c_x(t_r);
// the indicators are summed per lane and leave through integer LDS atomics.  The row is staged in LDS with 16-byte loads when
// it fits (rg_cmc_shot_regime) and the segments are gathered from there; otherwise the same body gathers from global memory.
// Integer atomics only: the bits do not depend on arrival order, stream or chunking.
#include "rg_common.h"
#include <limits.h>

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxIds = 4096;             // keys sorted in LDS: 4096 * (8 + 4 + 4) bytes = 64 KB for an fp64 matrix
constexpr int kMaxRepeat = 64;            // one lane per repeat in the rank pass
constexpr int kRowLdsBytes = 32768;       // a row at or below this is staged in LDS: four workgroups still share a CU's 160 KB

template <typename T>
__device__ __forceinline__ bool key_less(T da, int ja, T db, int jb) {
    return da < db || (da == db && ja < jb);          // by value: -0.0 == 0.0, +-inf are ordinary
}

__device__ __forceinline__ bool entry_valid(bool own_segment, int cam, int my_cam, int separate) {
    return (!own_segment || cam != my_cam) && !(separate && cam == my_cam);
}

// LDS (dynamic), n2 = nid rounded up to a power of two: T sd[n2] | int sj[n2] | int sx[n2]; sd is reused for the counts
template <typename T>
__global__ __launch_bounds__(kThreads) void cmc_shot_order_kernel(const T* __restrict__ dist, int G, int64_t ld, int nid, int n2,
                                                                 const int* __restrict__ seg_ptr, const int* __restrict__ seg_perm,
                                                                 const int* __restrict__ gcam, const int* __restrict__ qseg,
                                                                 const int* __restrict__ qcam, int separate, int* __restrict__ n_out,
                                                                 int* __restrict__ slot, int* __restrict__ high, int* __restrict__ status) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ int s_own_cnt, s_n;
    T* sd = reinterpret_cast<T*>(smem);
    int* sj = reinterpret_cast<int*>(sd + n2);
    int* sx = sj + n2;

    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, i = blockIdx.x;
    const T* row = dist + (int64_t)i * ld;
    const int my_cam = qcam[i], own = qseg[i];
    const T inf = (T)__builtin_huge_val();
    int* my_high = high + (int64_t)i * nid;
    int* my_slot = slot + (int64_t)i * nid;
    if (tid == 0) {
        s_own_cnt = 0;
        s_n = 0;
    }
    __syncthreads();

    // ---- 1. per segment: valid count and smallest valid key; every entry of the row is read once (the NaN check rides along)
    int flags = 0;
    for (int x = wid; x < nid; x += kWaves) {
        const int s0 = max(0, seg_ptr[x]), s1 = min(G, seg_ptr[x + 1]);
        int cnt = 0, bj = INT_MAX;
        T bd = inf;
        for (int e = s0 + lane; e < s1; e += 64) {
            const int j = seg_perm[e];
            if ((unsigned)j >= (unsigned)G) {           // a broken segment list: nothing is read for it
                flags |= 2;
                continue;
            }
            const T d = row[j];
            flags |= d != d;
            if (entry_valid(x == own, gcam[j], my_cam, separate)) {
                ++cnt;
                if (key_less(d, j, bd, bj)) {
                    bd = d;
                    bj = j;
                }
            }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            cnt += __shfl_xor(cnt, off, 64);
            const T od = __shfl_xor(bd, off, 64);
            const int oj = __shfl_xor(bj, off, 64);
            if (key_less(od, oj, bd, bj)) {
                bd = od;
                bj = oj;
            }
        }
        if (lane == 0) {
            sd[x] = cnt ? bd : inf;
            sj[x] = cnt ? bj : INT_MAX;
            sx[x] = x;
            my_high[x] = cnt;                           // in identity order for now; step 3 puts it in position order
            if (x == own) s_own_cnt = cnt;
        }
    }
    for (int t = nid + tid; t < n2; t += kThreads) {
        sd[t] = inf;
        sj[t] = INT_MAX;
        sx[t] = -1;
    }
    if (flags) atomicOr(status, flags);
    __syncthreads();
    const bool skipped = own < 0 || own >= nid || s_own_cnt == 0;     // uniform: no valid match, the reference `continue`s

    // ---- 2. bitonic sort of (sd, sj | sx) [0, n2) by (d, j)
    if (!skipped)
        for (int k = 2; k <= n2; k <<= 1)
            for (int s = k >> 1; s > 0; s >>= 1) {
                for (int t = tid; t < n2; t += kThreads) {
                    const int u = t ^ s;
                    if (u > t) {
                        const T dt = sd[t], du = sd[u];
                        const int jt = sj[t], ju = sj[u];
                        const bool up = (t & k) == 0;
                        if (key_less(du, ju, dt, jt) == up) {
                            const int xt = sx[t], xu = sx[u];
                            sd[t] = du;
                            sd[u] = dt;
                            sj[t] = ju;
                            sj[u] = jt;
                            sx[t] = xu;
                            sx[u] = xt;
                        }
                    }
                }
                __syncthreads();
            }

    // ---- 3. the counts come back from global memory into the LDS the distances leave, then go out in position order
    int* scnt = reinterpret_cast<int*>(sd);
    for (int x = tid; x < nid; x += kThreads) scnt[x] = my_high[x];
    __syncthreads();
    int mine = 0;
    for (int p = tid; p < nid; p += kThreads) {
        const int x = sx[p];
        const bool ok = !skipped && sj[p] != INT_MAX;   // the segments with a valid entry are a prefix of the sorted order
        my_slot[p] = ok ? x : -1;
        my_high[p] = ok ? scnt[x] : 0;
        mine += ok;
    }
    if (mine) atomicAdd(&s_n, mine);
    __syncthreads();
    if (tid == 0) n_out[i] = s_n;
}

// LDS (dynamic, kLds only): the row, shifted so that its 16-byte slots line up with those of the row in global memory
template <typename T, bool kLds>
__global__ __launch_bounds__(kThreads) void cmc_shot_rank_kernel(const T* __restrict__ dist, int q0, int G, int64_t ld, int nid,
                                                                const int* __restrict__ seg_ptr, const int* __restrict__ seg_perm,
                                                                const int* __restrict__ gcam, const int* __restrict__ qseg,
                                                                const int* __restrict__ qcam, int separate, const int* __restrict__ n_in,
                                                                const int* __restrict__ slot, const int* __restrict__ draws,
                                                                const int64_t* __restrict__ draw_off, int repeat, int topk,
                                                                int* __restrict__ rank, int* __restrict__ hist) {
    constexpr int VEC = 16 / (int)sizeof(T);
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ T s_td[kMaxRepeat];
    __shared__ int s_tj[kMaxRepeat];
    __shared__ int s_k[kMaxRepeat];
    __shared__ int s_pown;

    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, i = q0 + blockIdx.x;
    const int n = min(n_in[i], nid);
    int* my_rank = rank + (int64_t)i * repeat;
    if (n <= 0) {                                       // uniform: a skipped query draws nothing and adds nothing
        if (tid < repeat) my_rank[tid] = -1;
        return;
    }
    const T* row = dist + (int64_t)i * ld;
    const int my_cam = qcam[i], own = qseg[i];
    const int* my_slot = slot + (int64_t)i * nid;
    const int* u = draws + draw_off[blockIdx.x];        // [repeat][n], position order
    const T inf = (T)__builtin_huge_val();

    const T* src = row;
    if (kLds) {
        const int mis = (int)(((uintptr_t)row & 15u) / sizeof(T));
        T* srow = reinterpret_cast<T*>(smem) + mis;
        const int head = min(G, (VEC - mis) % VEC);
        for (int j = tid; j < head; j += kThreads) srow[j] = row[j];
        const int nvec = (G - head) / VEC;
        for (int v = tid; v < nvec; v += kThreads)
            *reinterpret_cast<uint4*>(srow + head + v * VEC) = *reinterpret_cast<const uint4*>(row + head + (int64_t)v * VEC);
        for (int j = head + nvec * VEC + tid; j < G; j += kThreads) srow[j] = row[j];
        src = srow;
    }
    if (tid < kMaxRepeat) {
        s_td[tid] = -inf;                               // a threshold nobody sets (a draw outside its range) counts nothing
        s_tj[tid] = INT_MIN;
        s_k[tid] = 0;
    }
    if (tid == 0) s_pown = -1;
    __syncthreads();
    for (int p = tid; p < n; p += kThreads)
        if (my_slot[p] == own) s_pown = p;
    __syncthreads();
    const int p_own = s_pown;
    if (p_own < 0 || own < 0 || own >= nid) {           // uniform; not what the order pass writes
        if (tid < repeat) my_rank[tid] = -1;
        return;
    }

    // ---- 1. t_r = the u[r][own]-th valid entry of the own segment in key order: every valid entry counts those before it
    {
        const int s0 = max(0, seg_ptr[own]), s1 = min(G, seg_ptr[own + 1]);
        for (int e = s0 + tid; e < s1; e += kThreads) {
            const int j = seg_perm[e];
            if ((unsigned)j >= (unsigned)G || !entry_valid(true, gcam[j], my_cam, separate)) continue;
            const T d = src[j];
            int before = 0;
            for (int e2 = s0; e2 < s1; ++e2) {
                const int j2 = seg_perm[e2];
                if ((unsigned)j2 >= (unsigned)G || !entry_valid(true, gcam[j2], my_cam, separate)) continue;
                before += key_less(src[j2], j2, d, j);
            }
            for (int r = 0; r < repeat; ++r)
                if (u[(int64_t)r * n + p_own] == before) {
                    s_td[r] = d;
                    s_tj[r] = j;
                }
        }
    }
    __syncthreads();

    // ---- 2. a wave per segment: lane r counts the segment's valid entries before t_r, then compares with its draw
    int kacc = 0;
    for (int p = wid; p < n; p += kWaves) {
        if (p == p_own) continue;
        const int x = my_slot[p];
        if ((unsigned)x >= (unsigned)nid) continue;
        const int s0 = max(0, seg_ptr[x]), s1 = min(G, seg_ptr[x + 1]);
        int c = 0;
        for (int base = s0; base < s1; base += 64) {
            const int e = base + lane;
            bool v = false;
            T d = inf;
            int j = INT_MAX;
            if (e < s1) {
                j = seg_perm[e];
                if ((unsigned)j < (unsigned)G) {
                    v = entry_valid(x == own, gcam[j], my_cam, separate);
                    d = src[j];
                }
            }
            for (int r = 0; r < repeat; ++r) {
                const unsigned long long b = __ballot(v && key_less(d, j, s_td[r], s_tj[r]));
                if (lane == r) c += __popcll(b);
            }
        }
        if (lane < repeat) kacc += u[(int64_t)lane * n + p] < c;
    }
    if (lane < repeat && kacc) atomicAdd(&s_k[lane], kacc);
    __syncthreads();
    if (tid < repeat) {
        const int k = s_k[tid];
        my_rank[tid] = k;
        if (k < topk) atomicAdd(&hist[k], 1);
    }
}

int shot_regime(int G, int nid, int is_double) {
    if (G < 1 || G > (1 << 30) || nid < 1 || nid > kMaxIds || nid > G) return -1;
    return (int64_t)G * (is_double ? 8 : 4) <= kRowLdsBytes ? 1 : 0;
}

template <typename K>
int allow_lds(K kernel, size_t lds, const char* who) {
    if (lds <= 48 * 1024) return RG_OK;
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    RG_REQUIRE(e == hipSuccess, "%s: %zu bytes of LDS refused (%s)", who, lds, hipGetErrorString(e));
    return RG_OK;
}

bool bad_matrix(const void* dist, int is_double, int Q, int G, int64_t ld) {
    return !dist || (is_double != 0 && is_double != 1) || Q < 1 || G < 1 || G > (1 << 30) || ld < G ||
           ((uintptr_t)dist & (is_double ? 7u : 3u)) != 0;
}

}  // namespace

extern "C" int64_t rg_cmc_shot_regime(int G, int nid, int is_double) {
    if (is_double != 0 && is_double != 1) return -1;
    return shot_regime(G, nid, is_double);
}

extern "C" int rg_cmc_shot_order(const void* dist, int is_double, int Q, int G, int64_t ld, int nid, const int* seg_ptr,
                                 const int* seg_perm, const int* gallery_cams, const int* query_seg, const int* query_cams,
                                 int separate_camera_set, int* n, int* slot, int* high, int* status, hipStream_t stream) {
    RG_REQUIRE(!bad_matrix(dist, is_double, Q, G, ld), "rg_cmc_shot_order: bad matrix (Q=%d, G=%d, ld=%lld; fp32 or fp64, aligned to its element)",
               Q, G, (long long)ld);
    RG_REQUIRE(nid >= 1 && nid <= kMaxIds && nid <= G, "rg_cmc_shot_order: 1 to %d identities (their keys are sorted in LDS) and no more than G, got %d",
               kMaxIds, nid);
    RG_REQUIRE(seg_ptr && seg_perm && gallery_cams && query_seg && query_cams && n && slot && high && status,
               "rg_cmc_shot_order: null segment / camera / output array");
    RG_REQUIRE((int64_t)Q * nid < ((int64_t)1 << 31), "rg_cmc_shot_order: Q * nid must stay below 2^31, got Q=%d nid=%d", Q, nid);
    RG_REQUIRE(separate_camera_set == 0 || separate_camera_set == 1, "rg_cmc_shot_order: separate_camera_set must be 0 or 1");
    int n2 = 1;
    while (n2 < nid) n2 <<= 1;
    const size_t lds = (size_t)n2 * ((is_double ? 8 : 4) + 8);
    rg::ProfScope prof(rg::FAM_MISC, stream, 0.0, (is_double ? 8.0 : 4.0) * Q * (double)G);
    if (hipMemsetAsync(status, 0, sizeof(int), stream) != hipSuccess) {
        rg::set_error("rg_cmc_shot_order: hipMemsetAsync failed");
        return RG_ERR_LAUNCH;
    }
    if (is_double) {
        if (int st = allow_lds(cmc_shot_order_kernel<double>, lds, "rg_cmc_shot_order")) return st;
        hipLaunchKernelGGL(cmc_shot_order_kernel<double>, dim3(Q), dim3(kThreads), lds, stream, (const double*)dist, G, ld, nid, n2, seg_ptr,
                           seg_perm, gallery_cams, query_seg, query_cams, separate_camera_set, n, slot, high, status);
    } else {
        if (int st = allow_lds(cmc_shot_order_kernel<float>, lds, "rg_cmc_shot_order")) return st;
        hipLaunchKernelGGL(cmc_shot_order_kernel<float>, dim3(Q), dim3(kThreads), lds, stream, (const float*)dist, G, ld, nid, n2, seg_ptr,
                           seg_perm, gallery_cams, query_seg, query_cams, separate_camera_set, n, slot, high, status);
    }
    return rg::check_launch("rg_cmc_shot_order");
}

extern "C" int rg_cmc_shot_rank(const void* dist, int is_double, int Q, int q0, int nq, int G, int64_t ld, int nid, const int* seg_ptr,
                                const int* seg_perm, const int* gallery_cams, const int* query_seg, const int* query_cams,
                                int separate_camera_set, const int* n, const int* slot, const int* draws, const int64_t* draw_off,
                                int repeat, int topk, int* rank, int* hist, hipStream_t stream) {
    RG_REQUIRE(!bad_matrix(dist, is_double, Q, G, ld), "rg_cmc_shot_rank: bad matrix (Q=%d, G=%d, ld=%lld; fp32 or fp64, aligned to its element)",
               Q, G, (long long)ld);
    RG_REQUIRE(q0 >= 0 && nq >= 1 && (int64_t)q0 + nq <= Q, "rg_cmc_shot_rank: queries [%d, %d + %d) outside the %d rows", q0, q0, nq, Q);
    RG_REQUIRE(nid >= 1 && nid <= kMaxIds && nid <= G, "rg_cmc_shot_rank: 1 to %d identities and no more than G, got %d", kMaxIds, nid);
    RG_REQUIRE(seg_ptr && seg_perm && gallery_cams && query_seg && query_cams && n && slot && draws && draw_off && rank && hist,
               "rg_cmc_shot_rank: null segment / camera / draw / output array");
    RG_REQUIRE(repeat >= 1 && repeat <= kMaxRepeat, "rg_cmc_shot_rank: 1 to %d repeats (one lane each), got %d", kMaxRepeat, repeat);
    RG_REQUIRE(topk >= 1 && (int64_t)Q * nid < ((int64_t)1 << 31) && (int64_t)Q * repeat < ((int64_t)1 << 31),
               "rg_cmc_shot_rank: need topk >= 1, Q * nid < 2^31 and Q * repeat < 2^31, got Q=%d nid=%d repeat=%d topk=%d", Q, nid, repeat, topk);
    RG_REQUIRE(separate_camera_set == 0 || separate_camera_set == 1, "rg_cmc_shot_rank: separate_camera_set must be 0 or 1");
    const int esz = is_double ? 8 : 4;
    const bool in_lds = shot_regime(G, nid, is_double) == 1;
    const size_t lds = in_lds ? (size_t)G * esz + 16 : 0;
    rg::ProfScope prof(rg::FAM_MISC, stream, 0.0, (double)esz * nq * (double)G);
#define RG_SHOT_RANK(T, L)                                                                                                              \
    do {                                                                                                                                \
        if (int st = allow_lds(cmc_shot_rank_kernel<T, L>, lds, "rg_cmc_shot_rank")) return st;                                         \
        hipLaunchKernelGGL((cmc_shot_rank_kernel<T, L>), dim3(nq), dim3(kThreads), lds, stream, (const T*)dist, q0, G, ld, nid, seg_ptr, \
                           seg_perm, gallery_cams, query_seg, query_cams, separate_camera_set, n, slot, draws, draw_off, repeat, topk,   \
                           rank, hist);                                                                                                 \
    } while (0)
    if (is_double) {
        if (in_lds) RG_SHOT_RANK(double, true); else RG_SHOT_RANK(double, false);
    } else {
        if (in_lds) RG_SHOT_RANK(float, true); else RG_SHOT_RANK(float, false);
    }
#undef RG_SHOT_RANK
    return rg::check_launch("rg_cmc_shot_rank");
}
