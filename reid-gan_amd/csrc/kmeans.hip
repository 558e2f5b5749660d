// k-means (Lloyd) pseudo-labelling on the device: `label_generator_kmeans` of CC/clustercontrast/models/kmeans.py, faiss's
// Clustering::train with spherical = false and nredo = 1, made deterministic.
//
//   rg_kmeans_assign   label[i] = argmin_j (csq[j] - 2 x_i . c_j), score[i] = that minimum.  The [N][D] x [K][D]^T product runs on
//                      v_mfma_f32_32x32x2_f32 (exact fp32 products, one k-ordered fma chain per score) and the argmin is taken
//                      in the epilogue on the accumulator registers, so the [N][K] scores never leave the workgroup.
//   rg_kmeans_tally    counts, their prefix sum, the members of every cluster in ascending row order (a stable counting sort
//                      without a sort: rank inside a 1024-row chunk + the chunk's offset), rows that changed, the objective.
//   rg_kmeans_update   centroids = member means (fp64 accumulation in `order`'s order), csq.
//   rg_kmeans_split    faiss's split_clusters without its RNG: the largest cluster donates to every empty one.
//
// The assignment tile is 128 rows x 128 centroids x 32 depth on 256 threads = 4 wave64 (2 x 2), every wave 2 x 2 MFMA blocks of
// 32 x 32.  Both operands have the depth as their unit-stride axis; they are staged through registers (overlapped with the
// MFMAs of the previous slab) into k-major LDS rows of 128 + 1 floats: the transposing writes and the 32-float operand reads
// are both conflict-free at that pitch.  The loaders return 0 beyond the row, centroid and depth ends.
//
// Column tiles are merged through an order-preserving 64-bit key (score bits, centroid index): the minimum of the keys is the
// lowest score and, among equal scores, the lowest index, whatever the order of arrival — a 64-bit integer atomicMin per row
// and workgroup when there is more than one column tile, a plain store when there is one.  No floating-point atomics anywhere.
#include "rg_common.h"

namespace {

typedef float floatx16 __attribute__((ext_vector_type(16)));
typedef unsigned long long u64;

constexpr int KM_MAX_N = 1 << 20, KM_MAX_K = 8192, KM_MAX_D = 8192;
constexpr int BM = 128, BN = 128, BK = 32, NT = 256, LD = BM + 1;
constexpr int CHUNK = 1024;          // rows per workgroup of the tally's rank kernel
constexpr u64 KEY_NONE = ~0ull;

// (score, index) -> a key whose unsigned order is (score ascending, index ascending); -0 is folded into +0 first
__device__ __forceinline__ u64 km_key(float s, int j) {
    unsigned u = __float_as_uint(s + 0.f);
    u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return ((u64)u << 32) | (unsigned)j;
}

__device__ __forceinline__ float km_key_score(u64 key) {
    unsigned u = (unsigned)(key >> 32);
    u = (u & 0x80000000u) ? (u & 0x7fffffffu) : ~u;
    return __uint_as_float(u);
}

// a 128(rows) x 32(depth) slab of a row-major [R][D] operand into 16 registers.  VEC (D % 4 == 0, 16-byte aligned rows): 4
// float4 per thread, 8 threads per row; otherwise 16 scalars per thread, 32 threads per row.
template <bool VEC>
__device__ __forceinline__ void km_stage(const float* __restrict__ base, int r0, int k0, int R, int D, int tid, float (&v)[16]) {
    if (VEC) {
        const int gk = k0 + 4 * (tid & 7);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int gr = r0 + (tid >> 3) + 32 * i;
            float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
            if (gr < R && gk < D) q = *reinterpret_cast<const float4*>(base + (int64_t)gr * D + gk);
            v[4 * i + 0] = q.x;
            v[4 * i + 1] = q.y;
            v[4 * i + 2] = q.z;
            v[4 * i + 3] = q.w;
        }
    } else {
        const int gk = k0 + (tid & 31);
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int gr = r0 + (tid >> 5) + 8 * i;
            v[i] = (gr < R && gk < D) ? base[(int64_t)gr * D + gk] : 0.f;
        }
    }
}

template <bool VEC>
__device__ __forceinline__ void km_commit(float (*S)[LD], int tid, const float (&v)[16]) {
    if (VEC) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) S[4 * (tid & 7) + j][(tid >> 3) + 32 * i] = v[4 * i + j];
    } else {
#pragma unroll
        for (int i = 0; i < 16; ++i) S[tid & 31][(tid >> 5) + 8 * i] = v[i];
    }
}

// grid (row tiles, column tiles).  keys != NULL: the per-row minimum goes to keys[row] by atomicMin (preset to KEY_NONE);
// keys == NULL (one column tile): label / score are written here.
template <bool VEC>
__global__ __launch_bounds__(NT) void kmeans_assign_kernel(const float* __restrict__ x, const float* __restrict__ c,
                                                           const float* __restrict__ csq, int N, int K, int D, u64* __restrict__ keys,
                                                           int* __restrict__ label, float* __restrict__ score) {
    __shared__ float As[BK][LD];
    __shared__ float Bs[BK][LD];
    __shared__ u64 red[2][BM];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int wm = wid >> 1, wn = wid & 1;
    const int l32 = lane & 31, kh = lane >> 5;
    const int m0 = blockIdx.x * BM, n0 = blockIdx.y * BN;

    floatx16 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;

    float ra[16], rb[16];
    km_stage<VEC>(x, m0, 0, N, D, tid, ra);
    km_stage<VEC>(c, n0, 0, K, D, tid, rb);
    for (int k0 = 0; k0 < D; k0 += BK) {
        __syncthreads();
        km_commit<VEC>(As, tid, ra);
        km_commit<VEC>(Bs, tid, rb);
        __syncthreads();
        if (k0 + BK < D) {
            km_stage<VEC>(x, m0, k0 + BK, N, D, tid, ra);
            km_stage<VEC>(c, n0, k0 + BK, K, D, tid, rb);
        }
#pragma unroll
        for (int ks = 0; ks < BK / 2; ++ks) {
            const int k = 2 * ks + kh;
            const float a0 = As[k][wm * 64 + l32], a1 = As[k][wm * 64 + 32 + l32];
            const float b0 = Bs[k][wn * 64 + l32], b1 = Bs[k][wn * 64 + 32 + l32];
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
        }
    }

    // the accumulator of a 32 x 32 block: column = lane & 31, row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5).  Per row: the two
    // column blocks in registers, then the 32 lanes of the half-wave, then the two waves of the row band through LDS.
    const int col0 = n0 + wn * 64 + l32, col1 = col0 + 32;
    const float q0 = col0 < K ? csq[col0] : 0.f, q1 = col1 < K ? csq[col1] : 0.f;
#pragma unroll
    for (int tm = 0; tm < 2; ++tm) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            u64 k0 = col0 < K ? km_key(fmaf(-2.f, acc[tm][0][r], q0), col0) : KEY_NONE;
            const u64 k1 = col1 < K ? km_key(fmaf(-2.f, acc[tm][1][r], q1), col1) : KEY_NONE;
            k0 = k1 < k0 ? k1 : k0;
#pragma unroll
            for (int off = 16; off > 0; off >>= 1) {
                const u64 o = __shfl_xor(k0, off, 64);
                k0 = o < k0 ? o : k0;
            }
            if (l32 == 0) red[wn][wm * 64 + tm * 32 + (r & 3) + 8 * (r >> 2) + 4 * kh] = k0;
        }
    }
    __syncthreads();
    if (tid < BM && m0 + tid < N) {
        const u64 a = red[0][tid], b = red[1][tid];
        const u64 key = b < a ? b : a;
        if (keys) {
            atomicMin(&keys[m0 + tid], key);
        } else {
            label[m0 + tid] = (int)(unsigned)(key & 0xffffffffu);
            score[m0 + tid] = km_key_score(key);
        }
    }
}

__global__ __launch_bounds__(256) void kmeans_decode_kernel(const u64* __restrict__ keys, int N, int* __restrict__ label,
                                                            float* __restrict__ score) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const u64 key = keys[i];
    label[i] = (int)(unsigned)(key & 0xffffffffu);
    score[i] = km_key_score(key);
}

// ---- tally -------------------------------------------------------------------------------------------------------------------
// workgroup b takes rows [b * CHUNK, ..): rank[i] = earlier rows of the chunk with i's label; the last row of a label in the
// chunk writes the label's count into hist[b][label] (zeroed before); part[b] = the chunk's share of the objective (fp64,
// a fixed tree); *changed += rows whose label differs from prev (integer atomic).  A label outside [0, K) is not counted.
__global__ __launch_bounds__(CHUNK) void kmeans_rank_kernel(const int* __restrict__ label, const int* __restrict__ prev,
                                                            const float* __restrict__ xsq, const float* __restrict__ score, int N,
                                                            int K, int* __restrict__ rank, int* __restrict__ hist,
                                                            double* __restrict__ part, int* __restrict__ changed) {
    __shared__ int lab[CHUNK];
    __shared__ double dred[CHUNK];
    const int t = threadIdx.x, b = blockIdx.x;
    const int i = b * CHUNK + t, n = min(CHUNK, N - b * CHUNK);
    int l = -1;
    if (i < N) {
        l = label[i];
        if (l < 0 || l >= K) l = -1;
    }
    lab[t] = l;
    dred[t] = i < N ? (double)xsq[i] + (double)score[i] : 0.0;
    __syncthreads();
    if (l >= 0) {
        int before = 0;
        bool later = false;
        for (int u = 0; u < n; ++u) {
            const bool same = lab[u] == l;
            before += (same && u < t) ? 1 : 0;
            later = later || (same && u > t);
        }
        rank[i] = before;
        if (!later) hist[(int64_t)b * K + l] = before + 1;
    }
    const int nchanged = __syncthreads_count(i < N && label[i] != prev[i]);
    for (int s = CHUNK / 2; s > 0; s >>= 1) {
        if (t < s) dred[t] += dred[t + s];
        __syncthreads();
    }
    if (t == 0) {
        part[b] = dred[0];
        if (nchanged) atomicAdd(changed, nchanged);
    }
}

// hist[.][j] -> its exclusive prefix sum over the chunks, cnt[j] = the total; thread 0 adds the objective up, chunk by chunk
__global__ __launch_bounds__(256) void kmeans_colscan_kernel(int* __restrict__ hist, int nb, int K, int* __restrict__ cnt,
                                                             const double* __restrict__ part, double* __restrict__ obj) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j == 0) {
        double s = 0.0;
        for (int b = 0; b < nb; ++b) s += part[b];
        *obj = s;
    }
    if (j >= K) return;
    int run = 0;
    for (int b = 0; b < nb; ++b) {
        const int v = hist[(int64_t)b * K + j];
        hist[(int64_t)b * K + j] = run;
        run += v;
    }
    cnt[j] = run;
}

__global__ __launch_bounds__(256) void kmeans_order_kernel(const int* __restrict__ label, const int* __restrict__ rank,
                                                           const int* __restrict__ hist, const int* __restrict__ rowptr, int N, int K,
                                                           int* __restrict__ order) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const int l = label[i];
    if (l < 0 || l >= K) return;
    const int pos = rowptr[l] + hist[(int64_t)(i / CHUNK) * K + l] + rank[i];
    if (pos >= 0 && pos < N) order[pos] = i;
}

// ---- update ------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double km_wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// block-wide fp64 sum in a fixed order (blockDim.x a multiple of 64, <= 1024); `red` holds >= 16 doubles
__device__ __forceinline__ double km_block_sum(double v, double* red) {
    v = km_wave_sum(v);
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = blockDim.x >> 6;
    __syncthreads();
    if (lane == 0) red[wid] = v;
    __syncthreads();
    double t = 0.0;
    for (int i = 0; i < nw; ++i) t += red[i];
    return t;
}

// workgroup (j, 256 columns): c[j][d] = float(sum_m double(x[order[m]][d]) / n) over the members in list order; an empty
// cluster keeps its row
__global__ __launch_bounds__(256) void kmeans_update_kernel(const float* __restrict__ x, const int* __restrict__ order,
                                                            const int* __restrict__ rowptr, int N, int D, float* __restrict__ c) {
    const int j = blockIdx.x, d = blockIdx.y * 256 + threadIdx.x, p0 = rowptr[j], p1 = rowptr[j + 1];
    if (p1 <= p0 || p0 < 0 || p1 > N || d >= D) return;
    double a = 0.0;
#pragma unroll 4
    for (int m = p0; m < p1; ++m) {
        const int r = order[m];
        if ((unsigned)r < (unsigned)N) a += (double)x[(int64_t)r * D + d];
    }
    c[(int64_t)j * D + d] = (float)(a / (double)(p1 - p0));
}

// workgroup j: csq[j] = float(sum_d double(c[j][d])^2) in a fixed order; an empty cluster keeps its csq
__global__ __launch_bounds__(256) void kmeans_csq_kernel(const float* __restrict__ c, const int* __restrict__ rowptr, int D,
                                                         float* __restrict__ csq) {
    __shared__ double red[16];
    const int j = blockIdx.x;
    if (rowptr[j + 1] <= rowptr[j]) return;
    double sq = 0.0;
    for (int d = threadIdx.x; d < D; d += 256) {
        const double v = (double)c[(int64_t)j * D + d];
        sq += v * v;
    }
    sq = km_block_sum(sq, red);
    if (threadIdx.x == 0) csq[j] = (float)sq;
}

// ---- split -------------------------------------------------------------------------------------------------------------------
// one workgroup: every empty cluster, in ascending index, takes the cluster with the currently largest count (ties: lowest index)
__global__ __launch_bounds__(1024) void kmeans_split_kernel(float* __restrict__ c, float* __restrict__ csq, int* __restrict__ cnt,
                                                            int K, int D, int* __restrict__ nsplit) {
    __shared__ int scnt[KM_MAX_K];
    __shared__ u64 kred[16];
    __shared__ double red[16];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    for (int t = tid; t < K; t += 1024) scnt[t] = cnt[t];
    __syncthreads();
    int ns = 0;
    for (int e = 0; e < K; ++e) {
        if (scnt[e] != 0) continue;                      // uniform: LDS read after a barrier
        u64 best = 0;
        for (int t = tid; t < K; t += 1024) {
            const int v = scnt[t] > 0 ? scnt[t] : 0;
            const u64 key = ((u64)(unsigned)v << 32) | (0xffffffffu - (unsigned)t);
            best = key > best ? key : best;
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const u64 o = __shfl_xor(best, off, 64);
            best = o > best ? o : best;
        }
        if (lane == 0) kred[wid] = best;
        __syncthreads();
        best = kred[0];
        for (int w = 1; w < 16; ++w) best = kred[w] > best ? kred[w] : best;
        const int donor = (int)(0xffffffffu - (unsigned)(best & 0xffffffffu)), dc = (int)(best >> 32);
        if (dc <= 0 || donor == e || donor < 0 || donor >= K) break;          // nothing to split from (uniform)
        double sqe = 0.0, sqd = 0.0;
        for (int d = tid; d < D; d += 1024) {
            const float s = (d & 1) ? -1.f / 1024.f : 1.f / 1024.f;
            const float v = c[(int64_t)donor * D + d];
            const float ve = v * (1.f + s), vd = v * (1.f - s);
            c[(int64_t)e * D + d] = ve;
            c[(int64_t)donor * D + d] = vd;
            sqe += (double)ve * (double)ve;
            sqd += (double)vd * (double)vd;
        }
        sqe = km_block_sum(sqe, red);
        sqd = km_block_sum(sqd, red);
        if (tid == 0) {
            csq[e] = (float)sqe;
            csq[donor] = (float)sqd;
            scnt[e] = dc / 2;
            scnt[donor] = dc - dc / 2;
        }
        ++ns;
        __syncthreads();
    }
    __syncthreads();
    for (int t = tid; t < K; t += 1024) cnt[t] = scnt[t];
    if (tid == 0 && ns) *nsplit += ns;
}

inline bool km_shape_ok(int N, int K, int D) {
    return K >= 1 && K <= KM_MAX_K && N >= K && N <= KM_MAX_N && D >= 1 && D <= KM_MAX_D;
}

inline size_t km_align(size_t v) { return (v + 255) & ~(size_t)255; }

}  // namespace

extern "C" int64_t rg_kmeans_assign_workspace(int N, int K, int D) {
    if (!km_shape_ok(N, K, D)) return 0;
    return K > BN ? km_align((size_t)N * sizeof(u64)) : 0;
}

extern "C" int rg_kmeans_assign(const float* x, const float* c, const float* csq, int N, int K, int D, int* label, float* score,
                                void* workspace, size_t workspace_bytes, hipStream_t stream) {
    RG_REQUIRE(x && c && csq && label && score, "rg_kmeans_assign: null argument");
    RG_REQUIRE(km_shape_ok(N, K, D), "rg_kmeans_assign: needs 1 <= K <= %d, K <= N <= %d, 1 <= D <= %d, got N=%d K=%d D=%d", KM_MAX_K,
               KM_MAX_N, KM_MAX_D, N, K, D);
    const size_t need = (size_t)rg_kmeans_assign_workspace(N, K, D);
    if (need && (!workspace || workspace_bytes < need)) {
        rg::set_error("rg_kmeans_assign: workspace of %zu bytes needed, %zu given", need, workspace_bytes);
        return RG_ERR_WORKSPACE;
    }
    u64* keys = need ? (u64*)workspace : nullptr;
    const bool vec = D % 4 == 0 && ((uintptr_t)x & 15) == 0 && ((uintptr_t)c & 15) == 0;
    rg::ProfScope prof(rg::FAM_MISC, stream, 2.0 * N * K * D, 4.0 * ((double)N * D + (double)K * D * rg::cdiv(N, BM)));
    if (keys && hipMemsetAsync(keys, 0xff, (size_t)N * sizeof(u64), stream) != hipSuccess) {
        rg::set_error("rg_kmeans_assign: clearing the keys failed");
        return RG_ERR_LAUNCH;
    }
    const dim3 grid(rg::cdiv(N, BM), rg::cdiv(K, BN));
    if (vec)
        hipLaunchKernelGGL(kmeans_assign_kernel<true>, grid, dim3(NT), 0, stream, x, c, csq, N, K, D, keys, label, score);
    else
        hipLaunchKernelGGL(kmeans_assign_kernel<false>, grid, dim3(NT), 0, stream, x, c, csq, N, K, D, keys, label, score);
    if (keys) hipLaunchKernelGGL(kmeans_decode_kernel, dim3(rg::cdiv(N, 256)), dim3(256), 0, stream, keys, N, label, score);
    return rg::check_launch("rg_kmeans_assign");
}

extern "C" int64_t rg_kmeans_tally_workspace(int N, int K) {
    if (!km_shape_ok(N, K, 1)) return 0;
    const size_t nb = (size_t)rg::cdiv(N, CHUNK);
    return km_align(nb * sizeof(double)) + km_align((size_t)N * sizeof(int)) + km_align(nb * K * sizeof(int));
}

extern "C" int rg_kmeans_tally(const int* label, const int* prev, const float* xsq, const float* score, int N, int K, int* cnt,
                               int* rowptr, int* order, int* changed, double* obj, void* workspace, size_t workspace_bytes,
                               hipStream_t stream) {
    RG_REQUIRE(label && prev && xsq && score && cnt && rowptr && order && changed && obj, "rg_kmeans_tally: null argument");
    RG_REQUIRE(km_shape_ok(N, K, 1), "rg_kmeans_tally: needs 1 <= K <= %d, K <= N <= %d, got N=%d K=%d", KM_MAX_K, KM_MAX_N, N, K);
    const size_t need = (size_t)rg_kmeans_tally_workspace(N, K);
    if (!workspace || workspace_bytes < need) {
        rg::set_error("rg_kmeans_tally: workspace of %zu bytes needed, %zu given", need, workspace_bytes);
        return RG_ERR_WORKSPACE;
    }
    const int nb = rg::cdiv(N, CHUNK);
    char* w = (char*)workspace;
    double* part = (double*)w;
    w += km_align((size_t)nb * sizeof(double));
    int* rank = (int*)w;
    w += km_align((size_t)N * sizeof(int));
    int* hist = (int*)w;
    rg::ProfScope prof(rg::FAM_MISC, stream, 0.0, 24.0 * N + 8.0 * nb * K);
    if (hipMemsetAsync(hist, 0, (size_t)nb * K * sizeof(int), stream) != hipSuccess ||
        hipMemsetAsync(changed, 0, sizeof(int), stream) != hipSuccess) {
        rg::set_error("rg_kmeans_tally: clearing the histogram failed");
        return RG_ERR_LAUNCH;
    }
    hipLaunchKernelGGL(kmeans_rank_kernel, dim3(nb), dim3(CHUNK), 0, stream, label, prev, xsq, score, N, K, rank, hist, part, changed);
    hipLaunchKernelGGL(kmeans_colscan_kernel, dim3(rg::cdiv(K, 256)), dim3(256), 0, stream, hist, nb, K, cnt, part, obj);
    hipLaunchKernelGGL(rg_scan_kernel<1024>, dim3(1), dim3(1024), 0, stream, cnt, K, rowptr);
    hipLaunchKernelGGL(kmeans_order_kernel, dim3(rg::cdiv(N, 256)), dim3(256), 0, stream, label, rank, hist, rowptr, N, K, order);
    return rg::check_launch("rg_kmeans_tally");
}

extern "C" int rg_kmeans_update(const float* x, const int* order, const int* rowptr, int N, int K, int D, float* c, float* csq,
                                hipStream_t stream) {
    RG_REQUIRE(x && order && rowptr && c && csq, "rg_kmeans_update: null argument");
    RG_REQUIRE(km_shape_ok(N, K, D), "rg_kmeans_update: needs 1 <= K <= %d, K <= N <= %d, 1 <= D <= %d, got N=%d K=%d D=%d", KM_MAX_K,
               KM_MAX_N, KM_MAX_D, N, K, D);
    rg::ProfScope prof(rg::FAM_MISC, stream, 0.0, 4.0 * ((double)N * D + (double)K * D));
    hipLaunchKernelGGL(kmeans_update_kernel, dim3(K, rg::cdiv(D, 256)), dim3(256), 0, stream, x, order, rowptr, N, D, c);
    hipLaunchKernelGGL(kmeans_csq_kernel, dim3(K), dim3(256), 0, stream, c, rowptr, D, csq);
    return rg::check_launch("rg_kmeans_update");
}

extern "C" int rg_kmeans_split(float* c, float* csq, int* cnt, int K, int D, int* nsplit, hipStream_t stream) {
    RG_REQUIRE(c && csq && cnt && nsplit, "rg_kmeans_split: null argument");
    RG_REQUIRE(K >= 1 && K <= KM_MAX_K && D >= 1 && D <= KM_MAX_D, "rg_kmeans_split: needs 1 <= K <= %d, 1 <= D <= %d, got K=%d D=%d",
               KM_MAX_K, KM_MAX_D, K, D);
    rg::ProfScope prof(rg::FAM_MISC, stream, 0.0, 8.0 * K);
    hipLaunchKernelGGL(kmeans_split_kernel, dim3(1), dim3(1024), 0, stream, c, csq, cnt, K, D, nsplit);
    return rg::check_launch("rg_kmeans_split");
}
