// k-reciprocal re-ranking (Zhong et al., CVPR 2017) after the initial ranking, entirely on the device:
//   Jaccard distance for DBSCAN        CC/clustercontrast/utils/faiss_rerank.py:31-127 (compute_jaccard_distance)
//   evaluation re-ranking              CC/clustercontrast/utils/rerank.py:32-99       (re_ranking)
// The reference fills a dense V[N][N] whose rows hold a few dozen to a few hundred non-zeros; here the encodings are row
// lists all the way (fixed capacity [N][cap] until the query expansion, CSR after it) plus their column lists, and the
// only dense objects are the similarity row blocks of the caller and the output.  No floating-point atomics: every sum
// has one fixed order, so two runs give the same bits and the Jaccard matrix is bit-symmetric.
#include "rg_common.h"

namespace {

constexpr int kMaxN = 65536;              // LDS bitmaps of the set kernels: 3 * N/8 bytes
constexpr int kJaccardMaxChunk = 16384;   // fp32 accumulators of one Jaccard workgroup: 64 KB, two workgroups per CU

// Turns the LDS bitmap `bits` (words of 32 columns) into the ascending index list out[0 .. min(count, cap)); returns the
// count.  `wpre` is `words` ints of LDS.
__device__ __forceinline__ int emit_bitmap(const unsigned* bits, int words, int* wpre, int* red, int* out, int cap) {
    const int per = (words + (int)blockDim.x - 1) / (int)blockDim.x;
    const int w0 = threadIdx.x * per, w1 = min(words, w0 + per);
    int s = 0;
    for (int w = w0; w < w1; ++w) s += __popc(bits[w]);
    int total;
    int run = block_excl_scan(s, red, &total);
    for (int w = w0; w < w1; ++w) {
        wpre[w] = run;
        run += __popc(bits[w]);
    }
    __syncthreads();
    if (out)
        for (int w = threadIdx.x; w < words; w += blockDim.x) {
            unsigned b = bits[w];
            int pos = wpre[w];
            while (b) {
                const int bit = __ffs(b) - 1;
                b &= b - 1;
                if (pos < cap) out[pos] = w * 32 + bit;
                ++pos;
            }
        }
    return total;
}

// R(i, k) = { j in rank[i][:k] : i in rank[j][:k] } for k = kf, united with every R(c, kh), c in R(i, kf), that lies to more
// than two thirds inside R(i, kf); one workgroup per row, output sorted and unique.  Indices outside [0, N) never match.
__global__ __launch_bounds__(256) void rerank_expand_kernel(const int* __restrict__ rank, int N, int R, int kf, int kh, int cap,
                                                            int* __restrict__ sets, int* __restrict__ counts) {
    extern __shared__ int sm[];
    __shared__ int red[17];
    const int words = (N + 31) >> 5, tid = threadIdx.x, i = blockIdx.x;
    unsigned* bitA = reinterpret_cast<unsigned*>(sm);
    unsigned* bitB = bitA + words;
    int* wpre = sm + 2 * words;
    int* fwd = wpre + words;
    int* isR = fwd + kf;
    int* len = isR + kf;
    int* inter = len + kf;
    int* mem = inter + kf;
    for (int w = tid; w < words; w += 256) bitA[w] = 0u;
    for (int p = tid; p < kf; p += 256) {
        fwd[p] = rank[(int64_t)i * R + p];
        len[p] = 0;
        inter[p] = 0;
    }
    __syncthreads();
    for (int p = tid; p < kf; p += 256) {
        const int j = fwd[p];
        bool found = false;
        if ((unsigned)j < (unsigned)N) {
            for (int q = 0; q < kf; ++q) found |= rank[(int64_t)j * R + q] == i;
            if (found) atomicOr(&bitA[j >> 5], 1u << (j & 31));
        }
        isR[p] = found;
    }
    __syncthreads();
    for (int w = tid; w < words; w += 256) bitB[w] = bitA[w];
    for (int idx = tid; idx < kf * kh; idx += 256) {
        const int p = idx / kh, q = idx - p * kh;
        int m = -1;
        if (isR[p]) {
            const int c = fwd[p], mm = rank[(int64_t)c * R + q];
            if ((unsigned)mm < (unsigned)N) {
                bool found = false;
                for (int t = 0; t < kh; ++t) found |= rank[(int64_t)mm * R + t] == c;
                if (found) {
                    m = mm;
                    atomicAdd(&len[p], 1);
                    if ((bitA[mm >> 5] >> (mm & 31)) & 1u) atomicAdd(&inter[p], 1);
                }
            }
        }
        mem[idx] = m;
    }
    __syncthreads();
    for (int idx = tid; idx < kf * kh; idx += 256) {
        const int m = mem[idx];
        if (m < 0) continue;
        const int p = idx / kh;
        if ((double)inter[p] > 2.0 / 3.0 * (double)len[p]) atomicOr(&bitB[m >> 5], 1u << (m & 31));
    }
    __syncthreads();
    const int n = emit_bitmap(bitB, words, wpre, red, sets + (int64_t)i * cap, cap);
    if (tid == 0) counts[i] = n;
}

// w[i][e] = softmax over the row's set of -(2 - 2 x_i . x_e)  (FEAT) or exp(-orig[i][e]) / sum  (!FEAT)
template <bool FEAT>
__global__ __launch_bounds__(256) void rerank_weights_kernel(const float* __restrict__ src, int D, int N, const int* __restrict__ sets,
                                                             const int* __restrict__ counts, int cap, float* __restrict__ w) {
    extern __shared__ float smf[];
    __shared__ float red[16];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, i = blockIdx.x;
    const int n = min(counts[i], cap);
    const int* set = sets + (int64_t)i * cap;
    float* d = smf + (FEAT ? D : 0);      // x_i first: its 16-byte reads need the array's own alignment
    if (FEAT) {
        float* xi = smf;
        const float* xr = src + (int64_t)i * D;
        for (int t = tid; t < D; t += 256) xi[t] = xr[t];
        __syncthreads();
        for (int e = wid; e < n; e += 4) {
            const int j = set[e];
            if ((unsigned)j >= (unsigned)N) {      // not a row: weight 0
                if (lane == 0) d[e] = -INFINITY;
                continue;
            }
            const float* xe = src + (int64_t)j * D;
            float s = 0.f;
            if ((D & 3) == 0) {
                const float4* xe4 = reinterpret_cast<const float4*>(xe);
                const float4* xi4 = reinterpret_cast<const float4*>(xi);
                for (int t = lane; t < (D >> 2); t += 64) {
                    const float4 a = xe4[t], b = xi4[t];
                    s += a.x * b.x + a.y * b.y + a.z * b.z + a.w * b.w;
                }
            } else {
                for (int t = lane; t < D; t += 64) s += xe[t] * xi[t];
            }
            s = rg_wave_sum(s);
            if (lane == 0) d[e] = -(2.f - 2.f * s);
        }
    } else {
        const float* orow = src + (int64_t)i * N;
        for (int e = tid; e < n; e += 256) d[e] = (unsigned)set[e] < (unsigned)N ? -orow[set[e]] : -INFINITY;
    }
    __syncthreads();
    float mx = 0.f;
    if (FEAT) {
        mx = -INFINITY;
        for (int e = tid; e < n; e += 256) mx = fmaxf(mx, d[e]);
        mx = rg_block_max(mx, red);
    }
    float s = 0.f;
    for (int e = tid; e < n; e += 256) {
        const float v = expf(d[e] - mx);
        d[e] = v;
        s += v;
    }
    s = rg_block_sum(s, red);
    for (int e = tid; e < n; e += 256) w[(int64_t)i * cap + e] = d[e] / s;
}

// Local query expansion: row i = mean of the sparse rows rank[i][:k2] (rank == NULL: row i itself, k2 == 1).
// FILL == false counts the union's columns, FILL == true writes the CSR row: columns ascending, terms added in rank
// order and divided by k2 (the order numpy's mean over the leading axis uses).
template <bool FILL>
__global__ __launch_bounds__(256) void rerank_qe_kernel(const int* __restrict__ rank, int R, int k2, int N, const int* __restrict__ sets,
                                                        const float* __restrict__ w, const int* __restrict__ counts, int cap,
                                                        int* __restrict__ rowcnt, const int* __restrict__ rowptr,
                                                        int* __restrict__ cols, float* __restrict__ vals) {
    extern __shared__ int sm[];
    __shared__ int red[17];
    __shared__ int src[64];
    const int words = (N + 31) >> 5, tid = threadIdx.x, i = blockIdx.x;
    unsigned* bits = reinterpret_cast<unsigned*>(sm);
    int* wpre = sm + words;
    for (int t = tid; t < words; t += 256) bits[t] = 0u;
    if (tid < k2) {
        const int r = rank ? rank[(int64_t)i * R + tid] : i;
        src[tid] = (unsigned)r < (unsigned)N ? r : -1;
    }
    __syncthreads();
    for (int l = 0; l < k2; ++l) {
        const int r = src[l];
        if (r < 0) continue;
        const int n = min(counts[r], cap);
        for (int e = tid; e < n; e += 256) {
            const int c = sets[(int64_t)r * cap + e];
            if ((unsigned)c < (unsigned)N) atomicOr(&bits[c >> 5], 1u << (c & 31));
        }
    }
    __syncthreads();
    const int total = emit_bitmap(bits, words, wpre, red, nullptr, 0);
    if (!FILL) {
        if (tid == 0) rowcnt[i] = total;
        return;
    }
    const int64_t base = rowptr[i];
    const float div = (float)k2;
    for (int t = tid; t < words; t += 256) {
        unsigned b = bits[t];
        int pos = wpre[t];
        while (b) {
            const int c = t * 32 + __ffs(b) - 1;
            b &= b - 1;
            float acc = 0.f;
            for (int l = 0; l < k2; ++l) {
                const int r = src[l];
                if (r < 0) continue;
                const int* set = sets + (int64_t)r * cap;
                int lo = 0, hi = min(counts[r], cap);
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if (set[mid] < c) lo = mid + 1; else hi = mid;
                }
                if (lo < min(counts[r], cap) && set[lo] == c) acc += w[(int64_t)r * cap + lo];
            }
            cols[base + pos] = c;
            vals[base + pos] = acc / div;
            ++pos;
        }
    }
}

__global__ void rerank_col_count_kernel(const int* __restrict__ cols, int64_t nnz, int* __restrict__ colcnt) {
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < nnz; p += (int64_t)gridDim.x * blockDim.x)
        atomicAdd(&colcnt[cols[p]], 1);
}

// column lists of the CSR encoding: one wave per row; the order inside a column is whatever the integer cursor hands
// out, which no result depends on (the rows of one column are distinct, each accumulator gets one term per column)
__global__ __launch_bounds__(256) void rerank_col_fill_kernel(const int* __restrict__ rowptr, const int* __restrict__ cols,
                                                              const float* __restrict__ vals, int N, int* __restrict__ cursor,
                                                              int* __restrict__ crow, float* __restrict__ cval) {
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (i >= N) return;
    for (int p = rowptr[i] + lane; p < rowptr[i + 1]; p += 64) {
        const int q = atomicAdd(&cursor[cols[p]], 1);
        crow[q] = i;
        cval[q] = vals[p];
    }
}

// out[i][j - col_off] = 1 - m / (2 - m), m = sum over the non-zero columns c of row i, ascending, of min(V[i][c], V[j][c]),
// for the columns j of one chunk [j0, j0 + W): the accumulators sit in LDS, all threads walk column c's list, one barrier
// per column.  orig != NULL: (1 - lambda) * jaccard + lambda * orig[i][j] (re_ranking); clamp: negative results become 0.
__global__ __launch_bounds__(256) void rerank_jaccard_kernel(const int* __restrict__ rowptr, const int* __restrict__ cols,
                                                             const float* __restrict__ vals, const int* __restrict__ colptr,
                                                             const int* __restrict__ crow, const float* __restrict__ cval, int N,
                                                             int col_off, int W, const float* __restrict__ orig, float one_minus_lambda,
                                                             float lambda, int clamp, float* __restrict__ out, int64_t ldo) {
    extern __shared__ float acc[];
    const int tid = threadIdx.x, i = blockIdx.x;
    const int j0 = col_off + blockIdx.y * W, j1 = min(N, j0 + W);
    for (int t = tid; t < j1 - j0; t += 256) acc[t] = 0.f;
    __syncthreads();
    const int pb = rowptr[i], pe = rowptr[i + 1];
    int b = 0, e = 0;
    float vi = 0.f;
    if (pb < pe) {
        const int c = cols[pb];
        vi = vals[pb];
        b = colptr[c];
        e = colptr[c + 1];
    }
    for (int p = pb; p < pe; ++p) {
        int nb = 0, ne = 0;
        float nvi = 0.f;
        if (p + 1 < pe) {                 // the next column's bounds are in flight while this one is walked
            const int c = cols[p + 1];
            nvi = vals[p + 1];
            nb = colptr[c];
            ne = colptr[c + 1];
        }
        for (int q = b + tid; q < e; q += 256) {
            const int j = crow[q];
            if (j >= j0 && j < j1) acc[j - j0] += fminf(vi, cval[q]);
        }
        __syncthreads();
        b = nb;
        e = ne;
        vi = nvi;
    }
    float* orow = out + (int64_t)i * ldo + (j0 - col_off);
    for (int t = tid; t < j1 - j0; t += 256) {
        const float m = acc[t];
        float v = 1.f - m / (2.f - m);
        if (orig) v = __fadd_rn(__fmul_rn(v, one_minus_lambda), __fmul_rn(orig[(int64_t)i * N + j0 + t], lambda));
        if (clamp && v < 0.f) v = 0.f;
        orow[t] = v;
    }
}

// element (r, c) of [[qq, qg], [qg^T, gg]]
__device__ __forceinline__ float assembled(const float* __restrict__ qg, const float* __restrict__ qq, const float* __restrict__ gg,
                                           int Q, int G, int r, int c) {
    if (r < Q) return c < Q ? qq[(int64_t)r * Q + c] : qg[(int64_t)r * G + (c - Q)];
    return c < Q ? qg[(int64_t)c * G + (r - Q)] : gg[(int64_t)(r - Q) * G + (c - Q)];
}

// colmax[c] = max_r A[r][c]^2 as the bit pattern of a non-negative float (integer max: order-free)
__global__ __launch_bounds__(256) void rerank_sq_colmax_kernel(const float* __restrict__ qg, const float* __restrict__ qq,
                                                               const float* __restrict__ gg, int Q, int G, int rows_per,
                                                               unsigned* __restrict__ colmax) {
    const int N = Q + G, c = blockIdx.x * 256 + threadIdx.x;
    if (c >= N) return;
    const int r0 = blockIdx.y * rows_per, r1 = min(N, r0 + rows_per);
    float m = 0.f;
    for (int r = r0; r < r1; ++r) {
        const float v = assembled(qg, qq, gg, Q, G, r, c);
        m = fmaxf(m, v * v);
    }
    atomicMax(&colmax[c], __float_as_uint(m));
}

// orig[c][r] = A[r][c]^2 / colmax[c]  (32 x 32 tiles through LDS: reads and writes both coalesced)
__global__ __launch_bounds__(256) void rerank_orig_dist_kernel(const float* __restrict__ qg, const float* __restrict__ qq,
                                                               const float* __restrict__ gg, int Q, int G,
                                                               const float* __restrict__ colmax, float* __restrict__ orig) {
    __shared__ float tile[32][33];
    const int N = Q + G, tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int c0 = blockIdx.x * 32, r0 = blockIdx.y * 32;
    for (int y = ty; y < 32; y += 8) {
        const int r = r0 + y, c = c0 + tx;
        float v = 0.f;
        if (r < N && c < N) {
            v = assembled(qg, qq, gg, Q, G, r, c);
            v = v * v;
        }
        tile[y][tx] = v;
    }
    __syncthreads();
    for (int y = ty; y < 32; y += 8) {
        const int c = c0 + y, r = r0 + tx;
        if (r < N && c < N) orig[(int64_t)c * N + r] = tile[tx][y] / colmax[c];
    }
}

inline bool sets_ok(int N, int cap) { return N > 0 && N <= kMaxN && cap > 0; }

}  // namespace

extern "C" int rg_rerank_expand(const int* rank, int N, int R, int kf, int kh, int* sets, int* counts, int cap, hipStream_t stream) {
    RG_REQUIRE(rank && sets && counts && sets_ok(N, cap), "rg_rerank_expand: bad arguments (1 <= N <= %d)", kMaxN);
    RG_REQUIRE(R > 0 && kf > 0 && kh > 0 && kf <= R && kh <= kf && kf <= 1024,
               "rg_rerank_expand: need 1 <= kh <= kf <= R (columns of rank) and kf <= 1024, got kf=%d kh=%d R=%d", kf, kh, R);
    const int words = (N + 31) / 32;
    const size_t lds = sizeof(int) * ((size_t)3 * words + 4 * (size_t)kf + (size_t)kf * kh);
    RG_REQUIRE(lds <= 60 * 1024, "rg_rerank_expand: kf * kh = %d does not fit the workgroup's LDS", kf * kh);
    rg::ProfScope prof(rg::FAM_CM, stream, 0.0, 4.0 * N * (double)kf * (kf + (double)kh * kh));
    hipLaunchKernelGGL(rerank_expand_kernel, dim3(N), dim3(256), lds, stream, rank, N, R, kf, kh, cap, sets, counts);
    return rg::check_launch("rg_rerank_expand");
}

extern "C" int rg_rerank_weights_feat(const float* x, int N, int D, const int* sets, const int* counts, int cap, float* w,
                                      hipStream_t stream) {
    RG_REQUIRE(x && sets && counts && w && sets_ok(N, cap) && D > 0, "rg_rerank_weights_feat: bad arguments");
    const size_t lds = sizeof(float) * ((size_t)cap + D);
    RG_REQUIRE(lds <= 60 * 1024, "rg_rerank_weights_feat: D + cap = %d floats do not fit the workgroup's LDS", D + cap);
    rg::ProfScope prof(rg::FAM_CM, stream, 0.0, 0.0);
    hipLaunchKernelGGL(rerank_weights_kernel<true>, dim3(N), dim3(256), lds, stream, x, D, N, sets, counts, cap, w);
    return rg::check_launch("rg_rerank_weights_feat");
}

extern "C" int rg_rerank_weights_dist(const float* orig, int N, const int* sets, const int* counts, int cap, float* w,
                                      hipStream_t stream) {
    RG_REQUIRE(orig && sets && counts && w && sets_ok(N, cap), "rg_rerank_weights_dist: bad arguments");
    const size_t lds = sizeof(float) * (size_t)cap;
    RG_REQUIRE(lds <= 60 * 1024, "rg_rerank_weights_dist: cap = %d floats do not fit the workgroup's LDS", cap);
    rg::ProfScope prof(rg::FAM_CM, stream, 0.0, 0.0);
    hipLaunchKernelGGL(rerank_weights_kernel<false>, dim3(N), dim3(256), lds, stream, orig, 0, N, sets, counts, cap, w);
    return rg::check_launch("rg_rerank_weights_dist");
}

static int qe_args_ok(const char* who, const int* rank, int R, int k2, int N, const int* sets, const int* counts, int cap) {
    RG_REQUIRE(sets && counts && sets_ok(N, cap), "%s: bad arguments (1 <= N <= %d)", who, kMaxN);
    RG_REQUIRE(k2 >= 1 && k2 <= 64 && (rank ? (R >= k2) : (k2 == 1)),
               "%s: need 1 <= k2 <= min(64, columns of rank) (k2 == 1 when rank is NULL), got k2=%d R=%d", who, k2, R);
    return RG_OK;
}

extern "C" int rg_rerank_qe_count(const int* rank, int R, int k2, int N, const int* sets, const int* counts, int cap, int* rowcnt,
                                  int* rowptr, hipStream_t stream) {
    if (int st = qe_args_ok("rg_rerank_qe_count", rank, R, k2, N, sets, counts, cap)) return st;
    RG_REQUIRE(rowcnt && rowptr, "rg_rerank_qe_count: bad arguments");
    const int words = (N + 31) / 32;
    rg::ProfScope prof(rg::FAM_CM, stream, 0.0, 0.0);
    hipLaunchKernelGGL(rerank_qe_kernel<false>, dim3(N), dim3(256), sizeof(int) * 2 * (size_t)words, stream, rank, R, k2, N, sets,
                       (const float*)nullptr, counts, cap, rowcnt, (const int*)nullptr, (int*)nullptr, (float*)nullptr);
    hipLaunchKernelGGL(rg_scan_kernel<1024>, dim3(1), dim3(1024), 0, stream, rowcnt, N, rowptr);
    return rg::check_launch("rg_rerank_qe_count");
}

extern "C" int rg_rerank_qe_fill(const int* rank, int R, int k2, int N, const int* sets, const float* w, const int* counts, int cap,
                                 const int* rowptr, int* cols, float* vals, hipStream_t stream) {
    if (int st = qe_args_ok("rg_rerank_qe_fill", rank, R, k2, N, sets, counts, cap)) return st;
    RG_REQUIRE(w && rowptr && cols && vals, "rg_rerank_qe_fill: bad arguments");
    const int words = (N + 31) / 32;
    rg::ProfScope prof(rg::FAM_CM, stream, 0.0, 0.0);
    hipLaunchKernelGGL(rerank_qe_kernel<true>, dim3(N), dim3(256), sizeof(int) * 2 * (size_t)words, stream, rank, R, k2, N, sets, w,
                       counts, cap, (int*)nullptr, rowptr, cols, vals);
    return rg::check_launch("rg_rerank_qe_fill");
}

extern "C" int rg_rerank_columns(const int* rowptr, const int* cols, const float* vals, int N, int64_t nnz, int* colptr, int* cursor,
                                 int* crow, float* cval, hipStream_t stream) {
    RG_REQUIRE(rowptr && cols && vals && colptr && cursor && crow && cval && N > 0 && N <= kMaxN && nnz > 0 && nnz < ((int64_t)1 << 31),
               "rg_rerank_columns: bad arguments");
    rg::ProfScope prof(rg::FAM_CM, stream, 0.0, 16.0 * (double)nnz);
    if (hipMemsetAsync(cursor, 0, sizeof(int) * (size_t)N, stream) != hipSuccess) {
        rg::set_error("rg_rerank_columns: hipMemsetAsync failed");
        return RG_ERR_LAUNCH;
    }
    int64_t g = rg::cdiv64(nnz, 256);
    if (g > 4096) g = 4096;
    hipLaunchKernelGGL(rerank_col_count_kernel, dim3((unsigned)g), dim3(256), 0, stream, cols, (int64_t)nnz, cursor);
    hipLaunchKernelGGL(rg_scan_kernel<1024>, dim3(1), dim3(1024), 0, stream, cursor, N, colptr);
    if (hipMemcpyAsync(cursor, colptr, sizeof(int) * (size_t)N, hipMemcpyDeviceToDevice, stream) != hipSuccess) {
        rg::set_error("rg_rerank_columns: hipMemcpyAsync failed");
        return RG_ERR_LAUNCH;
    }
    hipLaunchKernelGGL(rerank_col_fill_kernel, dim3(rg::cdiv(N, 4)), dim3(256), 0, stream, rowptr, cols, vals, N, cursor, crow, cval);
    return rg::check_launch("rg_rerank_columns");
}

extern "C" int rg_rerank_jaccard(const int* rowptr, const int* cols, const float* vals, const int* colptr, const int* crow,
                                 const float* cval, int N, int rows, int col_off, const float* orig, float lambda_value, int clamp,
                                 float* out, int chunk, hipStream_t stream) {
    RG_REQUIRE(rowptr && cols && vals && colptr && crow && cval && out && N > 0 && N <= kMaxN, "rg_rerank_jaccard: bad arguments");
    RG_REQUIRE(rows > 0 && rows <= N && col_off >= 0 && col_off < N, "rg_rerank_jaccard: rows=%d col_off=%d outside N=%d", rows, col_off, N);
    RG_REQUIRE(chunk >= 0 && chunk <= kJaccardMaxChunk, "rg_rerank_jaccard: chunk must be 0 (automatic) or at most %d columns, got %d",
               kJaccardMaxChunk, chunk);
    const int width = N - col_off;
    int W = chunk;
    if (W == 0) {                         // equal chunks of at most 64 KB of accumulators
        const int parts = rg::cdiv(width, kJaccardMaxChunk);
        W = rg::cdiv(rg::cdiv(width, parts), 64) * 64;
    }
    if (W > width) W = width;
    const int parts = rg::cdiv(width, W);
    rg::ProfScope prof(rg::FAM_CM, stream, 0.0, 4.0 * rows * (double)width);
    hipLaunchKernelGGL(rerank_jaccard_kernel, dim3(rows, parts), dim3(256), sizeof(float) * (size_t)W, stream, rowptr, cols, vals, colptr,
                       crow, cval, N, col_off, W, orig, (float)(1.0 - (double)lambda_value), lambda_value, clamp, out, (int64_t)width);
    return rg::check_launch("rg_rerank_jaccard");
}

extern "C" int rg_rerank_orig_dist(const float* q_g, const float* q_q, const float* g_g, int Q, int G, float* colmax, float* orig,
                                   hipStream_t stream) {
    RG_REQUIRE(q_g && q_q && g_g && colmax && orig && Q > 0 && G > 0 && Q + (int64_t)G <= kMaxN, "rg_rerank_orig_dist: bad arguments");
    const int N = Q + G;
    rg::ProfScope prof(rg::FAM_CM, stream, 0.0, 12.0 * N * (double)N);
    if (hipMemsetAsync(colmax, 0, sizeof(float) * (size_t)N, stream) != hipSuccess) {
        rg::set_error("rg_rerank_orig_dist: hipMemsetAsync failed");
        return RG_ERR_LAUNCH;
    }
    const int segs = rg::cdiv(N, 512), rows_per = rg::cdiv(N, segs);
    hipLaunchKernelGGL(rerank_sq_colmax_kernel, dim3(rg::cdiv(N, 256), segs), dim3(256), 0, stream, q_g, q_q, g_g, Q, G, rows_per,
                       reinterpret_cast<unsigned*>(colmax));
    hipLaunchKernelGGL(rerank_orig_dist_kernel, dim3(rg::cdiv(N, 32), rg::cdiv(N, 32)), dim3(256), 0, stream, q_g, q_q, g_g, Q, G, colmax,
                       orig);
    return rg::check_launch("rg_rerank_orig_dist");
}
