// DBSCAN on a precomputed, symmetric distance matrix d [N][ld], entirely on the device: the clustering step between
// compute_jaccard_distance and generate_cluster_features in CC/examples/cluster_contrast_train_usl.py:146-200, with the
// labels scikit-learn's DBSCAN(metric='precomputed') gives:
//   adj[i][j] = d[i][j] <= eps (the diagonal is an entry like any other), core[i] = |adj[i]| >= min_samples,
//   clusters = connected components of the core-core graph, numbered in ascending order of their lowest core index,
//   a non-core point takes the lowest cluster number among its core neighbours, or -1.
// The matrix is read twice (count, fill) into CSR neighbour lists; everything after that works on the lists.  Only integer
// atomics are used and every result is a fixed point that does not depend on the order they land in (the root of a
// component is its lowest core index), so two runs give the same bits.
#include "rg_common.h"
#include <hip/hip_fp16.h>
#include <limits.h>

namespace {

constexpr int kMaxN = 65536;
constexpr int kRowsPerBlock = 4;          // one wavefront per matrix row / per CSR row

__device__ __forceinline__ float to_f32(float v) { return v; }
__device__ __forceinline__ float to_f32(__half v) { return __half2float(v); }

// One wavefront walks row i in ascending column order: an unaligned head, 16-byte vectors, a tail.
// FILL == false: cnt[i] = entries <= eps.  FILL == true: nbr[rowptr[i] ..] = their columns, ascending (the position of an
// entry is the popcount of the ballots below it, so no cursor is shared), and core[i] = row length >= min_samples.
template <typename T, bool FILL>
__global__ __launch_bounds__(256) void dbscan_row_kernel(const T* __restrict__ d, int N, int64_t ld, float eps, int min_samples,
                                                         int* __restrict__ cnt, const int* __restrict__ rowptr, int* __restrict__ nbr,
                                                         int* __restrict__ core) {
    constexpr int VEC = 16 / (int)sizeof(T);
    const int lane = threadIdx.x & 63, i = blockIdx.x * kRowsPerBlock + (threadIdx.x >> 6);
    if (i >= N) return;                   // whole wavefronts leave: the ballots below stay full
    const T* row = d + (int64_t)i * ld;
    const unsigned long long below = (1ull << lane) - 1ull;
    int pos = 0, end = 0, mine = 0;
    if (FILL) {
        pos = rowptr[i];
        end = rowptr[i + 1];
        if (lane == 0) core[i] = (end - pos) >= min_samples;
    }
    // columns [c0, c1), one per lane and step
    auto scalar_span = [&](int c0, int c1) {
        for (int c = c0; c < c1; c += 64) {
            const int j = c + lane;
            const bool in = j < c1 && to_f32(row[j]) <= eps;
            if (FILL) {
                const unsigned long long b = __ballot(in);
                const int p = pos + __popcll(b & below);
                if (in && p < end) nbr[p] = j;
                pos += __popcll(b);
            } else {
                mine += in;
            }
        }
    };
    const int head = min(N, (int)(((16u - (unsigned)((uintptr_t)row & 15u)) & 15u) / sizeof(T)));
    scalar_span(0, head);
    const int nvec = (N - head) / VEC;
    for (int v0 = 0; v0 < nvec; v0 += 64) {
        const int v = v0 + lane;
        bool in[VEC];
#pragma unroll
        for (int k = 0; k < VEC; ++k) in[k] = false;
        if (v < nvec) {
            const uint4 raw = *reinterpret_cast<const uint4*>(row + head + (int64_t)v * VEC);
            T e[VEC];
            __builtin_memcpy(e, &raw, 16);
#pragma unroll
            for (int k = 0; k < VEC; ++k) in[k] = to_f32(e[k]) <= eps;
        }
        if (FILL) {
            int before = 0, step = 0;
#pragma unroll
            for (int k = 0; k < VEC; ++k) {
                const unsigned long long b = __ballot(in[k]);
                before += __popcll(b & below);
                step += __popcll(b);
            }
            int p = pos + before;
            const int j0 = head + v * VEC;
#pragma unroll
            for (int k = 0; k < VEC; ++k)
                if (in[k]) {
                    if (p < end) nbr[p] = j0 + k;
                    ++p;
                }
            pos += step;
        } else {
#pragma unroll
            for (int k = 0; k < VEC; ++k) mine += in[k];
        }
    }
    scalar_span(head + nvec * VEC, N);
    if (!FILL) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) mine += __shfl_xor(mine, off, 64);
        if (lane == 0) cnt[i] = mine;
    }
}

// parent[] holds a forest over the core points with parent[x] <= x (-1 for the others); every access while it is being
// built is an agent-scope atomic, and every value ever stored in parent[x] is an ancestor of x, so a stale read is still a
// valid one and every walk strictly descends: at most N steps.
__device__ __forceinline__ int parent_of(int* parent, int x) { return __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

template <bool HALVE>
__device__ __forceinline__ int find_root(int* parent, int x) {
    int p = parent_of(parent, x);
    while (p != x) {
        const int g = parent_of(parent, p);
        if (HALVE && g != p) __hip_atomic_store(parent + x, g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        x = p;
        p = g;
    }
    return x;
}

// the higher root is hooked under the lower one; a failed compare-and-swap means that root was hooked by another thread in
// the meantime, and the walk goes on from there (the pair of roots only descends: at most 2 N attempts)
__device__ __forceinline__ void unite(int* parent, int a, int b) {
    for (;;) {
        a = find_root<true>(parent, a);
        b = find_root<true>(parent, b);
        if (a == b) return;
        if (a < b) {
            const int t = a;
            a = b;
            b = t;
        }
        if (atomicCAS(parent + a, a, b) == a) return;
    }
}

__global__ void dbscan_parent_init_kernel(const int* __restrict__ core, int N, int* __restrict__ parent) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < N) parent[i] = core[i] ? i : -1;
}

// one wavefront per core row; every core-core edge is taken once, from its higher end (the matrix is symmetric)
__global__ __launch_bounds__(256) void dbscan_hook_kernel(const int* __restrict__ rowptr, const int* __restrict__ nbr,
                                                          const int* __restrict__ core, int N, int* parent) {
    const int lane = threadIdx.x & 63, i = blockIdx.x * kRowsPerBlock + (threadIdx.x >> 6);
    if (i >= N || !core[i]) return;
    for (int p = rowptr[i] + lane; p < rowptr[i + 1]; p += 64) {
        const int j = nbr[p];
        if ((unsigned)j < (unsigned)i && core[j]) unite(parent, i, j);
    }
}

// parent[i] = root of i (the hooks are complete: roots no longer change, and nothing but this thread writes parent[i])
__global__ void dbscan_flatten_kernel(int N, int* parent) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N || parent_of(parent, i) < 0) return;
    const int r = find_root<false>(parent, i);
    __hip_atomic_store(parent + i, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ void dbscan_root_flag_kernel(const int* __restrict__ parent, int N, int* __restrict__ isroot) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < N) isroot[i] = parent[i] == i;
}

// rootnum = exclusive prefix sum of the root flags: the cluster number of a root.  One wavefront per point.
__global__ __launch_bounds__(256) void dbscan_label_kernel(const int* __restrict__ rowptr, const int* __restrict__ nbr,
                                                           const int* __restrict__ parent, const int* __restrict__ rootnum, int N,
                                                           int64_t* __restrict__ labels) {
    const int lane = threadIdx.x & 63, i = blockIdx.x * kRowsPerBlock + (threadIdx.x >> 6);
    if (i >= N) return;
    const int own = parent[i];
    if (own >= 0) {
        if (lane == 0) labels[i] = rootnum[min(own, N - 1)];
        return;
    }
    int best = INT_MAX;
    for (int p = rowptr[i] + lane; p < rowptr[i + 1]; p += 64) {
        const int j = nbr[p];
        if ((unsigned)j < (unsigned)N) {
            const int r = parent[j];
            if (r >= 0) best = min(best, rootnum[min(r, N - 1)]);
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) best = min(best, __shfl_xor(best, off, 64));
    if (lane == 0) labels[i] = best == INT_MAX ? -1 : best;
}

// *count += entries of the upper triangle whose bits differ from their mirror's (32 x 32 tiles, both reads coalesced)
template <typename U>
__global__ __launch_bounds__(256) void dbscan_asym_kernel(const U* __restrict__ d, int N, int64_t ld, int* __restrict__ count) {
    __shared__ U tile[32][33];
    if (blockIdx.x < blockIdx.y) return;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int c0 = blockIdx.x * 32, r0 = blockIdx.y * 32;
    for (int y = ty; y < 32; y += 8) {
        const int r = c0 + y, c = r0 + tx;          // the mirrored tile, stored transposed
        tile[tx][y] = (r < N && c < N) ? d[(int64_t)r * ld + c] : (U)0;
    }
    __syncthreads();
    int bad = 0;
    for (int y = ty; y < 32; y += 8) {
        const int r = r0 + y, c = c0 + tx;
        if (r < N && c < N) bad += d[(int64_t)r * ld + c] != tile[y][tx];
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) bad += __shfl_xor(bad, off, 64);
    if ((threadIdx.x & 63) == 0 && bad) atomicAdd(count, bad);
}

inline bool matrix_ok(const void* d, int is_half, int N, int64_t ld) {
    return d && (is_half == 0 || is_half == 1) && N > 0 && N <= kMaxN && ld >= N && ((uintptr_t)d & (is_half ? 1u : 3u)) == 0;
}
inline bool lists_ok(const int* rowptr, const int* nbr, int N) { return rowptr && nbr && N > 0 && N <= kMaxN; }

}  // namespace

extern "C" int rg_dbscan_count(const void* d, int is_half, int N, int64_t ld, float eps, int* cnt, int* rowptr, hipStream_t stream) {
    RG_REQUIRE(matrix_ok(d, is_half, N, ld) && cnt && rowptr, "rg_dbscan_count: bad arguments (1 <= N <= %d, ld >= N)", kMaxN);
    RG_REQUIRE(eps == eps, "rg_dbscan_count: eps is NaN");
    rg::ProfScope prof(rg::FAM_MISC, stream, 0.0, (is_half ? 2.0 : 4.0) * N * (double)N);
    const dim3 grid(rg::cdiv(N, kRowsPerBlock));
    if (is_half)
        hipLaunchKernelGGL((dbscan_row_kernel<__half, false>), grid, dim3(256), 0, stream, (const __half*)d, N, ld, eps, 0, cnt,
                           (const int*)nullptr, (int*)nullptr, (int*)nullptr);
    else
        hipLaunchKernelGGL((dbscan_row_kernel<float, false>), grid, dim3(256), 0, stream, (const float*)d, N, ld, eps, 0, cnt,
                           (const int*)nullptr, (int*)nullptr, (int*)nullptr);
    hipLaunchKernelGGL(rg_scan_kernel<1024>, dim3(1), dim3(1024), 0, stream, cnt, N, rowptr);
    return rg::check_launch("rg_dbscan_count");
}

extern "C" int rg_dbscan_fill(const void* d, int is_half, int N, int64_t ld, float eps, int min_samples, const int* rowptr, int* nbr,
                              int* core, hipStream_t stream) {
    RG_REQUIRE(matrix_ok(d, is_half, N, ld) && rowptr && nbr && core, "rg_dbscan_fill: bad arguments (1 <= N <= %d, ld >= N)", kMaxN);
    RG_REQUIRE(eps == eps && min_samples >= 1, "rg_dbscan_fill: need min_samples >= 1 and eps not NaN, got min_samples=%d", min_samples);
    rg::ProfScope prof(rg::FAM_MISC, stream, 0.0, (is_half ? 2.0 : 4.0) * N * (double)N);
    const dim3 grid(rg::cdiv(N, kRowsPerBlock));
    if (is_half)
        hipLaunchKernelGGL((dbscan_row_kernel<__half, true>), grid, dim3(256), 0, stream, (const __half*)d, N, ld, eps, min_samples,
                           (int*)nullptr, rowptr, nbr, core);
    else
        hipLaunchKernelGGL((dbscan_row_kernel<float, true>), grid, dim3(256), 0, stream, (const float*)d, N, ld, eps, min_samples,
                           (int*)nullptr, rowptr, nbr, core);
    return rg::check_launch("rg_dbscan_fill");
}

extern "C" int rg_dbscan_components(const int* rowptr, const int* nbr, const int* core, int N, int* parent, hipStream_t stream) {
    RG_REQUIRE(lists_ok(rowptr, nbr, N) && core && parent, "rg_dbscan_components: bad arguments (1 <= N <= %d)", kMaxN);
    rg::ProfScope prof(rg::FAM_MISC, stream, 0.0, 0.0);
    hipLaunchKernelGGL(dbscan_parent_init_kernel, dim3(rg::cdiv(N, 256)), dim3(256), 0, stream, core, N, parent);
    hipLaunchKernelGGL(dbscan_hook_kernel, dim3(rg::cdiv(N, kRowsPerBlock)), dim3(256), 0, stream, rowptr, nbr, core, N, parent);
    hipLaunchKernelGGL(dbscan_flatten_kernel, dim3(rg::cdiv(N, 256)), dim3(256), 0, stream, N, parent);
    return rg::check_launch("rg_dbscan_components");
}

extern "C" int rg_dbscan_labels(const int* rowptr, const int* nbr, const int* parent, int N, int* isroot, int* rootnum, int64_t* labels,
                                hipStream_t stream) {
    RG_REQUIRE(lists_ok(rowptr, nbr, N) && parent && isroot && rootnum && labels, "rg_dbscan_labels: bad arguments (1 <= N <= %d)", kMaxN);
    rg::ProfScope prof(rg::FAM_MISC, stream, 0.0, 0.0);
    hipLaunchKernelGGL(dbscan_root_flag_kernel, dim3(rg::cdiv(N, 256)), dim3(256), 0, stream, parent, N, isroot);
    hipLaunchKernelGGL(rg_scan_kernel<1024>, dim3(1), dim3(1024), 0, stream, isroot, N, rootnum);
    hipLaunchKernelGGL(dbscan_label_kernel, dim3(rg::cdiv(N, kRowsPerBlock)), dim3(256), 0, stream, rowptr, nbr, parent, rootnum, N, labels);
    return rg::check_launch("rg_dbscan_labels");
}

extern "C" int rg_dbscan_asymmetry(const void* d, int is_half, int N, int64_t ld, int* count, hipStream_t stream) {
    RG_REQUIRE(matrix_ok(d, is_half, N, ld) && count, "rg_dbscan_asymmetry: bad arguments (1 <= N <= %d, ld >= N)", kMaxN);
    rg::ProfScope prof(rg::FAM_MISC, stream, 0.0, (is_half ? 2.0 : 4.0) * N * (double)N);
    if (hipMemsetAsync(count, 0, sizeof(int), stream) != hipSuccess) {
        rg::set_error("rg_dbscan_asymmetry: hipMemsetAsync failed");
        return RG_ERR_LAUNCH;
    }
    const dim3 grid(rg::cdiv(N, 32), rg::cdiv(N, 32));
    if (is_half)
        hipLaunchKernelGGL(dbscan_asym_kernel<unsigned short>, grid, dim3(256), 0, stream, (const unsigned short*)d, N, ld, count);
    else
        hipLaunchKernelGGL(dbscan_asym_kernel<unsigned>, grid, dim3(256), 0, stream, (const unsigned*)d, N, ld, count);
    return rg::check_launch("rg_dbscan_asymmetry");
}
