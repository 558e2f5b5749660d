// What the normalisation units share (norm_bn.hip, norm_dsbn.hip, norm_instnorm.hip, norm_ibn.hip, norm_fold.hip): the Chan
// statistics merge, the activation gradient, the 256-thread block sum, the buffer-resource loads / stores of the register kernels,
// the (lanes, units) dispatch lists, the slice count of the slice-parallel kernels and the RG_BN_REG switch.  Everything here has
// internal linkage: each unit compiles its own copy of what it uses.
#pragma once
#include "rg_common.h"
#include <type_traits>

namespace {

struct WStat {
    float n, mean, m2;
};

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

__device__ __forceinline__ float act_grad_from_out(float yv, int act, float slope) {
    switch (act) {
        case RG_ACT_RELU: return yv > 0.f ? 1.f : 0.f;
        case RG_ACT_LEAKY: return yv > 0.f ? 1.f : slope;
        case RG_ACT_TANH: return 1.f - yv * yv;
        default: return 1.f;
    }
}

// Sum over the 256 threads of a workgroup (`red`: 4 floats of LDS); every thread gets the total.  The one-workgroup-per-channel
// BatchNorm kernels, the 256-lane rows and channel_sum_small_kernel all reduce through this one fixed tree.
__device__ __forceinline__ float bn_block_sum(float v, float* red) {
    v = rg_wave_sum(v);
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) red[wid] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

// Buffer resource over a whole tensor: offsets past the end (NOOB) return zeros / drop the store, so the register kernels carry
// no bounds branches.
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

// The templated kernels exist for fixed lists of (lanes per row, float4 per lane) pairs; units = 0 are the loop kernels.
// with_lanes_units finds the runtime pair in a list and calls f with it as two std::integral_constant; false: not in the list.
template <int L, int U>
struct LU {};
template <class... P>
struct LUList {};

template <class F, int... L, int... U>
static bool with_lanes_units(LUList<LU<L, U>...>, int lanes, int units, F&& f) {
    return ((lanes == L && units == U && (f(std::integral_constant<int, L>{}, std::integral_constant<int, U>{}), true)) || ...);
}

// slices S per channel of the slice-parallel kernels (grid (S, C)) and the slice length *L, a multiple of 4
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

constexpr int64_t NORM_GRID_CAP = 4096;                // workgroups of the grid-stride kernels (rg::grid_for)

// development switch: RG_BN_REG=0 keeps the loop kernels (A/B timing); read once per process by every unit that dispatches on it
static const bool g_bn_reg = rg::env_int("RG_BN_REG", 1) != 0;

}  // namespace

namespace rg {

// rows_sum_pair_kernel is compiled in norm_fold.hip only; this is its launch for the other units (grid cdiv(C, 16))
void launch_rows_sum_pair(const float* a, const float* b, float* oa, float* ob, int N, int C, int split, float* oa2, float* ob2,
                          hipStream_t stream);

}  // namespace rg
