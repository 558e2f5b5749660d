// The split-K slab sum of the weight gradients, fp32 (conv_wgrad.hip) and fp8 (conv_f8.hip): element i of ws[splits][n] summed over
// the splits in ONE fixed tree, so every reducer gives the same value for the same slabs.  A workgroup of 256 threads takes 64
// elements (tx) x 4 split lanes (ty): small filter tensors with hundreds of splits stay parallel instead of one serial chain per
// thread.  Lane ty adds splits ty, ty + 8, ... and ty + 4, ty + 12, ... in two chains and then the chains; the four lanes meet in
// LDS as (r0 + r1) + (r2 + r3).  A reducer kernel is "sum, then its own last statement"; both functions are called by every thread of
// the workgroup (one barrier).  (No __restrict__ here: the kernels' own parameters carry it.)
#pragma once
#include "rg_common.h"

namespace {

// s = the sum of element i = blockIdx.x * 64 + tx; true in the lanes that hold it (ty == 0, i < n)
__device__ __forceinline__ bool splitk_sum(const float* ws, int64_t n, int splits, int64_t& i, float& s) {
    __shared__ float red[4][64];
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    i = (int64_t)blockIdx.x * 64 + tx;
    float s0 = 0.f, s1 = 0.f;
    if (i < n) {
        int k = ty;
        for (; k + 4 < splits; k += 8) {
            s0 += ws[(int64_t)k * n + i];
            s1 += ws[(int64_t)(k + 4) * n + i];
        }
        if (k < splits) s0 += ws[(int64_t)k * n + i];
    }
    red[ty][tx] = s0 + s1;
    __syncthreads();
    if (ty != 0 || i >= n) return false;
    s = (red[0][tx] + red[1][tx]) + (red[2][tx] + red[3][tx]);
    return true;
}

// n % 4 == 0, 16-byte aligned slabs: v = the sums of elements 4 i .. 4 i + 3, i = blockIdx.x * 64 + tx, four slab loads in flight;
// per element the value of splitk_sum.  True in the lanes that hold v (ty == 0, i < n / 4).
__device__ __forceinline__ bool splitk_sum4(const float* ws, int64_t n, int splits, int64_t& i, float4& v) {
    __shared__ float4 red[4][64];
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int64_t n4 = n >> 2;
    i = (int64_t)blockIdx.x * 64 + tx;
    const float4* w4 = reinterpret_cast<const float4*>(ws);
    float4 s0 = make_float4(0.f, 0.f, 0.f, 0.f), s1 = s0;
    if (i < n4) {
        int k = ty;
        for (; k + 12 < splits; k += 16) {
            const float4 a = w4[(int64_t)k * n4 + i], b = w4[(int64_t)(k + 4) * n4 + i];
            const float4 c = w4[(int64_t)(k + 8) * n4 + i], d = w4[(int64_t)(k + 12) * n4 + i];
            s0.x += a.x; s0.y += a.y; s0.z += a.z; s0.w += a.w;
            s1.x += b.x; s1.y += b.y; s1.z += b.z; s1.w += b.w;
            s0.x += c.x; s0.y += c.y; s0.z += c.z; s0.w += c.w;
            s1.x += d.x; s1.y += d.y; s1.z += d.z; s1.w += d.w;
        }
        for (; k + 4 < splits; k += 8) {
            const float4 a = w4[(int64_t)k * n4 + i], b = w4[(int64_t)(k + 4) * n4 + i];
            s0.x += a.x; s0.y += a.y; s0.z += a.z; s0.w += a.w;
            s1.x += b.x; s1.y += b.y; s1.z += b.z; s1.w += b.w;
        }
        if (k < splits) {
            const float4 a = w4[(int64_t)k * n4 + i];
            s0.x += a.x; s0.y += a.y; s0.z += a.z; s0.w += a.w;
        }
    }
    red[ty][tx] = make_float4(s0.x + s1.x, s0.y + s1.y, s0.z + s1.z, s0.w + s1.w);
    __syncthreads();
    if (ty != 0 || i >= n4) return false;
    const float4 r0 = red[0][tx], r1 = red[1][tx], r2 = red[2][tx], r3 = red[3][tx];
    v = make_float4((r0.x + r1.x) + (r2.x + r3.x), (r0.y + r1.y) + (r2.y + r3.y), (r0.z + r1.z) + (r2.z + r3.z),
                    (r0.w + r1.w) + (r2.w + r3.w));
    return true;
}

}  // namespace
