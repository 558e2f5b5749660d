// Device primitives that every convolution unit stands on, fp32 (conv_core.h) and fp8 (conv_f8.hip, f8_quant.hip) alike: the
// vector types of the MFMA and buffer builtins, division by a launch constant, the XCD remap of a flat workgroup id and raw buffer
// access.  Internal linkage, inline functions only: a unit pays for what it uses.
#pragma once
#include "rg_common.h"

typedef float floatx16 __attribute__((ext_vector_type(16)));
typedef int int4v __attribute__((ext_vector_type(4)));

namespace {

struct FastDiv {
    unsigned mul;
    unsigned shr;
    unsigned d;
};

static FastDiv make_fastdiv(unsigned d) {
    FastDiv f;
    f.d = d ? d : 1;
    if (f.d == 1) {
        f.mul = 0;
        f.shr = 0;
        return f;
    }
    unsigned l = 0;
    while ((1ull << l) < f.d) ++l;  // ceil(log2 d)
    const unsigned p = 31 + l;
    f.mul = (unsigned)(((1ull << p) + f.d - 1) / f.d);
    f.shr = p - 32;
    return f;
}

__device__ __forceinline__ int fdiv(int n, const FastDiv& f) {
    return f.d == 1 ? n : (int)(__umulhi((unsigned)n, f.mul) >> f.shr);
}

// XCD-aware bijective remap of the flat block id: blocks b, b+8, b+16.. share an XCD (and its L2),
// so give each XCD a contiguous chunk of the tile space.  Speed only, never correctness.
__device__ __forceinline__ int xcd_remap(int bid, int nwg) {
    const int q = nwg >> 3, r = nwg & 7;
    const int xcd = bid & 7, idx = bid >> 3;
    const int base = xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
    return base + idx;
}

// ---- raw buffer access: 32-bit byte offsets from a wave-uniform base, hardware range check (a load beyond
// num_records returns 0, a store is dropped).  An invalid lane simply carries OOB as its offset: no branches.
typedef __amdgpu_buffer_rsrc_t rsrc_t;
constexpr unsigned OOB = 0x80000000u;      // every tensor is < 2^31 bytes (checked on the host)

__device__ __forceinline__ rsrc_t make_rsrc(const void* p, unsigned bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), 0, bytes, 0x00020000);
}
__device__ __forceinline__ float bload(rsrc_t r, unsigned off) {
    return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, off, 0, 0));
}
__device__ __forceinline__ float4 bload4(rsrc_t r, unsigned off) {
    // bit_cast of the builtin's own 16-byte vector type (an implicit conversion to an ext_vector splats lane 0)
    typedef float f4v __attribute__((ext_vector_type(4)));
    const f4v v = __builtin_bit_cast(f4v, __builtin_amdgcn_raw_buffer_load_b128(r, off, 0, 0));
    return make_float4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ void bstore(rsrc_t r, unsigned off, float v) {
    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(int, v), r, off, 0, 0);
}
// AUX = 16: sc1, a write-through store (leaves the XCD's L2 for memory at once: what another XCD's workgroup may read in this launch)
template <int AUX>
__device__ __forceinline__ void bstore_aux(rsrc_t r, unsigned off, float v) {
    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(int, v), r, off, 0, AUX);
}

}  // namespace
