// Device core of the fp32 convolution kernels (conv_fwd.hip, conv_dgrad.hip, conv_wgrad.hip; overview in conv_igemm.hip): the kernel
// parameter blocks, the tile shapes, the split-bf16 MFMA k-step, the epilogues and the split-K stores, and the bf16-plane core
// (conv_planes_core.h), on the primitives the fp8 units share (conv_prims.h: dividers, XCD remap, buffer access).  Templates and
// inline functions only: a unit pays for what it instantiates.
#pragma once
#include "conv_plan.h"
#include "conv_prims.h"

namespace {

using rg::conv::BK;
using rg::conv::ConvGeom;
#ifndef RG_WAVES
#define RG_WAVES 3      // waves per SIMD the fwd / dgrad kernels are compiled for (register budget 512 / RG_WAVES): the split
                        // fragments (3 x 4 registers per 32 x 16 operand block) need the 168-register budget
#endif
constexpr int LPAD = 4;
constexpr int NT = 256;

struct Epilogue {
    const float* scale;  // per output channel (GEMM row) or nullptr
    const float* shift;  // per output channel or nullptr
    const float* res;    // same shape as the output or nullptr
    int act;
    float slope;
    const float* mask;   // same shape as the output or nullptr: after the residual add, v = mask > 0 ? v : 0 (the ReLU
                         // backward of the layer that produced this conv's input, whose output IS that input)
    float* rowsum;       // nullptr or [M][rowsum_cols]: per GEMM row, the sum of the FINAL values this wave stored (one
    int rowsum_cols;     // column per (class, n-tile, wave column) = the channel sums the BatchNorm fold of the layer
};                       // below needs, rg_bn_fold_wgrad `partials`), written in fixed order: deterministic

struct ConvP {
    const float* x;   // fwd: input, dgrad: dy, wgrad: input
    const float* w;   // fwd/dgrad: weights, wgrad: dy
    float* y;         // fwd: y, dgrad: dx, wgrad: dw or workspace
    Epilogue ep;
    int N, C, H, W, K, KH, KW, SH, SW, PH, PW, P, Q;
    int M, Ng, Kg;
    int a_vec4;
    int wshift;          // wgrad, VEC instantiation: the im2col operand is a SHIFTED copy of x (stride 1): float4 loads at the tap's offset
    int m_tiles, n_tiles;
    FastDiv d_rs, d_kw, d_pq, d_q;
    // split-K (fwd / dgrad: partial tiles to `partial`; wgrad: to y)
    int ktiles_per_split, splits;
    float* partial;
    unsigned* arrive;    // nullptr, or one arrival counter per output tile (zero between launches): the LAST split of a tile to arrive
                         // sums the tile's partials and applies the epilogue itself — no finishing launch (splitk_arrive_finish)
    // buffer-resource sizes (bytes, < 2^31) of x / w / y / partial, and extra dividers for the (r,s)-major orders
    unsigned x_bytes, w_bytes, y_bytes, partial_bytes;
    FastDiv d_c, d_k;
};

struct DgradClass : rg::conv::ParityClass {
    int Ngc, Kgc, ntiles, poff;                                // poff: first row-sum column block of the class
    int ktps, coff;                                            // split-K: k-tiles per split of THIS class, its first partial column
    FastDiv d_taps, d_nrw, d_hw, d_w;
};

struct DgradP {
    ConvP c;
    DgradClass cls[4];
    int ng_total;                                              // strided split-K: columns of one partial row (sum of the classes' Ngc)
};

template <int BM, int BN, int WM, int WN>
struct Tile {
    static constexpr int LDA = BM + LPAD;
    static constexpr int LDB = BN + LPAD;
    static constexpr int WTM = BM / WM;
    static constexpr int WTN = BN / WN;
    static constexpr int TBM = BM, TBN = BN, NTHREADS = 64 * WM * WN;
    static constexpr int TM = WTM / 32;
    static constexpr int TN = WTN / 32;
    static_assert(WM * WN == 4 || WM * WN == 8, "4 waves per workgroup (8 for the plane-path kernels' 128 x 128 tile)");
    static_assert(WTM % 32 == 0 && WTN % 32 == 0, "wave tile is a multiple of the 32x32 MFMA tile");
    // register staging sizes
    static constexpr int ACNT = (BM * BK / NT) < 4 ? 4 : (BM * BK / NT);
    static constexpr int BCNT = (BN * BK / NT) < 1 ? 1 : (BN * BK / NT);
};

// ---- matrix arithmetic of one 16-deep k-tile -------------------------------------------------------------------------------
// fp32 operands are split EXACTLY into three bf16 pieces each (x = hi + mid + lo with hi = bf16(x),
// mid = bf16(x - hi), lo = x - hi - mid, each rounded to nearest even: the residuals are exact fp32 subtractions and the last one
// has at most 8 significant bits, so it is a bf16 number; rounding rather than truncating keeps the residuals' signs independent
// of the operand's, so the dropped terms below do not add up to a bias — a truncating split underestimates every product by
// ~2^-24, measured as -4.7e-8 sum|a b| on same-sign data) and the product is evaluated as the six partial products whose weight
// is >= 2^-16 of the leading one
//     a*b ~ a_hi b_hi + (a_hi b_mid + a_mid b_hi) + (a_mid b_mid + a_hi b_lo + a_lo b_hi)
// on v_mfma_f32_32x32x16_bf16 (bf16 x bf16 products are exact in fp32, accumulation in fp32).  The three dropped products
// (mid*lo, lo*mid, lo*lo) are <= 2^-23 |a b| together: one fp32 rounding per product, i.e. the error model of the fp32 FMA chain
// the fp32 MFMA evaluates — measured against fp64 in tests/test_ops_gpu.py — at 6/16 of its matrix-pipe time (the bf16 MFMA
// issues 16x the FLOPs per cycle).  The split runs on the VALU after the fragment's ds_read_b32s (LDS tiles stay fp32, k-major),
// 4.5 VALU ops per element; small terms are accumulated first.
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef int int4r __attribute__((ext_vector_type(4)));

struct Split3 {
    int4r hi, mid, lo;      // 8 bf16 each: element j of the MFMA fragment = k index 8 * (lane >> 5) + j
};

typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef float float2r __attribute__((ext_vector_type(2)));
// two elements at a time: v_cvt_pk_bf16_f32 (round to nearest even) gives the packed pieces directly
__device__ __forceinline__ void split3_pair(float x0, float x1, int& hi, int& mid, int& lo) {
    const float2r x = {x0, x1};
    hi = __builtin_bit_cast(int, __builtin_convertvector(x, bf16x2));
    const float2r r = {x0 - __builtin_bit_cast(float, (unsigned)hi << 16), x1 - __builtin_bit_cast(float, (unsigned)hi & 0xffff0000u)};
    mid = __builtin_bit_cast(int, __builtin_convertvector(r, bf16x2));
    const float2r l = {r[0] - __builtin_bit_cast(float, (unsigned)mid << 16), r[1] - __builtin_bit_cast(float, (unsigned)mid & 0xffff0000u)};
    lo = __builtin_bit_cast(int, __builtin_convertvector(l, bf16x2));
}

__device__ __forceinline__ Split3 split3(const float (&x)[8]) {
    Split3 s;
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        int h, m, l;
        split3_pair(x[2 * d], x[2 * d + 1], h, m, l);
        s.hi[d] = h; s.mid[d] = m; s.lo[d] = l;
    }
    return s;
}

__device__ __forceinline__ floatx16 mfma_bf16(const int4r& a, const int4r& b, const floatx16& c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}

// acc += A(32 x 16) * B(16 x 32) in split arithmetic, small terms first
__device__ __forceinline__ void mma_split3(const Split3& a, const Split3& b, floatx16& acc) {
    acc = mfma_bf16(a.lo, b.hi, acc);
    acc = mfma_bf16(a.hi, b.lo, acc);
    acc = mfma_bf16(a.mid, b.mid, acc);
    acc = mfma_bf16(a.mid, b.hi, acc);
    acc = mfma_bf16(a.hi, b.mid, acc);
    acc = mfma_bf16(a.hi, b.hi, acc);
}

#ifndef RG_PINSCHED
#define RG_PINSCHED 1
#endif
#if RG_PINSCHED
#define RG_PIN() __builtin_amdgcn_sched_barrier(0)      // keep the (MFMA, split pair) groups in source order
#else
#define RG_PIN()
#endif

// One 16-deep k-step of a (TM x 32) x (TN x 32) wave tile from fp32 operands in LDS: ra(i, q) / rb(j, q) read element q (k index
// 8 * (lane >> 5) + q) of this lane's row of A block i / column of B block j.
// Software-pipelined by hand: the matrix pipe and the VALU do not overlap across the waves of a SIMD here (the co-resident
// workgroups run in phase: PMC showed VALU-busy + MFMA-busy = kernel time), so each wave hides its own split work behind its own
// MFMAs: block order (0,0), (1,0), .., (0,1), .. needs one new fragment per block; while the six MFMAs of a block issue, the
// fragment of the NEXT block is split, one element pair (9 VALU instructions) behind each of the first four.
template <int TM, int TN, typename RA, typename RB>
__device__ __forceinline__ void mma_kstep(RA ra, RB rb, floatx16 (&acc)[TM][TN]) {
    float xa[TM][8], xb[TN][8];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int q = 0; q < 8; ++q) xa[i][q] = ra(i, q);
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
        for (int q = 0; q < 8; ++q) xb[j][q] = rb(j, q);
    Split3 a[TM], b[TN];
    a[0] = split3(xa[0]);
    b[0] = split3(xb[0]);
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            // fragment the next block needs first: a[i + 1] in the first column, b[j + 1] at the end of a column
            const bool na = (j == 0 && i + 1 < TM), nb = (i + 1 == TM && j + 1 < TN);
            const int ia = i + 1 < TM ? i + 1 : 0, jb = j + 1 < TN ? j + 1 : 0;
            auto pair = [&](int d) {
                int h, m, l;
                if (na) {
                    split3_pair(xa[ia][2 * d], xa[ia][2 * d + 1], h, m, l);
                    a[ia].hi[d] = h; a[ia].mid[d] = m; a[ia].lo[d] = l;
                } else if (nb) {
                    split3_pair(xb[jb][2 * d], xb[jb][2 * d + 1], h, m, l);
                    b[jb].hi[d] = h; b[jb].mid[d] = m; b[jb].lo[d] = l;
                }
            };
            floatx16& c = acc[i][j];
            c = mfma_bf16(a[i].lo, b[j].hi, c);  pair(0);  RG_PIN();
            c = mfma_bf16(a[i].hi, b[j].lo, c);  pair(1);  RG_PIN();
            c = mfma_bf16(a[i].mid, b[j].mid, c);  pair(2);  RG_PIN();
            c = mfma_bf16(a[i].mid, b[j].hi, c);  pair(3);  RG_PIN();
            c = mfma_bf16(a[i].hi, b[j].mid, c);
            c = mfma_bf16(a[i].hi, b[j].hi, c);
        }
}

// One 16-deep k-tile of MFMAs.  `hook(q)`, q = 0..3, is called behind the last matrix instructions: the kernels use it to write
// the NEXT tile's staged registers into the other LDS buffer, so those ds_writes (and the vmcnt wait in front of them) issue in
// the shadow of the MFMAs instead of after them.
template <typename T, typename Hook>
__device__ __forceinline__ void mma_tile(const float (*As)[T::LDA], const float (*Bs)[T::LDB],
                                         floatx16 (&acc)[T::TM][T::TN], int wm, int wn, int lane, Hook hook) {
    const int l32 = lane & 31, kh = lane >> 5;
    static_assert(BK == 16, "one bf16 MFMA k-step per LDS tile");
    mma_kstep<T::TM, T::TN>([&](int i, int q) { return As[8 * kh + q][wm * T::WTM + i * 32 + l32]; },
                            [&](int j, int q) { return Bs[8 * kh + q][wn * T::WTN + j * 32 + l32]; }, acc);
    hook(0); hook(1); hook(2); hook(3);
}

// true when element e of a CNT-element staging array belongs to quarter q (q < 0: every quarter)
__device__ __forceinline__ constexpr bool in_quarter(int e, int cnt, int q) { return q < 0 || (e * 4) / cnt == q; }

template <int I> struct AuxTag { static constexpr int value = I; };

template <typename T>
__device__ __forceinline__ void zero_acc(floatx16 (&acc)[T::TM][T::TN]) {
#pragma unroll
    for (int i = 0; i < T::TM; ++i)
#pragma unroll
        for (int j = 0; j < T::TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
}

// Fused epilogue y = mask(act(acc * scale[m] + shift[m] + res)) for a tile whose column j of the wave starts at byte
// offset ob[j] (OOB when outside) and whose GEMM rows are `rstride` bytes apart.  Branch-free: per-row scale / shift
// are broadcast buffer loads shared by the TN column blocks, residual / mask are buffer loads at the store offset
// issued RB at a time before their first use (OOB lanes read 0 and their stores are dropped by the hardware).
template <typename T, int ACT>
__device__ __forceinline__ void store_tile_epilogue(const ConvP& p, const floatx16 (&acc)[T::TM][T::TN], const unsigned (&ob)[T::TN],
                                                    unsigned rstride, int mrow0, int pc) {
    const rsrc_t ro = make_rsrc(p.y, p.y_bytes);
    const rsrc_t rr = make_rsrc(p.ep.res ? (const void*)p.ep.res : (const void*)p.y, p.ep.res ? p.y_bytes : 0u);
    const rsrc_t rm = make_rsrc(p.ep.mask ? (const void*)p.ep.mask : (const void*)p.y, p.ep.mask ? p.y_bytes : 0u);
    const rsrc_t rsc = make_rsrc(p.ep.scale ? p.ep.scale : p.ep.shift, p.ep.scale ? (unsigned)p.M * 4u : 0u);
    const rsrc_t rsh = make_rsrc(p.ep.shift ? p.ep.shift : p.ep.scale, p.ep.shift ? (unsigned)p.M * 4u : 0u);
    const bool has_scale = p.ep.scale != nullptr, has_res = p.ep.res != nullptr, has_mask = p.ep.mask != nullptr;
    constexpr int RB = 8;          // rows per batch: bounds the live VGPRs of the epilogue
#pragma unroll
    for (int i = 0; i < T::TM; ++i)
#pragma unroll
        for (int rb = 0; rb < 16; rb += RB) {
            float sc[RB], sh[RB], rs[RB];
#pragma unroll
            for (int q = 0; q < RB; ++q) rs[q] = 0.f;
#pragma unroll
            for (int q = 0; q < RB; ++q) {
                const int r = rb + q;
                const unsigned moff = (unsigned)(mrow0 + i * 32 + (r & 3) + 8 * (r >> 2)) * 4u;
                sc[q] = has_scale ? bload(rsc, moff) : 1.f;      // zero-sized resources return 0 for every lane
                sh[q] = bload(rsh, moff);
            }
#pragma unroll
            for (int j = 0; j < T::TN; ++j) {
                // offsets are recomputed at each use (one mad + select) rather than kept live across the loads
                auto off_of = [&](int q) -> unsigned {
                    const int r = rb + q;
                    const int mo = i * 32 + (r & 3) + 8 * (r >> 2);
                    return (mrow0 + mo < p.M) ? ob[j] + (unsigned)mo * rstride : OOB;
                };
                float rv[RB];
                if (has_res) {
#pragma unroll
                    for (int q = 0; q < RB; ++q) rv[q] = bload(rr, off_of(q));
                }
                const bool colok = ob[j] != OOB;
                if (has_mask) {                      // mask folded into the residual registers: sign carries it
                    float mv[RB];
#pragma unroll
                    for (int q = 0; q < RB; ++q) mv[q] = bload(rm, off_of(q));
#pragma unroll
                    for (int q = 0; q < RB; ++q) {
                        float v = acc[i][j][rb + q] * sc[q] + sh[q];
                        if (has_res) v += rv[q];
                        if (ACT == RG_ACT_RELU) v = fmaxf(v, 0.f);
                        if (ACT == RG_ACT_LEAKY) v = v > 0.f ? v : v * p.ep.slope;
                        if (ACT == RG_ACT_TANH) v = tanhf(v);
                        v = mv[q] > 0.f ? v : 0.f;
                        bstore(ro, off_of(q), v);
                        if (p.ep.rowsum) rs[q] += colok ? v : 0.f;
                    }
                } else {
#pragma unroll
                    for (int q = 0; q < RB; ++q) {
                        float v = acc[i][j][rb + q] * sc[q] + sh[q];
                        if (has_res) v += rv[q];
                        if (ACT == RG_ACT_RELU) v = fmaxf(v, 0.f);
                        if (ACT == RG_ACT_LEAKY) v = v > 0.f ? v : v * p.ep.slope;
                        if (ACT == RG_ACT_TANH) v = tanhf(v);
                        bstore(ro, off_of(q), v);
                        if (p.ep.rowsum) rs[q] += colok ? v : 0.f;
                    }
                }
                __builtin_amdgcn_sched_barrier(0);      // keep the next batch's loads from being hoisted (VGPR pressure)
            }
            if (p.ep.rowsum) {                           // uniform: 32-lane butterfly per row, lane 0 of each half writes
                const int lane = threadIdx.x & 63;
#pragma unroll
                for (int q = 0; q < RB; ++q) {
                    float t = rs[q];
#pragma unroll
                    for (int o = 16; o > 0; o >>= 1) t += __shfl_xor(t, o, 64);
                    const int r = rb + q;
                    const int m = mrow0 + i * 32 + (r & 3) + 8 * (r >> 2);
                    if ((lane & 31) == 0 && m < p.M) p.ep.rowsum[(int64_t)m * p.ep.rowsum_cols + pc] = t;
                }
            }
        }
}

template <typename T>
__device__ __forceinline__ void store_tile_epilogue_any(const ConvP& p, const floatx16 (&acc)[T::TM][T::TN],
                                                        const unsigned (&ob)[T::TN], unsigned rstride, int mrow0, int pc) {
    switch (p.ep.act) {      // uniform
        case RG_ACT_RELU: store_tile_epilogue<T, RG_ACT_RELU>(p, acc, ob, rstride, mrow0, pc); break;
        case RG_ACT_LEAKY: store_tile_epilogue<T, RG_ACT_LEAKY>(p, acc, ob, rstride, mrow0, pc); break;
        case RG_ACT_TANH: store_tile_epilogue<T, RG_ACT_TANH>(p, acc, ob, rstride, mrow0, pc); break;
        default: store_tile_epilogue<T, RG_ACT_NONE>(p, acc, ob, rstride, mrow0, pc); break;
    }
}

// ---- split-K finish, four consecutive columns of one GEMM row (shared by conv_splitk_finish_vec_kernel and the in-kernel finish
// below, so that the two produce the same bits): left-to-right sum over the splits, then the epilogue ----
__device__ __forceinline__ float4 splitk_sum4(const float4* __restrict__ p4, int64_t sstride4, int64_t i, int splits) {
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    int s = 0;
    for (; s + 4 <= splits; s += 4) {
        const float4 a = p4[(int64_t)s * sstride4 + i], b = p4[(int64_t)(s + 1) * sstride4 + i];
        const float4 c = p4[(int64_t)(s + 2) * sstride4 + i], d = p4[(int64_t)(s + 3) * sstride4 + i];
        v.x = (((v.x + a.x) + b.x) + c.x) + d.x; v.y = (((v.y + a.y) + b.y) + c.y) + d.y;
        v.z = (((v.z + a.z) + b.z) + c.z) + d.z; v.w = (((v.w + a.w) + b.w) + c.w) + d.w;
    }
    for (; s < splits; ++s) {
        const float4 a = p4[(int64_t)s * sstride4 + i];
        v.x += a.x; v.y += a.y; v.z += a.z; v.w += a.w;
    }
    return v;
}

__device__ __forceinline__ void splitk_epilogue_store4(float* __restrict__ out, int64_t o, int m, float4 v, const Epilogue& ep) {
    if (ep.scale) { const float sc = ep.scale[m]; v.x *= sc; v.y *= sc; v.z *= sc; v.w *= sc; }
    if (ep.shift) { const float sh = ep.shift[m]; v.x += sh; v.y += sh; v.z += sh; v.w += sh; }
    if (ep.res) {
        const float4 r = *reinterpret_cast<const float4*>(ep.res + o);
        v.x += r.x; v.y += r.y; v.z += r.z; v.w += r.w;
    }
    v.x = rg_apply_act(v.x, ep.act, ep.slope); v.y = rg_apply_act(v.y, ep.act, ep.slope);
    v.z = rg_apply_act(v.z, ep.act, ep.slope); v.w = rg_apply_act(v.w, ep.act, ep.slope);
    if (ep.mask) {
        const float4 mk = *reinterpret_cast<const float4*>(ep.mask + o);
        if (!(mk.x > 0.f)) v.x = 0.f;
        if (!(mk.y > 0.f)) v.y = 0.f;
        if (!(mk.z > 0.f)) v.z = 0.f;
        if (!(mk.w > 0.f)) v.w = 0.f;
    }
    *reinterpret_cast<float4*>(out + o) = v;
}

// Split-K without the finishing launch (p.arrive != nullptr; the host sets it only when Ng % 4 == 0, PIX % 4 == 0 and every pointer is
// 16-byte aligned).  The L2s of the eight XCDs are not coherent with each other inside a kernel and a CU's L1 is never refreshed by
// other CUs' stores, so the hand-off follows the counter form of the split-K seam: every workgroup of a tile stores its raw
// accumulators to partial[split] WRITE-THROUGH (sc1: no L2-wide release fence; __threadfence() here measured +27 us per launch),
// every storing wave drains its stores (s_waitcnt vmcnt(0)), the workgroup meets at a barrier, and one lane counts the workgroup in
// on the tile's arrival counter (agent-scope atomic).  The workgroup that finds splits - 1 earlier arrivals is the last: one lane's
// agent-scope acquire (drops this CU's stale L1 lines), the wait for it, a barrier — then all waves read the tile's partials back in
// split order 0, 1, 2, ... (the finishing kernel's summation order: the result does not depend on which split came last) and write
// the finished outputs.  atomicInc wraps the counter to zero on that last arrival: clean for the next launch without a memset (the
// caller zeroes the counters once, rg_conv_splitk_arrivals).  Nobody waits for anybody: no workgroup can stall on one that has not
// been scheduled yet.
template <typename T>
__device__ __forceinline__ void splitk_arrive_finish(const ConvP& p, int m0, int n0, int Ng, int PIX, const FastDiv& d_pix) {
    __shared__ unsigned s_prev;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");        // every storing wave: its write-through partial stores have left
    __syncthreads();                                        // ... for all waves (and nobody reads operand LDS any more)
    if (threadIdx.x == 0) {
        const unsigned prev = atomicInc(p.arrive + blockIdx.x, (unsigned)p.splits - 1u);
        if (prev == (unsigned)p.splits - 1u) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        s_prev = prev;
    }
    __syncthreads();
    if (s_prev != (unsigned)p.splits - 1u) return;          // uniform
    constexpr int C4 = T::TBN / 4, RSTEP = T::NTHREADS / C4;
    static_assert(T::NTHREADS % C4 == 0, "whole rows per pass");
    const int c4 = threadIdx.x % C4;
    const int n = n0 + 4 * c4;
    if (n >= Ng) return;
    const int ng4 = Ng >> 2;
    const int64_t sstride4 = (int64_t)p.M * ng4;
    const float4* p4 = reinterpret_cast<const float4*>(p.partial);
    const int im = fdiv(n, d_pix);
    const int pix = n - im * PIX;
    for (int r = threadIdx.x / C4; r < T::TBM; r += RSTEP) {
        const int m = m0 + r;
        if (m >= p.M) break;
        const float4 v = splitk_sum4(p4, sstride4, (int64_t)m * ng4 + (n >> 2), p.splits);
        splitk_epilogue_store4(p.y, ((int64_t)im * p.M + m) * PIX + pix, m, v, p.ep);
    }
}

// Epilogue for outputs laid out [img][M][PIX] with n = img*PIX + pix (fwd: PIX = P*Q; stride-1 dgrad: PIX = H*W).
// With split-K the raw accumulators go to partial[(split*M + m)*Ng + n] instead.  Buffer stores: one VALU add per
// element, lanes outside the tensor carry OOB and are dropped by the hardware.
template <typename T>
__device__ __forceinline__ void store_tile_nchw(const ConvP& p, const floatx16 (&acc)[T::TM][T::TN], int m0, int n0,
                                                int wm, int wn, int lane, int Ng, int PIX, const FastDiv& d_pix,
                                                int split, int pcol = 0) {
    const int l32 = lane & 31, kh = lane >> 5;
    const int mrow0 = m0 + wm * T::WTM + 4 * kh;
    const bool plain = !p.ep.scale && !p.ep.shift && !p.ep.res && !p.ep.mask && !p.ep.rowsum && p.ep.act == RG_ACT_NONE;
    if (p.partial || plain) {
        const rsrc_t ro = p.partial ? make_rsrc(p.partial, p.partial_bytes) : make_rsrc(p.y, p.y_bytes);
        const unsigned rstride = (p.partial ? (unsigned)Ng : (unsigned)PIX) * 4u;    // bytes between GEMM rows
        auto store_raw = [&](auto aux_tag) {
#pragma unroll
            for (int j = 0; j < T::TN; ++j) {
                const int nn = n0 + wn * T::WTN + j * 32 + l32;
                unsigned ob = OOB;
                if (nn < Ng) {
                    if (p.partial) {
                        ob = (unsigned)(((split * p.M + mrow0) * (int64_t)Ng + nn) * 4);
                    } else {
                        const int im = fdiv(nn, d_pix);
                        ob = (unsigned)((((int64_t)im * p.M + mrow0) * PIX + (nn - im * PIX)) * 4);
                    }
                }
#pragma unroll
                for (int i = 0; i < T::TM; ++i)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int mo = i * 32 + (r & 3) + 8 * (r >> 2);
                        const unsigned off = (mrow0 + mo < p.M) ? ob + (unsigned)mo * rstride : OOB;
                        bstore_aux<decltype(aux_tag)::value>(ro, off, acc[i][j][r]);
                    }
            }
        };
        if (p.partial && p.arrive) {                            // uniform
            store_raw(AuxTag<16>());
            splitk_arrive_finish<T>(p, m0, n0, Ng, PIX, d_pix);
        } else {
            store_raw(AuxTag<0>());
        }
        return;
    }
    unsigned ob[T::TN];
#pragma unroll
    for (int j = 0; j < T::TN; ++j) {
        const int nn = n0 + wn * T::WTN + j * 32 + l32;
        ob[j] = OOB;
        if (nn < Ng) {
            const int im = fdiv(nn, d_pix);
            ob[j] = (unsigned)((((int64_t)im * p.M + mrow0) * PIX + (nn - im * PIX)) * 4);
        }
    }
    store_tile_epilogue_any<T>(p, acc, ob, (unsigned)PIX * 4u, mrow0, pcol);
}

// raw accumulators of a tile to partial[(split * M + m) * ncols + col0 + n] (strided data gradient with split-K: the classes'
// columns side by side, col0 = the class' first column)
template <typename T>
__device__ __forceinline__ void store_tile_partial_cols(const ConvP& p, const floatx16 (&acc)[T::TM][T::TN], int m0, int n0, int wm,
                                                        int wn, int lane, int Ng, int col0, int ncols, int split) {
    const int l32 = lane & 31, kh = lane >> 5;
    const int mrow0 = m0 + wm * T::WTM + 4 * kh;
    const rsrc_t ro = make_rsrc(p.partial, p.partial_bytes);
    const unsigned rstride = (unsigned)ncols * 4u;
#pragma unroll
    for (int j = 0; j < T::TN; ++j) {
        const int nn = n0 + wn * T::WTN + j * 32 + l32;
        const unsigned ob = nn < Ng ? (unsigned)((((int64_t)split * p.M + mrow0) * ncols + col0 + nn) * 4) : OOB;
#pragma unroll
        for (int i = 0; i < T::TM; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int mo = i * 32 + (r & 3) + 8 * (r >> 2);
                bstore(ro, (mrow0 + mo < p.M && ob != OOB) ? ob + (unsigned)mo * rstride : OOB, acc[i][j][r]);
            }
    }
}

// ---- host side of the parameter blocks ----
static void fill_common(ConvP& p, const ConvGeom& g) {
    p.N = g.N; p.C = g.C; p.H = g.H; p.W = g.W; p.K = g.K; p.KH = g.KH; p.KW = g.KW;
    p.SH = g.SH; p.SW = g.SW; p.PH = g.PH; p.PW = g.PW; p.P = g.P; p.Q = g.Q;
    p.d_rs = make_fastdiv(g.KH * g.KW);
    p.d_kw = make_fastdiv(g.KW);
    p.d_pq = make_fastdiv(g.P * g.Q);
    p.d_q = make_fastdiv(g.Q);
    p.a_vec4 = 0;
    p.wshift = 0;
    p.ktiles_per_split = 1 << 30;
    p.splits = 1;
    p.partial = nullptr;
    p.arrive = nullptr;
    p.x_bytes = p.w_bytes = p.y_bytes = p.partial_bytes = 0;
    p.d_c = make_fastdiv(g.C);
    p.d_k = make_fastdiv(g.K);
}

// byte sizes of the three tensors of a geometry (buffer resources: < 2^31, validate)
static unsigned x_bytes(const ConvGeom& g) { return (unsigned)((int64_t)g.N * g.C * g.H * g.W * 4); }
static unsigned w_bytes(const ConvGeom& g) { return (unsigned)((int64_t)g.K * g.C * g.KH * g.KW * 4); }
static unsigned y_bytes(const ConvGeom& g) { return (unsigned)((int64_t)g.N * g.K * g.P * g.Q * 4); }

// epilogue bits of a choice key: forward keys carry (residual, act), data-gradient keys (residual, mask, row sums, act)
static int ep_bits(const Epilogue& ep, bool dgrad) {
    return dgrad ? (int)(ep.res != nullptr) * 16 + (int)(ep.mask != nullptr) * 8 + (int)(ep.rowsum != nullptr) * 4 + ep.act
                 : (int)(ep.res != nullptr) * 4 + ep.act;
}

static unsigned finish_grid(int64_t n) {
    int64_t g = rg::cdiv64(n, 256);
    if (g > 4096) g = 4096;
    return (unsigned)(g < 1 ? 1 : g);
}

// the block tiles of the generic kernels (rg::conv::kTileBM x kTileBN) as BM, BN and the wave grid WM x WN
#define RG_TILE_SWITCH(tile, LAUNCH)      \
    switch (tile) {                       \
        case 0: LAUNCH(128, 128, 2, 2); break; \
        case 1: LAUNCH(64, 128, 2, 2); break;  \
        case 2: LAUNCH(64, 64, 2, 2); break;   \
        default: LAUNCH(32, 256, 1, 4); break; \
    }

#include "conv_planes_core.h"

}  // namespace
