// FP8 scaling states and quantisers of the fp8 convolution family (GEMMs and entry points of the convolutions: conv_f8.hip, which
// also describes the arithmetic).  What the two units share is the layouts written here and one dequantisation scale per tensor:
//   * operands are quantised ONCE by a transposing pass into layouts whose GEMM reduction axis is contiguous:
//       forward   y[k][pix]   = sum_{tap,c} W[k][tap][c]    * X[pix+tap][c]     X as [N][H*W][Cp]  ("NHWC"), W as [K][RS][Cp]
//       dgrad     dx[c][pix]  = sum_{tap,k} W^T[c][tap][k]  * DY[pix-tap][k]    DY as [N][P*Q][Kp],           W as [C][RS][Kp]
//       wgrad     dw[k][c,rs] = sum_{pix,n} DY[k][pix][n]   * X[c][pix+rs][n]   both as [C][H*W][Np] ("CHWN": the batch index is
//     the contiguous one, so a spatial filter shift never breaks the 16-byte alignment of a fragment);
//     channel / batch counts are padded to multiples of 16 with zeros, every staged access is one aligned 16-byte chunk whose
//     address comes from a per-chunk tap decode (raw buffer loads: chunks in the padding halo return 0);
//   * per-tensor scaling state float[4] = {amax in use, amax being collected, dequantisation scale, format max}: the
//     quantiser clamps to the format range, collects the next amax with an integer atomicMax (order independent, deterministic),
//     and rg_f8_roll_scales() switches all states of a network in one launch (delayed scaling; rg_f8_amax + roll gives
//     just-in-time scaling for calibration and tests).
#include "conv_prims.h"

namespace {

__host__ __device__ __forceinline__ constexpr float f8_max(int fmt) { return fmt == 0 ? 448.f : 57344.f; }   // e4m3fn, e5m2 (OCP)

// state[1] = max(state[1], max |x|)
__global__ __launch_bounds__(256) void f8_amax_kernel(const float* __restrict__ x, int64_t n, float* __restrict__ state) {
    __shared__ float red[16];
    float m = 0.f;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x * 4;
    int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if ((reinterpret_cast<uintptr_t>(x) & 15) == 0) {
        for (; i + 3 < n; i += stride) {
            const float4 v = *reinterpret_cast<const float4*>(x + i);
            m = fmaxf(fmaxf(m, fmaxf(fabsf(v.x), fabsf(v.y))), fmaxf(fabsf(v.z), fabsf(v.w)));
        }
    }
    for (; i < n; i += stride)
        for (int j = 0; j < 4 && i + j < n; ++j) m = fmaxf(m, fabsf(x[i + j]));
    m = rg_block_max(m, red);
    if (threadIdx.x == 0 && m > 0.f) atomicMax(reinterpret_cast<int*>(state + 1), __float_as_int(m));
}

// every state: {amax_cur, amax_next, dequant, fmax}: amax_cur <- amax_next (when something was collected), dequant = amax_cur / fmax
__global__ void f8_roll_kernel(float* __restrict__ states, int count) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    float* s = states + 4 * i;
    const float nxt = s[1];
    if (nxt > 0.f) s[0] = nxt;
    s[1] = 0.f;
    s[2] = s[0] > 0.f ? s[0] / s[3] : 1.f;
}

__device__ __forceinline__ unsigned pack4(float a, float b, float c, float d, int fmt) {
    int p = 0;
    if (fmt == 0) {
        p = __builtin_amdgcn_cvt_pk_fp8_f32(a, b, p, false);
        p = __builtin_amdgcn_cvt_pk_fp8_f32(c, d, p, true);
    } else {
        p = __builtin_amdgcn_cvt_pk_bf8_f32(a, b, p, false);
        p = __builtin_amdgcn_cvt_pk_bf8_f32(c, d, p, true);
    }
    return (unsigned)p;
}

// out[b][l][r] (r < Rp, bytes) = fp8(clamp(in[b*bs + r*rs + l] * fmax / amax_cur)), zeros for r >= R; amax_next collected.
// grid (l tiles of 64, r tiles of 64, B); the tile goes through LDS so that reads run along l and writes along r.
__global__ __launch_bounds__(256) void f8_quantize_transpose_kernel(const float* __restrict__ in, unsigned char* __restrict__ out,
                                                                    float* __restrict__ state, float* __restrict__ scale_out,
                                                                    int fmt, int R, int L, int Rp, int64_t bs, int64_t rs) {
    __shared__ float tile[64][65];
    __shared__ float red[16];
    const int t = threadIdx.x;
    const int l0 = blockIdx.x * 64, r0 = blockIdx.y * 64;
    const int64_t base = (int64_t)blockIdx.z * bs;
    const float amax = state[0];
    const float fmax = f8_max(fmt);
    const float q = amax > 0.f ? fmax / amax : 1.f;
    if (scale_out && t == 0 && blockIdx.x == 0 && blockIdx.y == 0 && blockIdx.z == 0) *scale_out = amax > 0.f ? amax / fmax : 1.f;
    float m = 0.f;
    {
        const int ll = t & 63, lr = t >> 6;
#pragma unroll 4
        for (int i = 0; i < 16; ++i) {
            const int r = r0 + lr + 4 * i;
            float v = 0.f;
            if (r < R && l0 + ll < L) v = in[base + (int64_t)r * rs + l0 + ll];
            m = fmaxf(m, fabsf(v));
            tile[lr + 4 * i][ll] = fminf(fmaxf(v * q, -fmax), fmax);
        }
    }
    __syncthreads();
    {
        const int ll = t >> 2, rq = t & 3;
        if (l0 + ll < L && r0 + rq * 16 < Rp) {
            unsigned w[4];
#pragma unroll
            for (int j = 0; j < 4; ++j)
                w[j] = pack4(tile[rq * 16 + 4 * j][ll], tile[rq * 16 + 4 * j + 1][ll], tile[rq * 16 + 4 * j + 2][ll],
                             tile[rq * 16 + 4 * j + 3][ll], fmt);
            uint4 v = make_uint4(w[0], w[1], w[2], w[3]);
            *reinterpret_cast<uint4*>(out + ((int64_t)blockIdx.z * L + l0 + ll) * Rp + r0 + rq * 16) = v;
        }
    }
    m = rg_block_max(m, red);
    if (t == 0 && m > 0.f) atomicMax(reinterpret_cast<int*>(state + 1), __float_as_int(m));
}

// Both operand layouts of one tensor in ONE pass over the fp32 data: in[n][c][l] -> a[n][l][cp] and b[c][l][np] (cp / np: c / n
// padded to 16 with zero bytes).  Tile = 16 n x 16 c x 64 l, grid (l tiles, c tiles, n tiles).  Thread (lq, c) reads, in pass n,
// the float4 of pixels 4 lq .. 4 lq + 3 of row (n, c) (coalesced 256-byte runs) and packs it into one word of 4 fp8 bytes.
//   layout b (n contiguous): byte j of the thread's own 16 words IS the 16-byte run b[c][4 lq + j][n0 .. n0 + 15] — assembled with
//     byte permutes in registers, no LDS;
//   layout a (c contiguous): the words go through a 16 KiB LDS tile [n][lq][c] (word index XOR-swizzled: conflict-free stores),
//     thread (n, lq) reads its 16 words back with four ds_read_b128 and permutes them into the four runs a[n][4 lq + j][c0 .. c0 + 15].
// (The first version moved single bytes through LDS: 128 ds_read_u8 per thread; this one issues 16 ds_write_b32 + 4 ds_read_b128.)
__device__ __forceinline__ unsigned byte_of4(unsigned w0, unsigned w1, unsigned w2, unsigned w3, int j) {
    // {w0.byte[j], w1.byte[j], w2.byte[j], w3.byte[j]}; v_perm_b32 selects from the 8 bytes of (hi : lo), selector bytes 0-3 = lo
    const unsigned sel = (unsigned)j | ((unsigned)(4 + j) << 8);
    const unsigned t01 = __builtin_amdgcn_perm(w1, w0, sel);          // bytes 0, 1 = w0[j], w1[j]
    const unsigned t23 = __builtin_amdgcn_perm(w3, w2, sel);
    return __builtin_amdgcn_perm(t23, t01, 0x05040100u);
}

// Gradient variant (yact != NULL and / or part != NULL): the tensor quantised is g = in * act'(yact) — the activation backward of the
// layer whose output gradient this is, never written out in fp32 — and part[tile][c] (tile = n tile * pixel tiles + pixel tile)
// receives the tile's sum of g per channel: the bias gradient is the column sum of `part` (rg_rows_sum_pair), fixed order.
__device__ __forceinline__ float f8_act_grad(float yv, int act, float slope) {      // `act` is uniform: selects, no branches
    const float neg = act == RG_ACT_LEAKY ? slope : 0.f;
    const float step = yv > 0.f ? 1.f : neg;
    return act == RG_ACT_TANH ? 1.f - yv * yv : (act == RG_ACT_NONE ? 1.f : step);
}

// Loads: every thread reads 16 float4 (one per sample of the tile) through a buffer resource that spans exactly the tile's samples —
// offsets outside it (samples beyond N, channels beyond C, pixels beyond L) return zeros, so the loads carry no branches and are
// issued eight samples at a time (the first version tested n / c / l per pass and waited for each load before the next: a
// 4-workgroup launch took 12 us).  VEC: L % 4 == 0 (one 16-byte load per sample), otherwise four dword loads.
template <bool VEC, bool HASY>
__global__ __launch_bounds__(256) void f8_quantize_dual_kernel(const float* __restrict__ in, unsigned char* __restrict__ a,
                                                               unsigned char* __restrict__ b, float* __restrict__ state,
                                                               float* __restrict__ scale_out, int fmt, int N, int C, int L,
                                                               int Cp, int Np, int xcd_groups, const float* __restrict__ yact,
                                                               int act, float slope, float* __restrict__ part) {
    __shared__ __attribute__((aligned(16))) unsigned tile[16 * 16 * 16];        // word (n, lq, c) at ((n*16 + lq)*16 + (c ^ 4*(lq>>2)))
    __shared__ float red[16];
    const int t = threadIdx.x;
    // 1-D grid, XCD-aware: workgroup ids are dealt round-robin to the 8 XCDs, so id % 8 picks the XCD and all (c, n) tiles of one
    // pixel tile are consecutive workgroups of ONE XCD — the 16-byte pieces they write into the same 64 / 128-byte rows of `a`
    // (c tiles) and `b` (n tiles) meet in that XCD's L2 and leave it as full lines
    // (maps with fewer than 16 pixel tiles keep the plain order — pixel tile fastest — which spreads them over all XCDs)
    const int ct = Cp >> 4, nt = Np >> 4;
    const int per = ct * nt;
    int ltile, r;
    if (xcd_groups) {
        const int xcd = blockIdx.x & 7, k = blockIdx.x >> 3;
        ltile = (k / per) * 8 + xcd;
        r = k - (k / per) * per;
    } else {
        const int lt = (L + 63) >> 6;
        r = blockIdx.x / lt;
        ltile = blockIdx.x - r * lt;
    }
    const int l0 = ltile * 64, c0 = (r % ct) * 16, n0 = (r / ct) * 16;
    if (l0 >= L) return;                                 // whole workgroup: the pixel-tile count is padded to a multiple of 8
    const float amax = state[0];
    const float fmax = f8_max(fmt);
    const float q = amax > 0.f ? fmax / amax : 1.f;
    if (scale_out && t == 0 && blockIdx.x == 0) *scale_out = amax > 0.f ? amax / fmax : 1.f;
    float m = 0.f;
    const int lq = t & 15, cr = t >> 4;                  // this thread's pixel quad and channel of the tile
    const int c = c0 + cr, l = l0 + 4 * lq;
    const int nvalid = N - n0 < 16 ? N - n0 : 16;
    const unsigned sstride = (unsigned)C * (unsigned)L * 4u;              // bytes per sample; 16 of them < 2^31 (host check)
    const unsigned win = (unsigned)nvalid * sstride;
    const rsrc_t rin = make_rsrc(in + (int64_t)n0 * C * L, win);
    const rsrc_t ry = make_rsrc(HASY ? yact + (int64_t)n0 * C * L : in, HASY ? win : 0u);
    unsigned o0[4];                                                     // VEC: o0[0] only
#pragma unroll
    for (int j = 0; j < 4; ++j) o0[j] = (c < C && l + j < L) ? ((unsigned)c * (unsigned)L + (unsigned)(l + j)) * 4u : OOB;
    unsigned wn[16];                                     // word of sample n0 + pass
    float csum = 0.f;                                    // this thread's share of the channel sum (16 samples x 4 pixels)
    constexpr int HB = HASY ? 8 : 16;                    // samples whose loads are in flight together (64 VGPRs either way)
#pragma unroll
    for (int half = 0; half < 16 / HB; ++half) {
        float4 vv[HB], yy[HASY ? HB : 1];
#pragma unroll
        for (int i = 0; i < HB; ++i) {
            const unsigned so = (unsigned)(half * HB + i) * sstride;
            if (VEC) {
                vv[i] = bload4(rin, o0[0] + so);
                if (HASY) yy[i] = bload4(ry, o0[0] + so);
            } else {
                vv[i] = make_float4(bload(rin, o0[0] + so), bload(rin, o0[1] + so), bload(rin, o0[2] + so), bload(rin, o0[3] + so));
                if (HASY) yy[i] = make_float4(bload(ry, o0[0] + so), bload(ry, o0[1] + so), bload(ry, o0[2] + so), bload(ry, o0[3] + so));
            }
        }
#pragma unroll
        for (int i = 0; i < HB; ++i) {
            const int pass = half * HB + i;
            float4 v = vv[i];
            if (HASY) {
                v.x *= f8_act_grad(yy[i].x, act, slope);
                v.y *= f8_act_grad(yy[i].y, act, slope);
                v.z *= f8_act_grad(yy[i].z, act, slope);
                v.w *= f8_act_grad(yy[i].w, act, slope);
            }
            csum += (v.x + v.y) + (v.z + v.w);
            m = fmaxf(fmaxf(m, fmaxf(fabsf(v.x), fabsf(v.y))), fmaxf(fabsf(v.z), fabsf(v.w)));
            wn[pass] = pack4(fminf(fmaxf(v.x * q, -fmax), fmax), fminf(fmaxf(v.y * q, -fmax), fmax),
                             fminf(fmaxf(v.z * q, -fmax), fmax), fminf(fmaxf(v.w * q, -fmax), fmax), fmt);
            if (a) tile[(pass * 16 + lq) * 16 + (cr ^ ((lq >> 2) << 2))] = wn[pass];
        }
    }
    if (part) {                                          // uniform; the 16 pixel-quad lanes of a channel are 16 consecutive lanes
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) csum += __shfl_xor(csum, o, 64);
        if (lq == 0 && c < C) part[((int64_t)(n0 >> 4) * ((L + 63) >> 6) + ltile) * C + c] = csum;
    }
    if (b && c < C) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (l + j >= L) break;
            const uint4 o = make_uint4(byte_of4(wn[0], wn[1], wn[2], wn[3], j), byte_of4(wn[4], wn[5], wn[6], wn[7], j),
                                       byte_of4(wn[8], wn[9], wn[10], wn[11], j), byte_of4(wn[12], wn[13], wn[14], wn[15], j));
            *reinterpret_cast<uint4*>(b + ((int64_t)c * L + l + j) * Np + n0) = o;
        }
    }
    if (a) {
        __syncthreads();
        const int nr = t >> 4;                           // (sample nr, pixel quad lq) of the tile
        if (n0 + nr < N) {
            uint4 w4[4];                                 // w4[k] = words of channels 4k .. 4k + 3
#pragma unroll
            for (int k = 0; k < 4; ++k)
                w4[k] = *reinterpret_cast<const uint4*>(&tile[(nr * 16 + lq) * 16 + ((k ^ (lq >> 2)) << 2)]);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (l + j >= L) break;
                const uint4 o = make_uint4(byte_of4(w4[0].x, w4[0].y, w4[0].z, w4[0].w, j), byte_of4(w4[1].x, w4[1].y, w4[1].z, w4[1].w, j),
                                           byte_of4(w4[2].x, w4[2].y, w4[2].z, w4[2].w, j), byte_of4(w4[3].x, w4[3].y, w4[3].z, w4[3].w, j));
                *reinterpret_cast<uint4*>(a + ((int64_t)(n0 + nr) * L + l + j) * Cp + c0) = o;
            }
        }
    }
    m = rg_block_max(m, red);
    if (t == 0 && m > 0.f) atomicMax(reinterpret_cast<int*>(state + 1), __float_as_int(m));
}

}  // namespace

// ---- scaling states -----------------------------------------------------------------------------------------------
extern "C" int rg_f8_amax(const float* x, int64_t n, float* state, hipStream_t stream) {
    RG_REQUIRE(x && state && n > 0, "rg_f8_amax: bad arguments");
    rg::ProfScope prof(rg::FAM_MISC, stream, 0.0, 4.0 * n);
    int64_t g = rg::cdiv64(n, 256 * 4 * 4);
    if (g > 2048) g = 2048;
    hipLaunchKernelGGL(f8_amax_kernel, dim3((unsigned)(g < 1 ? 1 : g)), dim3(256), 0, stream, x, n, state);
    return rg::check_launch("rg_f8_amax");
}

extern "C" int rg_f8_roll_scales(float* states, int count, hipStream_t stream) {
    RG_REQUIRE(states && count > 0, "rg_f8_roll_scales: bad arguments");
    hipLaunchKernelGGL(f8_roll_kernel, dim3(rg::cdiv(count, 256)), dim3(256), 0, stream, states, count);
    return rg::check_launch("rg_f8_roll_scales");
}

// out[b][l][r] (bytes, r padded to Rp = 16 * ceil(R / 16) with zeros) = fp8(in[b*bs + r*rs + l] * fmax / state[0]); fmt 0 e4m3, 1 e5m2
extern "C" int rg_f8_quantize(const float* in, void* out, float* state, float* scale_out, int fmt, int B, int R, int L,
                              int64_t bs, int64_t rs, hipStream_t stream) {
    RG_REQUIRE(in && out && state && (fmt == 0 || fmt == 1) && B > 0 && R > 0 && L > 0, "rg_f8_quantize: bad arguments");
    RG_REQUIRE(B <= 65535, "rg_f8_quantize: batch dimension %d exceeds the grid limit", B);
    const int Rp = rg::pad16(R);
    rg::ProfScope prof(rg::FAM_MISC, stream, 0.0, (double)B * L * (4.0 * R + Rp));
    hipLaunchKernelGGL(f8_quantize_transpose_kernel, dim3(rg::cdiv(L, 64), rg::cdiv(Rp, 64), B), dim3(256), 0, stream, in,
                       static_cast<unsigned char*>(out), state, scale_out, fmt, R, L, Rp, bs, rs);
    return rg::check_launch("rg_f8_quantize");
}

static void launch_quantize_dual(hipStream_t stream, unsigned wgs, const float* in, void* a, void* b, float* state, float* scale_out,
                                 int fmt, int N, int C, int L, int Cp, int Np, int xcd_groups, const float* yact, int act, float slope,
                                 float* part) {
    const bool vec = (L & 3) == 0;
#define RG_QD(V, Y)                                                                                                              \
    hipLaunchKernelGGL((f8_quantize_dual_kernel<V, Y>), dim3(wgs), dim3(256), 0, stream, in, static_cast<unsigned char*>(a),      \
                       static_cast<unsigned char*>(b), state, scale_out, fmt, N, C, L, Cp, Np, xcd_groups, yact, act, slope, part)
    if (vec && yact) RG_QD(true, true);
    else if (vec) RG_QD(true, false);
    else if (yact) RG_QD(false, true);
    else RG_QD(false, false);
#undef RG_QD
}

// Both layouts of in[N][C][L] in one pass: a [N][L][Cp] (may be NULL) and b [C][L][Np] (may be NULL); see rg_f8_quantize.
// Padding rows of `a` beyond C and of `b` beyond N are written as zeros only inside the 16-wide tiles that hold real data; callers
// allocate exactly Cp = 16*ceil(C/16), Np = 16*ceil(N/16), which those tiles cover.
extern "C" int rg_f8_quantize_dual(const float* in, void* a, void* b, float* state, float* scale_out, int fmt, int N, int C, int L,
                                   hipStream_t stream) {
    RG_REQUIRE(in && (a || b) && state && (fmt == 0 || fmt == 1) && N > 0 && C > 0 && L > 0, "rg_f8_quantize_dual: bad arguments");
    const int Cp = rg::pad16(C), Np = rg::pad16(N);
    const int lt = rg::cdiv(L, 64);
    const int xcd_groups = lt >= 16 ? 1 : 0;
    const int64_t wgs = (int64_t)(xcd_groups ? rg::cdiv(lt, 8) * 8 : lt) * (Cp / 16) * (Np / 16);
    RG_REQUIRE(wgs < (1ll << 31), "rg_f8_quantize_dual: tensor exceeds the grid limit");
    rg::ProfScope prof(rg::FAM_MISC, stream, 0.0, (double)L * (4.0 * N * C + (a ? (double)N * Cp : 0.0) + (b ? (double)C * Np : 0.0)));
    RG_REQUIRE((int64_t)C * L < (1ll << 24), "rg_f8_quantize_dual: C * L exceeds the 2^31-byte window of one 16-sample tile");
    launch_quantize_dual(stream, (unsigned)wgs, in, a, b, state, scale_out, fmt, N, C, L, Cp, Np, xcd_groups, nullptr, RG_ACT_NONE, 0.f,
                         nullptr);
    return rg::check_launch("rg_f8_quantize_dual");
}

// rows of `part` rg_f8_quantize_grad writes for [N][C][L]: one per (16-sample, 64-pixel) tile
extern "C" int rg_f8_grad_tiles(int N, int L) { return (rg::pad16(N) / 16) * rg::cdiv(L, 64); }

// The output-gradient operand of a convolution's backward in one pass over dy: g = dy * act'(yact) (yact NULL: g = dy) quantised
// into a [N][L][Cp] and / or b [C][L][Np] as rg_f8_quantize_dual does, with the per-tile channel sums of g in
// part[rg_f8_grad_tiles(N, L)][C] (NULL: not wanted).  Neither g nor a separate reduction pass over it touches memory.
extern "C" int rg_f8_quantize_grad(const float* dy, const float* yact, int act, float slope, void* a, void* b, float* part,
                                   float* state, float* scale_out, int fmt, int N, int C, int L, hipStream_t stream) {
    RG_REQUIRE(dy && (a || b || part) && state && (fmt == 0 || fmt == 1) && N > 0 && C > 0 && L > 0, "rg_f8_quantize_grad: bad arguments");
    RG_REQUIRE(act == RG_ACT_NONE || yact, "rg_f8_quantize_grad: the activation backward needs the forward output");
    const int Cp = rg::pad16(C), Np = rg::pad16(N);
    const int lt = rg::cdiv(L, 64);
    const int xcd_groups = lt >= 16 ? 1 : 0;
    const int64_t wgs = (int64_t)(xcd_groups ? rg::cdiv(lt, 8) * 8 : lt) * (Cp / 16) * (Np / 16);
    RG_REQUIRE(wgs < (1ll << 31), "rg_f8_quantize_grad: tensor exceeds the grid limit");
    const bool has_act = act != RG_ACT_NONE;
    rg::ProfScope prof(rg::FAM_MISC, stream, 0.0,
                       (double)L * ((has_act ? 8.0 : 4.0) * N * C + (a ? (double)N * Cp : 0.0) + (b ? (double)C * Np : 0.0)));
    RG_REQUIRE((int64_t)C * L < (1ll << 24), "rg_f8_quantize_grad: C * L exceeds the 2^31-byte window of one 16-sample tile");
    launch_quantize_dual(stream, (unsigned)wgs, dy, a, b, state, scale_out, fmt, N, C, L, Cp, Np, xcd_groups, has_act ? yact : nullptr,
                         act, slope, part);
    return rg::check_launch("rg_f8_quantize_grad");
}
