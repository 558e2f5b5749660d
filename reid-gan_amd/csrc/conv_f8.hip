// FP8 implicit-GEMM convolution family for gfx950 (MI355X): forward, data gradient, weight gradient on
// v_mfma_scale_f32_32x32x64_f8f6f4 (OCP e4m3 activations / filters, e5m2 gradients, per-tensor scales, fp32
// accumulate).  BASELINE config 5: the dual_gan two-generator path (CC/dual_gan/models/DPTN_model.py:216-225) asks for
// "fp8 MFMA convs"; the reference itself computes these layers in fp32 through cuDNN (nn.Conv2d / nn.ConvTranspose2d in
// CC/dual_gan/models/base_function.py:236-443), so this family has a DECLARED tolerance against the fp32 oracle and an
// exact CPU emulation of its own arithmetic (oracle/ref_fp8.py) for parity.
//
// Design (not a dtype switch of conv_igemm.hip: fp8 MFMA wants 8 reduction-contiguous BYTES per lane, so the data layout,
// not the kernel, is what changes):
//   * operands are quantised ONCE into layouts whose GEMM reduction axis is contiguous, 16-byte chunks of fp8 bytes with one
//     dequantisation scale per tensor (f8_quant.hip: the layouts, the scaling states, the quantisers);
//   * block tile BM x 128 x 64 bytes, 4 wave64 as 2 x 2, 32x32x64 MFMA tiles (one k-tile = one MFMA step per 32x32 block); LDS rows are 64 bytes with the 16-byte chunk
//     index XOR-swizzled by (row >> 2) & 3, which makes both the ds_write_b128 staging stores and the ds_read_b128 fragment
//     reads conflict-free; two ds_read_b128 per operand row feed one MFMA (lanes 0-31 take bytes 0-31 of the row, lanes 32-63
//     bytes 32-63, identically for both operands); a four-deep LDS-DMA ring, one barrier per k-tile, the next three tiles' loads in flight during the MFMAs.
#include "conv_plan.h"
#include "conv_prims.h"
#include "conv_reduce.h"

namespace {

using rg::conv::ConvGeom;
using rg::conv::fits_buffer;
using rg::pad16;

constexpr int NT = 256;
constexpr int BN = 128;
constexpr int ROWB = 64;                     // bytes of one LDS row = one k-tile
constexpr int NB = 4;                        // LDS buffers of the DMA ring: NB - 1 k-tiles in flight per workgroup

// ---------------------------------------------------------------------------------------------------------------
// GEMM core
// ---------------------------------------------------------------------------------------------------------------
struct F8Class : rg::conv::ParityClass {      // one stride-parity class of the data gradient (the single class of a stride-1 layer)
    int Ngc, Kc, ntiles;
    FastDiv d_nrw, d_hw, d_w;
};

struct F8P {
    const unsigned char* A;   // row operand of the GEMM rows m
    const unsigned char* B;   // row operand of the GEMM columns n
    unsigned a_bytes, b_bytes;
    float* out;               // fp32 result (NCHW activation, or dw / split-K partials for wgrad)
    unsigned out_bytes;
    const float* sa;          // dequantisation scales of the two operands (one device float each, written by the quantiser)
    const float* sb;
    const float* shift;       // per GEMM row (output channel) or null
    const float* res;         // like out or null
    int act;
    float slope;
    int M, Ng, Kc;            // rows, columns, 16-byte chunks along the reduction (fwd / wgrad; dgrad: per class)
    int m_tiles, n_tiles;
    int N, C, H, W, K, KH, KW, SH, SW, PH, PW, P, Q;
    int Cq;                   // 16-byte chunks per pixel of the gathered operand (fwd: Cp/16, dgrad: Kp/16, wgrad: Np/16)
    FastDiv d_cq, d_kw, d_pq, d_q, d_rs;
    int ktiles_per_split, splits;      // wgrad
    F8Class cls[4];
};

typedef int int8v __attribute__((ext_vector_type(8)));

// One 32x32x64 step: each lane supplies 32 reduction-contiguous bytes of its row of A and of B (lanes 0-31: bytes 0-31 of the
// 64-byte k-tile, lanes 32-63: bytes 32-63).  v_mfma_scale_f32_32x32x64_f8f6f4 with both block scales at 2^0 (E8M0 127) is
// the plain fp8 product at twice the issue rate of the 32x32x16 forms (the per-tensor scales are applied in the epilogue).
// FA / FB: 0 = e4m3, 1 = e5m2 — the instruction's own format codes.
template <int FA, int FB>
__device__ __forceinline__ floatx16 mfma8(int8v a, int8v b, floatx16 c) {
    return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a, b, c, FA, FB, 0, 127, 0, 127);
}

__device__ __forceinline__ unsigned lds_off(int row, int chunk) { return (unsigned)row * ROWB + (unsigned)((chunk ^ (row >> 2)) & 3) * 16u; }

// MODE 0 forward, 1 data gradient (class from the workgroup id, see below), 2 weight gradient (blockIdx.z = split)
// Operands reach LDS through an LDS-DMA ring (buffer_load ... lds, 16 bytes per lane): no staging registers, NB - 1 k-tiles in flight
// per workgroup.  A k-tile is only 64 reduction bytes = one MFMA step per 32x32 block (~100 ns of matrix work per workgroup), so the
// loop is bound by load LATENCY, not by issue: the ring plus 2-3 resident workgroups keeps ~10 tiles per CU in flight (the first
// version, a register-staged two-buffer loop, was measured slower: profiles/retired_switches.txt).
typedef __attribute__((address_space(3))) void lds_void_t;

template <int MODE, int BM, int FA, int FB>
__global__ __launch_bounds__(NT) void conv_f8_kernel(const F8P p) {
    constexpr int WTM = BM / 2, WTN = BN / 2;
    constexpr int TM = WTM / 32, TN = WTN / 32;
    constexpr int AR = BM / 64;              // A rows staged per thread (64 rows per pass)
    __shared__ __attribute__((aligned(16))) unsigned char lds[NB][(BM + BN) * ROWB];

    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int wm = wid >> 1, wn = wid & 1;
    // Data gradient with stride: the SH*SW parity classes of one tile write INTERLEAVED pixels of the same output rows (every
    // second float).  Their workgroups are laid out back to back on one XCD (id % 8 = XCD, classes fastest), so those half-written
    // lines meet in one L2 and leave it whole; launched class by class (grid z) the same bytes cost twice the HBM write time.
    int cls_idx = 0, tile_pre = -1;
    if (MODE == 1) {
        const int ncls = p.SH * p.SW;
        if (ncls > 1) {
            const int slots = p.m_tiles * p.n_tiles;           // n_tiles = the largest class
            const int xcd = blockIdx.x & 7, k = blockIdx.x >> 3;
            cls_idx = k % ncls;
            const int sl = k / ncls;
            const int q = slots >> 3, r = slots & 7;
            if (sl >= q + (xcd < r ? 1 : 0)) return;
            tile_pre = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + sl;
        }
    }
    const F8Class& cl = p.cls[cls_idx];
    const int ntl = MODE == 1 ? cl.ntiles : p.n_tiles;
    const int nwg = p.m_tiles * ntl;
    if (tile_pre < 0 && (int)blockIdx.x >= nwg) return;
    const int tile = tile_pre >= 0 ? tile_pre : xcd_remap(blockIdx.x, nwg);
    if (tile >= nwg) return;
    const int mt = tile % p.m_tiles, nt = tile / p.m_tiles;
    const int m0 = mt * BM, n0 = nt * BN;
    const int Ng = MODE == 1 ? cl.Ngc : p.Ng;
    const int Kc = MODE == 1 ? cl.Kc : p.Kc;
    const rsrc_t ra = make_rsrc(p.A, p.a_bytes), rb = make_rsrc(p.B, p.b_bytes);
    const int RS = p.KH * p.KW, HW = p.H * p.W, PQ = p.P * p.Q;
    const int ah = MODE == 1 ? cls_idx / p.SW : 0, aw = MODE == 1 ? cls_idx % p.SW : 0;

    // ---- per-thread staging rows: chunk (tid & 3) of rows (tid >> 2) + 64 i ----
    const int ch = tid & 3, srow = tid >> 2;
    int arow[AR];
    bool aok[AR];
#pragma unroll
    for (int i = 0; i < AR; ++i) {
        arow[i] = m0 + srow + 64 * i;
        aok[i] = arow[i] < p.M;
    }
    // gathered operand B: decode the two rows this thread stages
    int b_img[2], b_y[2], b_x[2];
    bool bok[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int n = n0 + srow + 64 * i;
        bok[i] = n < Ng;
        b_img[i] = b_y[i] = b_x[i] = 0;
        if (bok[i]) {
            if (MODE == 0) {                       // column = output pixel (img, pp, qq): top-left input position
                const int img = fdiv(n, p.d_pq);
                const int pq = n - img * PQ;
                const int pp = fdiv(pq, p.d_q);
                b_img[i] = img;
                b_y[i] = pp * p.SH - p.PH;
                b_x[i] = (pq - pp * p.Q) * p.SW - p.PW;
            } else if (MODE == 1) {                // column = input pixel (img, hc, wc) of this class
                const int img = fdiv(n, cl.d_hw);
                const int rem = n - img * cl.Hc * cl.Wc;
                const int hc = fdiv(rem, cl.d_w);
                const int wc = rem - hc * cl.Wc;
                b_img[i] = img;
                b_y[i] = (ah + p.SH * hc + p.PH - cl.r0) / p.SH;
                b_x[i] = (aw + p.SW * wc + p.PW - cl.s0) / p.SW;
            } else {                               // column = (c, r, s) of the filter
                const int c = fdiv(n, p.d_rs);
                const int rs = n - c * RS;
                const int r = fdiv(rs, p.d_kw);
                b_img[i] = c;
                b_y[i] = r - p.PH;
                b_x[i] = rs - r * p.KW - p.PW;
            }
        }
    }

    floatx16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    // byte offsets (or OOB) of the 16-byte chunks this thread fetches for k-tile kt; `chx` = its chunk of the 64-byte row
    auto tile_offsets = [&](int kt, int chx, unsigned (&oa)[AR], unsigned (&ob)[2]) {
        const int q = kt * 4 + chx;                // chunk index along the reduction
        const bool qok = q < Kc;
        const int t = fdiv(q, p.d_cq);             // fwd: filter tap; dgrad: tap of the class; wgrad: output pixel
        const int cc = q - t * p.Cq;
        if (MODE == 0) {
            const int r = fdiv(t, p.d_kw), s = t - r * p.KW;
#pragma unroll
            for (int i = 0; i < AR; ++i) oa[i] = (aok[i] && qok) ? (unsigned)(arow[i] * Kc + q) * 16u : OOB;
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int h = b_y[i] + r, w = b_x[i] + s;
                const bool ok = bok[i] && qok && (unsigned)h < (unsigned)p.H && (unsigned)w < (unsigned)p.W;
                ob[i] = ok ? (unsigned)(((b_img[i] * p.H + h) * p.W + w) * p.Cq + cc) * 16u : OOB;
            }
        } else if (MODE == 1) {
            const int j = fdiv(t, cl.d_nrw), jj = t - j * cl.nrw;
            const int rs = (cl.r0 + p.SH * j) * p.KW + cl.s0 + p.SW * jj;
#pragma unroll
            for (int i = 0; i < AR; ++i) oa[i] = (aok[i] && qok) ? (unsigned)((arow[i] * RS + rs) * p.Cq + cc) * 16u : OOB;
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int pp = b_y[i] - j, qq = b_x[i] - jj;
                const bool ok = bok[i] && qok && (unsigned)pp < (unsigned)p.P && (unsigned)qq < (unsigned)p.Q;
                ob[i] = ok ? (unsigned)(((b_img[i] * p.P + pp) * p.Q + qq) * p.Cq + cc) * 16u : OOB;
            }
        } else {
            const int pp = fdiv(t, p.d_q), qq = t - pp * p.Q;
#pragma unroll
            for (int i = 0; i < AR; ++i) oa[i] = (aok[i] && qok) ? (unsigned)((arow[i] * PQ + t) * p.Cq + cc) * 16u : OOB;
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int h = pp * p.SH + b_y[i], w = qq * p.SW + b_x[i];
                const bool ok = bok[i] && qok && (unsigned)h < (unsigned)p.H && (unsigned)w < (unsigned)p.W;
                ob[i] = ok ? (unsigned)((b_img[i] * HW + h * p.W + w) * p.Cq + cc) * 16u : OOB;
            }
        }
    };
    // LDS-DMA: lane l of wave w lands at (w*64 + l) * 16 bytes of the 4 KiB pass = row w*16 + l/4, physical chunk l%4, so the lane
    // fetches the LOGICAL chunk whose swizzled position that is (the XOR is an involution); out-of-range chunks arrive as zeros
    const int che = ch ^ ((srow >> 2) & 3);
    const unsigned lds_lane0 = (unsigned)__builtin_amdgcn_readfirstlane(wid) * 1024u;
    auto dma_tile = [&](int kt, int buf) {
        unsigned oa[AR], ob[2];
        tile_offsets(kt, che, oa, ob);
        unsigned char* base = lds[buf] + lds_lane0;
#pragma unroll
        for (int i = 0; i < AR; ++i)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(ra, (lds_void_t*)(base + i * 4096), 16, (int)oa[i], 0, 0, 0);
#pragma unroll
        for (int i = 0; i < 2; ++i)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rb, (lds_void_t*)(base + BM * ROWB + i * 4096), 16, (int)ob[i], 0, 0, 0);
    };

    const int nk = (Kc + 3) >> 2;
    int kt_begin = 0, kt_end = nk;
    if (MODE == 2) {
        kt_begin = (int)blockIdx.z * p.ktiles_per_split;
        kt_end = min(kt_begin + p.ktiles_per_split, nk);
    }
    const int l32 = lane & 31, lh = lane >> 5;
    auto compute_tile = [&](const unsigned char* As, const unsigned char* Bs) {
        int8v a[TM], b[TN];
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                const int row = wm * WTM + i * 32 + l32;
                const int4v lo = *reinterpret_cast<const int4v*>(As + lds_off(row, 2 * lh));
                const int4v hi = *reinterpret_cast<const int4v*>(As + lds_off(row, 2 * lh + 1));
                a[i] = int8v{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
            }
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                const int row = wn * WTN + j * 32 + l32;
                const int4v lo = *reinterpret_cast<const int4v*>(Bs + lds_off(row, 2 * lh));
                const int4v hi = *reinterpret_cast<const int4v*>(Bs + lds_off(row, 2 * lh + 1));
                b[j] = int8v{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
            }
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j) acc[i][j] = mfma8<FA, FB>(a[i], b[j], acc[i][j]);
    };
    constexpr int LPT = AR + 2;                    // DMA instructions per thread and k-tile
    const int nkt = kt_end - kt_begin;
#pragma unroll
    for (int sidx = 0; sidx < NB - 1; ++sidx)
        if (sidx < nkt) dma_tile(kt_begin + sidx, sidx);
    int buf = 0;
    for (int it = 0; it < nkt; ++it) {
        // tile `it` has landed once at most the younger tiles' DMAs (issued after it) are outstanding
        const int younger = min(NB - 2, nkt - 1 - it);
        if (younger >= 2) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * LPT) : "memory");
        else if (younger == 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(LPT) : "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();              // every wave's part of tile `it` is in LDS; every wave is done reading tile it-1
        if (it + NB - 1 < nkt) {
            int nbuf = buf + NB - 1;
            if (nbuf >= NB) nbuf -= NB;
            dma_tile(kt_begin + it + NB - 1, nbuf);              // into the buffer tile it-1 used
        }
        compute_tile(lds[buf], lds[buf] + BM * ROWB);
        if (++buf == NB) buf = 0;
    }

    // ---- epilogue ----
    const rsrc_t ro = make_rsrc(p.out, p.out_bytes);
    const int mrow0 = m0 + wm * WTM + 4 * lh;
    if (MODE == 2) {                               // raw partial sums [split][M][Ng]; the reduce kernel applies the scales
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const int nn = n0 + wn * WTN + j * 32 + l32;
            const unsigned ob = nn < Ng ? (unsigned)((((int64_t)blockIdx.z * p.M + mrow0) * Ng + nn) * 4) : OOB;
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int mo = i * 32 + (r & 3) + 8 * (r >> 2);
                    bstore(ro, (mrow0 + mo < p.M) ? ob + (unsigned)(mo * Ng) * 4u : OOB, acc[i][j][r]);
                }
        }
        return;
    }
    const float scale = p.sa[0] * p.sb[0];
    const bool has_shift = p.shift != nullptr, has_res = p.res != nullptr;       // uniform
    const rsrc_t rsh = make_rsrc(has_shift ? p.shift : p.sa, has_shift ? (unsigned)p.M * 4u : 0u);
    const rsrc_t rr = make_rsrc(has_res ? (const void*)p.res : (const void*)p.out, has_res ? p.out_bytes : 0u);
    const int PIX = MODE == 0 ? PQ : HW;
    // loads first, in batches (one wait per batch), then arithmetic and stores: a load -> wait -> store chain per element made the
    // first version of this epilogue cost more than the whole k-loop on the small DPTN layers
    float sh[TM][16];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) sh[i][r] = 0.f;
    if (has_shift) {
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) sh[i][r] = bload(rsh, (unsigned)(mrow0 + i * 32 + (r & 3) + 8 * (r >> 2)) * 4u);
    }
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        const int nn = n0 + wn * WTN + j * 32 + l32;
        unsigned ob = OOB;
        if (nn < Ng) {
            if (MODE == 0) {
                const int img = fdiv(nn, p.d_pq);
                ob = (unsigned)((((int64_t)img * p.M + mrow0) * PQ + (nn - img * PQ)) * 4);
            } else {
                const int img = fdiv(nn, cl.d_hw);
                const int rem = nn - img * cl.Hc * cl.Wc;
                const int hc = fdiv(rem, cl.d_w);
                const int wc = rem - hc * cl.Wc;
                ob = (unsigned)((((int64_t)img * p.M + mrow0) * HW + (ah + p.SH * hc) * p.W + aw + p.SW * wc) * 4);
            }
        }
        unsigned off[TM][16];
        float rv[TM][16];
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int mo = i * 32 + (r & 3) + 8 * (r >> 2);
                off[i][r] = (mrow0 + mo < p.M) ? ob + (unsigned)(mo * PIX) * 4u : OOB;
                rv[i][r] = 0.f;
            }
        if (has_res) {
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int r = 0; r < 16; ++r) rv[i][r] = bload(rr, off[i][r]);
        }
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r)
                bstore(ro, off[i][r], rg_apply_act(acc[i][j][r] * scale + sh[i][r] + rv[i][r], p.act, p.slope));
    }
}

// dw[i] = scale_a * scale_b * sum_s partial[s][i]   (the fixed summation tree of conv_reduce.h: deterministic)
__global__ __launch_bounds__(256) void f8_splitk_reduce_kernel(const float* __restrict__ ws, float* __restrict__ out, int64_t n,
                                                               int splits, const float* __restrict__ sa, const float* __restrict__ sb) {
    int64_t i;
    float s;
    if (!splitk_sum(ws, n, splits, i, s)) return;
    out[i] = s * (sa[0] * sb[0]);
}

// n % 4 == 0: float4 outputs, per element the values of f8_splitk_reduce_kernel
__global__ __launch_bounds__(256) void f8_splitk_reduce_vec_kernel(const float* __restrict__ ws, float* __restrict__ out, int64_t n,
                                                                   int splits, const float* __restrict__ sa,
                                                                   const float* __restrict__ sb) {
    int64_t i;
    float4 v;
    if (!splitk_sum4(ws, n, splits, i, v)) return;
    const float sc = sa[0] * sb[0];
    reinterpret_cast<float4*>(out)[i] = make_float4(v.x * sc, v.y * sc, v.z * sc, v.w * sc);
}

static void fill_geom(F8P& p, const ConvGeom& g) {
    p.N = g.N; p.C = g.C; p.H = g.H; p.W = g.W; p.K = g.K; p.KH = g.KH; p.KW = g.KW;
    p.SH = g.SH; p.SW = g.SW; p.PH = g.PH; p.PW = g.PW; p.P = g.P; p.Q = g.Q;
    p.d_kw = make_fastdiv(g.KW);
    p.d_pq = make_fastdiv(g.P * g.Q);
    p.d_q = make_fastdiv(g.Q);
    p.d_rs = make_fastdiv(g.KH * g.KW);
    p.ktiles_per_split = 1 << 30;
    p.splits = 1;
    p.shift = nullptr;
    p.res = nullptr;
    p.act = 0;
    p.slope = 0.f;
}

// (not rg::conv::validate: that one also refuses a first window lying wholly in the padding, which these entry points accept)
static int check_geom(const char* op, const ConvGeom& g) {
    RG_REQUIRE(g.N > 0 && g.C > 0 && g.H > 0 && g.W > 0 && g.K > 0 && g.KH > 0 && g.KW > 0 && g.SH > 0 && g.SW > 0 && g.PH >= 0 &&
                   g.PW >= 0 && g.P > 0 && g.Q > 0, "%s: bad dimension", op);
    RG_REQUIRE((int64_t)(g.P - 1) * g.SH - g.PH < g.H && (int64_t)(g.Q - 1) * g.SW - g.PW < g.W, "%s: output larger than input allows", op);
    RG_REQUIRE(fits_buffer((int64_t)g.N * g.C * g.H * g.W * 4) && fits_buffer((int64_t)g.N * g.K * g.P * g.Q * 4) &&
                   fits_buffer((int64_t)g.K * g.C * g.KH * g.KW * 4),
               "%s: every tensor must be smaller than 2 GiB (32-bit buffer offsets)", op);
    return RG_OK;
}

// fa / fb: formats of the A / B operand (0 e4m3, 1 e5m2; e5m2 x e5m2 is not instantiated)
template <int MODE, int BM>
static void launch_f8_formats(dim3 grid, hipStream_t stream, const F8P& p, int fa, int fb) {
    if (fa == 0 && fb == 0) hipLaunchKernelGGL((conv_f8_kernel<MODE, BM, 0, 0>), grid, dim3(NT), 0, stream, p);
    else if (fa == 0) hipLaunchKernelGGL((conv_f8_kernel<MODE, BM, 0, 1>), grid, dim3(NT), 0, stream, p);
    else hipLaunchKernelGGL((conv_f8_kernel<MODE, BM, 1, 0>), grid, dim3(NT), 0, stream, p);
}

template <int MODE>
static void launch_f8(dim3 grid, hipStream_t stream, const F8P& p, int bm, int fa, int fb) {
    if (bm == 128) launch_f8_formats<MODE, 128>(grid, stream, p, fa, fb);
    else launch_f8_formats<MODE, 64>(grid, stream, p, fa, fb);
}

}  // namespace

// ---- forward: y[N][K][P][Q] fp32 = act(sx * sw * conv(xq, wq) + shift + residual) ------------------------------------
// xq [N][H*W][Cp] (fmt_x: 0 e4m3 activations, 1 e5m2 — the data gradient of a transposed convolution), wq [K][KH*KW][Cp] e4m3
extern "C" int rg_conv2d_f8_fwd(const void* xq, const void* wq, const float* sx, const float* sw, int fmt_x, float* y, int N,
                                int C, int H, int W, int K, int KH, int KW, int SH, int SW, int PH, int PW, int P, int Q,
                                const float* shift, const float* residual, int act, float slope, hipStream_t stream) {
    const ConvGeom g = {N, C, H, W, K, KH, KW, SH, SW, PH, PW, P, Q};
    if (int e = check_geom("rg_conv2d_f8_fwd", g)) return e;
    RG_REQUIRE(xq && wq && sx && sw && y, "rg_conv2d_f8_fwd: null tensor");
    F8P p;
    fill_geom(p, g);
    const int Cp = pad16(C);
    p.A = static_cast<const unsigned char*>(wq);
    p.B = static_cast<const unsigned char*>(xq);
    p.a_bytes = (unsigned)((int64_t)K * KH * KW * Cp);
    p.b_bytes = (unsigned)((int64_t)N * H * W * Cp);
    p.out = y;
    p.out_bytes = (unsigned)((int64_t)N * K * P * Q * 4);
    p.sa = sw; p.sb = sx;
    p.shift = shift; p.res = residual; p.act = act; p.slope = slope;
    p.M = K; p.Ng = N * P * Q;
    p.Cq = Cp / 16;
    p.Kc = KH * KW * p.Cq;
    p.d_cq = make_fastdiv(p.Cq);
    const int bm = K <= 64 ? 64 : 128, fa = 0, fb = fmt_x;
    p.m_tiles = rg::cdiv(K, bm);
    p.n_tiles = rg::cdiv(p.Ng, BN);
    rg::ProfScope prof(rg::FAM_CONV_F8, stream, 2.0 * K * (double)p.Ng * C * KH * KW,
                       (double)N * H * W * Cp + (double)K * KH * KW * Cp + 4.0 * N * K * P * Q);
    const dim3 grid(p.m_tiles * p.n_tiles, 1, 1);
    launch_f8<0>(grid, stream, p, bm, fa, fb);
    return rg::check_launch("rg_conv2d_f8_fwd");
}

// ---- data gradient / transposed-convolution forward: dx[N][C][H][W] fp32 from dyq [N][P*Q][Kp] and wq_t [C][KH*KW][Kp] --------
extern "C" int rg_conv2d_f8_dgrad(const void* dyq, const void* wq_t, const float* sdy, const float* sw, int fmt_dy, float* dx,
                                  int N, int C, int H, int W, int K, int KH, int KW, int SH, int SW, int PH, int PW, int P,
                                  int Q, const float* shift, const float* residual, int act, float slope, hipStream_t stream) {
    const ConvGeom g = {N, C, H, W, K, KH, KW, SH, SW, PH, PW, P, Q};
    if (int e = check_geom("rg_conv2d_f8_dgrad", g)) return e;
    RG_REQUIRE(dyq && wq_t && sdy && sw && dx, "rg_conv2d_f8_dgrad: null tensor");
    RG_REQUIRE(SH <= 2 && SW <= 2, "rg_conv2d_f8_dgrad: stride > 2 not supported (got %d,%d)", SH, SW);
    F8P p;
    fill_geom(p, g);
    const int Kp = pad16(K);
    p.A = static_cast<const unsigned char*>(wq_t);
    p.B = static_cast<const unsigned char*>(dyq);
    p.a_bytes = (unsigned)((int64_t)C * KH * KW * Kp);
    p.b_bytes = (unsigned)((int64_t)N * P * Q * Kp);
    p.out = dx;
    p.out_bytes = (unsigned)((int64_t)N * C * H * W * 4);
    p.sa = sw; p.sb = sdy;
    p.shift = shift; p.res = residual; p.act = act; p.slope = slope;
    p.M = C;
    p.Cq = Kp / 16;
    p.d_cq = make_fastdiv(p.Cq);
    const int bm = C <= 64 ? 64 : 128, fa = 0, fb = fmt_dy;
    p.m_tiles = rg::cdiv(C, bm);
    int nt_max = 0;
    double flops = 0.0;
    for (int ah = 0; ah < SH; ++ah)
        for (int aw = 0; aw < SW; ++aw) {
            F8Class& cl = p.cls[ah * SW + aw];
            static_cast<rg::conv::ParityClass&>(cl) = rg::conv::parity_class(g, ah, aw);
            cl.Ngc = N * cl.Hc * cl.Wc;
            cl.Kc = cl.nrh * cl.nrw * p.Cq;
            cl.ntiles = rg::cdiv(cl.Ngc, BN);
            cl.d_nrw = make_fastdiv(cl.nrw);
            cl.d_hw = make_fastdiv(cl.Hc * cl.Wc);
            cl.d_w = make_fastdiv(cl.Wc);
            if (cl.ntiles > nt_max) nt_max = cl.ntiles;
            flops += 2.0 * C * (double)cl.Ngc * K * cl.nrh * cl.nrw;
        }
    p.Ng = 0; p.Kc = 0; p.n_tiles = nt_max;
    rg::ProfScope prof(rg::FAM_CONV_F8, stream, flops,
                       (double)N * P * Q * Kp + (double)C * KH * KW * Kp + 4.0 * N * C * H * W);
    const int slots = p.m_tiles * nt_max;
    const dim3 grid(SH * SW > 1 ? (unsigned)(8 * ((slots >> 3) + 1) * SH * SW) : (unsigned)slots, 1, 1);
    launch_f8<1>(grid, stream, p, bm, fa, fb);
    return rg::check_launch("rg_conv2d_f8_dgrad");
}

// ---- weight gradient: dw[K][C][KH][KW] fp32 from xq [C][H*W][Np] and dyq [K][P*Q][Np] (batch-contiguous layouts) --------------
namespace {
static void plan_f8_wgrad(int M, int Ng, int nk, int* bm, int* splits, int* per) {
    *bm = M <= 64 ? 64 : 128;
    const int tiles = rg::cdiv(M, *bm) * rg::cdiv(Ng, BN);
    int want = rg::cdiv(1024, tiles);
    if (want > nk / 8) want = nk / 8;          // >= 8 k-tiles (512 reduction bytes) per split
    if (want < 1) want = 1;
    if (want > 1024) want = 1024;
    while (want > 1 && (int64_t)want * M * Ng * 4 >= (1ll << 31)) --want;
    *per = rg::cdiv(nk, want);
    *splits = rg::cdiv(nk, *per);
}
}  // namespace

extern "C" size_t rg_conv2d_f8_wgrad_workspace(int N, int C, int K, int KH, int KW, int P, int Q) {
    const int Np = pad16(N);
    const int nk = rg::cdiv(P * Q * (Np / 16), 4);
    int bm, splits, per;
    plan_f8_wgrad(K, C * KH * KW, nk, &bm, &splits, &per);
    return (size_t)splits * (size_t)K * (size_t)C * KH * KW * sizeof(float);
}

extern "C" int rg_conv2d_f8_wgrad(const void* xq, const void* dyq, const float* sx, const float* sdy, int fmt_x, int fmt_dy,
                                  float* dw, int N, int C, int H, int W, int K, int KH, int KW, int SH, int SW, int PH, int PW,
                                  int P, int Q, void* workspace, size_t workspace_bytes, hipStream_t stream) {
    const ConvGeom g = {N, C, H, W, K, KH, KW, SH, SW, PH, PW, P, Q};
    if (int e = check_geom("rg_conv2d_f8_wgrad", g)) return e;
    RG_REQUIRE(xq && dyq && sx && sdy && dw, "rg_conv2d_f8_wgrad: null tensor");
    RG_REQUIRE(fmt_x != fmt_dy || fmt_x == 0, "rg_conv2d_f8_wgrad: e5m2 x e5m2 is not instantiated");
    F8P p;
    fill_geom(p, g);
    const int Np = pad16(N);
    p.A = static_cast<const unsigned char*>(dyq);
    p.B = static_cast<const unsigned char*>(xq);
    p.a_bytes = (unsigned)((int64_t)K * P * Q * Np);
    p.b_bytes = (unsigned)((int64_t)C * H * W * Np);
    RG_REQUIRE(fits_buffer((int64_t)K * P * Q * Np) && fits_buffer((int64_t)C * H * W * Np), "rg_conv2d_f8_wgrad: operand exceeds 2 GiB");
    p.sa = sdy; p.sb = sx;
    p.M = K; p.Ng = C * KH * KW;
    p.Cq = Np / 16;
    p.Kc = P * Q * p.Cq;
    p.d_cq = make_fastdiv(p.Cq);
    const int nk = rg::cdiv(p.Kc, 4);
    int bm, splits, per;
    plan_f8_wgrad(p.M, p.Ng, nk, &bm, &splits, &per);
    const size_t need = (size_t)splits * p.M * (size_t)p.Ng * sizeof(float);
    if (!workspace || need > workspace_bytes) {
        rg::set_error("rg_conv2d_f8_wgrad: workspace too small (%zu < %zu)", workspace_bytes, need);
        return RG_ERR_WORKSPACE;
    }
    p.splits = splits; p.ktiles_per_split = per;
    p.out = static_cast<float*>(workspace);
    p.out_bytes = (unsigned)need;
    p.m_tiles = rg::cdiv(p.M, bm);
    p.n_tiles = rg::cdiv(p.Ng, BN);
    const int fa = fmt_dy, fb = fmt_x;
    rg::ProfScope prof(rg::FAM_CONV_F8, stream, 2.0 * K * (double)C * KH * KW * N * P * Q,
                       (double)K * P * Q * Np + (double)C * H * W * Np + 4.0 * K * C * KH * KW);
    const dim3 grid(p.m_tiles * p.n_tiles, 1, splits);
    launch_f8<2>(grid, stream, p, bm, fa, fb);
    if (int e = rg::check_launch("rg_conv2d_f8_wgrad")) return e;
    const int64_t n = (int64_t)p.M * p.Ng;
    if ((n & 3) == 0 && ((reinterpret_cast<uintptr_t>(workspace) | reinterpret_cast<uintptr_t>(dw)) & 15) == 0)
        hipLaunchKernelGGL(f8_splitk_reduce_vec_kernel, dim3((unsigned)rg::cdiv64(n >> 2, 64)), dim3(256), 0, stream,
                           static_cast<const float*>(workspace), dw, n, splits, sdy, sx);
    else
        hipLaunchKernelGGL(f8_splitk_reduce_kernel, dim3((unsigned)rg::cdiv64(n, 64)), dim3(256), 0, stream,
                           static_cast<const float*>(workspace), dw, n, splits, sdy, sx);
    return rg::check_launch("rg_conv2d_f8_wgrad(reduce)");
}
