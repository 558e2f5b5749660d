// Data gradient (also the forward of ConvTranspose2d): dx[C, N*Hc*Wc] = w^T[C, K*taps] x gather(dy), one GEMM per stride-parity class
// (overview and arithmetic: conv_igemm.hip; plans and measured choices: conv_plan.h).  Kernels: the generic implicit GEMM
// (conv_dgrad_kernel, conv_dgrad_pl_kernel), the 1x1 LDS-DMA kernel, the tap-reuse 3x3 kernel (conv_halo.h), the small-C kernels and
// the strided split-K finisher; entry points rg_conv2d_dgrad, rg_conv2d_dgrad_workspace, rg_conv2d_dgrad_rowsum_cols.
#define RG_PLANES_DGRAD
#include "conv_halo.h"

namespace {

// ---------------------------------------------------------------------------------------------
// data gradient (also the forward of ConvTranspose2d), one GEMM per stride-parity class.
// MODE 0: weights [K][C][KH][KW], reduction order (ko, tap), scalar loads (any geometry)
// MODE 1: weights [K][KH*KW][C] (== the original tensor for 1x1), tap-major order k' = tap*K + ko, K % 16 == 0 and
//         C % 4 == 0: weight operand float4 along C, one bounds test per tile for dy
// MODE 2: MODE 1 layout + 1x1 / stride 1 / pad 0 with P*Q % 4 == 0: dy loads as float4 too (any K)
// ---------------------------------------------------------------------------------------------
template <int BM, int BN, int WM, int WN, int MODE>
__global__ __launch_bounds__(NT) __attribute__((amdgpu_waves_per_eu(RG_WAVES))) void conv_dgrad_kernel(const DgradP dp) {
    using T = Tile<BM, BN, WM, WN>;
    static_assert(BN >= 64, "the gather loader needs a wave-uniform k");
    __shared__ __attribute__((aligned(16))) float As[2][BK][T::LDA];
    __shared__ __attribute__((aligned(16))) float Bs[2][BK][T::LDB];
    const ConvP& p = dp.c;
    const int ci = blockIdx.z;
    const DgradClass& cl = dp.cls[ci];
    const int ah = ci / p.SW, aw = ci % p.SW;

    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int wm = wid / WN, wn = wid % WN;
    const int nwg = p.m_tiles * cl.ntiles;
    if ((int)blockIdx.x >= nwg) return;
    if (p.partial && (p.SH > 1 || p.SW > 1) && cl.Kgc <= 0) return;      // strided split-K: the finisher writes tap-less classes itself
    const int tile = xcd_remap(blockIdx.x, nwg);
    const int mt = tile % p.m_tiles, nt = tile / p.m_tiles;
    const int m0 = mt * BM, n0 = nt * BN;
    const int split = blockIdx.y;
    const int PQ = p.P * p.Q;
    const int RS = p.KH * p.KW;
    const int taps = cl.nrh * cl.nrw;
    const rsrc_t rw = make_rsrc(p.w, p.w_bytes), rdy = make_rsrc(p.x, p.x_bytes);

    // ---- B operand (dy) ----
    constexpr int BKSTEP = NT / BN > 0 ? NT / BN : 1;
    const int bcol = tid % BN;
    const int bk0 = __builtin_amdgcn_readfirstlane(tid / BN);
    constexpr int BV = BN / 4;
    constexpr int BVSTEP = NT / BV;
    constexpr int BVCNT = (BV * BK + NT - 1) / NT;
    const int vcol = tid % BV, vrow0 = tid / BV;
    bool bvalid;
    int hb = 0, wb = 0, imgb = 0;
    unsigned bvoff = OOB;
    if (MODE == 2) {
        const int n = n0 + 4 * vcol;
        bvalid = n < cl.Ngc && vrow0 < BK;
        if (bvalid) {
            const int img = fdiv(n, cl.d_hw);
            bvoff = (unsigned)((((int64_t)img * p.K + vrow0) * PQ + (n - img * PQ)) * 4);
        }
    } else {
        const int n = n0 + bcol;
        bvalid = n < cl.Ngc;
        if (bvalid) {
            const int img = fdiv(n, cl.d_hw);
            const int rem = n - img * cl.Hc * cl.Wc;
            const int hc = fdiv(rem, cl.d_w);
            const int wc = rem - hc * cl.Wc;
            hb = (ah + p.SH * hc + p.PH - cl.r0) / p.SH;
            wb = (aw + p.SW * wc + p.PW - cl.s0) / p.SW;
            imgb = img * p.K * PQ;
        }
    }

    // ---- A operand (weights), GEMM row m = input channel c ----
    constexpr int AKSTEP = NT / BM > 0 ? NT / BM : 1;
    constexpr int ACNT0 = (BM * BK / NT) < 1 ? 1 : (BM * BK / NT);
    const int acol = tid % BM, ak0 = tid / BM;
    constexpr int AV = BM / 4;
    constexpr int AVSTEP = NT / AV;
    constexpr int AVCNT = (AV * BK + NT - 1) / NT;
    const int avcol = tid % AV, avrow0 = tid / AV;
    // MODE 1/2: byte offset of (row k' = avrow0, m) inside one tap block of the [K][RS][C] tensor, or OOB
    const unsigned avoff = (MODE != 0 && m0 + 4 * avcol < p.M && avrow0 < BK)
                               ? (unsigned)(((int64_t)avrow0 * RS * p.C + m0 + 4 * avcol) * 4) : OOB;

    float ra[MODE == 0 ? ACNT0 : 1];
    float4 rav[MODE == 0 ? 1 : AVCNT];
    float rb[MODE == 2 ? 1 : T::BCNT];
    float4 rbv[MODE == 2 ? BVCNT : 1];
    floatx16 acc[T::TM][T::TN];
    zero_acc<T>(acc);

    auto load_tile = [&](int kt) {
        const int kbase = kt * BK;
        const bool ktail = kbase + BK > cl.Kgc;
        if (MODE == 0) {
            const int am = m0 + acol;
#pragma unroll
            for (int i = 0; i < ACNT0; ++i) {
                const int k = kbase + ak0 + i * AKSTEP;
                const int ko = fdiv(k, cl.d_taps);
                const int t = k - ko * taps;
                const int j = fdiv(t, cl.d_nrw);
                const int jj = t - j * cl.nrw;
                const int r = cl.r0 + p.SH * j, s = cl.s0 + p.SW * jj;
                const bool ok = am < p.M && k < cl.Kgc;
                ra[i] = bload(rw, ok ? (unsigned)((((int64_t)ko * p.C + am) * RS + r * p.KW + s) * 4) : OOB);
            }
#pragma unroll
            for (int i = 0; i < T::BCNT; ++i) {
                const int k = kbase + bk0 + i * BKSTEP;          // wave-uniform -> scalar unit
                const int ko = fdiv(k, cl.d_taps);
                const int t = k - ko * taps;
                const int j = fdiv(t, cl.d_nrw);
                const int jj = t - j * cl.nrw;
                const int pp = hb - j, qq = wb - jj;
                const bool ok = bvalid && k < cl.Kgc && (unsigned)pp < (unsigned)p.P && (unsigned)qq < (unsigned)p.Q;
                rb[i] = bload(rdy, ok ? (unsigned)(imgb + ko * PQ + pp * p.Q + qq) * 4u : OOB);
            }
            return;
        }
        // tap-major order: the whole tile shares one filter tap (scalar decode)
        const int tap = fdiv(kbase, p.d_k);
        const int ko0 = kbase - tap * p.K;
        const int j = fdiv(tap, cl.d_nrw);
        const int jj = tap - j * cl.nrw;
        const int rs = (cl.r0 + p.SH * j) * p.KW + cl.s0 + p.SW * jj;
        {
            const unsigned tbase = (unsigned)(((int64_t)ko0 * RS + rs) * p.C * 4);
            const unsigned kstride = (unsigned)(AVSTEP * RS * p.C) * 4u;
#pragma unroll
            for (int i = 0; i < AVCNT; ++i) {
                unsigned o = avoff + tbase + (unsigned)i * kstride;
                if (ktail && kbase + avrow0 + i * AVSTEP >= cl.Kgc) o = OOB;
                rav[i] = bload4(rw, o);
            }
        }
        if (MODE == 2) {
            const unsigned kstride = (unsigned)PQ * 4u;
#pragma unroll
            for (int i = 0; i < BVCNT; ++i) {
                unsigned o = bvoff + (unsigned)(kbase + i * BVSTEP) * kstride;
                if (ktail && kbase + vrow0 + i * BVSTEP >= cl.Kgc) o = OOB;
                rbv[i] = bload4(rdy, o);
            }
        } else {
            const int pp = hb - j, qq = wb - jj;
            const bool ok = bvalid && (unsigned)pp < (unsigned)p.P && (unsigned)qq < (unsigned)p.Q;
            const unsigned o0 = ok ? (unsigned)(imgb + (ko0 + bk0) * PQ + pp * p.Q + qq) * 4u : OOB;
            const unsigned kstride = (unsigned)(BKSTEP * PQ) * 4u;
#pragma unroll
            for (int i = 0; i < T::BCNT; ++i) rb[i] = bload(rdy, o0 + (unsigned)i * kstride);
        }
    };
    auto store_tile = [&](int buf, int q) {
        if (MODE == 0) {
#pragma unroll
            for (int i = 0; i < ACNT0; ++i)
                if (in_quarter(i, ACNT0, q)) As[buf][ak0 + i * AKSTEP][acol] = ra[i];
        } else {
#pragma unroll
            for (int i = 0; i < AVCNT; ++i) {
                const int kk = avrow0 + i * AVSTEP;
                if (kk < BK && in_quarter(i, AVCNT, q)) *reinterpret_cast<float4*>(&As[buf][kk][4 * avcol]) = rav[i];
            }
        }
        if (MODE == 2) {
#pragma unroll
            for (int i = 0; i < BVCNT; ++i) {
                const int kk = vrow0 + i * BVSTEP;
                if (kk < BK && in_quarter(i, BVCNT, q)) *reinterpret_cast<float4*>(&Bs[buf][kk][4 * vcol]) = rbv[i];
            }
        } else {
#pragma unroll
            for (int i = 0; i < T::BCNT; ++i)
                if (in_quarter(i, T::BCNT, q)) Bs[buf][bk0 + i * BKSTEP][bcol] = rb[i];
        }
    };

    const int nk = (cl.Kgc + BK - 1) / BK;
    const int kt_begin = split * cl.ktps;
    int kt_end = kt_begin + cl.ktps;
    if (kt_end > nk) kt_end = nk;
    if (kt_begin < kt_end) {
        load_tile(kt_begin);
        store_tile(0, -1);
    }
    __syncthreads();
    int cur = 0;
    for (int kt = kt_begin; kt < kt_end; ++kt) {
        const bool has_next = kt + 1 < kt_end;
        if (has_next) load_tile(kt + 1);
        mma_tile<T>(As[cur], Bs[cur], acc, wm, wn, lane, [&](int q) {
            if (has_next) store_tile(cur ^ 1, q);
        });
        __syncthreads();
        cur ^= 1;
    }

    if (p.SH == 1 && p.SW == 1) {       // one class: output pixels are contiguous, shared epilogue (+ split-K)
        store_tile_nchw<T>(p, acc, m0, n0, wm, wn, lane, cl.Ngc, p.H * p.W, cl.d_hw, split, (cl.poff + nt) * WN + wn);
        return;
    }
    if (p.partial) {                    // strided split-K: raw accumulators to partial[split][m][coff + n] (conv_splitk_finish_strided_kernel)
        store_tile_partial_cols<T>(p, acc, m0, n0, wm, wn, lane, cl.Ngc, cl.coff, dp.ng_total, split);
        return;
    }
    // strided classes: pixel (hc, wc) of the class lands on (ah + SH*hc, aw + SW*wc); same fused epilogue
    const int l32 = lane & 31, kh = lane >> 5;
    const int HW = p.H * p.W;
    const int mrow0 = m0 + wm * T::WTM + 4 * kh;
    unsigned ob[T::TN];
#pragma unroll
    for (int j = 0; j < T::TN; ++j) {
        const int nn = n0 + wn * T::WTN + j * 32 + l32;
        ob[j] = OOB;
        if (nn < cl.Ngc) {
            const int im = fdiv(nn, cl.d_hw);
            const int rem = nn - im * cl.Hc * cl.Wc;
            const int hc = fdiv(rem, cl.d_w);
            const int wc = rem - hc * cl.Wc;
            const int h = ah + p.SH * hc, w = aw + p.SW * wc;
            ob[j] = (unsigned)((((int64_t)im * p.C + mrow0) * HW + h * p.W + w) * 4);
        }
    }
    store_tile_epilogue_any<T>(p, acc, ob, (unsigned)HW * 4u, mrow0, (cl.poff + nt) * WN + wn);
}

// ---------------------------------------------------------------------------------------------
// 1x1 / stride 1 / pad 0 data gradient with LDS-DMA staging.  Both operands are k-major in memory exactly as the LDS tile wants
// them: the filter tile [16 ko][BM c] is 16 rows of W[K][C], the gradient tile [16 ko][128 pixels] 16 channel rows of dy — so
// `buffer_load_dwordx4 ... lds` moves them global -> LDS with no staging registers, no ds_write and no VALU (lane l of wave w lands at
// (w * 64 + l) * 16 bytes of a 4 KiB pass = row pass*R + (w*64 + l) / (ROWS/4), 16-byte column (w*64 + l) % (ROWS/4): lane-linear).
// Ring of NB = 3 LDS tiles: two k-tiles in flight per workgroup behind the one being multiplied, counted `s_waitcnt vmcnt`, ONE raw
// s_barrier per k-tile (a __syncthreads would drain the DMAs).  The unpadded k-major rows keep the fragment reads conflict-free
// (lane = row, consecutive floats).  Same epilogue, same split-K as conv_dgrad_kernel<MODE 2>, whose launches it replaces when the
// planner picks a 128-pixel tile.
// ---------------------------------------------------------------------------------------------
typedef __attribute__((address_space(3))) void lds_void_t;

template <int BM>
__global__ __launch_bounds__(NT) __attribute__((amdgpu_waves_per_eu(RG_WAVES))) void conv1x1_dma_kernel(const DgradP dp) {
    using T = Tile<BM, 128, 2, 2>;
    constexpr int NB = 3;
    constexpr int ATILE = BK * BM * 4, BTILE = BK * 128 * 4;          // bytes
    constexpr int APASS = ATILE / 4096, BPASS = BTILE / 4096;         // 4 KiB passes (256 lanes x 16 B) per tile
    constexpr int LPT = APASS + BPASS;                                // DMA instructions per thread and k-tile
    static_assert(APASS >= 1 && ATILE % 4096 == 0, "filter tile is a whole number of DMA passes");
    __shared__ __attribute__((aligned(16))) unsigned char lds[NB][ATILE + BTILE];
    const ConvP& p = dp.c;
    const DgradClass& cl = dp.cls[0];

    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int wm = wid >> 1, wn = wid & 1;
    const int l32 = lane & 31, kh = lane >> 5;
    const int nwg = p.m_tiles * cl.ntiles;
    if ((int)blockIdx.x >= nwg) return;
    const int tile = xcd_remap(blockIdx.x, nwg);
    const int mt = tile % p.m_tiles, nt = tile / p.m_tiles;
    const int m0 = mt * BM, n0 = nt * 128;
    const int split = blockIdx.y;
    const int PQ = p.P * p.Q;
    const rsrc_t rw = make_rsrc(p.w, p.w_bytes), rdy = make_rsrc(p.x, p.x_bytes);

    // ---- DMA source offsets of this lane (k row 0 of the pass) ----
    constexpr int ALANES = BM / 4, AROWS = 256 / ALANES;              // lanes per filter row, filter rows per pass
    const int acol = (tid % ALANES) * 4, arow = tid / ALANES;
    const unsigned aoff = (m0 + acol < p.M) ? (unsigned)((arow * p.C + m0 + acol) * 4) : OOB;      // W[ko][c]: row stride C
    const int bcol = (tid & 31) * 4, brow = tid >> 5;                 // 32 lanes per 128-pixel row, 8 rows per pass
    unsigned boff = OOB;
    {
        const int n = n0 + bcol;
        if (n < cl.Ngc) {
            const int img = fdiv(n, cl.d_hw);
            boff = (unsigned)((((int64_t)img * p.K + brow) * PQ + (n - img * PQ)) * 4);
        }
    }
    const unsigned lds_lane0 = (unsigned)__builtin_amdgcn_readfirstlane(wid) * 1024u;

    auto dma_tile = [&](int kt, int buf) {
        const int kbase = kt * BK;
        unsigned char* base = lds[buf] + lds_lane0;
#pragma unroll
        for (int i = 0; i < APASS; ++i) {
            const int k = kbase + arow + i * AROWS;
            const unsigned o = (aoff != OOB && k < p.K) ? aoff + (unsigned)((kbase + i * AROWS) * p.C) * 4u : OOB;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rw, (lds_void_t*)(base + i * 4096), 16, (int)o, 0, 0, 0);
        }
#pragma unroll
        for (int i = 0; i < BPASS; ++i) {
            const int k = kbase + brow + i * 8;
            const unsigned o = (boff != OOB && k < p.K) ? boff + (unsigned)((kbase + i * 8) * PQ) * 4u : OOB;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rdy, (lds_void_t*)(base + ATILE + i * 4096), 16, (int)o, 0, 0, 0);
        }
    };

    floatx16 acc[T::TM][T::TN];
    zero_acc<T>(acc);
    const int nk = (p.K + BK - 1) / BK;
    const int kt_begin = split * p.ktiles_per_split;
    int kt_end = kt_begin + p.ktiles_per_split;
    if (kt_end > nk) kt_end = nk;
    const int nkt = kt_end > kt_begin ? kt_end - kt_begin : 0;
#pragma unroll
    for (int sidx = 0; sidx < NB - 1; ++sidx)
        if (sidx < nkt) dma_tile(kt_begin + sidx, sidx);
    int buf = 0;
    for (int it = 0; it < nkt; ++it) {
        // tile `it` has landed once at most the younger tile's DMAs (issued after it) are outstanding
        if (it + 1 < nkt) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(LPT) : "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();          // every wave's part of tile `it` is in LDS; every wave is done reading tile it-1
        if (it + NB - 1 < nkt) {
            int nbuf = buf + NB - 1;
            if (nbuf >= NB) nbuf -= NB;
            dma_tile(kt_begin + it + NB - 1, nbuf);          // into the buffer tile it-1 used
        }
        const float* As = reinterpret_cast<const float*>(lds[buf]);
        const float* Bs = reinterpret_cast<const float*>(lds[buf] + ATILE);
        mma_kstep<T::TM, T::TN>([&](int i, int q) { return As[(8 * kh + q) * BM + wm * T::WTM + i * 32 + l32]; },
                                [&](int j, int q) { return Bs[(8 * kh + q) * 128 + wn * T::WTN + j * 32 + l32]; }, acc);
        if (++buf == NB) buf = 0;
    }
    store_tile_nchw<T>(p, acc, m0, n0, wm, wn, lane, cl.Ngc, p.H * p.W, cl.d_hw, split, (cl.poff + nt) * 2 + wn);
}

// Data gradient for layers with <= 4 input channels (the RGB stem, FD/reid/models/resnet.py via torchvision conv1;
// the generator's 64 -> 3 output ConvTranspose, FD/fdgan/networks.py:133-138).  A 32-row MFMA tile would be > 87 %
// padding there, so this is a direct VALU kernel: one thread per input pixel of one stride-parity class (uniform
// tap set per block), all C channels in registers, the filter bank [K][KH*KW][4] staged once in LDS (broadcast
// float4 reads), dy read coalesced along the row.
template <int CMAX>
__global__ __launch_bounds__(256) void conv_dgrad_smallc_kernel(const DgradP dp) {
    extern __shared__ __attribute__((aligned(16))) float wl[];      // [K][RS][CMAX]
    const ConvP& p = dp.c;
    const int ci = blockIdx.z;
    const DgradClass& cl = dp.cls[ci];
    const int ah = ci / p.SW, aw = ci % p.SW;
    const int RS = p.KH * p.KW, PQ = p.P * p.Q, HW = p.H * p.W;
    for (int i = threadIdx.x; i < p.K * RS * CMAX; i += blockDim.x) {
        const int c = i % CMAX, t = i / CMAX;          // t = ko*RS + rs
        const int ko = t / RS, rs = t - ko * RS;
        wl[i] = c < p.C ? p.w[((int64_t)ko * p.C + c) * RS + rs] : 0.f;
    }
    __syncthreads();
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= cl.Ngc) return;
    const int img = fdiv(n, cl.d_hw);
    const int rem = n - img * cl.Hc * cl.Wc;
    const int hc = fdiv(rem, cl.d_w);
    const int wc = rem - hc * cl.Wc;
    const int h = ah + p.SH * hc, w = aw + p.SW * wc;
    const int hb = (h + p.PH - cl.r0) / p.SH, wb = (w + p.PW - cl.s0) / p.SW;
    const float* dyb = p.x + (int64_t)img * p.K * PQ;
    float acc[CMAX];
#pragma unroll
    for (int c = 0; c < CMAX; ++c) acc[c] = 0.f;
    for (int j = 0; j < cl.nrh; ++j) {
        const int pp = hb - j;
        if ((unsigned)pp >= (unsigned)p.P) continue;
        for (int jj = 0; jj < cl.nrw; ++jj) {
            const int qq = wb - jj;
            if ((unsigned)qq >= (unsigned)p.Q) continue;
            const int rs = (cl.r0 + p.SH * j) * p.KW + cl.s0 + p.SW * jj;
            const float* src = dyb + pp * p.Q + qq;
            const float* wrow = wl + rs * CMAX;
#pragma unroll 4
            for (int ko = 0; ko < p.K; ++ko) {
                const float v = src[(int64_t)ko * PQ];
                const float4 wv = *reinterpret_cast<const float4*>(wrow + (int64_t)ko * RS * CMAX);
                acc[0] += v * wv.x;
                if (CMAX > 1) acc[1] += v * wv.y;
                if (CMAX > 2) acc[2] += v * wv.z;
                if (CMAX > 3) acc[3] += v * wv.w;
            }
        }
    }
#pragma unroll
    for (int c = 0; c < CMAX; ++c) {
        if (c < p.C) {
            float v = acc[c];
            if (p.ep.scale) v *= p.ep.scale[c];
            if (p.ep.shift) v += p.ep.shift[c];
            const int64_t o = ((int64_t)img * p.C + c) * HW + h * p.W + w;
            if (p.ep.res) v += p.ep.res[o];
            v = rg_apply_act(v, p.ep.act, p.ep.slope);
            if (p.ep.mask && !(p.ep.mask[o] > 0.f)) v = 0.f;
            p.y[o] = v;
        }
    }
}

// Register-tiled form of the small-C data gradient for <= 4 taps per axis and class (7x7 / 2, 4x4 / 2, 3x3 / 1):
// lanes run along a class row (coalesced loads of dy), each thread owns PX consecutive class ROWS of one column, so
// one broadcast filter read serves PX pixels and the PX + NRH - 1 gradient rows are loaded once per channel and
// slide across the vertical taps in registers.  The plain kernel above issues one global load and one LDS read per
// 3 FMAs and is bound by the load path.  Branch-free inner loops: rows / columns outside dy are buffer loads with an
// out-of-range offset (-> 0).
template <int PX, int NRH, int NRW>
__device__ __forceinline__ void smallc_px_accumulate(const ConvP& p, const DgradClass& cl, const float* wl, int img,
                                                     int hb0, int wb, float (&acc)[PX][3]) {
    constexpr int WR = PX + NRH - 1;
    const int RS = p.KH * p.KW, PQ = p.P * p.Q;
    const rsrc_t rdy = make_rsrc(p.x, p.x_bytes);
    // pixel i (class row hc0 + i), tap (j, jj) reads dy[pp = hb0 + i - j][q = wb - jj]: window row r = i + NRH-1 - j
    const unsigned imgoff = (unsigned)img * (unsigned)p.K * (unsigned)PQ * 4u;
    unsigned off[WR][NRW];
#pragma unroll
    for (int r = 0; r < WR; ++r) {
        const int pp = hb0 - (NRH - 1) + r;
        const unsigned rowoff = (unsigned)pp < (unsigned)p.P ? imgoff + (unsigned)(pp * p.Q) * 4u : OOB;
#pragma unroll
        for (int jj = 0; jj < NRW; ++jj) {
            const int q = wb - jj;
            const unsigned qo = (unsigned)q < (unsigned)p.Q ? (unsigned)q * 4u : OOB;
            off[r][jj] = ((rowoff | qo) & OOB) ? OOB : rowoff + qo;
        }
    }
    const float* wbase = wl + (cl.r0 * p.KW + cl.s0) * 4;
#pragma unroll 2
    for (int ko = 0; ko < p.K; ++ko) {
        float v[WR][NRW];
        const unsigned koff = (unsigned)ko * (unsigned)PQ * 4u;          // an out-of-range offset stays out of range
#pragma unroll
        for (int r = 0; r < WR; ++r)
#pragma unroll
            for (int jj = 0; jj < NRW; ++jj) v[r][jj] = bload(rdy, off[r][jj] + koff);
#pragma unroll
        for (int j = 0; j < NRH; ++j)
#pragma unroll
            for (int jj = 0; jj < NRW; ++jj) {
                const float4 wv = *reinterpret_cast<const float4*>(wbase + (ko * RS + p.SH * j * p.KW + p.SW * jj) * 4);
#pragma unroll
                for (int i = 0; i < PX; ++i) {
                    acc[i][0] += v[i + NRH - 1 - j][jj] * wv.x;
                    acc[i][1] += v[i + NRH - 1 - j][jj] * wv.y;
                    acc[i][2] += v[i + NRH - 1 - j][jj] * wv.z;
                }
            }
    }
}

template <int PX>
__global__ __launch_bounds__(256) void conv_dgrad_smallc_px_kernel(const DgradP dp) {
    extern __shared__ __attribute__((aligned(16))) float wl[];      // [K][RS][4]
    const ConvP& p = dp.c;
    // block id = 8*ncls*a + 8*ci + x -> pixel region 8a + x of class ci: the classes of one region read the same rows
    // of dy, so they run back to back on the same XCD (ids are dealt round-robin over the 8 XCDs) and share its L2
    const int ncls = p.SH * p.SW;
    const int ci = (blockIdx.x >> 3) % ncls;
    const int region = (int)(blockIdx.x / (8 * ncls)) * 8 + (blockIdx.x & 7);
    const DgradClass& cl = dp.cls[ci];
    const int ah = ci / p.SW, aw = ci % p.SW;
    const int RS = p.KH * p.KW, HW = p.H * p.W;
    const int Hg = (cl.Hc + PX - 1) / PX;
    if (cl.Hc <= 0 || cl.Wc <= 0 || region * (int)blockDim.x >= p.N * Hg * cl.Wc) return;   // uniform
    for (int i = threadIdx.x; i < p.K * RS * 4; i += blockDim.x) {
        const int c = i & 3, t = i >> 2;               // t = ko*RS + rs
        wl[i] = c < p.C ? p.w[(int64_t)(t / RS) * p.C * RS + c * RS + (t % RS)] : 0.f;
    }
    __syncthreads();
    const int n = region * blockDim.x + threadIdx.x;
    if (n >= p.N * Hg * cl.Wc) return;
    const int img = n / (Hg * cl.Wc);
    const int rem = n - img * Hg * cl.Wc;
    const int hg = rem / cl.Wc;
    const int wc = rem - hg * cl.Wc;
    const int hc0 = hg * PX;
    const int hb0 = (ah + p.SH * hc0 + p.PH - cl.r0) / p.SH;
    const int wb = (aw + p.SW * wc + p.PW - cl.s0) / p.SW;
    float acc[PX][3];
#pragma unroll
    for (int i = 0; i < PX; ++i) acc[i][0] = acc[i][1] = acc[i][2] = 0.f;
#define RG_SMALLC_CASE(NRH_, NRW_) \
    case NRH_ * 8 + NRW_: smallc_px_accumulate<PX, NRH_, NRW_>(p, cl, wl, img, hb0, wb, acc); break
    switch (cl.nrh * 8 + cl.nrw) {                      // uniform per block
        RG_SMALLC_CASE(1, 1); RG_SMALLC_CASE(1, 2); RG_SMALLC_CASE(1, 3); RG_SMALLC_CASE(1, 4);
        RG_SMALLC_CASE(2, 1); RG_SMALLC_CASE(2, 2); RG_SMALLC_CASE(2, 3); RG_SMALLC_CASE(2, 4);
        RG_SMALLC_CASE(3, 1); RG_SMALLC_CASE(3, 2); RG_SMALLC_CASE(3, 3); RG_SMALLC_CASE(3, 4);
        RG_SMALLC_CASE(4, 1); RG_SMALLC_CASE(4, 2); RG_SMALLC_CASE(4, 3); RG_SMALLC_CASE(4, 4);
        default: break;                                 // no tap reaches this class: zeros (+ epilogue)
    }
#undef RG_SMALLC_CASE
    const int w = aw + p.SW * wc;
#pragma unroll
    for (int i = 0; i < PX; ++i) {
        if (hc0 + i >= cl.Hc) break;
        const int h = ah + p.SH * (hc0 + i);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if (c < p.C) {
                float v = acc[i][c];
                if (p.ep.scale) v *= p.ep.scale[c];
                if (p.ep.shift) v += p.ep.shift[c];
                const int64_t o = ((int64_t)img * p.C + c) * HW + h * p.W + w;
                if (p.ep.res) v += p.ep.res[o];
                v = rg_apply_act(v, p.ep.act, p.ep.slope);
                if (p.ep.mask && !(p.ep.mask[o] > 0.f)) v = 0.f;
                p.y[o] = v;
            }
        }
    }
}

#include "conv_planes.h"

// Strided data gradient with split-K: partial[s][m][col] holds the classes' columns side by side; column col of class ci is pixel
// (img, hc, wc) of that stride-parity class = output pixel (ah + SH hc, aw + SW wc).  One thread per OUTPUT element (m, img, h, w):
// its class and column follow from (h, w), the stores are coalesced along w and the partial loads are SW interleaved unit-stride
// streams (one per column parity).  Same epilogue as the one-class finisher.
__global__ __launch_bounds__(256) void conv_splitk_finish_strided_kernel(const float* __restrict__ partial, float* __restrict__ out,
                                                                         const DgradP dp, int splits, FastDiv d_hw, FastDiv d_w,
                                                                         FastDiv d_nhw) {
    const ConvP& p = dp.c;
    const int ncols = dp.ng_total;
    const int HW = p.H * p.W, NHW = p.N * HW;
    const int64_t total = (int64_t)p.M * NHW, slab = (int64_t)p.M * ncols;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int m = fdiv((int)i, d_nhw);
        const int r = (int)i - m * NHW;
        const int im = fdiv(r, d_hw);
        const int hw = r - im * HW;
        const int h = fdiv(hw, d_w), w = hw - h * p.W;
        const int ah = h % p.SH, aw = w % p.SW;               // SH, SW <= 2
        const DgradClass& cl = dp.cls[ah * p.SW + aw];
        const int col = cl.coff + (im * cl.Hc + h / p.SH) * cl.Wc + w / p.SW;
        const float* pp = partial + (int64_t)m * ncols + col;
        float v = 0.f;
        if (cl.Kgc > 0)                                       // classes without filter taps (1x1 / stride 2: three of four) hold no partials
            for (int s = 0; s < splits; ++s) v += pp[(int64_t)s * slab];
        const int64_t o = ((int64_t)im * p.M + m) * HW + hw;
        if (p.ep.scale) v *= p.ep.scale[m];
        if (p.ep.shift) v += p.ep.shift[m];
        if (p.ep.res) v += p.ep.res[o];
        v = rg_apply_act(v, p.ep.act, p.ep.slope);
        if (p.ep.mask && !(p.ep.mask[o] > 0.f)) v = 0.f;
        out[o] = v;
    }
}

}  // namespace

using namespace rg::conv;

// MODE of the loader (conv_dgrad_kernel) from mode; the plane kernels (conv_planes.h) have 4 or 8 waves
#define RG_DGRAD_LAUNCH_K(KERNEL, NTH, BM_, BN_, WM_, WN_)                                                          \
    if (mode == 2) hipLaunchKernelGGL((KERNEL<BM_, BN_, WM_, WN_, 2>), grid, dim3(NTH), 0, stream, dp);             \
    else if (mode == 1) hipLaunchKernelGGL((KERNEL<BM_, BN_, WM_, WN_, 1>), grid, dim3(NTH), 0, stream, dp);        \
    else hipLaunchKernelGGL((KERNEL<BM_, BN_, WM_, WN_, 0>), grid, dim3(NTH), 0, stream, dp)
#define RG_DGRAD_LAUNCH(BM_, BN_, WM_, WN_) RG_DGRAD_LAUNCH_K(conv_dgrad_kernel, NT, BM_, BN_, WM_, WN_)
#define RG_DGRAD_PL_LAUNCH(BM_, BN_, WM_, WN_) RG_DGRAD_LAUNCH_K(conv_dgrad_pl_kernel, 64 * WM_ * WN_, BM_, BN_, WM_, WN_)

namespace {

// The stride-parity classes of a data gradient and what its plan depends on.  Only classes that have filter taps do MFMA work (a
// 1x1 / stride-2 layer has ONE such class, the others only zero-fill), and their reductions differ: a strided launch is planned on
// the columns that carry work, and on the DEEPEST class when its reductions may split (the classes' workgroups start together, so an
// unsplit launch lasts as long as its deepest class — 4 taps against a mean of 2.25 for 3x3 / 2 — and planning on the mean depth kept
// the layer4 gradients unsplit on 64 x 64 tiles: l4.0.conv2 95 -> 71 us, l4.0.down 83 -> 71 us with four splits,
// profiles/r04_strided_dgrad.txt), on their mean depth otherwise.
struct DgradShape {
    int64_t ng_max, kg_max;      // the widest class, the deepest class
    int64_t ng_eff, kg_eff;      // columns of the classes with taps, their mean depth
    int64_t ng_total;            // columns of all classes: one partial row of a strided split-K launch
    double flops;
    // Strided classes may split their reductions too: the 3x3 / 1x1 stride-2 layers of layer3 /
    // layer4 have 32-128 tiles for 256 CUs and class depths that differ 4x (1, 2, 2 and 4 taps); every class is cut into the same
    // number of splits of ITS depth, the partial columns of the classes lie side by side and conv_splitk_finish_strided_kernel
    // scatters the sums to the classes' pixels with the fused epilogue.
    bool ssplit;
};
static DgradShape dgrad_classes(const ConvGeom& g, DgradClass* cls) {
    DgradShape s = {0, 0, 0, 0, 0, 0.0, false};
    double kw_sum = 0.0;
    for (int ah = 0; ah < g.SH; ++ah)
        for (int aw = 0; aw < g.SW; ++aw) {
            DgradClass& cl = cls[ah * g.SW + aw];
            static_cast<ParityClass&>(cl) = parity_class(g, ah, aw);
            cl.Ngc = g.N * cl.Hc * cl.Wc;
            cl.Kgc = g.K * cl.nrh * cl.nrw;
            cl.d_taps = make_fastdiv(cl.nrh * cl.nrw);
            cl.d_nrw = make_fastdiv(cl.nrw);
            cl.d_hw = make_fastdiv(cl.Hc * cl.Wc);
            cl.d_w = make_fastdiv(cl.Wc);
            cl.coff = (int)s.ng_total;
            s.ng_total += cl.Ngc;
            if (cl.Ngc > s.ng_max) s.ng_max = cl.Ngc;
            if (cl.Kgc > s.kg_max) s.kg_max = cl.Kgc;
            s.flops += 2.0 * g.C * (double)cl.Ngc * cl.Kgc;
            if (cl.Kgc > 0) {
                s.ng_eff += cl.Ngc;
                kw_sum += (double)cl.Ngc * cl.Kgc;
            }
        }
    s.kg_eff = s.ng_eff > 0 ? (int64_t)(kw_sum / (double)s.ng_eff) : s.kg_max;
    s.ssplit = s.ng_eff > 0 && (int64_t)g.C * g.N * g.H * g.W < (1ll << 31);
    return s;
}
// the depth a strided launch is planned on (see above)
static int64_t strided_kg(const DgradShape& s) { return s.ssplit ? s.kg_max : s.kg_eff; }

// Layers the tap-reuse kernel takes: the data gradient of a 3x3 / stride 1 / pad 1 convolution on maps halo_geom accepts ...
static bool dgrad_halo_geom(const ConvGeom& g) {
    return g.SH == 1 && g.SW == 1 && g.KH == 3 && g.KW == 3 && g.PH == 1 && g.PW == 1 && g.P == g.H && g.Q == g.W && g.K % BK == 0 &&
           g.C % 4 == 0 && g.C >= 64 && halo_geom(g.H, g.W);
}
// ... whose caller passed the [K][9][C] filters, float4-aligned like the gradient (wk: see dgrad_impl)
static bool dgrad_halo_operands(const float* dy, const float* wk) { return wk && aligned16(dy); }

struct DgradOps {                // operands of one data gradient; ep: scale .. rowsum_cols as the entry point got them
    const float *dy, *w, *w_krsc;
    float* dx;
    Epilogue ep;
};

struct DgradCall {
    const ConvGeom& g;
    const DgradOps& o;
    Workspace ws;                // (a planning call: as if the queried workspace were supplied)
    hipStream_t stream;
    int* dry;
    DgradP dp;                   // classes, operands, epilogue: what no plan changes
    DgradShape s;
    bool one_class;
    int mode;                    // weight operand layout / loader (conv_dgrad_kernel MODE)
};

const int kTileWN[4] = {2, 2, 2, 4};               // wave columns of the tile shapes in RG_TILE_SWITCH
// row-sum column blocks the launch of plan q writes (0: split-K has no fused row sums)
static int rowsum_cols_of(const DgradCall& c, const Plan& q) {
    if (q.splits > 1) return 0;
    int nts = 0;
    for (int i = 0; i < c.g.SH * c.g.SW; ++i) nts += rg::cdiv(c.dp.cls[i].Ngc, kTileBN[q.tile]);
    return nts * kTileWN[q.tile];
}
#define RG_REQUIRE_ROWSUM_COLS(ep, cols)                                                                                     \
    RG_REQUIRE(!(ep).rowsum || ((cols) > 0 && (ep).rowsum_cols == (cols)),                                                   \
               "rg_conv2d_dgrad: rowsum_cols %d does not match this launch (%d; query rg_conv2d_dgrad_rowsum_cols)", (ep).rowsum_cols, \
               (cols))

// RGB-sized outputs (C <= 4): direct kernels
static int dgrad_smallc(const DgradCall& c) {
    const ConvGeom& g = c.g;
    DgradP dp = c.dp;
    const int ncls = g.SH * g.SW;
    const size_t lds = (size_t)g.K * g.KH * g.KW * 4 * sizeof(float);
    RG_REQUIRE(!dp.c.ep.rowsum, "rg_conv2d_dgrad: row sums are not available on the small-C path (query rg_conv2d_dgrad_rowsum_cols)");
    dp.c.Ng = (int)c.s.ng_max;
    dp.c.Kg = g.K * g.KH * g.KW;
    rg::ProfScope prof(rg::FAM_CONV_DGRAD, c.stream, c.s.flops, alg_bytes(g));
    bool few_taps = g.C <= 3;
    int gmax = 0;
    for (int i = 0; i < ncls; ++i) {
        few_taps = few_taps && dp.cls[i].nrw <= 4 && dp.cls[i].nrh <= 4;
        const int gi = g.N * rg::cdiv(dp.cls[i].Hc, 4) * dp.cls[i].Wc;
        if (gi > gmax) gmax = gi;
    }
    if (few_taps && gmax > 0)
        hipLaunchKernelGGL((conv_dgrad_smallc_px_kernel<4>), dim3(((rg::cdiv(gmax, 256) + 7) / 8) * 8 * ncls), dim3(256), lds, c.stream,
                           dp);
    else
        hipLaunchKernelGGL((conv_dgrad_smallc_kernel<4>), dim3(rg::cdiv(dp.c.Ng, 256), 1, ncls), dim3(256), lds, c.stream, dp);
    return rg::check_launch("rg_conv2d_dgrad(small-C)");
}

// one generic launch of plan pl, or (planning call) the row-sum column blocks it would write
static int dgrad_run_plan(const DgradCall& c, Plan pl) {
    const ConvGeom& g = c.g;
    hipStream_t stream = c.stream;
    const int mode = c.mode, ncls = g.SH * g.SW;
    DgradP dp = c.dp;
    ConvP& p = dp.c;
    const int ncols = (int)(c.one_class ? c.s.ng_max : c.s.ng_total);      // columns of one partial row
    p.partial_bytes = (unsigned)fit_splits(pl, p.M, ncols, c.ws, (size_t)1 << 31);
    for (int i = 0; i < ncls; ++i)             // k-tiles per split: the plan's for one class, each class' own depth / splits otherwise
        dp.cls[i].ktps = c.one_class ? pl.ktiles_per_split
                                     : (pl.splits > 1 ? (int)rg::cdiv64(rg::cdiv64(dp.cls[i].Kgc > 0 ? dp.cls[i].Kgc : 1, BK), pl.splits) : (1 << 30));
    p.m_tiles = pl.m_tiles;
    int nt_max = 0, nt_sum = 0;
    for (int i = 0; i < ncls; ++i) {
        dp.cls[i].ntiles = rg::cdiv(dp.cls[i].Ngc, kTileBN[pl.tile]);
        dp.cls[i].poff = nt_sum;
        nt_sum += dp.cls[i].ntiles;
        if (dp.cls[i].ntiles > nt_max) nt_max = dp.cls[i].ntiles;
    }
    const int cols = rowsum_cols_of(c, pl);
    if (c.dry) {
        *c.dry = cols;
        return RG_OK;
    }
    RG_REQUIRE_ROWSUM_COLS(p.ep, cols);
    p.n_tiles = nt_max;
    p.Ng = (int)c.s.ng_max;
    p.Kg = g.K * g.KH * g.KW;
    p.splits = pl.splits; p.ktiles_per_split = pl.ktiles_per_split;
    p.partial = pl.splits > 1 ? static_cast<float*>(c.ws.ptr) : nullptr;
    p.arrive = (pl.splits > 1 && c.one_class) ? splitk_arrivals(stream, p.m_tiles * nt_max, p.partial, p.y, p.M, p.Ng, g.H * g.W, p.ep)
                                              : nullptr;
    rg::ProfScope prof(rg::FAM_CONV_DGRAD, stream, c.s.flops, alg_bytes(g));
    const dim3 grid(p.m_tiles * nt_max, pl.splits, ncls);
    const TuneKey tk = tune_key(2, g, mode, pl.tile, pl.splits, ep_bits(p.ep, true));
    // (the 64 x 128 eight-wave form has four wave columns: not with fused row sums, whose column count the caller sized for two)
    choose_impl(2, tk, stream, (pl.tile == 0 || (pl.tile == 1 && !p.ep.rowsum)) ? 3 : 2, [&](int impl) {
        if (impl == 2) {
            if (pl.tile == 0) { RG_DGRAD_PL_LAUNCH(128, 128, 4, 2); }
            else { RG_DGRAD_PL_LAUNCH(64, 128, 2, 4); }
        } else if (impl) {
            RG_TILE_SWITCH(pl.tile, RG_DGRAD_PL_LAUNCH);
        } else if (mode == 2 && (pl.tile == 0 || pl.tile == 1) && g.C % 4 == 0) {
            // 1x1 / stride 1: both operands are lane-linear in memory -> LDS-DMA ring (conv1x1_dma_kernel)
            if (pl.tile == 0) hipLaunchKernelGGL((conv1x1_dma_kernel<128>), grid, dim3(NT), 0, stream, dp);
            else hipLaunchKernelGGL((conv1x1_dma_kernel<64>), grid, dim3(NT), 0, stream, dp);
        } else {
            RG_TILE_SWITCH(pl.tile, RG_DGRAD_LAUNCH);
        }
    });
    if (pl.splits > 1 && !p.arrive) {
        if (int e = rg::check_launch("rg_conv2d_dgrad")) return e;
        if (c.one_class) launch_finish(stream, p.partial, p.y, p.M, p.Ng, g.H * g.W, make_fastdiv(g.H * g.W), pl.splits, p.ep);
        else hipLaunchKernelGGL(conv_splitk_finish_strided_kernel, dim3(finish_grid((int64_t)p.M * g.N * g.H * g.W)), dim3(256), 0, stream,
                                p.partial, p.y, dp, pl.splits, make_fastdiv(g.H * g.W), make_fastdiv(g.W), make_fastdiv(g.N * g.H * g.W));
    }
    return rg::check_launch("rg_conv2d_dgrad");
}

// `dry` != nullptr: plan only (as if the queried workspace were supplied) and report the number of row-sum column blocks the
// launch would write (0: split-K or the small-C kernel, which have no fused row sums); nothing is launched.
int dgrad_impl(const ConvGeom& g, const DgradOps& o, const Workspace& ws, hipStream_t stream, int* dry, bool allow_halo = true) {
    if (int e = validate("rg_conv2d_dgrad", g)) return e;
    RG_REQUIRE(dry || (o.dy && o.w && o.dx), "rg_conv2d_dgrad: null tensor");
    RG_REQUIRE(g.SH <= 2 && g.SW <= 2, "rg_conv2d_dgrad: stride > 2 not supported (got %d,%d)", g.SH, g.SW);
    if (dry) *dry = 0;
    DgradCall c = {g, o, dry ? Workspace{dry, ~(size_t)0} : ws, stream, dry};
    ConvP& p = c.dp.c;
    fill_common(p, g);
    p.x = o.dy; p.w = o.w; p.y = o.dx;
    p.ep = o.ep;
    p.M = g.C;
    p.x_bytes = y_bytes(g); p.w_bytes = w_bytes(g); p.y_bytes = x_bytes(g);
    c.s = dgrad_classes(g, c.dp.cls);
    c.dp.ng_total = (int)c.s.ng_total;
    c.one_class = g.SH == 1 && g.SW == 1;
    if (g.C <= 4 && (size_t)g.K * g.KH * g.KW * 4 * sizeof(float) <= 64 * 1024) return dry ? RG_OK : dgrad_smallc(c);
    // weight operand layout / loader: w_krsc, or for 1x1 filters the original tensor, which already has that layout
    const bool is1x1 = g.KH == 1 && g.KW == 1;
    const float* wk = is1x1 ? (aligned16(o.w) ? o.w : nullptr) : ((o.w_krsc && aligned16(o.w_krsc)) ? o.w_krsc : nullptr);
    c.mode = 0;
    if (wk && g.C % 4 == 0) {
        if (is1x1 && c.one_class && g.PH == 0 && g.PW == 0 && ((g.P * g.Q) % 4 == 0) && aligned16(o.dy)) c.mode = 2;
        else if (g.K % 16 == 0) c.mode = 1;
        if (c.mode) p.w = wk;
    }
    // (a planning call has no pointers: rg_hip/ops/conv.py always passes the [K][9][C] copy for such layers)
    if (allow_halo && dgrad_halo_geom(g) && (dry || dgrad_halo_operands(o.dy, wk))) {
        const HaloPlan hpl = halo_plan(p.M, c.s.ng_max, g.K, &c.ws);
        const int cols = hpl.splits > 1 ? 0 : hpl.n_tiles * 2;
        if (dry) {
            *dry = cols;
            return RG_OK;
        }
        RG_REQUIRE_ROWSUM_COLS(o.ep, cols);
        ConvP ph = p;
        ph.w = wk;
        ph.Ng = (int)c.s.ng_max;
        ph.Kg = g.K * g.KH * g.KW;
        auto launch_halo = [&]() -> int {
            rg::ProfScope prof(rg::FAM_CONV_DGRAD, stream, c.s.flops, alg_bytes(g));
            return halo_launch<true>(ph, g.K, g.H, g.W, hpl, ws.ptr, stream, "rg_conv2d_dgrad(3x3 tap reuse)");
        };
        // the tap-reuse kernel and the generic kernels compete per geometry, as in the forward pass — with fused row sums only
        // when the generic plan writes the same row-sum columns (their count is the caller's contract with the planning query:
        // both unsplit on 128-pixel tiles with two wave columns -> the same column per (n-tile, wave column))
        bool can_tune = tune_enabled();
        if (can_tune && o.ep.rowsum) {
            int gcols = -1;
            can_tune = dgrad_impl(g, DgradOps(), Workspace(), nullptr, &gcols, false) == RG_OK && gcols == cols;
        }
        if (!can_tune) return launch_halo();
        return choose_status(tune_key(32, g, 0, 0, 0, ep_bits(o.ep, true)), stream, 2,
                             [&](int i) { return i ? dgrad_impl(g, o, ws, stream, nullptr, false) : launch_halo(); });
    }
    const Plan pl = c.one_class ? plan_gemm(p.M, c.s.ng_max, c.s.kg_max, true) : plan_gemm(p.M, c.s.ng_eff > 0 ? c.s.ng_eff : c.s.ng_max, strided_kg(c.s), c.s.ssplit);
    // measured plan choice (plan_candidates): with fused row sums only plans that write the column count the caller sized
    // (rg_conv2d_dgrad_rowsum_cols reports the model's plan) qualify
    Plan cands[kMaxCand];
    int nc = 1;
    cands[0] = pl;
    if (!dry && (c.one_class || c.s.ng_eff > 0)) {
        Plan all[kMaxCand];
        const int na = c.one_class ? plan_candidates(p.M, c.s.ng_max, c.s.kg_max, all, kMaxCand)
                                   : plan_candidates(p.M, c.s.ng_eff, strided_kg(c.s), all, kMaxCand);
        // (strided classes: the partial columns of all classes lie side by side, ng_total columns per split)
        const size_t ws_all = plans_workspace(all, na, p.M, c.one_class ? c.s.ng_max : c.s.ng_total);
        if (na > 1 && all[0].tile == pl.tile && all[0].splits == pl.splits && ws.ptr && ws_all <= ws.bytes && ws_all < (1ull << 31)) {
            const int want = rowsum_cols_of(c, pl);
            for (int i = 1; i < na; ++i)
                if ((c.one_class || c.s.ssplit || all[i].splits == 1) && (!o.ep.rowsum || rowsum_cols_of(c, all[i]) == want))
                    cands[nc++] = all[i];
        }
    }
    const TuneKey pk = tune_key(128, g, c.mode, nc, o.ep.rowsum ? o.ep.rowsum_cols : 0, ep_bits(o.ep, true));
    return choose_status(pk, stream, nc, [&](int i) { return dgrad_run_plan(c, cands[i]); });
}

}  // namespace

extern "C" size_t rg_conv2d_dgrad_workspace(int N, int C, int H, int W, int K, int KH, int KW, int SH, int SW) {
    ConvGeom g = {N, C, H, W, K, KH, KW, SH, SW, 0, 0, 0, 0};
    const int64_t Ng = (int64_t)N * H * W;
    Plan cands[kMaxCand];
    if (SH != 1 || SW != 1) {
        // strided: the classes' partial columns side by side (all N*H*W pixels); the plan depends on the class depths, which do not
        // depend on the padding (the classes' tap counts are a permutation): the classes of padding 0
        if (SH > 2 || SW > 2) return 0;
        DgradClass cls[4];
        const DgradShape s = dgrad_classes(g, cls);
        if (!s.ssplit || C <= 4) return 0;
        const int nc = plan_candidates(C, s.ng_eff, strided_kg(s), cands, kMaxCand);
        int smax = 1;
        for (int i = 0; i < nc; ++i) smax = cands[i].splits > smax ? cands[i].splits : smax;
        // one split more than planned: a padding whose classes order differently may plan one more
        const size_t need = smax > 1 ? splitk_bytes(smax + 1, C, Ng) : 0;
        if (need < (1ull << 31)) return need;
        return cands[0].splits > 1 ? splitk_bytes(cands[0].splits + 1, C, Ng) : 0;
    }
    const int nc = plan_candidates(C, Ng, (int64_t)K * KH * KW, cands, kMaxCand);
    size_t need = plans_workspace(cands, nc, C, Ng);
    if (need >= (1ull << 31)) need = splitk_bytes(cands[0].splits, C, Ng);
    g.PH = g.PW = 1; g.P = H; g.Q = W;          // the one padding the tap-reuse kernel takes
    if (dgrad_halo_geom(g)) {
        const size_t hn = splitk_bytes(halo_plan(C, Ng, K, nullptr).splits, C, Ng);
        if (hn > need) need = hn;
    }
    return need;
}

// w_krsc: the weights re-laid out as [K][KH*KW][C] by rg_weights_to_krsc (may be NULL; for 1x1 filters the
// original tensor already has that layout and is used directly).
extern "C" int rg_conv2d_dgrad(const float* dy, const float* w, const float* w_krsc, float* dx, int N, int C, int H,
                               int W, int K, int KH, int KW, int SH, int SW, int PH, int PW, int P, int Q,
                               const float* scale, const float* shift, const float* residual, int act, float slope,
                               const float* relu_mask, float* rowsum, int rowsum_cols, void* workspace,
                               size_t workspace_bytes, hipStream_t stream) {
    const ConvGeom g = {N, C, H, W, K, KH, KW, SH, SW, PH, PW, P, Q};
    const DgradOps o = {dy, w, w_krsc, dx, Epilogue{scale, shift, residual, act, slope, relu_mask, rowsum, rowsum_cols}};
    return dgrad_impl(g, o, Workspace{workspace, workspace_bytes}, stream, nullptr);
}

// Number of row-sum column blocks rg_conv2d_dgrad writes for this geometry when given the workspace of
// rg_conv2d_dgrad_workspace (0: the launch uses split-K or the small-C kernel, which do not produce row sums).
extern "C" int rg_conv2d_dgrad_rowsum_cols(int N, int C, int H, int W, int K, int KH, int KW, int SH, int SW, int PH, int PW,
                                           int P, int Q) {
    const ConvGeom g = {N, C, H, W, K, KH, KW, SH, SW, PH, PW, P, Q};
    int cols = 0;
    if (dgrad_impl(g, DgradOps(), Workspace(), nullptr, &cols) != RG_OK) return 0;
    return cols;
}
