// Weight gradient: dw[K, C*KH*KW] = dy[K, N*P*Q] x im2col(x)^T, split over N*P*Q (overview and arithmetic: conv_igemm.hip; plans and
// measured choices: conv_plan.h).  Kernels: the generic implicit GEMM (conv_wgrad_kernel, conv_wgrad_pl_kernel), the thin-layer
// kernels, the split-K reductions and the filter re-layout; entry points rg_conv2d_wgrad, rg_conv2d_wgrad_fold,
// rg_conv2d_wgrad_workspace, rg_weights_to_krsc, rg_weights_to_krsc_multi.
#define RG_PLANES_WGRAD
#include "conv_thin.h"
#include "conv_reduce.h"

namespace {

// grid (C, slices): block (c, s) reduces pixels [s*per_slice, (s+1)*per_slice) for the KH*KW taps of channel c and the KO
// output channels; partial layout [slice][KO][C][KH*KW]
template <int KH, int KW, int KO>
__global__ __launch_bounds__(256) void conv_wgrad_k1_kernel(const ThinP t) {
    constexpr int RS = KH * KW;
    __shared__ float red[4][KO * RS];
    const int Ng = t.N * t.P * t.Q;
    const int PQ = t.P * t.Q;
    const int c = blockIdx.x;
    const int beg = blockIdx.y * t.per_slice;
    const int end = min(beg + t.per_slice, Ng);
    const rsrc_t rx = make_rsrc(t.x, t.x_bytes);
    float acc[KO][KH][KW];
#pragma unroll
    for (int k = 0; k < KO; ++k)
#pragma unroll
        for (int r = 0; r < KH; ++r)
#pragma unroll
            for (int s = 0; s < KW; ++s) acc[k][r][s] = 0.f;
    for (int pix = beg + threadIdx.x; pix < end; pix += 256) {
        const int img = fdiv(pix, t.d_pq);
        const int pq = pix - img * PQ;
        const int pp = fdiv(pq, t.d_q), qq = pq - pp * t.Q;
        const int h0 = pp * t.SH - t.PH, w0 = qq * t.SW - t.PW;
        float g[KO];
#pragma unroll
        for (int k = 0; k < KO; ++k) g[k] = t.a[(img * KO + k) * PQ + pq];
        const int base = (img * t.C + c) * t.H;
#pragma unroll
        for (int r = 0; r < KH; ++r)
#pragma unroll
            for (int s = 0; s < KW; ++s) {
                const int h = h0 + r, w = w0 + s;
                const bool ok = (unsigned)h < (unsigned)t.H && (unsigned)w < (unsigned)t.W;
                const float xv = bload(rx, ok ? (unsigned)((base + h) * t.W + w) * 4u : OOB);
#pragma unroll
                for (int k = 0; k < KO; ++k) acc[k][r][s] += g[k] * xv;
            }
    }
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < KO; ++k)
#pragma unroll
        for (int r = 0; r < KH; ++r)
#pragma unroll
            for (int s = 0; s < KW; ++s) {
                const float v = rg_wave_sum(acc[k][r][s]);
                if (lane == 0) red[wid][(k * KH + r) * KW + s] = v;
            }
    __syncthreads();
    if (threadIdx.x < KO * RS) {
        const int k = threadIdx.x / RS, tap = threadIdx.x - k * RS;
        t.partial[(((int64_t)blockIdx.y * KO + k) * t.C + c) * RS + tap] =
            (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
    }
}

// Weight gradient of 3x3 / stride 1 / pad <= 1 layers with Q % 4 == 0 (the Output blocks: 64 -> 3 on a full-resolution map): four
// output pixels of a row per thread.  Their six input columns per filter row are one 16-byte load plus the two neighbours — 9 load
// instructions for four pixels instead of 36 (206 -> 164 us at 128 x 64 x 128 x 64; the same idea made the forward kernel slower).
__device__ __forceinline__ void thin_px4_offsets(const ThinP& t, int pix, unsigned (&ol)[3], unsigned (&om)[3], unsigned (&orr)[3],
                                                 int& img, int& pq) {
    const int PQ = t.P * t.Q;
    img = fdiv(pix, t.d_pq);
    pq = pix - img * PQ;
    const int pp = fdiv(pq, t.d_q), qq = pq - pp * t.Q;
    const int h0 = pp - t.PH, w0 = qq - t.PW;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const int h = h0 + r;
        const bool hok = (unsigned)h < (unsigned)t.H;
        const unsigned row = (unsigned)((img * t.C * t.H + h) * t.W) * 4u;      // channel 0; + c * H * W * 4 per channel
        ol[r] = (hok && w0 >= 0) ? row + (unsigned)w0 * 4u : OOB;
        om[r] = hok ? row + (unsigned)(w0 + 1) * 4u : OOB;                     // columns w0 + 1 .. w0 + 4: inside the row (host check)
        orr[r] = (hok && w0 + 5 < t.W) ? row + (unsigned)(w0 + 5) * 4u : OOB;
    }
}

template <int KO>
__global__ __launch_bounds__(256) void conv_wgrad_k1_px4_kernel(const ThinP t) {
    __shared__ float red[4][KO * 9];
    const int Ng = t.N * t.P * t.Q;
    const int PQ = t.P * t.Q;
    const int c = blockIdx.x;
    const int beg = blockIdx.y * t.per_slice;                      // per_slice % 4 == 0 (host)
    const int end = min(beg + t.per_slice, Ng);
    const rsrc_t rx = make_rsrc(t.x, t.x_bytes);
    const unsigned co = (unsigned)c * (unsigned)(t.H * t.W) * 4u;
    float acc[KO][3][3];
#pragma unroll
    for (int k = 0; k < KO; ++k)
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int s = 0; s < 3; ++s) acc[k][r][s] = 0.f;
    for (int pix = beg + threadIdx.x * 4; pix < end; pix += 1024) {
        unsigned ol[3], om[3], orr[3];
        int img, pq;
        thin_px4_offsets(t, pix, ol, om, orr, img, pq);
        float g[KO][4];
#pragma unroll
        for (int k = 0; k < KO; ++k) {
            const float4 gv = *reinterpret_cast<const float4*>(t.a + (int64_t)(img * KO + k) * PQ + pq);
            g[k][0] = gv.x; g[k][1] = gv.y; g[k][2] = gv.z; g[k][3] = gv.w;
        }
        float v[3][6];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            v[r][0] = bload(rx, ol[r] + co);
            const float4 m = bload4(rx, om[r] + co);
            v[r][1] = m.x; v[r][2] = m.y; v[r][3] = m.z; v[r][4] = m.w;
            v[r][5] = bload(rx, orr[r] + co);
        }
#pragma unroll
        for (int k = 0; k < KO; ++k)
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int s = 0; s < 3; ++s)
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc[k][r][s] += g[k][j] * v[r][j + s];
    }
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < KO; ++k)
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int s = 0; s < 3; ++s) {
                const float v = rg_wave_sum(acc[k][r][s]);
                if (lane == 0) red[wid][(k * 3 + r) * 3 + s] = v;
            }
    __syncthreads();
    if (threadIdx.x < KO * 9) {
        const int k = threadIdx.x / 9, tap = threadIdx.x - k * 9;
        t.partial[(((int64_t)blockIdx.y * KO + k) * t.C + c) * 9 + tap] =
            (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
    }
}

// w[K][C][RS] -> wt[K][RS][C]
__global__ void weights_to_krsc_kernel(const float* __restrict__ w, float* __restrict__ wt, int64_t total, int C, int RS) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % C);
        const int64_t t = i / C;
        const int rs = (int)(t % RS);
        const int64_t k = t / RS;
        wt[i] = w[(k * C + c) * RS + rs];
    }
}

// The re-layout of EVERY filter of a network in one launch (the per-filter launches were 57 per step of the joint trainer, 5 us
// each, after every optimizer step).  Table in device memory, 6 int64 words per filter: w, wt, K, C, RS, first block; KRSC_CHUNK
// elements per workgroup.
constexpr int KRSC_CHUNK = 2048;
__global__ __launch_bounds__(256) void weights_to_krsc_multi_kernel(const long long* __restrict__ tab, int count) {
    int lo = 0, hi = count - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (tab[(int64_t)mid * 6 + 5] <= (long long)blockIdx.x) lo = mid; else hi = mid - 1;
    }
    const long long* e = tab + (int64_t)lo * 6;
    const float* w = reinterpret_cast<const float*>(e[0]);
    float* wt = reinterpret_cast<float*>(e[1]);
    const int C = (int)e[3], RS = (int)e[4];
    const int64_t total = e[2] * C * RS;
    const int64_t beg = ((long long)blockIdx.x - e[5]) * KRSC_CHUNK;
    for (int64_t i = beg + threadIdx.x; i < beg + KRSC_CHUNK && i < total; i += 256) {
        const int c = (int)(i % C);
        const int64_t t = i / C;
        const int rs = (int)(t % RS);
        const int64_t k = t / RS;
        wt[i] = w[(k * C + c) * RS + rs];
    }
}

// ---------------------------------------------------------------------------------------------
// weight gradient: dw[K][C*KH*KW] = dy[K][N*P*Q] x im2col(x)^T; the reduction (output pixels) is split across
// blockIdx.z, partial tiles go to a workspace and a second kernel sums them.  Lanes run along the reduction axis
// (16 consecutive output pixels: coalesced rows of dy and x); each thread owns fixed GEMM rows / columns.
// Column order: (c, r, s) as in the checkpoint layout, or — p.a_vec4 != 0, C % 16 == 0 — (r, s)-major n' = rs*C + c,
// which lets a whole 16..128-column tile share one filter tap (one padding test per k-tile instead of one per
// element); the finishing kernel then writes dw back in [K][C][KH][KW] order.
// ---------------------------------------------------------------------------------------------
// VEC: 1x1 / stride 1 / pad 0 with P*Q % 4 == 0 — both operands are [rows][pixels] with the reduction axis
// contiguous, so each lane loads 4 consecutive pixels of one row (float4) instead of 4 scalar loads.
// VECA: only the dy operand that way (any filter, P*Q % 4 == 0); the im2col operand keeps the scalar gather.
template <int BM, int BN, int WM, int WN, bool VEC, bool VECA>
__global__ __launch_bounds__(NT) void conv_wgrad_kernel(const ConvP p) {
    using T = Tile<BM, BN, WM, WN>;
    __shared__ float As[2][BK][T::LDA];
    __shared__ float Bs[2][BK][T::LDB];

    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int wm = wid / WN, wn = wid % WN;
    // Workgroups of one split read the same slice of dy and x (every tile row shares dy rows, every tile column x columns),
    // workgroups of different splits share nothing: with a multiple of 8 splits, split s lives entirely on XCD s % 8 (block
    // ids are dealt round-robin over the XCDs in x-then-z order), so each slice is pulled into ONE L2 instead of all eight
    // (measured before: 4.8x the algorithmic bytes fetched).  Otherwise: the tile remap inside each split.
    int tile_id, split;
    if ((gridDim.z & 7) == 0) {
        const unsigned lin = blockIdx.z * gridDim.x + blockIdx.x;
        const unsigned xcd = lin & 7, idx = lin >> 3;
        split = (int)(xcd + 8 * (idx / gridDim.x));
        tile_id = (int)(idx % gridDim.x);
    } else {
        split = blockIdx.z;
        tile_id = xcd_remap(blockIdx.x, gridDim.x);
    }
    const int mt = tile_id % p.m_tiles, nt = tile_id / p.m_tiles;
    const int m0 = mt * BM, n0 = nt * BN;
    const rsrc_t rdy = make_rsrc(p.w, p.w_bytes), rx = make_rsrc(p.x, p.x_bytes);

    const int kk = tid & 15, r0 = tid >> 4;  // lanes run along the reduction (pixel) axis
    constexpr int ACNT = BM / 16, BCNT = BN / 16;
    const int PQ = p.P * p.Q, HW = p.H * p.W, RS = p.KH * p.KW;
    const bool rsc = p.a_vec4 != 0;
    // no padding and every window inside the image: no bounds test at all (all 1x1 layers)
    const bool nopad = p.PH == 0 && p.PW == 0 && (p.P - 1) * p.SH + p.KH <= p.H && (p.Q - 1) * p.SW + p.KW <= p.W;
    // (r,s)-major and the whole column tile inside one tap: one bounds test per lane per k-tile
    const bool same_rs = rsc && (fdiv(n0, p.d_c) == fdiv(min(n0 + BN, p.Ng) - 1, p.d_c));

    // per-thread GEMM rows (dy channels) and columns (c, r, s): fixed for the whole reduction
    unsigned aoff[ACNT];          // byte offset of row m inside one image of dy, or OOB
#pragma unroll
    for (int i = 0; i < ACNT; ++i) {
        const int m = m0 + r0 + 16 * i;
        aoff[i] = m < p.M ? (unsigned)m * (unsigned)PQ * 4u : OOB;
    }
    int coff[BCNT], crs[BCNT];    // element offset c*HW + r*W + s, packed (r,s) or -1
#pragma unroll
    for (int i = 0; i < BCNT; ++i) {
        const int n = n0 + r0 + 16 * i;
        if (n < p.Ng) {
            int c, rs;
            if (rsc) {
                rs = fdiv(n, p.d_c);
                c = n - rs * p.C;
            } else {
                c = fdiv(n, p.d_rs);
                rs = n - c * RS;
            }
            const int r = fdiv(rs, p.d_kw);
            const int s = rs - r * p.KW;
            coff[i] = c * HW + r * p.W + s;
            crs[i] = (r << 16) | s;
        } else {
            coff[i] = 0;
            crs[i] = -1;
        }
    }

    float ra[ACNT < 4 ? 4 : ACNT], rb[BCNT < 4 ? 4 : BCNT];
    floatx16 acc[T::TM][T::TN];
    zero_acc<T>(acc);

    // VEC: thread v owns row (v >> 2) + 64*i and the pixel quad (v & 3)*4 of every k-tile
    constexpr int AVN = (BM * 4 + NT - 1) / NT, BVN = (BN * 4 + NT - 1) / NT;
    const int vrow = tid >> 2, vkq = (tid & 3) * 4;
    unsigned avoff[AVN], bvoff[BVN];
#pragma unroll
    for (int i = 0; i < AVN; ++i) {
        const int m = m0 + vrow + 64 * i;
        avoff[i] = (vrow + 64 * i < BM && m < p.M) ? (unsigned)m * (unsigned)PQ * 4u : OOB;
    }
    int vrr[BVN], vss[BVN];               // p.wshift: tap offset (r - PH, s - PW) of the row's column n = (c, r, s)
#pragma unroll
    for (int i = 0; i < BVN; ++i) {
        const int n = n0 + vrow + 64 * i;
        int c = n;
        vrr[i] = vss[i] = 0;
        if (p.wshift) {
            c = fdiv(n, p.d_rs);
            const int rs = n - c * RS;
            const int r = fdiv(rs, p.d_kw);
            vrr[i] = r - p.PH;
            vss[i] = rs - r * p.KW - p.PW;
        }
        bvoff[i] = (vrow + 64 * i < BN && n < p.Ng) ? (unsigned)c * (unsigned)HW * 4u : OOB;
    }

    auto load_tile = [&](int kt) {
        if (VEC || VECA) {
            const int g = kt * BK + vkq;
            const bool gvalid = g < p.Kg;
            const int img = gvalid ? fdiv(g, p.d_pq) : 0;
            const int pq = g - img * PQ;
            const unsigned ab = gvalid ? (unsigned)(img * p.K * PQ + pq) * 4u : OOB;
#pragma unroll
            for (int i = 0; i < AVN; ++i) {
                const float4 t = bload4(rdy, ((ab | avoff[i]) & OOB) ? OOB : ab + avoff[i]);
                ra[4 * i + 0] = t.x; ra[4 * i + 1] = t.y; ra[4 * i + 2] = t.z; ra[4 * i + 3] = t.w;
            }
            if (VEC && p.wshift) {
                // stride-1 filter tap (r, s): the four output pixels (pp, q0 .. q0 + 3) read x at (pp + r - PH, q0 + s - PW ..), four
                // CONSECUTIVE floats (Q % 4 == 0 keeps a quad inside one row).  One column may fall off either end of the row
                // (|s - PW| <= 1): the load is moved one element inwards and the vector shifted, so every address stays inside
                // the row (dword-aligned dwordx4 buffer loads are legal; nothing relies on partial out-of-range returns)
                const int pp = fdiv(pq, p.d_q);
                const int q0 = pq - pp * p.Q;
#pragma unroll
                for (int i = 0; i < BVN; ++i) {
                    const int hh = pp + vrr[i], wb = q0 + vss[i];
                    const bool ok = gvalid && bvoff[i] != OOB && (unsigned)hh < (unsigned)p.H;
                    const bool neg = wb < 0, over = wb + 3 >= p.W;
                    const int e = img * p.C * HW + hh * p.W + wb + (neg ? 1 : 0) - (over ? 1 : 0);
                    const float4 t = bload4(rx, ok ? (unsigned)e * 4u + bvoff[i] : OOB);
                    rb[4 * i + 0] = neg ? 0.f : (over ? t.y : t.x);
                    rb[4 * i + 1] = neg ? t.x : (over ? t.z : t.y);
                    rb[4 * i + 2] = neg ? t.y : (over ? t.w : t.z);
                    rb[4 * i + 3] = neg ? t.z : (over ? 0.f : t.w);
                }
                return;
            }
            if (VEC) {
                const unsigned bb = gvalid ? (unsigned)(img * p.C * HW + pq) * 4u : OOB;
#pragma unroll
                for (int i = 0; i < BVN; ++i) {
                    const float4 t = bload4(rx, ((bb | bvoff[i]) & OOB) ? OOB : bb + bvoff[i]);
                    rb[4 * i + 0] = t.x; rb[4 * i + 1] = t.y; rb[4 * i + 2] = t.z; rb[4 * i + 3] = t.w;
                }
                return;
            }
        }
        const int g = kt * BK + kk;  // global output-pixel index n*P*Q + p*Q + q
        const bool gvalid = g < p.Kg;
        int img = 0, h0 = 0, w0 = 0, pq = 0;
        if (gvalid) {
            img = fdiv(g, p.d_pq);
            pq = g - img * PQ;
            const int pp = fdiv(pq, p.d_q);
            const int qq = pq - pp * p.Q;
            h0 = pp * p.SH - p.PH;
            w0 = qq * p.SW - p.PW;
        }
        if (!VECA) {
            const unsigned abase = gvalid ? (unsigned)(img * p.K * PQ + pq) * 4u : OOB;
#pragma unroll
            for (int i = 0; i < ACNT; ++i) ra[i] = bload(rdy, (abase | aoff[i]) & OOB ? OOB : abase + aoff[i]);
        }
        const int xb = img * p.C * HW + h0 * p.W + w0;      // element index of (img, 0, h0, w0); may sit in the padding
        if (nopad) {
#pragma unroll
            for (int i = 0; i < BCNT; ++i)
                rb[i] = bload(rx, (gvalid && crs[i] >= 0) ? (unsigned)(xb + coff[i]) * 4u : OOB);
        } else if (same_rs) {
            const int r = crs[0] >> 16, s = crs[0] & 0xffff;
            const int h = h0 + r, w = w0 + s;
            const bool ok = gvalid && (unsigned)h < (unsigned)p.H && (unsigned)w < (unsigned)p.W;
#pragma unroll
            for (int i = 0; i < BCNT; ++i) rb[i] = bload(rx, (ok && crs[i] >= 0) ? (unsigned)(xb + coff[i]) * 4u : OOB);
        } else {
#pragma unroll
            for (int i = 0; i < BCNT; ++i) {
                const int r = crs[i] >> 16, s = crs[i] & 0xffff;
                const int h = h0 + r, w = w0 + s;
                const bool ok = gvalid && crs[i] >= 0 && (unsigned)h < (unsigned)p.H && (unsigned)w < (unsigned)p.W;
                rb[i] = bload(rx, ok ? (unsigned)(xb + coff[i]) * 4u : OOB);
            }
        }
    };
    auto store_tile = [&](int buf, int q) {
        if (VEC || VECA) {
#pragma unroll
            for (int i = 0; i < AVN; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (vrow + 64 * i < BM && in_quarter(4 * i + j, 4 * AVN, q)) As[buf][vkq + j][vrow + 64 * i] = ra[4 * i + j];
        }
        if (VEC) {
#pragma unroll
            for (int i = 0; i < BVN; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (vrow + 64 * i < BN && in_quarter(4 * i + j, 4 * BVN, q)) Bs[buf][vkq + j][vrow + 64 * i] = rb[4 * i + j];
            return;
        }
        if (!VECA) {
#pragma unroll
            for (int i = 0; i < ACNT; ++i)
                if (in_quarter(i, ACNT, q)) As[buf][kk][r0 + 16 * i] = ra[i];
        }
#pragma unroll
        for (int i = 0; i < BCNT; ++i)
            if (in_quarter(i, BCNT, q)) Bs[buf][kk][r0 + 16 * i] = rb[i];
    };

    const int nk_total = (p.Kg + BK - 1) / BK;
    const int kt_begin = split * p.ktiles_per_split;
    int kt_end = kt_begin + p.ktiles_per_split;
    if (kt_end > nk_total) kt_end = nk_total;

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

    // partial (or final) tile: [split][M][Ng], columns contiguous
    const int l32 = lane & 31, kh = lane >> 5;
    const rsrc_t ro = make_rsrc(p.y, p.y_bytes);
    const int mrow0 = m0 + wm * T::WTM + 4 * kh;
    const unsigned rstride = (unsigned)p.Ng * 4u;
#pragma unroll
    for (int j = 0; j < T::TN; ++j) {
        const int nn = n0 + wn * T::WTN + j * 32 + l32;
        const unsigned ob = nn < p.Ng ? (unsigned)((((int64_t)split * p.M + mrow0) * p.Ng + nn) * 4) : OOB;
#pragma unroll
        for (int i = 0; i < T::TM; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int mo = i * 32 + (r & 3) + 8 * (r >> 2);
                bstore(ro, (mrow0 + mo < p.M) ? ob + (unsigned)mo * rstride : OOB, acc[i][j][r]);
            }
    }
}

// dw[i] = sum_s ws[s][i]; with rsc != 0 the partial columns are (r,s)-major (n' = rs*C + c) and are written back in
// the checkpoint order [K][C][RS].  Deterministic: the fixed summation tree of conv_reduce.h.
__global__ __launch_bounds__(256) void splitk_reduce_kernel(const float* __restrict__ ws, float* __restrict__ out,
                                                            int64_t n, int splits, int rsc, int C, int RS) {
    int64_t i;
    float s;
    if (!splitk_sum(ws, n, splits, i, s)) return;
    if (!rsc) {
        out[i] = s;
        return;
    }
    const int64_t crs = (int64_t)C * RS;
    const int64_t m = i / crs;
    const int np = (int)(i - m * crs);
    const int rs = np / C, c = np - rs * C;
    out[m * crs + (int64_t)c * RS + rs] = s;
}

// n % 4 == 0: float4 outputs, per element the values of splitk_reduce_kernel
__global__ __launch_bounds__(256) void splitk_reduce_vec_kernel(const float* __restrict__ ws, float* __restrict__ out, int64_t n,
                                                                int splits, int rsc, int C, int RS) {
    int64_t i;
    float4 v;
    if (!splitk_sum4(ws, n, splits, i, v)) return;
    if (!rsc) {
        reinterpret_cast<float4*>(out)[i] = v;
        return;
    }
    const int64_t crs = (int64_t)C * RS;
    const float vv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int64_t e = i * 4 + j;
        const int64_t m = e / crs;
        const int np = (int)(e - m * crs);
        const int rs = np / C, c = np - rs * C;
        out[m * crs + (int64_t)c * RS + rs] = vv[j];
    }
}

// Split-K reduction of the weight gradient of a convolution whose frozen-statistics BatchNorm is folded into it (norm_fold.hip, "conv +
// frozen-statistics BatchNorm"): ONE workgroup per filter row k sums the slabs of its row (float4 columns, the summation tree of
// splitk_reduce_vec_kernel, conv_reduce.h, written out here inside the row loop: same G bit for bit), and finishes the fold while G
// is in registers — dgamma[k] = invstd (sum_m W G - mean sum g), dbeta[k] = sum g (from the slice partials), dW = scale[k] G.  Replaces splitk_reduce_vec_kernel + bn_fold_wgrad_kernel:
// one launch, one write and one read of G less per folded layer (106 layers per FD-GAN step).  M % 4 == 0, 16-byte aligned buffers.
__global__ __launch_bounds__(256) void splitk_reduce_fold_kernel(const float* __restrict__ ws, float* __restrict__ out,
                                                                 const float* __restrict__ w, int M, int64_t n, int splits,
                                                                 const float* __restrict__ scale, const float* __restrict__ invstd,
                                                                 const float* __restrict__ mean, const float* __restrict__ sum_g,
                                                                 const float* __restrict__ part, int S, float* __restrict__ dbeta,
                                                                 float* __restrict__ dgamma) {
    __shared__ float4 red[4][64];
    __shared__ float redf[16];
    const int k = blockIdx.x;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int M4 = M >> 2;
    const int64_t n4 = n >> 2;
    const float4* w4 = reinterpret_cast<const float4*>(ws);
    const float4* f4 = reinterpret_cast<const float4*>(w);
    float4* o4 = reinterpret_cast<float4*>(out);
    const float sc = scale[k];
    float dot = 0.f;
    for (int c0 = 0; c0 < M4; c0 += 64) {
        const int c = c0 + tx;
        const int64_t i = (int64_t)k * M4 + c;
        float4 s0 = make_float4(0.f, 0.f, 0.f, 0.f), s1 = s0;
        if (c < M4) {
            int q = ty;
            for (; q + 12 < splits; q += 16) {
                const float4 a = w4[(int64_t)q * n4 + i], b = w4[(int64_t)(q + 4) * n4 + i];
                const float4 cc = w4[(int64_t)(q + 8) * n4 + i], d = w4[(int64_t)(q + 12) * n4 + i];
                s0.x += a.x; s0.y += a.y; s0.z += a.z; s0.w += a.w;
                s1.x += b.x; s1.y += b.y; s1.z += b.z; s1.w += b.w;
                s0.x += cc.x; s0.y += cc.y; s0.z += cc.z; s0.w += cc.w;
                s1.x += d.x; s1.y += d.y; s1.z += d.z; s1.w += d.w;
            }
            for (; q + 4 < splits; q += 8) {
                const float4 a = w4[(int64_t)q * n4 + i], b = w4[(int64_t)(q + 4) * n4 + i];
                s0.x += a.x; s0.y += a.y; s0.z += a.z; s0.w += a.w;
                s1.x += b.x; s1.y += b.y; s1.z += b.z; s1.w += b.w;
            }
            if (q < splits) {
                const float4 a = w4[(int64_t)q * n4 + i];
                s0.x += a.x; s0.y += a.y; s0.z += a.z; s0.w += a.w;
            }
        }
        red[ty][tx] = make_float4(s0.x + s1.x, s0.y + s1.y, s0.z + s1.z, s0.w + s1.w);
        __syncthreads();
        if (ty == 0 && c < M4) {
            const float4 r0 = red[0][tx], r1 = red[1][tx], r2 = red[2][tx], r3 = red[3][tx];
            const float4 v = make_float4((r0.x + r1.x) + (r2.x + r3.x), (r0.y + r1.y) + (r2.y + r3.y), (r0.z + r1.z) + (r2.z + r3.z),
                                         (r0.w + r1.w) + (r2.w + r3.w));
            if (dgamma) {
                const float4 wv = f4[i];
                dot += (wv.x * v.x + wv.y * v.y) + (wv.z * v.z + wv.w * v.w);
            }
            o4[i] = make_float4(v.x * sc, v.y * sc, v.z * sc, v.w * sc);
        }
        __syncthreads();
    }
    float sg = 0.f;
    if (part) {                       // channel sum of g from slice / tile partials (the tree of bn_fold_wgrad_kernel)
        float t = 0.f;
        for (int s = threadIdx.x; s < S; s += 256) t += part[(int64_t)k * S + s];
        sg = rg_block_sum(t, redf);
        if (dbeta && threadIdx.x == 0) dbeta[k] = sg;
    } else if (sum_g) {
        sg = sum_g[k];
    }
    if (dgamma) {
        const float t = rg_block_sum(dot, redf);
        if (threadIdx.x == 0) dgamma[k] = invstd[k] * (t - mean[k] * sg);
    }
}

#include "conv_planes.h"

}  // namespace

using namespace rg::conv;

extern "C" int rg_weights_to_krsc(const float* w, float* w_krsc, int K, int C, int KH, int KW, hipStream_t stream) {
    RG_REQUIRE(w && w_krsc && K > 0 && C > 0 && KH > 0 && KW > 0, "rg_weights_to_krsc: bad arguments");
    const int64_t total = (int64_t)K * C * KH * KW;
    rg::ProfScope prof(rg::FAM_MISC, stream, 0.0, 8.0 * total);
    hipLaunchKernelGGL(weights_to_krsc_kernel, dim3(finish_grid(total)), dim3(256), 0, stream, w, w_krsc, total, C,
                       KH * KW);
    return rg::check_launch("rg_weights_to_krsc");
}

extern "C" int rg_krsc_chunk(void) { return KRSC_CHUNK; }

// table: device memory, `count` entries of 6 int64 words {w, w_krsc, K, C, KH*KW, first block}; blocks of rg_krsc_chunk() elements
extern "C" int rg_weights_to_krsc_multi(const void* table, int count, int total_blocks, hipStream_t stream) {
    RG_REQUIRE(table && count > 0 && total_blocks > 0, "rg_weights_to_krsc_multi: bad arguments");
    rg::ProfScope prof(rg::FAM_CONV_FWD, stream, 0.0, 8.0 * (double)total_blocks * KRSC_CHUNK);
    hipLaunchKernelGGL(weights_to_krsc_multi_kernel, dim3(total_blocks), dim3(256), 0, stream, static_cast<const long long*>(table),
                       count);
    return rg::check_launch("rg_weights_to_krsc_multi");
}

extern "C" int rg_bn_fold_wgrad(const float* w, float* g, const float* scale, const float* invstd, const float* running_mean,
                                const float* sum_g, const float* partials, int n_slices, float* dbeta, float* dgamma, int K,
                                int M, hipStream_t stream);        // norm_fold.hip

// VEC / VECA of the loader (conv_wgrad_kernel) from vec / veca; the plane kernels (conv_planes.h) have 4 or 8 waves
#define RG_WGRAD_LAUNCH_K(KERNEL, NTH, BM_, BN_, WM_, WN_)                                                          \
    if (vec) hipLaunchKernelGGL((KERNEL<BM_, BN_, WM_, WN_, true, true>), grid, dim3(NTH), 0, stream, p);           \
    else if (veca) hipLaunchKernelGGL((KERNEL<BM_, BN_, WM_, WN_, false, true>), grid, dim3(NTH), 0, stream, p);    \
    else hipLaunchKernelGGL((KERNEL<BM_, BN_, WM_, WN_, false, false>), grid, dim3(NTH), 0, stream, p)
#define RG_WGRAD_LAUNCH(BM_, BN_, WM_, WN_) RG_WGRAD_LAUNCH_K(conv_wgrad_kernel, NT, BM_, BN_, WM_, WN_)
#define RG_WGRAD_PL_LAUNCH(BM_, BN_, WM_, WN_) RG_WGRAD_LAUNCH_K(conv_wgrad_pl_kernel, 64 * WM_ * WN_, BM_, BN_, WM_, WN_)
// the weight-gradient plans use three of the four tiles (plan_wgrad)
#define RG_WGRAD_TILE_SWITCH(tile, LAUNCH)     \
    switch (tile) {                            \
        case 0: LAUNCH(128, 128, 2, 2); break; \
        case 2: LAUNCH(64, 64, 2, 2); break;   \
        default: LAUNCH(32, 256, 1, 4); break; \
    }

namespace {

// thin layers, four pixels per thread (conv_wgrad_k1_px4_kernel): 3x3 / stride 1 / pad <= 1 rows of float4 multiples
static bool thin_px4(const ConvGeom& g, const float* dy) {
    return g.KH == 3 && g.KW == 3 && g.SH == 1 && g.SW == 1 && g.PH <= 1 && g.PW <= 1 && (g.Q & 3) == 0 &&
           g.Q + 2 - 2 * g.PW == g.W && aligned16(dy) && ((g.P * g.Q) & 3) == 0;
}
#define THIN_PX4_DISPATCH(KERNEL, g, grid, stream, t)                                                 \
    do {                                                                                              \
        if (g.K == 1) hipLaunchKernelGGL((KERNEL<1>), grid, dim3(256), 0, stream, t);                 \
        else if (g.K == 2) hipLaunchKernelGGL((KERNEL<2>), grid, dim3(256), 0, stream, t);            \
        else if (g.K == 3) hipLaunchKernelGGL((KERNEL<3>), grid, dim3(256), 0, stream, t);            \
        else hipLaunchKernelGGL((KERNEL<4>), grid, dim3(256), 0, stream, t);                          \
    } while (0)
// thin layers: pixels per slice so that ~2048 workgroups exist (>= 512 pixels each)
static int thin_wgrad_per_slice(int C, int64_t Ng) {
    int64_t slices = rg::cdiv64(2048, C);
    if (slices > Ng / 512) slices = Ng / 512;
    if (slices < 1) slices = 1;
    return (int)((rg::cdiv64(Ng, slices) + 3) / 4 * 4);      // a multiple of four pixels (conv_wgrad_k1_px4_kernel)
}

// RG_WGRAD_RSC=1 (README "Environment switches", read once per process): (r,s)-major columns where the geometry allows
static bool wgrad_rsc_enabled() {
    static const bool on = rg::env_int("RG_WGRAD_RSC", 0) != 0;
    return on;
}

static void launch_reduce(hipStream_t stream, const float* ws, float* out, int64_t n, int splits, int rsc, int C, int RS) {
    if (aligned16(ws, out) && (n & 3) == 0)
        hipLaunchKernelGGL(splitk_reduce_vec_kernel, dim3((unsigned)rg::cdiv64(n >> 2, 64)), dim3(256), 0, stream, ws, out, n, splits, rsc,
                           C, RS);
    else
        hipLaunchKernelGGL(splitk_reduce_kernel, dim3((unsigned)rg::cdiv64(n, 64)), dim3(256), 0, stream, ws, out, n, splits, rsc, C, RS);
}

struct FoldArgs {                 // folded frozen-statistics BatchNorm behind the convolution (rg_conv2d_wgrad_fold)
    const float *w, *scale, *invstd, *mean, *sum_g, *partials;
    int n_slices;
    float *dbeta, *dgamma;
};
static int fold_after(const FoldArgs* f, float* dw, int K, int M, hipStream_t stream) {
    return rg_bn_fold_wgrad(f->w, dw, f->scale, f->invstd, f->mean, f->sum_g, f->partials, f->n_slices, f->dbeta, f->dgamma, K, M,
                            stream);
}

struct WgradOps {
    const float *x, *dy;
    float* dw;
    const FoldArgs* fold;         // or nullptr
};

struct WgradCall {
    const ConvGeom& g;
    const WgradOps& o;
    Workspace ws;
    hipStream_t stream;
    ConvP p;                      // geometry, operands, GEMM sizes: what the plan does not decide
};

static int wgrad_thin(const WgradCall& c, int per, int slices) {
    const ConvGeom& g = c.g;
    const FoldArgs* fold = c.o.fold;
    ThinP t;
    thin_fill(t, c.o.x, c.o.dy, static_cast<float*>(c.ws.ptr), g, per);
    rg::ProfScope prof(rg::FAM_CONV_WGRAD, c.stream, 2.0 * (double)g.K * c.p.Ng * c.p.Kg, alg_bytes(g));
    const dim3 grid(g.C, slices);
    if (thin_px4(g, c.o.dy)) THIN_PX4_DISPATCH(conv_wgrad_k1_px4_kernel, g, grid, c.stream, t);
    else THIN_DISPATCH(conv_wgrad_k1_kernel, g, grid, c.stream, t);
    if (int e = rg::check_launch("rg_conv2d_wgrad(thin)")) return e;
    launch_reduce(c.stream, static_cast<const float*>(c.ws.ptr), c.o.dw, (int64_t)g.K * c.p.Ng, slices, 0, g.C, g.KH * g.KW);
    if (int e = rg::check_launch("rg_conv2d_wgrad(thin reduce)")) return e;
    return fold ? fold_after(fold, c.o.dw, g.K, c.p.Ng, c.stream) : RG_OK;
}

// one generic launch of plan pl: kernel + split-K reduction (+ folded-BatchNorm finish)
static int wgrad_run_plan(const WgradCall& c, const Plan& pl) {
    const ConvGeom& g = c.g;
    const FoldArgs* fold = c.o.fold;
    hipStream_t stream = c.stream;
    float* dw = c.o.dw;
    ConvP p = c.p;
    p.m_tiles = pl.m_tiles; p.n_tiles = pl.n_tiles;
    p.splits = pl.splits; p.ktiles_per_split = pl.ktiles_per_split;
    const size_t need = (size_t)pl.splits * p.M * (size_t)p.Ng * sizeof(float);      // see rg_conv2d_wgrad_workspace
    if (need > c.ws.bytes || !c.ws.ptr) {
        rg::set_error("rg_conv2d_wgrad: workspace too small (%zu < %zu)", c.ws.bytes, need);
        return RG_ERR_WORKSPACE;
    }
    RG_REQUIRE(need < (1ull << 31), "rg_conv2d_wgrad: partial buffer exceeds 2 GiB");
    // (r,s)-major columns (RG_WGRAD_RSC=1): always through the workspace (the finishing kernel restores the checkpoint order)
    const bool rsc = wgrad_rsc_enabled() && (g.KH * g.KW > 1) && (g.C % 16 == 0);
    const bool via_ws = pl.splits > 1 || rsc;
    float* const partial = static_cast<float*>(c.ws.ptr);
    p.a_vec4 = rsc ? 1 : 0;
    p.y = via_ws ? partial : dw;
    p.x_bytes = x_bytes(g);
    p.w_bytes = y_bytes(g);
    p.y_bytes = via_ws ? (unsigned)need : w_bytes(g);
    const dim3 grid(p.m_tiles * p.n_tiles, 1, pl.splits);
    {
        rg::ProfScope prof(rg::FAM_CONV_WGRAD, stream, 2.0 * p.M * (double)p.Ng * p.Kg, alg_bytes(g));
        const bool veca = aligned16(c.o.x, c.o.dy) && ((g.P * g.Q) % 4 == 0);
        bool vec = veca && g.KH == 1 && g.KW == 1 && g.SH == 1 && g.SW == 1 && g.PH == 0 && g.PW == 0;
        if (!vec && !rsc && veca && g.SH == 1 && g.SW == 1 && g.PW <= 1 && g.KW <= g.PW + 2 && g.Q % 4 == 0 &&
            g.W >= 4 && g.KW * g.KH > 1) {
            vec = true;                  // im2col operand = shifted float4 loads of x (conv_wgrad_kernel, p.wshift)
            p.wshift = 1;
        }
        const TuneKey tk = tune_key(4, g, (vec ? 2 : 0) + (veca ? 1 : 0) + p.wshift * 4, pl.tile, pl.splits, 0);
        choose_impl(4, tk, stream, pl.tile == 0 ? 3 : 2, [&](int impl) {
            if (impl == 2) { RG_WGRAD_PL_LAUNCH(128, 128, 4, 2); }
            else if (impl) { RG_WGRAD_TILE_SWITCH(pl.tile, RG_WGRAD_PL_LAUNCH); }
            else { RG_WGRAD_TILE_SWITCH(pl.tile, RG_WGRAD_LAUNCH); }
        });
        if (int e = rg::check_launch("rg_conv2d_wgrad")) return e;
        if (via_ws) {
            const int64_t n = (int64_t)p.M * p.Ng;
            if (fold && !rsc && (p.Ng & 3) == 0 && aligned16(partial, dw, fold->w)) {
                // reduction + BatchNorm-fold finish in one launch (one workgroup per filter)
                hipLaunchKernelGGL(splitk_reduce_fold_kernel, dim3(p.M), dim3(256), 0, stream, partial, dw, fold->w, p.Ng, n, pl.splits,
                                   fold->scale, fold->invstd, fold->mean, fold->sum_g, fold->partials, fold->n_slices, fold->dbeta,
                                   fold->dgamma);
                return rg::check_launch("rg_conv2d_wgrad(reduce + fold)");
            }
            launch_reduce(stream, partial, dw, n, pl.splits, rsc ? 1 : 0, g.C, g.KH * g.KW);
        }
    }
    if (int e = rg::check_launch("rg_conv2d_wgrad(reduce)")) return e;
    return fold ? fold_after(fold, dw, g.K, g.C * g.KH * g.KW, stream) : RG_OK;
}

int wgrad_impl(const ConvGeom& g, const WgradOps& o, const Workspace& ws, hipStream_t stream) {
    if (int e = validate("rg_conv2d_wgrad", g)) return e;
    RG_REQUIRE(o.x && o.dy && o.dw, "rg_conv2d_wgrad: null tensor");
    RG_REQUIRE(g.KH < 65536 && g.KW < 65536, "rg_conv2d_wgrad: filter too large");
    WgradCall c = {g, o, ws, stream};
    ConvP& p = c.p;
    fill_common(p, g);
    p.x = o.x; p.w = o.dy;
    p.ep = Epilogue{nullptr, nullptr, nullptr, 0, 0.f, nullptr, nullptr, 0};
    p.M = g.K; p.Ng = g.C * g.KH * g.KW; p.Kg = g.N * g.P * g.Q;
    if (thin_filter(g)) {
        const int per = thin_wgrad_per_slice(g.C, p.Kg);
        const int slices = rg::cdiv(p.Kg, per);
        if (ws.ptr && (size_t)slices * (size_t)g.K * (size_t)p.Ng * sizeof(float) <= ws.bytes) return wgrad_thin(c, per, slices);
    }
    Plan cands[8];
    int nc = wgrad_plan_candidates(p.M, p.Ng, p.Kg, cands, 8);
    for (int i = 1; i < nc; ++i)                 // a caller with the model plan's scratch only: the model's plan only
        if (!ws.ptr || (size_t)cands[i].splits * p.M * (size_t)p.Ng * sizeof(float) > ws.bytes) nc = 1;
    const TuneKey pk = tune_key(256, g, o.fold ? 1 : 0, nc, cands[0].splits, 0);
    return choose_status(pk, stream, nc, [&](int i) { return wgrad_run_plan(c, cands[i]); });
}

}  // namespace

extern "C" size_t rg_conv2d_wgrad_workspace(int N, int C, int K, int KH, int KW, int P, int Q) {
    const ConvGeom g = {N, C, 0, 0, K, KH, KW, 0, 0, 0, 0, P, Q};       // what a weight-gradient plan depends on
    const int64_t Ng = (int64_t)N * P * Q;
    if (thin_filter(g)) return (size_t)rg::cdiv64(Ng, thin_wgrad_per_slice(C, Ng)) * (size_t)K * (size_t)C * KH * KW * sizeof(float);
    Plan cands[8];
    const int nc = wgrad_plan_candidates(K, C * KH * KW, Ng, cands, 8);
    int smax = 0;
    for (int i = 0; i < nc; ++i) smax = cands[i].splits > smax ? cands[i].splits : smax;
    return (size_t)smax * (size_t)K * (size_t)C * KH * KW * sizeof(float);
}

extern "C" int rg_conv2d_wgrad(const float* x, const float* dy, float* dw, int N, int C, int H, int W, int K, int KH,
                               int KW, int SH, int SW, int PH, int PW, int P, int Q, void* workspace,
                               size_t workspace_bytes, hipStream_t stream) {
    const ConvGeom g = {N, C, H, W, K, KH, KW, SH, SW, PH, PW, P, Q};
    return wgrad_impl(g, WgradOps{x, dy, dw, nullptr}, Workspace{workspace, workspace_bytes}, stream);
}

// Weight gradient of a convolution with a folded frozen-statistics BatchNorm behind it, finished in the same call:
// G = wgrad(x, dy); dgamma = invstd (sum_m w G - mean sum_g); dbeta = sum_g (when it comes as slice partials); dw = scale G
// (arguments as rg_bn_fold_wgrad; dgamma / dbeta may be NULL).  With split-K the finish runs inside the reduction launch.
extern "C" int rg_conv2d_wgrad_fold(const float* x, const float* dy, float* dw, int N, int C, int H, int W, int K, int KH, int KW,
                                    int SH, int SW, int PH, int PW, int P, int Q, const float* w, const float* scale,
                                    const float* invstd, const float* running_mean, const float* sum_g, const float* partials,
                                    int n_slices, float* dbeta, float* dgamma, void* workspace, size_t workspace_bytes,
                                    hipStream_t stream) {
    RG_REQUIRE(w && scale, "rg_conv2d_wgrad_fold: null filters / scale");
    RG_REQUIRE(!dgamma || (invstd && running_mean && (sum_g || partials)), "rg_conv2d_wgrad_fold: dgamma needs invstd, mean and the sums");
    RG_REQUIRE(!partials || n_slices > 0, "rg_conv2d_wgrad_fold: partials need their slice count");
    const ConvGeom g = {N, C, H, W, K, KH, KW, SH, SW, PH, PW, P, Q};
    const FoldArgs f{w, scale, invstd, running_mean, sum_g, partials, n_slices, dbeta, dgamma};
    return wgrad_impl(g, WgradOps{x, dy, dw, &f}, Workspace{workspace, workspace_bytes}, stream);
}
