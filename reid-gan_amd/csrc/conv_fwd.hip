// Forward convolution: y[K, N*P*Q] = w[K, C*KH*KW] x im2col(x) (overview and arithmetic: conv_igemm.hip; plans and measured choices:
// conv_plan.h).  Kernels: the generic implicit GEMM (conv_fwd_kernel, conv_fwd_pl_kernel), the tap-reuse 3x3 kernel (conv_halo.h) and
// the thin-layer kernel (conv_fwd_k1_kernel); entry points rg_conv2d_fwd, rg_conv2d_fwd_workspace.
#define RG_PLANES_FWD
#include "conv_halo.h"
#include "conv_thin.h"

namespace {

// A operand loader shared by fwd (weights [M][Kg], k contiguous): float4 along k (AVEC) or scalar.
template <int BM, bool AVEC>
struct ALoadK {
    static constexpr int NA = AVEC ? ((BM * 4 + NT - 1) / NT) : (BM * BK / NT);
    unsigned off[NA];
    int kq[NA];
    __device__ __forceinline__ void init(int tid, int m0, int M, int Kg) {
#pragma unroll
        for (int i = 0; i < NA; ++i) {
            const int v = tid + NT * i;
            const int row = AVEC ? (v >> 2) : (v >> 4);
            kq[i] = AVEC ? (v & 3) * 4 : (v & 15);
            const bool ok = (AVEC ? v < BM * 4 : v < BM * BK) && (m0 + row < M);
            off[i] = ok ? (unsigned)(((int64_t)(m0 + row) * Kg + kq[i]) * 4) : OOB;
        }
    }
};

// ---------------------------------------------------------------------------------------------
// forward.  BMODE 0: generic gather, reduction order (c, r, s), weights [K][C][KH][KW]
//           BMODE 1: (r, s)-major order k' = rs*C + c, weights [K][KH*KW][C], C % 16 == 0: one bounds test per tile
//           BMODE 2: 1x1 / stride 1 / pad 0 with H*W % 4 == 0: pixel operand as float4
// ---------------------------------------------------------------------------------------------
template <int BM, int BN, int WM, int WN, int BMODE, bool AVEC>
__global__ __launch_bounds__(NT) __attribute__((amdgpu_waves_per_eu(RG_WAVES))) void conv_fwd_kernel(const ConvP p) {
    using T = Tile<BM, BN, WM, WN>;
    static_assert(BN >= 64, "the gather loader needs a wave-uniform k");
    __shared__ __attribute__((aligned(16))) float As[2][BK][T::LDA];
    __shared__ __attribute__((aligned(16))) float Bs[2][BK][T::LDB];

    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int wm = wid / WN, wn = wid % WN;
    const int tile = xcd_remap(blockIdx.x, gridDim.x);
    const int mt = tile % p.m_tiles, nt = tile / p.m_tiles;
    const int m0 = mt * BM, n0 = nt * BN;
    const int split = blockIdx.y;
    const int HW = p.H * p.W;
    const int RS = p.KH * p.KW;
    const rsrc_t rw = make_rsrc(p.w, p.w_bytes), rx = make_rsrc(p.x, p.x_bytes);

    ALoadK<BM, AVEC> al;
    al.init(tid, m0, p.M, p.Kg);

    // ---- B operand set-up ----
    constexpr int BKSTEP = NT / BN > 0 ? NT / BN : 1;
    const int bcol = tid % BN;
    const int bk0 = __builtin_amdgcn_readfirstlane(tid / BN);
    constexpr int BV = BN / 4;
    constexpr int BVSTEP = NT / BV;
    constexpr int BVCNT = (BV * BK + NT - 1) / NT;
    const int vcol = tid % BV, vrow0 = tid / BV;

    bool bvalid;
    int h0 = 0, w0 = 0, pixb = 0;     // pixb: element index of (img, c=0, h0, w0); may be "negative" inside padding
    unsigned bvoff = OOB;             // BMODE 2: byte offset of (img, k = vrow0, pix)
    if (BMODE == 2) {
        const int n = n0 + 4 * vcol;
        bvalid = n < p.Ng && vrow0 < BK;
        if (bvalid) {
            const int img = fdiv(n, p.d_pq);
            bvoff = (unsigned)((((int64_t)img * p.C + vrow0) * HW + (n - img * HW)) * 4);
        }
    } else {
        const int n = n0 + bcol;
        bvalid = n < p.Ng;
        if (bvalid) {
            const int img = fdiv(n, p.d_pq);
            const int pq = n - img * p.P * p.Q;
            const int pp = fdiv(pq, p.d_q);
            const int qq = pq - pp * p.Q;
            h0 = pp * p.SH - p.PH;
            w0 = qq * p.SW - p.PW;
            pixb = img * p.C * HW + h0 * p.W + w0;
        }
    }

    float ra[AVEC ? 4 * ALoadK<BM, AVEC>::NA : ALoadK<BM, AVEC>::NA];
    float rb[BMODE == 2 ? 1 : T::BCNT];
    float4 rbv[BMODE == 2 ? BVCNT : 1];
    floatx16 acc[T::TM][T::TN];
    zero_acc<T>(acc);

    auto load_tile = [&](int kt) {
        const int kbase = kt * BK;
        const unsigned kb4 = (unsigned)kbase * 4u;
        const bool ktail = kbase + BK > p.Kg;                    // uniform; only the last tile of ragged Kg
#pragma unroll
        for (int i = 0; i < ALoadK<BM, AVEC>::NA; ++i) {
            unsigned o = al.off[i] + kb4;
            if (ktail && kbase + al.kq[i] >= p.Kg) o = OOB;
            if (AVEC) {
                const float4 t = bload4(rw, o);
                ra[4 * i + 0] = t.x; ra[4 * i + 1] = t.y; ra[4 * i + 2] = t.z; ra[4 * i + 3] = t.w;
            } else {
                ra[i] = bload(rw, o);
            }
        }
        if (BMODE == 2) {
            const unsigned kstride = (unsigned)HW * 4u;
#pragma unroll
            for (int i = 0; i < BVCNT; ++i) {
                unsigned o = bvoff + (unsigned)(kbase + i * BVSTEP) * kstride;
                if (ktail && kbase + vrow0 + i * BVSTEP >= p.Kg) o = OOB;
                rbv[i] = bload4(rx, o);
            }
        } else if (BMODE == 1) {
            const int rs = fdiv(kbase, p.d_c);                   // scalar: the whole tile shares (r, s)
            const int c0 = kbase - rs * p.C;
            const int r = fdiv(rs, p.d_kw);
            const int s = rs - r * p.KW;
            const int h = h0 + r, w = w0 + s;
            const bool ok = bvalid && (unsigned)h < (unsigned)p.H && (unsigned)w < (unsigned)p.W;
            const unsigned o0 = ok ? (unsigned)(pixb + r * p.W + s + (c0 + bk0) * HW) * 4u : OOB;
            const unsigned cstride = (unsigned)(BKSTEP * HW) * 4u;
#pragma unroll
            for (int i = 0; i < T::BCNT; ++i) rb[i] = bload(rx, o0 + (unsigned)i * cstride);
        } else {
#pragma unroll
            for (int i = 0; i < T::BCNT; ++i) {
                const int k = kbase + bk0 + i * BKSTEP;          // wave-uniform -> scalar unit
                const int c = fdiv(k, p.d_rs);
                const int rs = k - c * RS;
                const int r = fdiv(rs, p.d_kw);
                const int s = rs - r * p.KW;
                const int h = h0 + r, w = w0 + s;
                const bool ok = bvalid && k < p.Kg && (unsigned)h < (unsigned)p.H && (unsigned)w < (unsigned)p.W;
                rb[i] = bload(rx, ok ? (unsigned)(pixb + c * HW + r * p.W + s) * 4u : OOB);
            }
        }
    };
    auto store_tile = [&](int buf, int q) {
        constexpr int NA = ALoadK<BM, AVEC>::NA;
#pragma unroll
        for (int i = 0; i < NA; ++i) {
            const int v = tid + NT * i;
            if (AVEC) {
                const int row = v >> 2, kq = (v & 3) * 4;
                if (v < BM * 4) {
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (in_quarter(4 * i + j, 4 * NA, q)) As[buf][kq + j][row] = ra[4 * i + j];
                }
            } else {
                if (v < BM * BK && in_quarter(i, NA, q)) As[buf][v & 15][v >> 4] = ra[i];
            }
        }
        if (BMODE == 2) {
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

    const int nk = (p.Kg + BK - 1) / BK;
    const int kt_begin = split * p.ktiles_per_split;
    int kt_end = kt_begin + p.ktiles_per_split;
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
    store_tile_nchw<T>(p, acc, m0, n0, wm, wn, lane, p.Ng, p.P * p.Q, p.d_pq, split);
}

#include "conv_planes.h"

template <int KH, int KW, int KO>
__global__ __launch_bounds__(256) void conv_fwd_k1_kernel(const ThinP t) {
    const int Ng = t.N * t.P * t.Q;
    const int pix = blockIdx.x * 256 + threadIdx.x;
    if (pix >= Ng) return;
    const int img = fdiv(pix, t.d_pq);
    const int pq = pix - img * t.P * t.Q;
    const int pp = fdiv(pq, t.d_q), qq = pq - pp * t.Q;
    const int h0 = pp * t.SH - t.PH, w0 = qq * t.SW - t.PW;
    const rsrc_t rx = make_rsrc(t.x, t.x_bytes);
    unsigned off[KH][KW];
#pragma unroll
    for (int r = 0; r < KH; ++r)
#pragma unroll
        for (int s = 0; s < KW; ++s) {
            const int h = h0 + r, w = w0 + s;
            off[r][s] = ((unsigned)h < (unsigned)t.H && (unsigned)w < (unsigned)t.W)
                            ? (unsigned)((img * t.C * t.H + h) * t.W + w) * 4u : OOB;
        }
    const int c0 = blockIdx.y * t.per_slice;
    const int c1 = min(c0 + t.per_slice, t.C);
    const unsigned cstride = (unsigned)(t.H * t.W) * 4u;
    float acc[KO];
#pragma unroll
    for (int k = 0; k < KO; ++k) acc[k] = 0.f;
#pragma unroll 2
    for (int c = c0; c < c1; ++c) {
        const float* wc = t.a + c * (KH * KW);          // uniform: scalar loads; output channel k at + k*C*KH*KW
        const unsigned co = (unsigned)c * cstride;      // an out-of-range offset stays out of range
#pragma unroll
        for (int r = 0; r < KH; ++r)
#pragma unroll
            for (int s = 0; s < KW; ++s) {
                const float xv = bload(rx, off[r][s] + co);
#pragma unroll
                for (int k = 0; k < KO; ++k) acc[k] += xv * wc[k * t.C * (KH * KW) + r * KW + s];
            }
    }
#pragma unroll
    for (int k = 0; k < KO; ++k) t.partial[((int64_t)blockIdx.y * KO + k) * Ng + pix] = acc[k];
}

}  // namespace

using namespace rg::conv;

// BMODE / AVEC of the loader (conv_fwd_kernel) from bmode / avec; the plane kernels (conv_planes.h) have 4 or 8 waves
#define RG_FWD_LAUNCH_K(KERNEL, NTH, BM_, BN_, WM_, WN_)                                                              \
    if (bmode == 2) hipLaunchKernelGGL((KERNEL<BM_, BN_, WM_, WN_, 2, true>), grid, dim3(NTH), 0, stream, p);         \
    else if (bmode == 1) hipLaunchKernelGGL((KERNEL<BM_, BN_, WM_, WN_, 1, true>), grid, dim3(NTH), 0, stream, p);    \
    else if (avec) hipLaunchKernelGGL((KERNEL<BM_, BN_, WM_, WN_, 0, true>), grid, dim3(NTH), 0, stream, p);          \
    else hipLaunchKernelGGL((KERNEL<BM_, BN_, WM_, WN_, 0, false>), grid, dim3(NTH), 0, stream, p)
#define RG_FWD_LAUNCH(BM_, BN_, WM_, WN_) RG_FWD_LAUNCH_K(conv_fwd_kernel, NT, BM_, BN_, WM_, WN_)
#define RG_FWD_PL_LAUNCH(BM_, BN_, WM_, WN_) RG_FWD_LAUNCH_K(conv_fwd_pl_kernel, 64 * WM_ * WN_, BM_, BN_, WM_, WN_)

namespace {

// thin layers: channels per slice so that ~2048 workgroups exist (>= 4 channels each)
static int thin_fwd_per_slice(int C, int64_t Ng) {
    int64_t slices = rg::cdiv64(2048, rg::cdiv64(Ng, 256));
    if (slices > C / 4) slices = C / 4;
    if (slices < 1) slices = 1;
    return (int)rg::cdiv64(C, slices);
}

// Layers the tap-reuse kernel takes: 3x3 / stride 1 / pad 1 on maps halo_geom accepts (fewer than 64 output rows: the 32 x 256 tile
// of the generic kernel wastes less than a half-empty 64-row tile) ...
static bool fwd_halo_geom(const ConvGeom& g) {
    return g.KH == 3 && g.KW == 3 && g.SH == 1 && g.SW == 1 && g.PH == 1 && g.PW == 1 && g.C % BK == 0 && g.K >= 64 &&
           halo_geom(g.H, g.W);
}
// ... whose caller passed the [K][9][C] filters, float4-aligned like the input
static bool fwd_halo_operands(const float* x, const float* w_krsc) { return w_krsc && aligned16(w_krsc, x); }

struct FwdCall {
    const ConvGeom& g;
    const float *x, *w, *w_krsc;
    float* y;
    Workspace ws;
    hipStream_t stream;
    ConvP p;            // geometry, operands, epilogue, GEMM sizes: what neither the path nor the plan decides
};

static int fwd_thin(const FwdCall& c, int per, int slices) {
    const ConvGeom& g = c.g;
    ThinP t;
    thin_fill(t, c.x, c.w, static_cast<float*>(c.ws.ptr), g, per);
    rg::ProfScope prof(rg::FAM_CONV_FWD, c.stream, 2.0 * (double)g.K * c.p.Ng * c.p.Kg, alg_bytes(g));
    const dim3 grid(rg::cdiv(c.p.Ng, 256), slices);
    THIN_DISPATCH(conv_fwd_k1_kernel, g, grid, c.stream, t);      // (a four-pixel forward was measured: 136 us against 120)
    if (int e = rg::check_launch("rg_conv2d_fwd(thin)")) return e;
    launch_finish(c.stream, t.partial, c.y, g.K, c.p.Ng, g.P * g.Q, c.p.d_pq, slices, c.p.ep);
    return rg::check_launch("rg_conv2d_fwd(thin finish)");
}

static int fwd_halo(const FwdCall& c, const HaloPlan& hpl) {
    ConvP ph = c.p;
    ph.w = c.w_krsc;
    rg::ProfScope prof(rg::FAM_CONV_FWD, c.stream, 2.0 * ph.M * (double)ph.Ng * ph.Kg, alg_bytes(c.g));
    return halo_launch<false>(ph, c.g.C, c.g.H, c.g.W, hpl, c.ws.ptr, c.stream, "rg_conv2d_fwd(3x3 tap reuse)");
}

// one generic launch: p with the loader's operands, bmode / avec the loader (conv_fwd_kernel), pl the plan
static int fwd_run_plan(const FwdCall& c, ConvP p, int bmode, bool avec, Plan pl) {
    const ConvGeom& g = c.g;
    hipStream_t stream = c.stream;
    p.partial_bytes = (unsigned)fit_splits(pl, p.M, p.Ng, c.ws);
    p.m_tiles = pl.m_tiles; p.n_tiles = pl.n_tiles;
    p.splits = pl.splits; p.ktiles_per_split = pl.ktiles_per_split;
    p.partial = pl.splits > 1 ? static_cast<float*>(c.ws.ptr) : nullptr;
    p.arrive = pl.splits > 1 ? splitk_arrivals(stream, p.m_tiles * p.n_tiles, p.partial, c.y, p.M, p.Ng, g.P * g.Q, p.ep) : nullptr;
    rg::ProfScope prof(rg::FAM_CONV_FWD, stream, 2.0 * p.M * (double)p.Ng * p.Kg, alg_bytes(g));
    const dim3 grid(p.m_tiles * p.n_tiles, pl.splits, 1);
    const TuneKey tk = tune_key(1, g, bmode * 2 + (avec ? 1 : 0), pl.tile, pl.splits, ep_bits(p.ep, false));
    choose_impl(1, tk, stream, pl.tile <= 1 ? 3 : 2, [&](int impl) {
        if (impl == 2) {                  // eight waves: 128 x 128 as 4 x 2 waves of 32 x 64, 64 x 128 as 2 x 4 waves of 32 x 32
            if (pl.tile == 0) { RG_FWD_PL_LAUNCH(128, 128, 4, 2); }
            else { RG_FWD_PL_LAUNCH(64, 128, 2, 4); }
        }
        else if (impl) { RG_TILE_SWITCH(pl.tile, RG_FWD_PL_LAUNCH); }
        else { RG_TILE_SWITCH(pl.tile, RG_FWD_LAUNCH); }
    });
    if (pl.splits > 1 && !p.arrive) {
        if (int e = rg::check_launch("rg_conv2d_fwd")) return e;
        launch_finish(stream, p.partial, c.y, p.M, p.Ng, g.P * g.Q, p.d_pq, pl.splits, p.ep);
    }
    return rg::check_launch("rg_conv2d_fwd");
}

// the generic implicit GEMM: loader from the geometry and the pointers, plan measured among plan_candidates
static int fwd_generic(const FwdCall& c) {
    const ConvGeom& g = c.g;
    ConvP p = c.p;
    const bool is1x1 = g.KH == 1 && g.KW == 1;
    const bool avec = (p.Kg % 4 == 0) && aligned16(c.w, c.x);
    int bmode = 0;
    if (avec && is1x1 && g.SH == 1 && g.SW == 1 && g.PH == 0 && g.PW == 0 && ((g.H * g.W) % 4 == 0)) bmode = 2;
    else if (avec && g.C % 16 == 0 && (is1x1 || (c.w_krsc && aligned16(c.w_krsc)))) {
        bmode = 1;
        if (!is1x1) p.w = c.w_krsc;
    }
    Plan cands[kMaxCand];
    int nc = plan_candidates(p.M, p.Ng, p.Kg, cands, kMaxCand);
    if (nc > 1 && (plans_workspace(cands, nc, p.M, p.Ng) > c.ws.bytes || !c.ws.ptr)) nc = 1;     // not the queried scratch
    const TuneKey pk = tune_key(64, g, bmode * 2 + (avec ? 1 : 0), nc, 0, ep_bits(p.ep, false));
    return choose_status(pk, c.stream, nc, [&](int i) { return fwd_run_plan(c, p, bmode, avec, cands[i]); });
}

}  // namespace

extern "C" size_t rg_conv2d_fwd_workspace(int N, int C, int K, int KH, int KW, int P, int Q) {
    // the query has no stride / padding: it sizes the stride-1 / pad-1 layer (H x W = P x Q), the only one the tap-reuse kernel takes
    const ConvGeom g = {N, C, P, Q, K, KH, KW, 1, 1, 1, 1, P, Q};
    const int64_t Ng = (int64_t)N * P * Q;
    if (thin_filter(g)) return (size_t)rg::cdiv(C, thin_fwd_per_slice(C, Ng)) * (size_t)K * (size_t)Ng * sizeof(float);
    Plan cands[kMaxCand];
    const int nc = plan_candidates(K, Ng, (int64_t)C * KH * KW, cands, kMaxCand);
    size_t need = plans_workspace(cands, nc, K, Ng);
    if (fwd_halo_geom(g)) {
        const size_t hn = splitk_bytes(halo_plan(K, Ng, C, nullptr).splits, K, Ng);
        if (hn > need) need = hn;
    }
    return need;
}

// w_krsc (optional): weights re-laid out as [K][KH*KW][C] (rg_weights_to_krsc); with C % 16 == 0 it selects the
// (r,s)-major reduction order whose pixel gather tests the padding bounds once per 16-deep k-tile.
extern "C" int rg_conv2d_fwd(const float* x, const float* w, const float* w_krsc, float* y, int N, int C, int H, int W,
                             int K, int KH, int KW, int SH, int SW, int PH, int PW, int P, int Q, const float* scale,
                             const float* shift, const float* residual, int act, float slope, void* workspace,
                             size_t workspace_bytes, hipStream_t stream) {
    const ConvGeom g = {N, C, H, W, K, KH, KW, SH, SW, PH, PW, P, Q};
    if (int e = validate("rg_conv2d_fwd", g)) return e;
    RG_REQUIRE(x && w && y, "rg_conv2d_fwd: null tensor");
    FwdCall c = {g, x, w, w_krsc, y, Workspace{workspace, workspace_bytes}, stream};
    ConvP& p = c.p;
    fill_common(p, g);
    p.x = x; p.w = w; p.y = y;
    p.ep = Epilogue{scale, shift, residual, act, slope, nullptr, nullptr, 0};
    p.M = K; p.Ng = N * P * Q; p.Kg = C * KH * KW;
    p.x_bytes = x_bytes(g); p.w_bytes = w_bytes(g); p.y_bytes = y_bytes(g);
    if (thin_filter(g)) {
        const int per = thin_fwd_per_slice(C, p.Ng);
        const int slices = rg::cdiv(C, per);
        if (workspace && (size_t)slices * (size_t)K * (size_t)p.Ng * sizeof(float) <= workspace_bytes) return fwd_thin(c, per, slices);
    }
    // 3x3 / stride 1 / pad 1 layers: the tap-reuse kernel or the generic implicit GEMM on the (r,s)-major filters — whichever is
    // faster for the geometry, measured once like the kernel implementations (RG_CONV_TUNE=0: always the tap-reuse kernel)
    if (fwd_halo_geom(g) && fwd_halo_operands(x, w_krsc)) {
        const HaloPlan hpl = halo_plan(p.M, p.Ng, C, &c.ws);
        if (!tune_enabled()) return fwd_halo(c, hpl);
        return choose_status(tune_key(16, g, 0, 0, 0, ep_bits(p.ep, false)), stream, 2,
                             [&](int i) { return i ? fwd_generic(c) : fwd_halo(c, hpl); });
    }
    return fwd_generic(c);
}
