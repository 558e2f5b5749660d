// Tap-reuse 3x3 / stride 1 / pad 1 kernel, shared by the forward pass (conv_fwd.hip, DGRAD false) and the data gradient
// (conv_dgrad.hip, DGRAD true), with its geometry test, plan and launch; included after conv_finish.h.
#pragma once
#include "conv_finish.h"

namespace {

// ---------------------------------------------------------------------------------------------
// 3x3 / stride 1 / pad 1 with TAP REUSE (forward, and the data gradient of such a layer, which is the same convolution with
// the filter taps flipped and the channel roles swapped).
// The generic kernels gather the pixel operand once per filter tap: nine L2 -> LDS passes over the same activations.  With a
// 128-pixel tile that is 12 KB of operands per 0.26 MFLOP, and at ~6 TB/s of L2 delivery the 64 / 128-channel layers of the trunk
// are bound by that traffic, not by the matrix pipe.  Here the reduction runs channel-block outer, tap inner: for every block of
// 16 reduction channels the workgroup loads ONE halo tile of the activations — its 128 output pixels (whole rows of one image, or
// whole small images) plus the one-pixel border, zero outside the image — and all nine taps read their pixel operand from that
// tile at a constant offset ((r-1) * (W+2) + (s-1)); only the filter operand (16 x BM floats) is fetched per tap.  Pixel-operand
// traffic drops 5-6 x and each barrier interval holds the same 8 MFMA k-steps as before but only the filter loads.
// Requirements (checked on the host): W in {4..64} a power of two, tile rows dividing H or whole images per tile, reduction
// channels % 16 == 0, filters in the [K][9][C] copy.
// ---------------------------------------------------------------------------------------------
struct HaloP {
    ConvP c;             // x: input tensor of the convolution being computed (fwd: x, dgrad: dy); w: [K][9][C] filters; y: output
    int Cred;            // channels of that input tensor (the reduction): fwd C, dgrad K
    int HP, Wh, slab;    // halo positions per tile, halo row length W + 2, positions per image of the tile (rows + 2) * Wh
    int cblocks, cb_per_split;
    FastDiv d_hp, d_slab, d_wh, d_hw, d_w;
};

// 128-row tiles: 184-194 registers; at the 168 of three waves per SIMD the compiler spilled 23-46 of them to scratch inside the
// loop (two waves per SIMD: forward +1 %, data gradient +4.5 % on the trunk's 3x3 layers, same box); 64-row tiles fit at three
template <int BM, bool DGRAD, int NH>
__global__ __launch_bounds__(NT) __attribute__((amdgpu_waves_per_eu(BM == 128 ? 2 : 3))) void conv3x3_halo_kernel(const HaloP hp) {
    using T = Tile<BM, 128, 2, 2>;
    const ConvP& p = hp.c;
    __shared__ __attribute__((aligned(16))) float As[2][BK][T::LDA];
    __shared__ __attribute__((aligned(16))) float Hs[2][NH * NT];     // [16 channels][HP positions], flat

    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int wm = wid >> 1, wn = wid & 1;
    const int l32 = lane & 31, kh = lane >> 5;
    const int tile = xcd_remap(blockIdx.x, gridDim.x);
    const int mt = tile % p.m_tiles, nt = tile / p.m_tiles;
    const int m0 = mt * BM, n0 = nt * 128;
    const int split = blockIdx.y;
    const int HW = p.H * p.W, HP = hp.HP, Wh = hp.Wh;
    const rsrc_t rw = make_rsrc(p.w, p.w_bytes), rx = make_rsrc(p.x, p.x_bytes);

    // tile origin: 128 % W == 0, so a tile starts at the beginning of a row (and covers whole rows / whole images)
    const int img0 = fdiv(n0, hp.d_hw);
    const int h0 = fdiv(n0 - img0 * HW, hp.d_w);

    // ---- pixel-operand positions of this lane inside the halo tile (two 32-pixel column blocks of the wave) ----
    int pos[T::TN];
#pragma unroll
    for (int j = 0; j < T::TN; ++j) {
        const int pl = wn * T::WTN + j * 32 + l32;
        const int il = fdiv(pl, hp.d_hw);                      // 0 when the tile lies inside one image (H*W >= 128)
        const int rem = pl - il * HW;
        const int hl = fdiv(rem, hp.d_w);
        pos[j] = il * hp.slab + (hl + 1) * Wh + (rem - hl * p.W) + 1;
    }

    // ---- halo loader: element f = tid + 256 i of [16][HP]; byte offset of channel block 0, OOB outside the image ----
    unsigned hoff[NH];
#pragma unroll
    for (int i = 0; i < NH; ++i) {
        const int f = tid + NT * i;
        const int ch = fdiv(f, hp.d_hp);
        const int ps = f - ch * HP;
        const int il = fdiv(ps, hp.d_slab);
        const int r2 = ps - il * hp.slab;
        const int hh = fdiv(r2, hp.d_wh);
        const int ww = r2 - hh * Wh - 1;
        const int img = img0 + il, h = h0 + hh - 1;
        const bool ok = ch < BK && img < p.N && (unsigned)h < (unsigned)p.H && (unsigned)ww < (unsigned)p.W;
        hoff[i] = ok ? (unsigned)((((int64_t)img * hp.Cred + ch) * p.H + h) * p.W + ww) * 4u : OOB;
    }
    const unsigned cbstride = (unsigned)(BK * HW) * 4u;        // bytes between channel blocks of the input tensor

    // ---- filter-operand loader ----
    constexpr int NA = BM / 64;                                // float4 per thread and tile (BM * 16 / 4 / 256)
    unsigned aoff[NA];
    int arow[NA], akq[NA];                                     // fwd: (row m, k quad); dgrad: (k row, m quad)
#pragma unroll
    for (int i = 0; i < NA; ++i) {
        const int v = tid + NT * i;
        if (!DGRAD) {
            arow[i] = v >> 2;
            akq[i] = (v & 3) * 4;
            aoff[i] = (m0 + arow[i] < p.M) ? (unsigned)(((int64_t)(m0 + arow[i]) * 9 * hp.Cred + akq[i]) * 4) : OOB;
        } else {
            arow[i] = v / (BM / 4);
            akq[i] = (v - arow[i] * (BM / 4)) * 4;
            aoff[i] = (m0 + akq[i] < p.M) ? (unsigned)(((int64_t)arow[i] * 9 * p.M + m0 + akq[i]) * 4) : OOB;
        }
    }
    float4 ra[NA];
    float hv[NH];
    floatx16 acc[T::TM][T::TN];
    zero_acc<T>(acc);

    auto load_a = [&](int cb, int t) {
        // fwd: w[m][t][cb*16 + kq..]; dgrad: w[cb*16 + kk][8 - t][m..] (the flipped tap of the transposed filter)
        const unsigned kb4 = DGRAD ? (unsigned)(((int64_t)cb * BK * 9 + (8 - t)) * p.M) * 4u
                                   : (unsigned)(t * hp.Cred + cb * BK) * 4u;
#pragma unroll
        for (int i = 0; i < NA; ++i) ra[i] = bload4(rw, aoff[i] == OOB ? OOB : aoff[i] + kb4);
    };
    auto store_a = [&](int buf) {
#pragma unroll
        for (int i = 0; i < NA; ++i) {
            if (!DGRAD) {
                As[buf][akq[i] + 0][arow[i]] = ra[i].x;
                As[buf][akq[i] + 1][arow[i]] = ra[i].y;
                As[buf][akq[i] + 2][arow[i]] = ra[i].z;
                As[buf][akq[i] + 3][arow[i]] = ra[i].w;
            } else {
                *reinterpret_cast<float4*>(&As[buf][arow[i]][akq[i]]) = ra[i];
            }
        }
    };
    auto load_h = [&](int cb) {
        const unsigned o = (unsigned)cb * cbstride;
#pragma unroll
        for (int i = 0; i < NH; ++i) hv[i] = bload(rx, hoff[i] == OOB ? OOB : hoff[i] + o);
    };
    auto store_h = [&](int buf) {
#pragma unroll
        for (int i = 0; i < NH; ++i) Hs[buf][tid + NT * i] = hv[i];
    };

    const int cb_begin = split * hp.cb_per_split;
    int cb_end = cb_begin + hp.cb_per_split;
    if (cb_end > hp.cblocks) cb_end = hp.cblocks;
    if (cb_begin < cb_end) {
        load_h(cb_begin);
        load_a(cb_begin, 0);
        store_h(0);
        store_a(0);
    }
    __syncthreads();
    int ab = 0, hb = 0;
    for (int cb = cb_begin; cb < cb_end; ++cb) {
        const bool more_cb = cb + 1 < cb_end;
        for (int t = 0; t < 9; ++t) {
            const bool last = !more_cb && t == 8;
            if (t == 0 && more_cb) load_h(cb + 1);             // lands during the nine taps of this block
            if (!last) load_a(t == 8 ? cb + 1 : cb, t == 8 ? 0 : t + 1);
            const int r = (t * 11) >> 5;                       // t / 3 for t < 9
            const int toff = (r - 1) * Wh + (t - 3 * r - 1);
            const float* hsb = Hs[hb];
            mma_kstep<T::TM, T::TN>([&](int i, int q) { return As[ab][8 * kh + q][wm * T::WTM + i * 32 + l32]; },
                                    [&](int j, int q) { return hsb[(8 * kh + q) * HP + pos[j] + toff]; }, acc);
            if (!last) store_a(ab ^ 1);
            if (t == 8 && more_cb) store_h(hb ^ 1);
            __syncthreads();
            ab ^= 1;
        }
        hb ^= 1;
    }
    store_tile_nchw<T>(p, acc, m0, n0, wm, wn, lane, p.Ng, HW, hp.d_hw, split, nt * 2 + wn);
}

// ---- geometry test, plan, launch ----
// H x W maps a 128-pixel tile covers with whole rows of one image or whole small images (the layer-shape part
// of the eligibility is the family's: fwd_halo_geom / dgrad_halo_geom)
static bool halo_geom(int H, int W, int* HP, int* Wh, int* slab) {
    if (W < 4 || W > 64 || (W & (W - 1))) return false;
    const int R = 128 / W;                      // rows of a 128-pixel tile
    int rows, imgs;
    if (R <= H) {
        if (H % R) return false;
        rows = R;
        imgs = 1;
    } else {
        if (R % H) return false;                // whole images per tile
        rows = H;
        imgs = R / H;
    }
    *Wh = W + 2;
    *slab = (rows + 2) * (W + 2);
    *HP = imgs * *slab;
    return *HP <= 288;
}
static bool halo_geom(int H, int W) {
    int hp, wh, slab;
    return halo_geom(H, W, &hp, &wh, &slab);
}
struct HaloPlan {
    int bm, m_tiles, n_tiles, splits, per;
};
// ws: the caller's scratch (a launch: a plan whose partials it cannot hold runs unsplit), nullptr: the plan to size the scratch for
static HaloPlan halo_plan(int M, int64_t Ng, int Cred, const rg::conv::Workspace* ws) {
    HaloPlan pl;
    pl.bm = M <= 64 ? 64 : 128;
    pl.m_tiles = rg::cdiv(M, pl.bm);
    pl.n_tiles = (int)rg::cdiv64(Ng, 128);
    const int cblocks = Cred / BK;
    const int64_t tiles = (int64_t)pl.m_tiles * pl.n_tiles;
    const int target = 512;
    int64_t want = tiles >= (3 * target) / 4 ? 1 : rg::cdiv64(target, tiles);       // ~2 workgroups per CU
    if (want > cblocks / 2) want = cblocks / 2;                     // >= 2 channel blocks (18 k-tiles) per split
    if (want > 16) want = 16;
    if (want < 1) want = 1;
    while (want > 1 && want * (int64_t)M * Ng * 4 >= (1ll << 31)) --want;
    pl.per = (int)rg::cdiv64(cblocks, want);
    pl.splits = rg::cdiv(cblocks, pl.per);
    if (ws && !ws->holds(rg::conv::splitk_bytes(pl.splits, M, Ng))) {
        pl.splits = 1;
        pl.per = cblocks;
    }
    return pl;
}
// p: x / w (krsc) / y / ep / M / Ng / byte sizes filled by the caller; returns the launch status
template <bool DGRAD>
static int halo_launch(ConvP p, int Cred, int H, int W, const HaloPlan& pl, void* workspace, hipStream_t stream, const char* op) {
    HaloP hp;
    int HPv, Wh, slab;
    halo_geom(H, W, &HPv, &Wh, &slab);
    p.m_tiles = pl.m_tiles; p.n_tiles = pl.n_tiles;
    p.splits = pl.splits;
    p.partial = pl.splits > 1 ? static_cast<float*>(workspace) : nullptr;
    p.partial_bytes = (unsigned)rg::conv::splitk_bytes(pl.splits, p.M, p.Ng);
    p.arrive = pl.splits > 1 ? splitk_arrivals(stream, pl.m_tiles * pl.n_tiles, p.partial, p.y, p.M, p.Ng, H * W, p.ep) : nullptr;
    hp.c = p;
    hp.Cred = Cred;
    hp.HP = HPv; hp.Wh = Wh; hp.slab = slab;
    hp.cblocks = Cred / BK;
    hp.cb_per_split = pl.per;
    hp.d_hp = make_fastdiv(HPv);
    hp.d_slab = make_fastdiv(slab);
    hp.d_wh = make_fastdiv(Wh);
    hp.d_hw = make_fastdiv(H * W);
    hp.d_w = make_fastdiv(W);
    const dim3 grid(pl.m_tiles * pl.n_tiles, pl.splits, 1);
    const bool small = 16 * HPv <= 13 * NT;
    if (pl.bm == 128) {
        if (small) hipLaunchKernelGGL((conv3x3_halo_kernel<128, DGRAD, 13>), grid, dim3(NT), 0, stream, hp);
        else hipLaunchKernelGGL((conv3x3_halo_kernel<128, DGRAD, 18>), grid, dim3(NT), 0, stream, hp);
    } else {
        if (small) hipLaunchKernelGGL((conv3x3_halo_kernel<64, DGRAD, 13>), grid, dim3(NT), 0, stream, hp);
        else hipLaunchKernelGGL((conv3x3_halo_kernel<64, DGRAD, 18>), grid, dim3(NT), 0, stream, hp);
    }
    if (pl.splits > 1 && !p.arrive) {
        if (int e = rg::check_launch(op)) return e;
        launch_finish(stream, p.partial, p.y, p.M, p.Ng, H * W, make_fastdiv(H * W), pl.splits, p.ep);
    }
    return rg::check_launch(op);
}

}  // namespace
