// Host side of the fp32 convolution library that the family units (conv_fwd.hip, conv_dgrad.hip, conv_wgrad.hip) share: the
// geometry of a call (conv_f8.hip uses it too), the tile / split-K plan, the tune switch and the measured choice.  Everything declared
// here is defined ONCE, in conv_igemm.hip, which also owns the state behind it (the choice table and its file, the pick knob, the
// forced plan / plane mask, the split-K arrival registry).  No device code: the planner compiles without a kernel.
#pragma once
#include "rg_common.h"

#include <array>

namespace rg {
namespace conv {

constexpr int BK = 16;                              // depth of one k-tile
constexpr int kTileBM[4] = {128, 64, 64, 32};       // block tiles of the generic kernels (RG_TILE_SWITCH)
constexpr int kTileBN[4] = {128, 128, 64, 256};
constexpr int kMaxCand = 16;                        // candidates of one measured choice (3 kernel implementations; up to 16 tile / split plans)

// x [N][C][H][W] * w [K][C][KH][KW] -> y [N][K][P][Q], whichever of the three is being computed
struct ConvGeom {
    int N, C, H, W, K, KH, KW, SH, SW, PH, PW, P, Q;
};
// algorithmic HBM bytes of one conv launch: one read of each operand + one write of the result (fp32)
inline double alg_bytes(const ConvGeom& g) {
    return 4.0 * ((double)g.N * g.C * g.H * g.W + (double)g.K * g.C * g.KH * g.KW + (double)g.N * g.K * g.P * g.Q);
}
int validate(const char* op, const ConvGeom& g);
// a tensor of this many bytes can sit behind one buffer resource (32-bit byte offsets, OOB = 2^31)
inline bool fits_buffer(int64_t bytes) { return bytes > 0 && bytes < (1ll << 31); }

// Stride-parity class (ah, aw) of a data gradient: the input pixels (ah + SH hc, aw + SW wc), Hc x Wc of them per image, receive
// the filter taps (r0 + SH j, s0 + SW jj), nrh x nrw of them.  A stride-1 layer has the one class (0, 0): every pixel, every tap.
struct ParityClass {
    int r0, s0, nrh, nrw, Hc, Wc;
};
inline ParityClass parity_class(const ConvGeom& g, int ah, int aw) {
    ParityClass c;
    c.r0 = (ah + g.PH) % g.SH;
    c.s0 = (aw + g.PW) % g.SW;
    c.nrh = c.r0 < g.KH ? (g.KH - c.r0 + g.SH - 1) / g.SH : 0;
    c.nrw = c.s0 < g.KW ? (g.KW - c.s0 + g.SW - 1) / g.SW : 0;
    c.Hc = ah < g.H ? (g.H - ah + g.SH - 1) / g.SH : 0;
    c.Wc = aw < g.W ? (g.W - aw + g.SW - 1) / g.SW : 0;
    return c;
}

// the caller's scratch
struct Workspace {
    void* ptr;
    size_t bytes;
    bool holds(size_t need) const { return need <= bytes && (!need || ptr); }
};

template <typename... P>
inline bool aligned16(const P*... p) {
    return ((... | reinterpret_cast<uintptr_t>(p)) & 15) == 0;
}

// RG_CONV_TUNE (README "Environment switches", read once per process): kernel implementation, tap-reuse against generic path and
// tile / split plan are measured choices; 0: the round-3 kernels, the tap-reuse kernel and the cost model's plan
bool tune_enabled();

// Tile (index into kTileBM / kTileBN) and split-K depth of one GEMM launch: forward, data gradient and weight gradient.
struct Plan {
    int tile, m_tiles, n_tiles, splits, ktiles_per_split;
};
inline size_t splitk_bytes(int splits, int M, int64_t Ng) { return splits > 1 ? (size_t)splits * M * (size_t)Ng * sizeof(float) : 0; }
// the partial-tile bytes of `pl`; a plan whose partials `ws` cannot hold (or that exceed `limit`) falls back to unsplit
inline size_t fit_splits(Plan& pl, int M, int64_t Ng, const Workspace& ws, size_t limit = ~(size_t)0) {
    const size_t need = splitk_bytes(pl.splits, M, Ng);
    if (need < limit && ws.holds(need)) return need;
    pl.splits = 1;
    pl.ktiles_per_split = 1 << 30;
    return 0;
}
Plan plan_gemm(int M, int64_t Ng, int64_t Kg, bool allow_split);
// out[0]: the cost model's plan; then the alternatives a measurement may prefer.  Their order is data (the choice file stores indices).
int plan_candidates(int M, int64_t Ng, int64_t Kg, Plan* out, int max_out);
int wgrad_plan_candidates(int M, int Ng, int64_t Kg, Plan* out, int max_out);
size_t plans_workspace(const Plan* pl, int n, int M, int64_t Ng);

// Key of a measured choice: kind (1 / 2 / 4 kernel implementation of forward / data gradient / weight gradient, 16 / 32 tap-reuse
// against generic path, 64 / 128 / 256 plan), the geometry, four fields of the kind's own.
typedef std::array<int, 16> TuneKey;
inline TuneKey tune_key(int kind, const ConvGeom& g, int f12, int f13, int f14, int f15) {
    return TuneKey{kind, g.N, g.C, g.H, g.W, g.K, g.KH, g.KW, g.SH, g.SW, g.PH, g.PW, f12, f13, f14, f15};
}

// Runs the candidate chosen for `key` among `ncand` through run(ctx, index) and returns its index (conv_igemm.hip, "measured choice").
int choose_impl(int family_bit, const TuneKey& key, hipStream_t stream, int ncand, void (*run)(void*, int), void* ctx);
template <typename Run>
inline int choose_impl(int family_bit, const TuneKey& key, hipStream_t stream, int ncand, Run run) {
    return choose_impl(family_bit, key, stream, ncand, [](void* ctx, int c) { (*static_cast<Run*>(ctx))(c); }, &run);
}
// Candidates that are whole launches with a status (a path, a plan): run(index) -> status; the first non-zero status.
template <typename Run>
inline int choose_status(const TuneKey& key, hipStream_t stream, int ncand, Run run) {
    if (ncand <= 1) return run(0);
    int st = RG_OK;
    choose_impl(0, key, stream, ncand, [&](int c) {
        const int e = run(c);
        if (e && !st) st = e;
    });
    return st;
}

// the arrival counters a one-class split-K launch of `tiles` output tiles on `stream` may use, or nullptr (-> finishing kernel)
unsigned* splitk_arrivals(hipStream_t stream, int tiles);

}  // namespace conv
}  // namespace rg
