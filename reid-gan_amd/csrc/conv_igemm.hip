// Implicit-GEMM 2-D convolution for gfx950 (MI355X): forward, data-gradient and weight-gradient, fp32 tensors.
// Arithmetic: every fp32 operand is split exactly into three bf16 pieces and each product is evaluated as six
// v_mfma_f32_32x32x16_bf16 partial products with fp32 accumulation (see "matrix arithmetic of one 16-deep k-tile" in conv_core.h).
//
// Replaces what cuDNN/ATen do for the reference's nn.Conv2d / nn.ConvTranspose2d layers:
//   ResNet-50 trunk           CC/clustercontrast/models/resnet_ibn_a.py:70-159 (layout pin), FD/reid/models/resnet.py:65-75
//   CustomPoseGenerator       FD/fdgan/networks.py:86-138  (Conv 4x4/2, (8,4) valid, ConvTranspose 4x4/2, (8,4))
//   NLayerDiscriminator       FD/fdgan/networks.py:206-232 (Conv 4x4/2, 4x4/1)
// ConvTranspose2d forward == dgrad of the conv with the same weight tensor; its dgrad == conv fwd.
//
// GEMM views (all tensors NCHW fp32, weights [K][C][KH][KW]):
//   fwd   : y[K, N*P*Q]      = w[K, C*KH*KW]          x im2col(x)[C*KH*KW, N*P*Q]
//   dgrad : dx[C, N*Hc*Wc]   = w^T[C, K*taps]         x gather(dy)[K*taps, N*Hc*Wc]   per stride-parity class
//   wgrad : dw[K, C*KH*KW]   = dy[K, N*P*Q]           x im2col(x)^T[N*P*Q, C*KH*KW]   split over N*P*Q
//
// Loader variants (chosen on the host from the geometry):
//   * the reduction index k is wave-uniform in the gather loaders, so its (c,r,s) / (k,tap) decomposition runs on
//     the scalar unit (one readfirstlane); per lane only the bounds test and the address add remain;
//   * 1x1 / stride 1 / pad 0 layers (half of ResNet-50) load the pixel operand as float4 (16 B per lane);
//   * dgrad reads weights re-laid out as [K][KH*KW][C] (rg_weights_to_krsc, one tiny pass per layer per step) so the
//     weight operand is contiguous along the GEMM row and loads as float4 as well;
//   * layers whose M x N tile count cannot fill 256 CUs (8x4 and 16x8 maps at batch 32) split the reduction over
//     blockIdx.y; partial tiles go to a workspace and a finishing kernel sums them and applies the epilogue.
//
// Work decomposition: 256-thread workgroup = 4 wave64; block tile BM x BN x 16, each wave owns a
// (BM/WM) x (BN/WN) sub-tile made of 32x32 MFMA tiles.  Operand tiles are staged global -> VGPR ->
// LDS, k-major ([16][BM+4] / [16][BN+4]) so that the MFMA operand reads (lane = row, lane>>5 = k)
// are bank-conflict free ds_read_b32; LDS is double buffered, one barrier per k-tile, and the
// next tile's global loads are issued before the current tile's MFMAs.  The flat tile id is
// remapped so that every XCD (private 4 MiB L2) works on a contiguous range of pixel tiles.
//
// This unit is the library's host side (conv_plan.h): the tune switch, the tile / split-K cost model and its candidate lists, the
// measured choice with its file cache, the test knobs and the split-K arrival registry.  The kernels and the entry points that launch
// them are in conv_fwd.hip, conv_dgrad.hip and conv_wgrad.hip, on the shared device code of conv_core.h (arithmetic, loaders,
// epilogues), conv_halo.h (tap-reuse 3x3), conv_finish.h (split-K finishers), conv_thin.h and conv_planes.h (bf16-plane kernels).
// conv_prims.h (dividers, XCD remap, buffer access) and conv_reduce.h (the split-K slab sum of the weight gradients) are shared with
// the fp8 units, conv_f8.hip and f8_quant.hip, which also take ConvGeom and the stride-parity classes from conv_plan.h.
#include "conv_plan.h"

#include <stdio.h>
#include <string.h>
#include <atomic>
#include <map>
#include <mutex>
#include <vector>

namespace rg {
namespace conv {

bool tune_enabled() {
    static const bool on = env_int("RG_CONV_TUNE", 1) != 0;
    return on;
}

int validate(const char* op, const ConvGeom& g) {
    const int N = g.N, C = g.C, H = g.H, W = g.W, K = g.K, KH = g.KH, KW = g.KW, SH = g.SH, SW = g.SW, PH = g.PH, PW = g.PW, P = g.P, Q = g.Q;
    RG_REQUIRE(N > 0 && C > 0 && H > 0 && W > 0 && K > 0 && KH > 0 && KW > 0, "%s: non-positive dimension", op);
    RG_REQUIRE(SH > 0 && SW > 0 && PH >= 0 && PW >= 0 && P > 0 && Q > 0, "%s: bad stride/pad/output size", op);
    RG_REQUIRE((P - 1) * SH - PH + KH - 1 >= 0 && (Q - 1) * SW - PW + KW - 1 >= 0, "%s: inconsistent geometry", op);
    // every output pixel must start inside the padded input
    RG_REQUIRE((int64_t)(P - 1) * SH - PH < H && (int64_t)(Q - 1) * SW - PW < W, "%s: output larger than input allows", op);
    RG_REQUIRE((int64_t)N * P * Q < (1ll << 31) && (int64_t)C * KH * KW < (1ll << 31) && (int64_t)N * H * W < (1ll << 31) &&
                   (int64_t)C * H * W < (1ll << 31) && (int64_t)K * P * Q < (1ll << 31) &&
                   (int64_t)K * KH * KW < (1ll << 31),
               "%s: dimension product exceeds 2^31", op);
    RG_REQUIRE(fits_buffer((int64_t)N * C * H * W * 4) && fits_buffer((int64_t)N * K * P * Q * 4) &&
                   fits_buffer((int64_t)K * C * KH * KW * 4),
               "%s: every tensor must be smaller than 2 GiB (32-bit buffer offsets)", op);
    return RG_OK;
}

// Development override: RG_CONV_FORCE="tile,splits" (tile 0..3 or -1, splits >= 1 or -1) pins the choice.
static int g_force_tile = -2, g_force_splits = -2;
static void force_override(int* tile, int* splits) {
    if (g_force_tile == -2) {
        g_force_tile = -1;
        g_force_splits = -1;
        const char* e = getenv("RG_CONV_FORCE");
        if (e) sscanf(e, "%d,%d", &g_force_tile, &g_force_splits);
    }
    if (g_force_tile >= 0 && g_force_tile <= 3) *tile = g_force_tile;
    if (g_force_splits >= 1) *splits = g_force_splits;
}

static Plan make_plan(int M, int64_t Ng, int64_t nk, int tile, int splits) {
    Plan pl;
    pl.tile = tile;
    pl.m_tiles = rg::cdiv(M, kTileBM[tile]);
    pl.n_tiles = (int)rg::cdiv64(Ng, kTileBN[tile]);
    pl.ktiles_per_split = (int)rg::cdiv64(nk, splits);
    pl.splits = (int)rg::cdiv64(nk, pl.ktiles_per_split);
    return pl;
}

// Tile + split-K choice for the fwd / dgrad GEMMs (M x Ng outputs, Kg reduction), allow_split = single-class output.
// A small cost model instead of thresholds: 256 CUs, up to 4 co-resident workgroups per CU sharing each SIMD's
// matrix pipe.  Measured pipe utilisation vs co-residency (PMC, round 1): ~0.55 alone, ~0.7 with two, ~0.85 with
// three or more.  Work that does not divide into 256-wide rounds leaves CUs idle (wave quantisation), so the split
// count is chosen to land on full rounds; split-K pays for its partial tiles (write + read in the finishing kernel).
Plan plan_gemm(int M, int64_t Ng, int64_t Kg, bool allow_split) {
    const int64_t nk = rg::cdiv64(Kg > 0 ? Kg : 1, BK);
    int cand[2], ncand = 0;
    if (M <= 32) cand[ncand++] = 3;
    else if (M <= 64) { if (Ng >= 128) cand[ncand++] = 1; cand[ncand++] = 2; }
    else { if (Ng >= 128) cand[ncand++] = 0; cand[ncand++] = 2; }
    // utilisation of a SIMD's matrix pipe with r co-resident workgroups per CU, relative efficiency of each tile
    // shape (loads + LDS traffic per MFMA), fixed per-workgroup cost (first-tile latency, epilogue) in cycles
    static const double util[5] = {1.0, 0.60, 0.85, 0.90, 0.92};
    static const double tile_eff[4] = {1.0, 0.92, 0.85, 0.85};
    const double fixed = 6000.0;
    double best = 1e300;
    int tile = cand[0];
    int best_s = 1;
    for (int ci = 0; ci < ncand; ++ci) {
        const int t = cand[ci];
        const int64_t tiles = (int64_t)rg::cdiv(M, kTileBM[t]) * rg::cdiv64(Ng, kTileBN[t]);
        const double mfma_per_ktile = (kTileBM[t] / 64.0) * (kTileBN[t] / 64.0) * 8.0 * 64.0 / tile_eff[t];
        const int smax = allow_split ? 16 : 1;
        for (int s = 1; s <= smax; ++s) {
            if (s > 1 && (nk / s < 8 || (int64_t)s * M * Ng * 4 >= (1ll << 31))) break;
            const int64_t kt = rg::cdiv64(nk, s);
            const int64_t B = tiles * rg::cdiv64(nk, kt);
            const double bt = kt * mfma_per_ktile + fixed;
            const int64_t r = rg::cdiv64(B, 256);
            double time = r <= 4 ? r * bt / util[r] : (double)B / 256.0 * bt / util[4];
            if (s > 1) time += 2400.0 + (double)(s + 1) * M * (double)Ng * 4.0 / 3.0e12 * 2.0e9;   // finishing kernel
            if (time < best * 0.97) {        // prefer bigger tiles / fewer splits unless clearly better
                best = time;
                tile = t;
                best_s = s;
            }
        }
    }
    int splits = best_s;
    force_override(&tile, &splits);
    if (!allow_split) splits = 1;
    return make_plan(M, Ng, nk, tile, splits);
}

// The cost model above was fitted to the round-1..3 kernels; against the eight-wave plane kernels it is off by one tile size or
// one split step on about a third of the ResNet geometries (tools/sweep_tiles.py, round 4: forward -6 %, data gradient -4 % with the
// best forced plan per layer).  So the PLAN is a measured choice too: the model's plan first, then every other tile of the shape
// class with 1 / 2 / 3 / 4 / 6 / 8 splits that keeps >= 4 k-tiles per split and <= 1 536 workgroups; an alternative has to beat the
// model's plan by 3 % (choose_impl).  RG_CONV_TUNE=0 / a forced plan / a GEMM under 1 GFLOP: the model's plan only.
static const double kPlanTuneMinFlop = 1.0e9;      // below 1 GFLOP a launch takes ~10 us whatever the plan: not worth ~100 timed launches
int plan_candidates(int M, int64_t Ng, int64_t Kg, Plan* out, int max_out) {
    out[0] = plan_gemm(M, Ng, Kg, true);
    int n = 1;
    if (g_force_tile >= 0 || g_force_splits >= 1 || !tune_enabled() || M <= 32) return n;
    if (2.0 * M * (double)Ng * (double)Kg < kPlanTuneMinFlop) return n;      // launch-bound sizes: nothing to choose between
    const int64_t nk = rg::cdiv64(Kg > 0 ? Kg : 1, BK);
    int tiles[3], nt = 0;
    if (Ng >= 128) {
        if (M > 64) tiles[nt++] = 0;
        tiles[nt++] = 1;
    }
    tiles[nt++] = 2;
    static const int ss[6] = {1, 2, 3, 4, 6, 8};
    for (int ti = 0; ti < nt && n < max_out; ++ti)
        for (int si = 0; si < 6 && n < max_out; ++si) {
            const int t = tiles[ti], sp = ss[si];
            if (sp > 1 && (nk / sp < 4 || (int64_t)sp * M * Ng * 4 >= (1ll << 31))) continue;
            const int64_t wgs = (int64_t)rg::cdiv(M, kTileBM[t]) * rg::cdiv64(Ng, kTileBN[t]);
            if (sp > 1 && wgs * sp > 1536) continue;
            const Plan pl = make_plan(M, Ng, nk, t, sp);
            bool dup = false;
            for (int i = 0; i < n; ++i) dup = dup || (out[i].tile == pl.tile && out[i].splits == pl.splits);
            if (!dup) out[n++] = pl;
        }
    return n;
}
size_t plans_workspace(const Plan* pl, int n, int M, int64_t Ng) {
    size_t need = 0;
    for (int i = 0; i < n; ++i) {
        const size_t b = splitk_bytes(pl[i].splits, M, Ng);
        if (b > need) need = b;
    }
    return need;
}

static Plan plan_wgrad(int M, int Ng, int64_t Kg) {
    Plan pl;
    // the reduction (N*P*Q) is long, so parallelism comes from split-K: always take the largest tile that fits
    // (a 64x64 tile issues 2x the LDS reads and 4x the loader instructions per MFMA of the 128x128 one)
    pl.tile = (M <= 32) ? 3 : ((M <= 64 || Ng <= 64) ? 2 : 0);     // (64 x 128 for M = 64 measured 8-10 % slower than 64 x 64 here)
    pl.m_tiles = rg::cdiv(M, kTileBM[pl.tile]);
    pl.n_tiles = rg::cdiv(Ng, kTileBN[pl.tile]);
    const int64_t nk = rg::cdiv64(Kg, BK);
    const int64_t mn = (int64_t)pl.m_tiles * pl.n_tiles;
    // 1024 workgroups = one full round at the kernel's 4 workgroups per CU (measured: 512 / 768 / 896 / 1024 / 1152 / 1280 /
    // 1536 -> 71.9 / 75.2 / 75.7 / 78.5 / 75.3 / 77.7 / 76.9 TFLOP/s over the FD-GAN step's wgrad launches; the fwd cost
    // model over-splits here)
    int64_t want = rg::cdiv64(1024, mn);
    if (want > nk / 16) want = nk / 16;   // >= 16 k-tiles per split keeps partial traffic small
    if (want < 1) want = 1;
    if (want > 512) want = 512;
    while (want > 1 && want * (int64_t)M * Ng * 4 >= (1ll << 31)) --want;
    if (want >= 8) {
        // a multiple of 8 splits (see the kernel's split -> XCD mapping); trailing splits may be empty (they store zeros)
        int64_t w8 = (want + 4) / 8 * 8;
        while (w8 > 8 && w8 * (int64_t)M * Ng * 4 >= (1ll << 31)) w8 -= 8;
        if (w8 * (int64_t)M * Ng * 4 < (1ll << 31) && w8 <= nk) {
            pl.ktiles_per_split = (int)rg::cdiv64(nk, w8);
            pl.splits = (int)w8;
            return pl;
        }
    }
    pl.ktiles_per_split = (int)rg::cdiv64(nk, want);
    pl.splits = (int)rg::cdiv64(nk, pl.ktiles_per_split);
    return pl;
}

// Measured split depth (choose_impl, like plan_candidates for the forward / data-gradient GEMMs): the model's split count first,
// then 1/2, 3/4, 3/2 and 2x of it (multiples of 8 from 8 up: the kernel's split -> XCD mapping), >= 8 k-tiles per split.  What is
// timed is the whole call: kernel + split-K reduction (+ folded-BatchNorm finish).
int wgrad_plan_candidates(int M, int Ng, int64_t Kg, Plan* out, int max_out) {
    out[0] = plan_wgrad(M, Ng, Kg);
    int n = 1;
    if (!tune_enabled()) return n;
    if (2.0 * M * (double)Ng * (double)Kg < kPlanTuneMinFlop) return n;
    const int64_t nk = rg::cdiv64(Kg, BK);
    const int base = out[0].splits;
    const int alts[4] = {base / 2, base * 3 / 4, base * 3 / 2, base * 2};
    for (int i = 0; i < 4 && n < max_out; ++i) {
        int64_t sp = alts[i];
        if (sp >= 8) sp = (sp + 4) / 8 * 8;
        if (sp < 1) sp = 1;
        if (sp > 512) sp = 512;
        if (sp > 1 && nk / sp < 8) continue;
        if (sp * (int64_t)M * Ng * 4 >= (1ll << 31)) continue;
        Plan pl = out[0];
        pl.ktiles_per_split = (int)rg::cdiv64(nk, sp);
        pl.splits = sp >= 8 ? (int)sp : (int)rg::cdiv64(nk, pl.ktiles_per_split);
        if (pl.splits > nk) continue;
        bool dup = false;
        for (int j = 0; j < n; ++j) dup = dup || out[j].splits == pl.splits;
        if (!dup) out[n++] = pl;
    }
    return n;
}

// ---- arrival counters for split-K without the finishing launch (rg_conv_splitk_arrivals) ----
// The library never allocates: the caller registers, per stream, a zero-initialised buffer of 32-bit counters that stays alive and is
// touched by nothing else.  Launches on one stream are ordered and every launch leaves its counters at zero (atomicInc wraps on the
// last arrival), so one buffer per stream serves every launch on it.  Not used inside a stream capture: a captured launch would carry
// the capture stream's counters into replays on whatever stream the graph is launched on, next to eager launches that use them.
// Measured (profiles/r04_splitk_inkernel.txt): a wash — the FD-GAN step 34.24-34.34 ms with the finishing kernels, 34.53-34.62 ms with
// the in-kernel finish on the same box (what a launch boundary costs, 1.5-1.9 us, is what the last arriver's acquire and its serial
// read of the tile's partials cost), so rg_hip registers counters only on request (RG_SPLITK_INKERNEL=1) and the default stays the
// finishing kernel.  The first form tried — __threadfence() in every workgroup — cost +27 us per split launch (36.9 vs 32.8 ms).
struct Arrivals { unsigned* ptr; int count; };
static std::map<hipStream_t, Arrivals> g_arrivals;
static std::mutex g_arrivals_mu;
static std::atomic<int> g_inkernel_launches{0};
unsigned* splitk_arrivals(hipStream_t stream, int tiles) {
    Arrivals a = {nullptr, 0};
    {
        std::lock_guard<std::mutex> lock(g_arrivals_mu);
        auto it = g_arrivals.find(stream);
        if (it != g_arrivals.end()) a = it->second;
    }
    if (!a.ptr || tiles > a.count) return nullptr;
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(stream, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone) {
        (void)hipGetLastError();
        return nullptr;
    }
    ++g_inkernel_launches;
    return a.ptr;
}

// Two implementations of the generic fwd / dgrad / wgrad kernels exist: the round-3 kernels (fp32 LDS tiles, every reading wave
// splits its fragments) and the bf16-plane path of conv_planes.h (operands split once on their way into LDS).  Neither wins
// everywhere: measured per layer they differ by up to +-20 % in both directions (profiles/r04_planes_vs_r03.txt: the plane path
// gains on the deep 1x1 layers and the 1x1 / shifted weight gradients, loses on the gather-loaded 4x4 layers).  So the choice is
// MEASURED, once per (family, geometry, plan): the first call of a geometry outside a stream capture runs both (one warm-up and
// one timed launch each, HIP events on the launch stream), keeps the faster (the plane path has to win by 3 %) and re-runs it if
// it was not the last one, so the output of every call — the first included — comes from the kernel that serves the geometry
// from then on: run-to-run bit-identity inside a process is untouched.  RG_CONV_TUNE=0: always the round-3 kernels.
// rg_conv_set_planes(mask): force the plane path per family (1 forward, 2 data gradient, 4 weight gradient).
static int g_planes_mask = 0;
static bool planes_enabled(int family_bit) { return (g_planes_mask & family_bit) != 0; }
static std::map<TuneKey, int> g_tune;
static std::mutex g_tune_mu;
// RG_CONV_TUNE_CACHE=<file>: measured choices are appended to the file (one line of 17 integers per geometry) and loaded from it by
// the next process, which then measures only what it has not seen — profiling runs (no measuring launches inside the trace) and
// runs that must repeat another process's kernels bit for bit use it
static void tune_cache_load_locked() {
    static bool loaded = false;
    if (loaded) return;
    loaded = true;
    const char* path = getenv("RG_CONV_TUNE_CACHE");
    FILE* f = path ? fopen(path, "r") : nullptr;
    if (!f) return;
    TuneKey k;
    int choice;
    for (;;) {
        bool ok = true;
        for (int i = 0; i < 16 && ok; ++i) ok = fscanf(f, "%d", &k[i]) == 1;
        if (!ok || fscanf(f, "%d", &choice) != 1) break;
        g_tune[k] = choice < 0 ? 0 : (choice >= kMaxCand ? kMaxCand - 1 : choice);
    }
    fclose(f);
}
static void tune_cache_append_locked(const TuneKey& k, int choice) {
    const char* path = getenv("RG_CONV_TUNE_CACHE");
    FILE* f = path ? fopen(path, "a") : nullptr;
    if (!f) return;
    for (int i = 0; i < 16; ++i) fprintf(f, "%d ", k[i]);
    fprintf(f, "%d\n", choice);
    fclose(f);
}

// rg_conv_set_pick / rg_conv_pick_log (tests): a pinned key kind (the key's first field: 1 / 2 / 4 implementation, 16 / 32 path,
// 64 / 128 / 256 plan; slot = log2(kind)) runs candidate min(index, ncand - 1) without measuring, synchronising or touching g_tune;
// while any kind is pinned every choice appends {key[16], ncand, index run} to the log
static std::atomic<int> g_pick[9] = {{-1}, {-1}, {-1}, {-1}, {-1}, {-1}, {-1}, {-1}, {-1}};
static std::atomic<int> g_pick_pinned{0};
static std::vector<int> g_pick_records;
static std::mutex g_pick_mu;
static const size_t kPickLogMax = 18u << 16;
static int pick_slot(int kind) {
    if (kind <= 0 || (kind & (kind - 1)) || kind > 256 || kind == 8) return -1;
    return __builtin_ctz(kind);
}
static void pick_record(const TuneKey& key, int ncand, int choice) {
    std::lock_guard<std::mutex> lock(g_pick_mu);
    if (g_pick_records.size() + 18 > kPickLogMax) return;
    g_pick_records.insert(g_pick_records.end(), key.begin(), key.end());
    g_pick_records.push_back(ncand);
    g_pick_records.push_back(choice);
}

typedef void (*RunFn)(void*, int);
static int choose_impl_measured(int family_bit, const TuneKey& key, hipStream_t stream, int ncand, RunFn run_fn, void* ctx) {
    const auto run = [&](int c) { run_fn(ctx, c); return c; };
    if (planes_enabled(family_bit)) {
        return run((planes_enabled(8) && ncand > 2) ? 2 : 1);
    }
    if (!tune_enabled()) return run(0);
    {                                 // the lock covers the table only, never a launch: measurements may nest (path choice below)
        std::unique_lock<std::mutex> lock(g_tune_mu);
        tune_cache_load_locked();
        auto it = g_tune.find(key);
        if (it != g_tune.end() && it->second < ncand) {
            const int c = it->second;
            lock.unlock();
            return run(c);
        }
    }
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(stream, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone) {
        (void)hipGetLastError();
        return run(0);                // no host synchronisation inside a capture: round-3 kernel, nothing recorded
    }
    if (ncand > kMaxCand) ncand = kMaxCand;
    hipEvent_t ev[2 * kMaxCand];
    bool ok = true;
    for (int i = 0; i < 2 * ncand; ++i) ok = hipEventCreate(&ev[i]) == hipSuccess && ok;
    float t[kMaxCand] = {0.f};
    if (ok) {
        // the candidates are timed on an otherwise idle GPU: work other streams were given earlier (weight gradients on the side
        // stream, D_pd on the auxiliary stream) would otherwise run beside some candidates and not others
        (void)hipDeviceSynchronize();
        for (int c = 0; c < ncand; ++c) run(c);       // warm-up (first launch of a code object loads it)
        for (int c = 0; c < ncand; ++c) {
            ok = hipEventRecord(ev[2 * c], stream) == hipSuccess && ok;
            run(c);
            ok = hipEventRecord(ev[2 * c + 1], stream) == hipSuccess && ok;
        }
        ok = hipEventSynchronize(ev[2 * ncand - 1]) == hipSuccess && ok;
        for (int c = 0; c < ncand && ok; ++c) ok = hipEventElapsedTime(&t[c], ev[2 * c], ev[2 * c + 1]) == hipSuccess;
    }
    for (int i = 0; i < 2 * ncand; ++i) (void)hipEventDestroy(ev[i]);
    if (!ok) {
        (void)hipGetLastError();
        return run(0);
    }
    int choice = 0;                   // a plane-path candidate has to win by 3 %
    float best = t[0];
    for (int c = 1; c < ncand; ++c)
        if (t[c] < 0.97f * best) { best = t[c]; choice = c; }
    {
        std::lock_guard<std::mutex> lock(g_tune_mu);
        g_tune[key] = choice;
        tune_cache_append_locked(key, choice);
    }
    if (choice != ncand - 1) run(choice);             // the result must come from the chosen kernel
    return choice;
}

// run(0): round-3 kernel, run(1): plane path, run(2) (ncand == 3: 128 x 128 tiles only): plane path with EIGHT waves per workgroup
// (4 x 2 waves of 32 x 64: the staging work per thread halves and four waves per SIMD hide each other's waits; +8 % on the
// micro-benchmark's 128 x 128 tile).  Each: the kernel launch only; split-K finishers follow.  Returns the implementation that ran
// LAST (= the chosen one).
int choose_impl(int family_bit, const TuneKey& key, hipStream_t stream, int ncand, RunFn run_fn, void* ctx) {
    if (g_pick_pinned.load() == 0) return choose_impl_measured(family_bit, key, stream, ncand, run_fn, ctx);
    const int slot = pick_slot(key[0]);
    const int pin = slot >= 0 ? g_pick[slot].load() : -1;
    const int c = pin >= 0 ? (pin < ncand ? pin : ncand - 1) : choose_impl_measured(family_bit, key, stream, ncand, run_fn, ctx);
    if (pin >= 0) run_fn(ctx, c);
    pick_record(key, ncand, c);
    return c;
}

}  // namespace conv
}  // namespace rg

using namespace rg::conv;

// development knob (tools/sweep_tiles.py): pin the planner's tile / split choice at run time; (-1, -1) releases it
extern "C" int rg_conv_set_force(int tile, int splits) {
    g_force_tile = tile;
    g_force_splits = splits;
    return RG_OK;
}

// development knob (tests, tools/bench_conv.py): kernel families on the bf16-plane operand path (bit 0 fwd, 1 dgrad, 2 wgrad);
// returns the previous mask
extern "C" int rg_conv_set_planes(int mask) {
    const int old = g_planes_mask;
    g_planes_mask = mask & 15;
    return old;
}

// development knob (tests/test_conv_candidates_gpu.py): pin the measured choice of one key kind to a candidate index (-1 releases
// it); returns the previous index, or RG_ERR_INVALID - 1 for an unknown kind / an index below -1
extern "C" int rg_conv_set_pick(int kind, int index) {
    const int slot = pick_slot(kind);
    if (slot < 0 || index < -1) {
        rg::set_error("rg_conv_set_pick: kind %d / index %d (kinds 1, 2, 4, 16, 32, 64, 128, 256; index >= -1)", kind, index);
        return RG_ERR_INVALID - 1;
    }
    std::lock_guard<std::mutex> lock(g_pick_mu);
    const int old = g_pick[slot].exchange(index);
    if ((old >= 0) != (index >= 0)) g_pick_pinned += index >= 0 ? 1 : -1;
    return old;
}

// copies up to max_records records of 18 ints (key[16], ncand, index run) logged while a kind was pinned into buf (may be NULL),
// clears the log and returns how many records it held
extern "C" int rg_conv_pick_log(int* buf, int max_records) {
    std::lock_guard<std::mutex> lock(g_pick_mu);
    const int n = (int)(g_pick_records.size() / 18);
    const int m = buf ? (n < max_records ? n : (max_records > 0 ? max_records : 0)) : 0;
    if (m > 0) memcpy(buf, g_pick_records.data(), (size_t)m * 18 * sizeof(int));
    g_pick_records.clear();
    return n;
}

// number of choices the first-call chooser has measured so far (kernel implementation per (family, geometry, plan); tap-reuse vs
// generic path and tile / split plan per geometry); out[0] / out[1] (may be NULL): how many of the kernel-implementation choices
// went to the round-3 kernels / the plane path
extern "C" int rg_conv_tune_stats(int* out) {
    std::lock_guard<std::mutex> lock(g_tune_mu);
    int n[2] = {0, 0};
    for (const auto& kv : g_tune)
        if (kv.first[0] == 1 || kv.first[0] == 2 || kv.first[0] == 4) ++n[kv.second ? 1 : 0];      // out[1]: plane path, four or eight waves
    if (out) { out[0] = n[0]; out[1] = n[1]; }
    return (int)g_tune.size();
}

// Registers (count > 0) or removes (counters == NULL) the arrival counters of split-K launches on `stream`: `count` zero-initialised
// 32-bit words that the caller keeps alive and never writes.  With them the split forward / unit-stride data-gradient launches on
// that stream finish inside the convolution kernel (the last split of a tile to arrive sums the tile's partials in split order: the
// finishing kernel's values bit for bit); without them — or for launches with more tiles than `count`, or inside a stream capture —
// a finishing kernel follows as before.
extern "C" int rg_conv_splitk_arrivals(void* counters, int count, hipStream_t stream) {
    RG_REQUIRE(!counters || count > 0, "rg_conv_splitk_arrivals: count must be positive");
    RG_REQUIRE((reinterpret_cast<uintptr_t>(counters) & 3) == 0, "rg_conv_splitk_arrivals: counters must be 4-byte aligned");
    std::lock_guard<std::mutex> lock(g_arrivals_mu);
    if (counters) g_arrivals[stream] = Arrivals{static_cast<unsigned*>(counters), count};
    else g_arrivals.erase(stream);
    return RG_OK;
}

// test / development query: split-K launches that finished inside the convolution kernel so far (this process)
extern "C" int rg_conv_splitk_inkernel_count(void) { return g_inkernel_launches.load(); }
