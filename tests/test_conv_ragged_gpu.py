"""GPU: every candidate kernel of the fp32 convolution library at RAGGED geometries, per element against an fp64 reference.

tests/test_conv_candidates_gpu.py runs every candidate at the bench's geometries (large batches, channel counts that are multiples
of 16, power-of-two maps).  This file runs them where rows, columns, depth and pixel groups are all partial: each tile shape, each
split count, each implementation (default, plane path, eight-wave plane path), each loader mode and each direct kernel, on the
smallest shapes that reach the regime (every tensor far below 4 MB).  Same discipline as the bench sweep (tests/conv_sweep.py):
outputs, row sums, dgamma / dbeta and the workspace are NaN before EVERY launch, a NaN guard sits behind the output, and the bound
is per element, 2^-20 (|a| (*) |b|) plus the epilogue's own terms.

Two layers of pinning: rg_conv_set_pick enumerates the implementations (kinds 1 / 2 / 4) and tap-reuse against generic (kinds 16 /
32); rg_conv_set_force(tile, splits) sets the plan of the forward / data-gradient GEMMs, which at these sizes have one plan only
(the weight-gradient plan is not forced: its tile and split count follow K, C*KH*KW and N*P*Q, so the cases reach them by shape).
The workspace and the row-sum column count are queried AFTER forcing.  Which tile, split count and loader actually ran is read back
from the pick log (fields 12-14 of the kind-1/2/4 keys; make_plan may clip a forced split count) and DECLARED below is asserted to be
covered by what the log reported.  The direct kernels (thin, small-C) make no logged choice: for them the log must hold no record
at all, so no GEMM ran in their place; the dispatch line is cited next to each table.

The host model of the dispatch (fwd_route .. wgrad_regime) restates the conditions of csrc/conv_fwd.hip, conv_dgrad.hip,
conv_wgrad.hip and conv_igemm.hip; tests/test_conv_ragged_cpu.py checks the tables against it without a GPU, and the GPU run checks
it against the log.

Run with -s for the RATIO lines (profiles/conv_ragged_ratios.txt keeps them)."""
import math

import pytest
import torch

from tests import conv_sweep as S

pytestmark = pytest.mark.gpu

BK = 16
TILE_BM = (128, 64, 64, 32)
TILE_BN = (128, 128, 64, 256)
CROSS_SPLITS = (1, 2, 3, 5)
CROSS = tuple((t, s) for t in range(4) for s in CROSS_SPLITS)
MODEL = ((-1, -1),)

# forward epilogues: (scale, shift, residual, act)
EPI_F = {"none": (0, 0, 0, S.ACT_NONE), "scale shift res leaky": (1, 1, 1, S.ACT_LEAKY), "shift tanh": (0, 1, 0, S.ACT_TANH),
         "res relu": (0, 0, 1, S.ACT_RELU)}
# data-gradient epilogues: (scale, shift, residual, mask, row sums, act); row sums exist unsplit only
EPI_D = {"none": (0, 0, 0, 0, 0, S.ACT_NONE), "res mask": (0, 0, 1, 1, 0, S.ACT_NONE), "res mask rowsum": (0, 0, 1, 1, 1, S.ACT_NONE),
         "scale shift tanh": (1, 1, 0, 0, 0, S.ACT_TANH), "shift leaky": (0, 1, 0, 0, 0, S.ACT_LEAKY)}
ALL_F = tuple(EPI_F)
ALL_D = tuple(EPI_D)
NO_ROWSUM_D = tuple(e for e in EPI_D if not EPI_D[e][4])

# geometry: (N, C, H, W, K, KH, KW, SH, SW, PH, PW); a case: (geometry, plans, epilogues)
# ---- forward ----
# thin kernels (conv_fwd.hip rg_conv2d_fwd: `if (thin_filter(g))` -> fwd_thin; conv_thin.h thin_filter: K <= 4, 3x3 or 4x4 with K = 1)
FWD_THIN = [
    ((3, 40, 9, 7, 1, 3, 3, 2, 2, 1, 1), MODEL, ALL_F[:3]),        # K = 1, stride 2, 60 pixels, ten channel slices
    ((2, 3, 11, 13, 2, 3, 3, 1, 1, 0, 0), MODEL, ALL_F[:3]),       # K = 2, pad 0, one slice of three channels, 198 pixels
    ((2, 37, 13, 11, 3, 3, 3, 1, 1, 1, 1), MODEL, ALL_F[:3]),      # K = 3, 286 pixels: a second, ragged workgroup; ragged slices
    ((1, 130, 20, 12, 4, 3, 3, 1, 1, 1, 1), MODEL, ALL_F[:3]),     # K = 4, 240 pixels
    ((5, 130, 9, 8, 1, 4, 4, 1, 1, 1, 1), MODEL, ALL_F[:3]),       # 4x4, K = 1, 280 pixels
    ((2, 8, 9, 9, 1, 4, 4, 2, 2, 0, 0), MODEL, ALL_F[:3]),         # 4x4 / 2 / pad 0, 18 pixels
]
# tap-reuse against generic (kind 16; conv_fwd.hip fwd_halo_geom: 3x3 / 1 / 1, C % 16 == 0, K >= 64, conv_halo.h halo_geom)
FWD_HALO = [
    ((5, 32, 4, 4, 160, 3, 3, 1, 1, 1, 1), MODEL, ALL_F[:2]),      # W 4: 8 images per tile = 288 halo positions (the limit), 5 images
                                                                   # only; two row tiles; C = 32: one split
    ((3, 64, 8, 8, 80, 3, 3, 1, 1, 1, 1), MODEL, ALL_F[:2]),       # W 8: 2 images per tile, the second tile half empty; ragged 128-row
                                                                   # tile; C = 64: two splits
    ((1, 64, 16, 16, 96, 3, 3, 1, 1, 1, 1), MODEL, ALL_F[:2]),     # W 16: 8 rows of one image per tile; K = 96
    ((1, 128, 8, 32, 64, 3, 3, 1, 1, 1, 1), MODEL, ALL_F[:2]),     # W 32: 4 rows per tile; 64-row tile; four splits
    ((1, 64, 4, 64, 96, 3, 3, 1, 1, 1, 1), MODEL, ALL_F[:2]),      # W 64: 2 rows per tile, 264 halo positions (just under the limit)
    ((3, 32, 8, 4, 72, 3, 3, 1, 1, 1, 1), MODEL, ALL_F[:2]),       # W 4, H 8: 4 images per tile (240 positions), 3 images only
]
# generic, the full cross product tile x splits x implementation x epilogue; K, N*P*Q and C*KH*KW all off the tile sizes
FWD_CROSS = [
    ((3, 148, 6, 6, 72, 1, 1, 1, 1, 0, 0), CROSS, ALL_F),          # bmode 2: 1x1 / 1 / 0, H*W % 4 == 0 (float4 pixel operand)
    ((2, 144, 9, 7, 40, 1, 1, 2, 2, 0, 0), CROSS, ALL_F),          # bmode 1: a 1x1 stride 2 on an odd map
    ((2, 48, 7, 6, 80, 3, 3, 1, 1, 1, 1), CROSS, ALL_F),           # bmode 1: (r,s)-major gather from the KRSC copy (W 6: not tap reuse)
    ((2, 24, 9, 7, 40, 3, 3, 2, 2, 1, 1), CROSS, ALL_F),           # bmode 0, avec: 3x3 / 2 on an odd map
    ((2, 3, 19, 13, 8, 7, 7, 2, 2, 3, 3), CROSS, ALL_F),           # bmode 0, scalar weights (147 % 4 != 0): the 7x7 / 2 / 3 stem
    ((2, 5, 7, 5, 37, 3, 3, 1, 1, 2, 2), CROSS, ALL_F),            # bmode 0, scalar weights (45 % 4 != 0): pad 2, three k-tiles
    ((2, 12, 6, 10, 136, 5, 5, 1, 1, 2, 2), CROSS, ALL_F),         # bmode 0, avec: 5x5 / 1 / 2, two row tiles of 128 (136 rows)
    ((3, 48, 8, 4, 72, 8, 4, 1, 1, 0, 0), CROSS + ((2, 8), (3, 8)), ALL_F),   # the (8, 4) valid filter: 3 pixels, 96 k-tiles
]
# generic, the model's plan with every implementation
FWD_MODEL = [
    ((2, 18, 10, 6, 64, 4, 4, 2, 2, 1, 1), MODEL, ALL_F),          # 4x4 / 2 / 1
    ((2, 32, 12, 6, 130, 3, 3, 1, 1, 1, 1), MODEL, ALL_F),         # 130 rows, 144 pixels: the 128-row tiles by the model
    ((5, 20, 10, 10, 12, 1, 1, 1, 1, 0, 0), MODEL, ALL_F),         # 1x1, 12 rows: the 32 x 256 tile by the model, 500 pixels
    ((2, 7, 9, 8, 33, 3, 3, 2, 2, 0, 0), MODEL, ALL_F),            # pad 0, stride 2, 63 depth
    ((1, 6, 9, 11, 9, 7, 7, 1, 1, 3, 3), MODEL, ALL_F),            # 7x7 / 1 / 3
]

# ---- data gradient ----
# small-C direct kernels (conv_dgrad.hip dgrad_impl: `if (g.C <= 4 && ...) return dgrad_smallc(c)`; dgrad_smallc: the four-pixel
# kernel for C <= 3 with at most 4 taps per axis and class, the plain kernel otherwise)
DGRAD_SMALLC = [
    ((2, 3, 19, 13, 8, 7, 7, 2, 2, 3, 3), MODEL, NO_ROWSUM_D),     # four-pixel: C = 3, 7x7 / 2 (4 + 3 taps); odd pixel-quad counts
    ((1, 3, 9, 7, 5, 3, 3, 1, 1, 1, 1), MODEL, NO_ROWSUM_D),       # four-pixel, stride 1: 3 row quads of 7 (21 groups)
    ((2, 2, 10, 6, 6, 4, 4, 2, 2, 1, 1), MODEL, NO_ROWSUM_D),      # four-pixel, C = 2
    ((3, 1, 6, 5, 7, 3, 3, 1, 1, 1, 1), MODEL, NO_ROWSUM_D),       # four-pixel, C = 1
    ((1, 3, 12, 9, 4, 5, 5, 1, 1, 2, 2), MODEL, NO_ROWSUM_D),      # plain: 5 taps per axis
    ((2, 4, 10, 6, 6, 3, 3, 2, 2, 1, 1), MODEL, NO_ROWSUM_D),      # plain: C = 4, stride 2
    ((2, 4, 7, 9, 5, 3, 3, 1, 1, 1, 1), MODEL, NO_ROWSUM_D),       # plain: C = 4, stride 1
]
# tap-reuse against generic (kind 32; conv_dgrad.hip dgrad_halo_geom: 3x3 / 1 / 1, K % 16 == 0, C % 4 == 0, C >= 64)
DGRAD_HALO = [
    ((3, 64, 8, 8, 80, 3, 3, 1, 1, 1, 1), MODEL, ALL_D),           # C = 64: the 64-row tile; a half-empty second pixel tile
    ((2, 68, 8, 16, 32, 3, 3, 1, 1, 1, 1), MODEL, ALL_D),          # C = 68: ragged 128-row tile; K = 32: one split, fused row sums
    ((1, 128, 8, 32, 64, 3, 3, 1, 1, 1, 1), MODEL, ALL_D),         # C = 128, K = 64: two splits
]
DGRAD_CROSS = [
    ((3, 36, 6, 6, 148, 1, 1, 1, 1, 0, 0), CROSS, ALL_D),          # mode 2: 1x1 / 1 / 0 (the LDS-DMA ring on tiles 0 / 1)
    ((2, 40, 7, 6, 48, 3, 3, 1, 1, 1, 1), CROSS, ALL_D),           # mode 1: KRSC weights, K % 16 == 0
    ((2, 37, 7, 5, 24, 3, 3, 1, 1, 1, 1), CROSS, ALL_D),           # mode 0: C % 4 != 0
    ((2, 24, 9, 7, 48, 3, 3, 2, 2, 1, 1), CROSS, ALL_D),           # four parity classes of different sizes (odd H and W), mode 1
    ((3, 21, 10, 9, 32, 4, 4, 2, 2, 1, 1), CROSS, ALL_D),          # 4x4 / 2 on an odd width: a column no output touches; mode 0
]
DGRAD_MODEL = [
    ((2, 64, 9, 7, 48, 1, 1, 2, 2, 0, 0), MODEL, ALL_D),           # 1x1 / 2: three classes are empty, their pixels are epilogue(0)
    ((2, 36, 10, 8, 16, 3, 3, 2, 2, 1, 1), MODEL, ALL_D),          # 3x3 / 2, P, Q of a ConvTranspose2d with output padding 1
    ((2, 136, 6, 10, 12, 5, 5, 1, 1, 2, 2), MODEL, ALL_D),         # 136 rows x 120 pixels
    ((3, 72, 8, 4, 48, 8, 4, 1, 1, 0, 0), MODEL, ALL_D),           # the (8, 4) filter as ConvTranspose2d: 1x1 -> 8x4
    ((4, 20, 8, 4, 6, 4, 4, 2, 2, 1, 1), MODEL, ALL_D),            # ConvTranspose2d 4x4 / 2 role (test_conv_transpose), K = 6
]

# ---- weight gradient ----  a case: (geometry, fold variants); fold: 0 unfolded, 1 partials (8 slices), 2 sum_g
# thin kernels (conv_wgrad.hip wgrad_impl: `if (thin_filter(g))` -> wgrad_thin; thin_px4: the four-pixel form)
WGRAD_THIN = [
    ((3, 8, 6, 8, 1, 3, 3, 1, 1, 1, 1), (0, 1)),                   # four-pixel, K = 1, one slice
    ((2, 33, 16, 12, 2, 3, 3, 1, 1, 1, 1), (0,)),                  # four-pixel, K = 2
    ((1, 64, 34, 18, 3, 3, 3, 1, 1, 0, 0), (0,)),                  # four-pixel, K = 3, pad 0
    ((6, 8, 16, 12, 4, 3, 3, 1, 1, 1, 1), (0, 2)),                 # four-pixel, K = 4, 1152 pixels: two slices
    ((3, 40, 9, 7, 1, 3, 3, 2, 2, 1, 1), (0,)),                    # scalar (stride 2), K = 1
    ((2, 37, 11, 9, 2, 3, 3, 2, 2, 1, 1), (0, 1)),                 # scalar, K = 2
    ((2, 5, 9, 7, 3, 3, 3, 1, 1, 1, 1), (0,)),                     # scalar (Q % 4 != 0), K = 3
    ((2, 9, 7, 9, 4, 3, 3, 1, 1, 0, 0), (0,)),                     # scalar (Q = 7), K = 4, pad 0
    ((5, 130, 20, 12, 1, 4, 4, 1, 1, 1, 1), (0,)),                 # scalar 4x4, 1045 pixels: two ragged slices
]
# generic: every loader key (field 12 = vec * 2 + veca + wshift * 4), tiles 0 / 2 / 3 through K and C*KH*KW, split counts through
# N*P*Q (conv_igemm.hip plan_wgrad)
WGRAD_GENERIC = [
    ((2, 20, 7, 5, 40, 3, 3, 1, 1, 1, 1), (0, 1)),                 # key 0 (P*Q = 35), tile 2, unsplit: the two-launch fold finish
    ((2, 20, 8, 6, 136, 3, 3, 1, 1, 1, 1), (0, 1)),                # key 1: Q % 4 != 0 just fails wshift; tile 0 (136 x 180), unsplit
    ((25, 20, 16, 8, 24, 3, 3, 2, 2, 1, 1), (0, 1)),               # key 1: stride 2 fails wshift; tile 3, three splits, fused fold
    ((50, 20, 9, 9, 40, 4, 4, 1, 1, 1, 1), (0, 2)),                # key 1: KW > PW + 2 fails wshift; tile 2, sixteen splits
    ((4, 36, 8, 8, 72, 1, 1, 1, 1, 0, 0), (0, 1)),                 # key 3 (1x1 float4), tile 2 (36 columns), unsplit
    ((13, 80, 8, 8, 136, 1, 1, 1, 1, 0, 0), (0, 1)),               # key 3, tile 0 (136 x 80), three splits
    ((2, 20, 97, 16, 40, 3, 3, 1, 1, 1, 1), (0, 1)),               # key 7 (wshift), tile 2, 194 k-tiles in 16 splits of 13: the last is empty
    ((12, 5, 9, 8, 130, 3, 3, 1, 1, 1, 1), (0, 1, 2)),             # key 7, tile 2 (45 columns, % 4 != 0: the two-launch finish), three splits
    ((9, 7, 11, 9, 20, 3, 3, 1, 1, 0, 0), (0, 1)),                 # key 0 (P*Q = 63), tile 3, two splits; 63 columns: two-launch finish
    ((13, 24, 8, 8, 136, 3, 3, 1, 1, 1, 1), (0, 1)),               # key 7, tile 0 (136 x 216), three splits, fused fold
    ((4, 6, 8, 4, 20, 4, 4, 2, 2, 1, 1), (0,)),                    # the ConvTranspose2d roles of test_conv_transpose (x and dy swapped)
    ((3, 48, 8, 4, 72, 8, 4, 1, 1, 0, 0), (0,)),                   # ... and of the (8, 4) filter
]

FWD_GROUPS = [("thin", FWD_THIN), ("tap reuse", FWD_HALO)] + [("cross %d" % i, [c]) for i, c in enumerate(FWD_CROSS)] + \
             [("model plan", FWD_MODEL)]
DGRAD_GROUPS = [("small C", DGRAD_SMALLC), ("tap reuse", DGRAD_HALO)] + [("cross %d" % i, [c]) for i, c in enumerate(DGRAD_CROSS)] + \
               [("model plan", DGRAD_MODEL)]
WGRAD_GROUPS = [("thin", WGRAD_THIN), ("generic", WGRAD_GENERIC)]


# ---- host model of the dispatch (what the source decides from the geometry; pointers from torch are 16-byte aligned) ----
def out_hw(geom):
    N, C, H, W, K, KH, KW, SH, SW, PH, PW = geom
    return S._out_hw(H, W, KH, KW, SH, SW, PH, PW)


def cdiv(a, b):
    return -(-a // b)


def split_class(s):
    return "1" if s == 1 else ("2-7" if s < 8 else "8+")


def clip_splits(kg, splits):
    """make_plan: the split count a forced one becomes"""
    nk = cdiv(max(kg, 1), BK)
    return cdiv(nk, cdiv(nk, splits))


def thin_filter(geom):
    N, C, H, W, K, KH, KW = geom[:7]
    return 1 <= K <= 4 and ((KH == 4 and KW == 4 and K == 1) or (KH == 3 and KW == 3))


def halo_geom(H, W):
    """(halo positions of a 128-pixel tile) or None"""
    if W < 4 or W > 64 or W & (W - 1):
        return None
    R = 128 // W
    if R <= H:
        if H % R:
            return None
        rows, imgs = R, 1
    else:
        if R % H:
            return None
        rows, imgs = H, R // H
    hp = imgs * (rows + 2) * (W + 2)
    return hp if hp <= 288 else None


def n_impl(fam, tile, rowsum=False):
    if fam == "wgrad":
        return 3 if tile == 0 else 2
    if fam == "dgrad" and tile == 1 and rowsum:
        return 2
    return 3 if tile <= 1 else 2


def fwd_route(geom):
    N, C, H, W, K, KH, KW, SH, SW, PH, PW = geom
    if thin_filter(geom):
        return "thin"
    if (KH, KW, SH, SW, PH, PW) == (3, 3, 1, 1, 1, 1) and C % BK == 0 and K >= 64 and halo_geom(H, W):
        return "tap reuse"
    return "generic"


def fwd_loader(geom):
    """field 12 of the kind-1 key: bmode * 2 + avec (fwd_generic); the test passes the KRSC copy whenever C % 16 == 0"""
    N, C, H, W, K, KH, KW, SH, SW, PH, PW = geom
    is1x1 = KH == 1 and KW == 1
    avec = (C * KH * KW) % 4 == 0
    if avec and is1x1 and (SH, SW, PH, PW) == (1, 1, 0, 0) and (H * W) % 4 == 0:
        return 5
    if avec and C % 16 == 0:
        return 3
    return 1 if avec else 0


def dgrad_classes(geom):
    """[(pixels, depth)] of the stride-parity classes (conv_dgrad.hip dgrad_classes)"""
    N, C, H, W, K, KH, KW, SH, SW, PH, PW = geom
    out = []
    for ah in range(SH):
        for aw in range(SW):
            r0, s0 = (ah + PH) % SH, (aw + PW) % SW
            nrh = cdiv(KH - r0, SH) if r0 < KH else 0
            nrw = cdiv(KW - s0, SW) if s0 < KW else 0
            hc = cdiv(H - ah, SH) if ah < H else 0
            wc = cdiv(W - aw, SW) if aw < W else 0
            out.append((N * hc * wc, K * nrh * nrw, nrh, nrw))
    return out


def dgrad_route(geom):
    N, C, H, W, K, KH, KW, SH, SW, PH, PW = geom
    P, Q = out_hw(geom)
    if C <= 4 and K * KH * KW * 16 <= 64 * 1024:
        few = C <= 3 and all(c[2] <= 4 and c[3] <= 4 for c in dgrad_classes(geom))
        return "small C four-pixel" if few else "small C plain"
    if (KH, KW, SH, SW, PH, PW) == (3, 3, 1, 1, 1, 1) and (P, Q) == (H, W) and K % BK == 0 and C % 4 == 0 and C >= 64 and halo_geom(H, W):
        return "tap reuse"
    return "generic"


def dgrad_mode(geom):
    """field 12 of the kind-2 key (dgrad_impl); the test passes the KRSC copy whenever C % 4 == 0"""
    N, C, H, W, K, KH, KW, SH, SW, PH, PW = geom
    P, Q = out_hw(geom)
    if C % 4:
        return 0
    if KH == 1 and KW == 1 and SH == 1 and SW == 1 and PH == 0 and PW == 0 and (P * Q) % 4 == 0:
        return 2
    return 1 if K % 16 == 0 else 0


def dgrad_depth(geom):
    """the depth the data-gradient GEMM is planned on: the deepest class (one class: K * KH * KW)"""
    return max(c[1] for c in dgrad_classes(geom))


def wgrad_regime(geom):
    """(loader key, tile, splits) of the generic weight gradient: wgrad_run_plan's key, plan_wgrad's plan"""
    N, C, H, W, K, KH, KW, SH, SW, PH, PW = geom
    P, Q = out_hw(geom)
    veca = (P * Q) % 4 == 0
    vec = veca and (KH, KW, SH, SW, PH, PW) == (1, 1, 1, 1, 0, 0)
    wshift = int(not vec and veca and SH == 1 and SW == 1 and PW <= 1 and KW <= PW + 2 and Q % 4 == 0 and W >= 4 and KH * KW > 1)
    key = (2 if (vec or wshift) else 0) + (1 if veca else 0) + 4 * wshift
    M, Ng, Kg = K, C * KH * KW, N * P * Q
    tile = 3 if M <= 32 else (2 if (M <= 64 or Ng <= 64) else 0)
    mn = cdiv(M, TILE_BM[tile]) * cdiv(Ng, TILE_BN[tile])
    nk = cdiv(Kg, BK)
    want = max(1, min(cdiv(1024, mn), nk // 16, 512))
    if want >= 8:
        w8 = (want + 4) // 8 * 8
        if w8 <= nk:
            return key, tile, w8
    return key, tile, cdiv(nk, cdiv(nk, want))


def wgrad_route(geom):
    return "thin" if thin_filter(geom) else "generic"


def wgrad_thin_form(geom):
    N, C, H, W, K, KH, KW, SH, SW, PH, PW = geom
    P, Q = out_hw(geom)
    px4 = (KH, KW, SH, SW) == (3, 3, 1, 1) and PH <= 1 and PW <= 1 and Q % 4 == 0 and Q + 2 - 2 * PW == W and (P * Q) % 4 == 0
    per = (cdiv(N * P * Q, max(1, min(cdiv(2048, C), N * P * Q // 512))) + 3) // 4 * 4
    return ("four-pixel" if px4 else "scalar"), cdiv(N * P * Q, per)


def modelled_regimes():
    """the regimes the tables reach according to the host model: generic kernels under a FORCED plan (forward, data gradient) or
    plan_wgrad's plan (weight gradient), and the two paths of each tap-reuse choice"""
    out = set()
    for _, cases in FWD_GROUPS:
        for geom, plans, epis in cases:
            route = fwd_route(geom)
            if route == "tap reuse":
                out |= {("fwd path", 0), ("fwd path", 1)}
            for tile, s in plans:
                if route == "generic" and tile >= 0:
                    kg = geom[1] * geom[5] * geom[6]
                    for impl in range(n_impl("fwd", tile)):
                        out.add(("fwd", fwd_loader(geom), tile, split_class(clip_splits(kg, s)), impl))
    for _, cases in DGRAD_GROUPS:
        for geom, plans, epis in cases:
            route = dgrad_route(geom)
            if route == "tap reuse":
                out |= {("dgrad path", 0), ("dgrad path", 1)}
            for tile, s in plans:
                if route == "generic" and tile >= 0:
                    strided = "strided" if geom[7] * geom[8] > 1 else "one class"
                    for impl in range(n_impl("dgrad", tile)):
                        out.add(("dgrad", dgrad_mode(geom), strided, tile, split_class(clip_splits(dgrad_depth(geom), s)), impl))
    for _, cases in WGRAD_GROUPS:
        for geom, folds in cases:
            if wgrad_route(geom) == "generic":
                key, tile, s = wgrad_regime(geom)
                for impl in range(n_impl("wgrad", tile)):
                    out.add(("wgrad", key, tile, split_class(s), impl))
    return out


# ---- the regimes this file claims ----
def _declared():
    d = {("fwd path", 0), ("fwd path", 1), ("dgrad path", 0), ("dgrad path", 1)}
    for tile in range(4):
        for sc in ("1", "2-7"):
            for impl in range(n_impl("fwd", tile)):
                d |= {("fwd", key, tile, sc, impl) for key in (0, 1, 3, 5)}            # every (bmode, avec) the loader can take
                d |= {("dgrad", mode, "one class", tile, sc, impl) for mode in (0, 1, 2)}
                d |= {("dgrad", mode, "strided", tile, sc, impl) for mode in (0, 1)}   # (mode 2 is one class by definition)
    for tile in (2, 3):                                                                # the (8, 4) filter, eight splits of 12 k-tiles
        d |= {("fwd", 3, tile, "8+", impl) for impl in range(2)}
    for key, tile, sc in ((0, 2, "1"), (1, 0, "1"), (1, 3, "2-7"), (1, 2, "8+"), (3, 2, "1"), (3, 0, "2-7"), (7, 2, "8+"),
                          (7, 2, "2-7"), (0, 3, "2-7"), (7, 0, "2-7")):
        d |= {("wgrad", key, tile, sc, impl) for impl in range(n_impl("wgrad", tile))}
    return d


DECLARED = _declared()
REACHED = {}                                        # regime -> worst ratio, filled by the tests below in file order


def regime_of(key, idx):
    """the regime a pick-log record (key, index run) stands for, or None (plan keys)"""
    kind = key[0]
    if kind == 1:
        return ("fwd", key[12], key[13], split_class(key[14]), idx)
    if kind == 2:
        return ("dgrad", key[12], "strided" if key[8] * key[9] > 1 else "one class", key[13], split_class(key[14]), idx)
    if kind == 4:
        return ("wgrad", key[12], key[13], split_class(key[14]), idx)
    if kind == 16:
        return ("fwd path", idx)
    if kind == 32:
        return ("dgrad path", idx)
    return None


def _lib():
    from rg_hip.lib import lib
    return lib


class _Pinned(object):
    """one test item: nothing pinned or forced before, every kind pinned inside (no choice is measured or recorded), released after;
    rg_conv_tune_stats unchanged"""

    def __init__(self, dev, fam, group):
        self.lib, self.dev, self.fam, self.group = _lib(), dev, fam, group

    def __enter__(self):
        lib = self.lib
        self.stats = lib.rg_conv_tune_stats(None)
        self.stream = torch.cuda.current_stream().cuda_stream
        self.sw = S._Sweep(lib)
        lib.rg_conv_pick_log(None, 0)
        self.was = [lib.rg_conv_set_pick(kind, 0) for kind in S.ALL_KINDS]
        return self

    def __exit__(self, et, ev, tb):
        lib = self.lib
        lib.rg_conv_set_force(-1, -1)
        for kind in S.ALL_KINDS:
            lib.rg_conv_set_pick(kind, -1)
        lib.rg_conv_pick_log(None, 0)
        torch.cuda.synchronize()
        if et is not None:
            return False
        sw = self.sw
        assert self.was == [-1] * len(S.ALL_KINDS), "a kind was pinned before the test: %s" % (self.was,)
        for (key, idx), ratio in sw.ran.items():
            r = regime_of(key, idx)
            if r is not None:
                REACHED[r] = max(REACHED.get(r, 0.0), ratio)
        worst = max(sw.worst.values()) if sw.worst else 0.0
        print("\nconv ragged %s / %s: %d calls, %d candidates, worst |out - ref| / tol %.4f" %
              (self.fam, self.group, sw.calls[self.fam], sw.count[self.fam], worst))
        for name in sorted(sw.worst):
            print("RATIO %s [%s] %s %.4f" % (self.fam, self.group, name, sw.worst[name]))
        assert not sw.bad, "%d candidates exceed the per-element bound:\n%s" % (len(sw.bad), "\n".join(sw.bad[:40]))
        assert lib.rg_conv_tune_stats(None) == self.stats, "a pinned run measured or recorded a choice"
        return False


def _direct(sw, route):
    """a direct kernel makes no logged choice: any record means a GEMM (or a path / plan choice) ran in its place"""
    assert not sw.recs, ("%s: the pick log holds %s" % (route, sorted(sw.recs)))


def _check_logged(sw, ran, fam, want_loader, tile, depth, splits, label):
    """the kernel records of one sweep ran the forced tile, the clipped split count and the modelled loader"""
    kind = {"fwd": 1, "dgrad": 2}[fam]
    seen = 0
    for recs in ran:
        for key, idx in recs:
            if key[0] != kind:
                continue
            seen += 1
            assert key[12] == want_loader, (label, "loader", key[12], want_loader)
            if tile >= 0:
                assert key[13] == tile, (label, "tile", key[13], tile)
                assert key[14] == clip_splits(depth, splits), (label, "splits", key[14], clip_splits(depth, splits))
    assert seen, (label, "no kernel record")


def _run_fwd(ctx, geom, plans, epis, gen):
    lib, dev, sw, stream = ctx.lib, ctx.dev, ctx.sw, ctx.stream
    N, C, H, W, K, KH, KW, SH, SW, PH, PW = geom
    P, Q = out_hw(geom)
    route = fwd_route(geom)
    x = torch.randn(N, C, H, W, device=dev, generator=gen)
    w = torch.randn(K, C, KH, KW, device=dev, generator=gen) / math.sqrt(C * KH * KW)
    wk = w.permute(0, 2, 3, 1).reshape(K, KH * KW, C).contiguous() if (KH * KW > 1 and C % 16 == 0) else None
    scale = torch.rand(K, device=dev, generator=gen) + 0.5
    shift = torch.randn(K, device=dev, generator=gen) * 0.1
    res = torch.randn(N, K, P, Q, device=dev, generator=gen)
    acc, acc_abs = S.ref_fwd(x.double(), w.double(), (SH, SW), (PH, PW))
    buf, y, guard = S._nan_buffer(N * K * P * Q, dev)
    y = y.view(N, K, P, Q)
    refs = {}
    for epi in epis:
        hs, hh, hr, act = EPI_F[epi]
        refs[epi] = S.ref_epilogue(acc, acc_abs, scale.double() if hs else None, shift.double() if hh else None,
                                   res.double() if hr else None, act)
    for tile, splits in plans:
        lib.rg_conv_set_force(tile, splits)
        ws = S._workspace(lib.rg_conv2d_fwd_workspace(N, C, K, KH, KW, P, Q), dev)       # follows the forced plan
        for epi in epis:
            hs, hh, hr, act = EPI_F[epi]
            ref, tol = refs[epi]
            label = "%s plan %s epi '%s'" % (geom, (tile, splits), epi)

            def launch():
                buf.fill_(math.nan)
                if ws is not None:
                    ws.fill_(math.nan)
                lib.rg_conv2d_fwd(x.data_ptr(), w.data_ptr(), None if wk is None else wk.data_ptr(), y.data_ptr(), N, C, H, W, K, KH,
                                  KW, SH, SW, PH, PW, P, Q, scale.data_ptr() if hs else None, shift.data_ptr() if hh else None,
                                  res.data_ptr() if hr else None, act, S.SLOPE, None if ws is None else ws.data_ptr(),
                                  0 if ws is None else ws.numel() * 4, stream)

            def check():
                if route == "thin":
                    _direct(sw, "forward thin %s" % (geom,))
                return {"fwd " + route: S._guard_ok(S._ratio(y, ref, tol), guard)}

            ran = sw.sweep("fwd", label, launch, check)
            if route != "thin":
                _check_logged(sw, ran, "fwd", fwd_loader(geom), tile, C * KH * KW, splits, label)
            if route == "tap reuse":
                assert {idx for recs in ran for key, idx in recs if key[0] == 16} == {0, 1}, (label, "tap reuse and generic")


def _run_dgrad(ctx, geom, plans, epis, gen):
    lib, dev, sw, stream = ctx.lib, ctx.dev, ctx.sw, ctx.stream
    N, C, H, W, K, KH, KW, SH, SW, PH, PW = geom
    P, Q = out_hw(geom)
    route = dgrad_route(geom)
    dy = torch.randn(N, K, P, Q, device=dev, generator=gen)
    w = torch.randn(K, C, KH, KW, device=dev, generator=gen) / math.sqrt(K * KH * KW)
    wk = w.permute(0, 2, 3, 1).reshape(K, KH * KW, C).contiguous() if (KH * KW > 1 and C % 4 == 0) else None
    scale = torch.rand(C, device=dev, generator=gen) + 0.5
    shift = torch.randn(C, device=dev, generator=gen) * 0.1
    res = torch.randn(N, C, H, W, device=dev, generator=gen)
    mask = torch.randn(N, C, H, W, device=dev, generator=gen)
    acc, acc_abs = S.ref_dgrad(dy.double(), w.double(), (H, W), (SH, SW), (PH, PW))
    buf, dx, guard = S._nan_buffer(N * C * H * W, dev)
    dx = dx.view(N, C, H, W)
    refs = {}
    for epi in epis:
        hs, hh, hr, hm, want_rs, act = EPI_D[epi]
        ref, tol = S.ref_epilogue(acc, acc_abs, scale.double() if hs else None, shift.double() if hh else None,
                                  res.double() if hr else None, act, mask=mask if hm else None)
        refs[epi] = (ref, tol) + S.ref_rowsum(ref, tol)
    rowsum_runs = 0
    for tile, splits in plans:
        lib.rg_conv_set_force(tile, splits)
        ws = S._workspace(lib.rg_conv2d_dgrad_workspace(N, C, H, W, K, KH, KW, SH, SW), dev)      # follows the forced plan
        cols = lib.rg_conv2d_dgrad_rowsum_cols(N, C, H, W, K, KH, KW, SH, SW, PH, PW, P, Q)       # ... and so do the row-sum columns
        for epi in epis:
            hs, hh, hr, hm, want_rs, act = EPI_D[epi]
            if want_rs and cols <= 0:
                continue                      # a split plan has no fused row sums (the query says so): nothing to launch
            ref, tol, rs_ref, rs_tol = refs[epi]
            rs = torch.empty(C, cols, dtype=torch.float32, device=dev) if want_rs else None
            rowsum_runs += 1 if want_rs else 0
            label = "%s plan %s epi '%s'" % (geom, (tile, splits), epi)

            def launch():
                buf.fill_(math.nan)
                if ws is not None:
                    ws.fill_(math.nan)
                if rs is not None:
                    rs.fill_(math.nan)
                lib.rg_conv2d_dgrad(dy.data_ptr(), w.data_ptr(), None if wk is None else wk.data_ptr(), dx.data_ptr(), N, C, H, W, K, KH,
                                    KW, SH, SW, PH, PW, P, Q, scale.data_ptr() if hs else None, shift.data_ptr() if hh else None,
                                    res.data_ptr() if hr else None, act, S.SLOPE, mask.data_ptr() if hm else None,
                                    None if rs is None else rs.data_ptr(), cols if want_rs else 0,
                                    None if ws is None else ws.data_ptr(), 0 if ws is None else ws.numel() * 4, stream)

            def check():
                if route.startswith("small C"):
                    _direct(sw, "data gradient %s %s" % (route, geom,))
                out = {"dgrad " + route: S._guard_ok(S._ratio(dx, ref, tol), guard)}
                if rs is not None:
                    out["dgrad row sums"] = S._ratio(rs.double().sum(1), rs_ref, rs_tol)
                return out

            ran = sw.sweep("dgrad", label, launch, check)
            if route == "generic":
                _check_logged(sw, ran, "dgrad", dgrad_mode(geom), tile, dgrad_depth(geom), 1 if want_rs else splits, label)
            if want_rs:
                assert all(key[14] == 1 for recs in ran for key, idx in recs if key[0] == 2), (label, "row sums from a split launch")
    return rowsum_runs


def _run_wgrad(ctx, geom, folds, gen):
    lib, dev, sw, stream = ctx.lib, ctx.dev, ctx.sw, ctx.stream
    N, C, H, W, K, KH, KW, SH, SW, PH, PW = geom
    P, Q = out_hw(geom)
    route = wgrad_route(geom)
    x = torch.randn(N, C, H, W, device=dev, generator=gen)
    dy = torch.randn(N, K, P, Q, device=dev, generator=gen) / math.sqrt(N * P * Q)
    G, G_abs = S.ref_wgrad(x.double(), dy.double(), (KH, KW), (SH, SW), (PH, PW))
    ws = S._workspace(lib.rg_conv2d_wgrad_workspace(N, C, K, KH, KW, P, Q), dev)
    buf, dw, guard = S._nan_buffer(K * C * KH * KW, dev)
    dw = dw.view(K, C, KH, KW)
    nsl = 8
    wf = torch.randn(K, C, KH, KW, device=dev, generator=gen) / math.sqrt(C * KH * KW)
    scale = torch.rand(K, device=dev, generator=gen) + 0.5
    invstd = torch.rand(K, device=dev, generator=gen) + 0.5
    mean = torch.randn(K, device=dev, generator=gen) * 0.3
    partials = torch.randn(K, nsl, device=dev, generator=gen)
    sum_g = torch.randn(K, device=dev, generator=gen)
    dgamma = torch.empty(K, dtype=torch.float32, device=dev)
    dbeta = torch.empty(K, dtype=torch.float32, device=dev)
    for fold in folds:
        label = "%s fold %d" % (geom, fold)
        if fold:
            want = S.ref_fold(G, G_abs, wf.double(), scale.double(), invstd.double(), mean.double(),
                              partials=partials.double() if fold == 1 else None, sum_g=sum_g.double() if fold == 2 else None)
        else:
            want = {"wgrad": (G, G_abs * S.TOL + S.TINY)}

        def launch():
            buf.fill_(math.nan)
            ws.fill_(math.nan)
            dgamma.fill_(math.nan)
            dbeta.fill_(math.nan)
            if not fold:
                lib.rg_conv2d_wgrad(x.data_ptr(), dy.data_ptr(), dw.data_ptr(), N, C, H, W, K, KH, KW, SH, SW, PH, PW, P, Q,
                                    ws.data_ptr(), ws.numel() * 4, stream)
            else:
                lib.rg_conv2d_wgrad_fold(x.data_ptr(), dy.data_ptr(), dw.data_ptr(), N, C, H, W, K, KH, KW, SH, SW, PH, PW, P, Q,
                                         wf.data_ptr(), scale.data_ptr(), invstd.data_ptr(), mean.data_ptr(),
                                         sum_g.data_ptr() if fold == 2 else None, partials.data_ptr() if fold == 1 else None,
                                         nsl if fold == 1 else 0, dbeta.data_ptr() if fold == 1 else None, dgamma.data_ptr(),
                                         ws.data_ptr(), ws.numel() * 4, stream)

        def check():
            if route == "thin":
                _direct(sw, "weight gradient thin %s" % (geom,))
            out = {}
            for name, (ref, tol) in want.items():
                got = {"wgrad": dw, "wgrad fold dgamma": dgamma, "wgrad fold dbeta": dbeta}[name]
                r = S._ratio(got, ref, tol)
                out[name + (" thin" if route == "thin" else "")] = S._guard_ok(r, guard) if name == "wgrad" else r
            return out

        ran = sw.sweep("wgrad", label, launch, check)
        if route == "generic":
            key, tile, splits = wgrad_regime(geom)
            got = {(k[12], k[13], k[14]) for recs in ran for k, idx in recs if k[0] == 4}
            assert got == {(key, tile, splits)}, (label, got, (key, tile, splits))


@pytest.mark.parametrize("group", [g for g, _ in FWD_GROUPS])
def test_forward_every_candidate_at_ragged_geometries(dev, group):
    cases = dict(FWD_GROUPS)[group]
    with _Pinned(dev, "fwd", group) as ctx:
        for i, (geom, plans, epis) in enumerate(cases):
            _run_fwd(ctx, geom, plans, epis, torch.Generator(device=dev).manual_seed(2000 + 16 * len(group) + i))


@pytest.mark.parametrize("group", [g for g, _ in DGRAD_GROUPS])
def test_data_gradient_every_candidate_at_ragged_geometries(dev, group):
    cases = dict(DGRAD_GROUPS)[group]
    with _Pinned(dev, "dgrad", group) as ctx:
        rowsum_runs = 0
        for i, (geom, plans, epis) in enumerate(cases):
            rowsum_runs += _run_dgrad(ctx, geom, plans, epis, torch.Generator(device=dev).manual_seed(3000 + 16 * len(group) + i))
        if group != "small C":                  # (the small-C kernels have no fused row sums: their query reports 0 columns)
            assert rowsum_runs > 0, "no launch of the group wrote fused row sums"


@pytest.mark.parametrize("group", [g for g, _ in WGRAD_GROUPS])
def test_weight_gradient_every_candidate_at_ragged_geometries(dev, group):
    cases = dict(WGRAD_GROUPS)[group]
    with _Pinned(dev, "wgrad", group) as ctx:
        for i, (geom, folds) in enumerate(cases):
            _run_wgrad(ctx, geom, folds, torch.Generator(device=dev).manual_seed(4000 + 16 * len(group) + i))


def test_declared_regimes_were_reached(dev):
    """runs after the sweeps of this file (file order): what rg_conv_pick_log reported covers DECLARED, and nothing stayed pinned"""
    lib = _lib()
    for kind in S.ALL_KINDS:
        was = lib.rg_conv_set_pick(kind, -1)
        assert was == -1, "kind %d was left pinned at %d" % (kind, was)
    for r in sorted(REACHED, key=str):
        print("RATIO regime %s %.4f" % (" ".join(str(v) for v in r), REACHED[r]))
    missing = sorted(DECLARED - set(REACHED), key=str)
    assert not missing, "%d declared regimes were not reached: %s" % (len(missing), missing[:20])
