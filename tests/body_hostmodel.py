"""Host model of the units that run between the convolutions — csrc/eltwise.hip, csrc/gan_extra.hip, csrc/bgemm.hip,
csrc/resize.hip, csrc/retrieval.hip — the comparison partner of tests/test_body_elementwise_gpu.py, tied to float32 torch by
tests/test_body_hostmodel_cpu.py.  No tests and no GPU here.  Ref, compare, check, exact, f32, family and gen are those of
tests/head_hostmodel.py; the kinds and their constants below are this module's own.

Three parts:

  dispatch mirrors   the two grid_for caps (4096 eltwise, 8192 gan_extra / resize / retrieval) and trips; the float4 / tail
                     split of act_fwd, act_bwd and axpby; the rg_pair_cat chunk rule; the PX choice of rg_l2norm_channels_*;
                     the vector-route predicate of rg_reflection_pad2d_* with its pointer terms; make_paddiv / pdiv in Python
                     integers; the spectral-norm limits, batch size and backward kernel switch; the bgemm tile and load
                     mappings; the wave-per-row launches.  The case lists are BUILT from them.
  fp64 references    every entry point of the five files except rg_fill and rg_spin_us, taking the float32 tensors the C ABI
                     takes; each backward takes the forward outputs it is handed (y, norm, p, sigma, u, v, w_sn).
  error budgets      Ref(value, M, kind); an element passes when |got - value| <= C_KIND[kind] * 2^-24 * (M + 2^-102), M the
                     fp64 sum of the absolute values of the terms THAT element is made of, plus a condition term where the
                     formula is ill-conditioned:
                         ew           a short chain of products and sums: sum of |term| (axpby, sub_square, mix_rows, the
                                      avgpool backward, add_outer_terms); (a - b)^2 counts d^2 + 2 |d| (|a| + |b|)
                         sum          sum / mean of |term| (avgpool, reflection-pad backward, row_sqsum); segment_mean, a
                                      serial sum of any length: (sum |x_j| + sum_j |S_j|) / n with S_j the partial sums in
                                      list order (each addition rounds relative to its partial sum) — and, on the device,
                                      exactly the float32 model that adds in list order
                         tanh         forward |y| + |x| (1 - y^2); backward |dy| (1 + y^2): 1 - y^2 cancels near |y| = 1
                         norm         y: 3 |y| (the division by a rounded norm: the sum of squares, the root, the quotient);
                                      norm: its own value
                         norm_bwd     (|dy| + |y| (|k| + sum |y dy|)) / max(norm, eps) + |dx|, k the projection <y, dy>
                         softmax      p (3 + |z| + |z - max| + sum_j p_j (|z_j| + |z_j - max|)), z = scale x: the exponent
                                      carries the rounding of z and of the difference, the denominator their average
                         softmax_bwd  |scale| p (|dp| + |dot| + sum |p dp|) + 2 |ds|
                         bicubic      per axis the weight matrix A and its error proxy E = sum over the taps of (|monomials|
                                      of the Horner form + |dc/dt| (|r| + 2)): the coefficient polynomials are evaluated at a
                                      t = r - floor(r) that carries the rounding of the source coordinate r (a fused or
                                      unfused scale * (o + 0.5) - 0.5; the interpolant is continuous across a floor that
                                      falls the other way).  Output: 2 |Ay||x||Ax| + Ey |x| |Ax| + |Ay| |x| Ex, then
                                      (that + |v| + |mean|) / |std| + |result|; the backward likewise with |dy|
                         sn           the power-iteration chain, each link inheriting the one before: t = W^T u: sum |W u|;
                                      v = t / max(|t|, eps): Mt / den + |v| (2 + sum(Mt |t|) / |t|^2); s = W v: sum |W| (|v| +
                                      Mv); u' likewise from s; sigma = u'.s: sum (Mu |s| + |u'| Ms + |u' s|); 1 / sigma:
                                      Msigma / sigma^2 + 1 / |sigma|; w_sn: |W| M(1 / sigma) + |w_sn|
                         sn_bwd       (|dw_sn| + (|c| + sum_{K M} |dw_sn w_sn|) |u v|) |1 / sigma| + |result| (+ |dw| when
                                      accumulating), c the dot product over all K * M terms
                         gemm         |alpha| sum_k |a b| + |beta c|; an element outside the written range: its old value, M = 0
                         exact        M = 0: a copy, a selection, an untouched element or ONE correctly rounded float32
                                      operation, modelled in float32 — ReLU / LeakyReLU and their backward (x * slope, dy *
                                      slope), pair_cat, copy_channels (with accumulate: one rounded sum), reflection-pad
                                      forward, the dropout mask, its zeros and the kept x * (1.f / (1.f - p)) (the library is
                                      built without fast-math: the reciprocal and the product are each correctly rounded),
                                      top-k indices and values, the eval-mode u, v and uv_saved

Contracts taken from the reference (torch): ReLU / LeakyReLU / tanh with the backward through the OUTPUT y (negative branch at
y == 0 and y == -0.0); F.normalize with clamp_min's gradient (passes at norm >= eps, a zero row gets dy / eps); F.avg_pool2d in
floor mode (zero gradient in the ragged rim); F.pad(mode='reflect'); F.interpolate(mode='bicubic', align_corners=False), A =
-0.75, clamped taps, source coordinate in float32; torch.nn.utils.spectral_norm with one power iteration; faiss order for top-k
(value descending, index ascending, -0.0 == 0.0, +-inf ordinary values); segment members added in list order; a mixed row that
is both idx_a[j] and idx_b[j] gets both terms; the dropout mask of oracle.ref_torch.dropout_keep_mask with the clocked seed
seed + 0xD1B54A32D192ED03 * clock mod 2^64.

The constants are NOT taken from the kernels: tests/test_body_hostmodel_cpu.py evaluates every case with plain float32 torch on
the CPU and C_KIND = max(8, 4 x ratio).  Measured (torch 2.10, CPU, one thread):

    kind          float32 torch ratio    C_KIND
    ew            2.04                   8.15
    sum           2.37                   9.49
    tanh          1.46                   8
    norm          3.20                   12.79
    norm_bwd      2.52                   10.09
    softmax       0.62                   8
    softmax_bwd   0.72                   8
    bicubic       0.50                   8
    sn            1.26                   8
    sn_bwd        1.40                   8
    gemm          6.58                   26.32
    exact         0                      0

The larger ratios are torch's own summation order: `gemm` is driven by the `offset` family at K = 33 (33 products of one sign
added serially round the same way every time), `norm` by the 2051-element rows of the `constant` family.
"""
import collections
import math

import torch

from oracle import ref_torch
from tests.head_hostmodel import FILL, TINY_M, U24, Ref, Worst, cdiv, exact, f32, family, gen  # noqa: F401
from tests.head_hostmodel import compare as _compare

C_KIND = {"ew": 8.15, "sum": 9.49, "tanh": 8.0, "norm": 12.79, "norm_bwd": 10.09, "softmax": 8.0, "softmax_bwd": 8.0, "bicubic": 8.0,
          "sn": 8.0, "sn_bwd": 8.0, "gemm": 26.32, "exact": 0.0}

ACT_NONE, ACT_RELU, ACT_LEAKY, ACT_TANH = 0, 1, 2, 3
ACTS = (ACT_NONE, ACT_RELU, ACT_LEAKY, ACT_TANH)
M64 = (1 << 64) - 1
CLOCK_MUL = 0xD1B54A32D192ED03


def compare(got, ref):
    return _compare(got, ref, C_KIND)


def check(got, ref, what):
    w = compare(got, ref)
    assert w.ok, "%s: worst element %s err %.3e > budget %.3e (%s, max err/(2^-24 M) = %.2f)" % (
        what, w.index, w.err, w.budget, ref.kind, w.ratio)
    return w.ratio


def _d(t):
    return None if t is None else t.detach().double()


def _s32(v):
    return torch.tensor(float(v), dtype=torch.float32)


# ---- dispatch mirrors --------------------------------------------------------------------------------------------------------
GRID_CAP = {"eltwise": 4096, "gan": 8192, "resize": 8192, "retrieval": 8192}


def grid_for(unit, items):
    return max(1, min(cdiv(items, 256), GRID_CAP[unit]))


def trips(unit, items):
    return cdiv(items, grid_for(unit, items) * 256)


def vec_split(n):
    """act_fwd / act_bwd / axpby: (float4 units, tail elements, workgroups); the grid is grid_for(n / 4 + 1)"""
    return n >> 2, n & 3, grid_for("eltwise", n // 4 + 1)


def vec_trips(n):
    nv, _, g = vec_split(n)
    return cdiv(nv, g * 256)


def pair_cat_launch(per):
    """rg_pair_cat: (vector route, chunks = gridDim.x, trips of a thread)"""
    vec = (per & 3) == 0
    units = per // 4 if vec else per
    chunks = max(1, min(1024, cdiv(units, 1024)))
    return vec, chunks, cdiv(units, chunks * 256)


def l2c_px(N, HW):
    """rg_l2norm_channels_*: pixels per workgroup; 256 / PX channel groups"""
    return 64 if cdiv(HW, 64) * N >= 1024 else 16


def pad_vec_route(W, pad, *addrs):
    """rg_reflection_pad2d_fwd (addrs: x) / _bwd (addrs: dx, x_act or 0): the float4 kernels"""
    a = 0
    for v in addrs:
        a |= v
    return (W & 3) == 0 and pad <= 3 and W >= 8 and (a & 15) == 0


PadDiv = collections.namedtuple("PadDiv", "mul shr d")


def make_paddiv(d):
    d = d if d else 1
    if d == 1:
        return PadDiv(0, 0, 1)
    l = 0
    while (1 << l) < d:
        l += 1
    p = 31 + l
    return PadDiv((((1 << p) + d - 1) // d) & 0xFFFFFFFF, p - 32, d)


def pdiv(n, f):
    return n if f.d == 1 else ((n * f.mul) >> 32) >> f.shr


SN_SINGLE_MAX, SN_SLICES, SN_MAX_M, SN_MAX_K, SN_MAX_BATCH, SN_THREADS = 16384, 64, 12288, 1024, 16, 1024


def sn_bwd_kernel(K, M):
    return "sliced" if K * M > SN_SINGLE_MAX else "single"


def sn_slice_per(n):
    return cdiv(n, SN_SLICES)


def sn_workspace(K, M):
    return SN_SLICES * 4 if K * M > SN_SINGLE_MAX else 0


def sn_row_trips(K):
    """rows of W v per wave: 16 waves"""
    return cdiv(K, SN_THREADS // 64)


TB, TK = 64, 16


def bgemm_launch(M, N, K, a_ms, b_ns):
    """(tiles m, tiles n, k tiles, a_rc, b_rc)"""
    return cdiv(M, TB), cdiv(N, TB), cdiv(K, TK), a_ms == 1, b_ns == 1


def wave_rows(rows):
    """softmax_rows / row_sqsum: (workgroups, waves of the last one that have a row)"""
    return cdiv(rows, 4), (rows - 1) % 4 + 1


# ---- eltwise.hip ---------------------------------------------------------------------------------------------------------------
def act_fwd(x, act, slope=0.0):
    if act == ACT_NONE:
        return exact(x)
    if act == ACT_RELU:
        return exact(torch.where(x > 0, x, torch.zeros_like(x)))
    if act == ACT_LEAKY:
        return exact(torch.where(x > 0, x, x * _s32(slope)))
    xd = _d(x)
    y = torch.tanh(xd)
    return Ref(y, y.abs() + torch.where(torch.isfinite(xd), xd.abs() * (1.0 - y * y), torch.zeros_like(y)), "tanh")


def act_bwd(dy, y, act, slope=0.0):
    """through the forward OUTPUT y; ReLU / leaky take the negative branch at y == 0 and y == -0.0"""
    if act == ACT_NONE:
        return exact(dy)
    if act == ACT_RELU:
        return exact(torch.where(y > 0, dy, dy * _s32(0.0)))
    if act == ACT_LEAKY:
        return exact(torch.where(y > 0, dy, dy * _s32(slope)))
    gd, yd = _d(dy), _d(y)
    return Ref(gd * (1.0 - yd * yd), gd.abs() * (1.0 + yd * yd), "tanh")


def axpby(a, b, alpha, beta):
    al, be = f32(alpha), f32(beta)
    v = al * _d(a)
    if b is None:
        return Ref(v, v.abs(), "ew")
    return Ref(v + be * _d(b), v.abs() + (be * _d(b)).abs(), "ew")


def sub_square_fwd(a, b):
    ad, bd = _d(a), _d(b)
    d = ad - bd
    return Ref(d * d, d * d + 2.0 * d.abs() * (ad.abs() + bd.abs()), "ew")


def sub_square_bwd(a, b, dy):
    ad, bd, g = _d(a), _d(b), _d(dy)
    v = 2.0 * (ad - bd) * g
    M = 2.0 * (ad.abs() + bd.abs()) * g.abs()
    return Ref(v, M, "ew"), Ref(-v, M, "ew")


def pair_cat(a, b, take_a):
    """out[:B] = a, out[B:][i] = take_a[i] ? a[i] : b[i]"""
    B = a.shape[0]
    t = torch.zeros(B, dtype=torch.bool) if take_a is None else take_a != 0
    second = torch.where(t.reshape([B] + [1] * (a.dim() - 1)), a, b)
    return exact(torch.cat([a, second]))


def dropout_seed(seed, clock=None):
    return seed & M64 if clock is None else (seed + CLOCK_MUL * clock) & M64


def dropout(x, p, seed, clock=None, strict=False):
    """(y, keep): keep iff hash >= thr (strict: the mutant with >), kept x * (1.f / (1.f - p)) in float32"""
    n = x.numel()
    s = dropout_seed(seed, clock)
    keep = ref_torch.dropout_keep_mask(n, p, s).reshape(x.shape)
    if strict:
        keep = keep & ~dropout_at_threshold(n, p, s).reshape(x.shape)
    sc = _s32(1.0) / (_s32(1.0) - _s32(p))
    return exact(torch.where(keep, x * sc, torch.zeros_like(x))), keep


def dropout_hash(n, seed):
    import numpy as np
    idx = np.arange(n, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = (np.uint64((seed * 0x100000001B3) & M64) + idx) + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return (z >> np.uint64(32)).astype(np.int64)


def dropout_at_threshold(n, p, seed):
    thr = int(min(float(_s32(p)) * 4294967296.0, 4294967295.0))
    return torch.from_numpy(dropout_hash(n, seed) == thr)


def l2norm_fwd(x, eps, dim=1):
    """F.normalize(x, dim): (y, norm); rows: [rows, D], channels: [N, C, HW]"""
    e = f32(eps)
    xd = _d(x)
    nr = xd.pow(2).sum(dim, keepdim=True).sqrt()
    y = xd / nr.clamp_min(e)
    nr = nr.squeeze(dim)
    return Ref(y, 3.0 * y.abs(), "norm"), Ref(nr, nr.clone(), "norm")


def l2norm_bwd(y, dy, norm, eps, dim=1, strict=False):
    """dx = (dy - y <y, dy> [norm >= eps]) / max(norm, eps) from the y and norm it is handed.  strict: the mutant `norm > eps`"""
    e = f32(eps)
    yd, gd, nr = _d(y), _d(dy), _d(norm).unsqueeze(dim)
    dot = (yd * gd).sum(dim, keepdim=True)
    Md = (yd * gd).abs().sum(dim, keepdim=True)
    on = (nr > e) if strict else (nr >= e)
    k = torch.where(on, dot, torch.zeros_like(dot))
    Mk = torch.where(on, Md + dot.abs(), torch.zeros_like(dot))
    inv = 1.0 / nr.clamp_min(e)
    v = (gd - yd * k) * inv
    return Ref(v, (gd.abs() + yd.abs() * Mk) * inv + v.abs(), "norm_bwd")


def copy_channels(src, dst, Cc, sc0, dc0, accumulate):
    """float32 model: dst[:, dc0:dc0 + Cc] (+)= src[:, sc0:sc0 + Cc]; everything else as it was"""
    out = dst.clone()
    s = src[:, sc0:sc0 + Cc]
    out[:, dc0:dc0 + Cc] = out[:, dc0:dc0 + Cc] + s if accumulate else s
    return exact(out)


def mix_rows_fwd(src, ia, ib, lam):
    l, l1 = f32(lam), float(_s32(1.0) - _s32(lam))
    R = src.shape[0]
    s = _d(src).reshape(R, -1)
    a, b = l * s[ia], l1 * s[ib]
    return Ref(a + b, a.abs() + b.abs(), "ew")


def mix_rows_bwd(g, ia, ib, lam, rows_src, once=False):
    """dsrc[r] = sum_j lam g[j] [ia[j] == r] + (1 - lam) g[j] [ib[j] == r].  once: the mutant that counts a row that is both
    ia[j] and ib[j] once"""
    l, l1 = f32(lam), float(_s32(1.0) - _s32(lam))
    n = ia.numel()
    gd = _d(g).reshape(n, -1)
    v = torch.zeros(rows_src, gd.shape[1], dtype=torch.float64)
    M = torch.zeros_like(v)
    for j in range(n):
        a, b = int(ia[j]), int(ib[j])
        v[a] += l * gd[j]
        M[a] += (l * gd[j]).abs()
        if not (once and a == b):
            v[b] += l1 * gd[j]
            M[b] += (l1 * gd[j]).abs()
    return Ref(v, M, "ew")


# ---- gan_extra.hip -------------------------------------------------------------------------------------------------------------
def avgpool_fwd(x, k):
    N, C, H, W = x.shape
    P, Q = H // k, W // k
    xd = _d(x)[:, :, :P * k, :Q * k].reshape(N, C, P, k, Q, k)
    return Ref(xd.mean((3, 5)), xd.abs().mean((3, 5)), "sum")


def avgpool_bwd(dy, H, W, k, rim=0.0):
    """the adjoint of the floor-mode pool: zero in the ragged rim (rim: the mutant's value there)"""
    N, C, P, Q = dy.shape
    v = torch.full((N, C, H, W), float(rim), dtype=torch.float64)
    M = torch.zeros_like(v)
    t = _d(dy).repeat_interleave(k, 2).repeat_interleave(k, 3) / (k * k)
    v[:, :, :P * k, :Q * k] = t
    M[:, :, :P * k, :Q * k] = t.abs()
    return Ref(v, M, "ew")


def reflect_index(n, pad, shift=0):
    """input index of every padded position (shift: the mutant whose left mirror is off by one)"""
    i = torch.arange(-pad, n + pad)
    m = torch.where(i < 0, -i + shift, i)
    m = torch.where(m >= n, 2 * (n - 1) - m, m)
    return m.clamp(0, n - 1)


def reflection_pad_fwd(x, pad, act=ACT_NONE, slope=0.0, shift=0):
    H, W = x.shape[2:]
    a = act_fwd(x, act, slope).value
    return exact(a[:, :, reflect_index(H, pad)][:, :, :, reflect_index(W, pad, shift)])


def reflection_pad_bwd(dy, H, W, pad, x_act=None, act=ACT_NONE, slope=0.0):
    N, C = dy.shape[:2]
    g = _d(dy)
    ih, iw = reflect_index(H, pad), reflect_index(W, pad)

    def adj(t):
        t = torch.zeros(N, C, H, t.shape[3], dtype=torch.float64).index_add_(2, ih, t)
        return torch.zeros(N, C, H, W, dtype=torch.float64).index_add_(3, iw, t)
    v, M = adj(g), adj(g.abs())
    if act != ACT_NONE:
        gr = torch.where(x_act > 0, torch.ones_like(x_act), torch.full_like(x_act, slope if act == ACT_LEAKY else 0.0)).double()
        v, M = v * gr, M * gr.abs()
    return Ref(v, M, "sum")


def _normalise(t, Mt, e):
    """t / max(|t|, eps) with the error proxy of the quotient"""
    n = t.pow(2).sum().sqrt()
    den = n.clamp_min(e)
    out = t / den
    rel = float((Mt * t.abs()).sum() / (n * n)) if float(n) > 0 else 0.0
    return out, Mt / den + out.abs() * (2.0 + rel)


def spectral_norm_fwd(w, u, v, training, eps, old_u=False):
    """{u, v, sigma [2], w_sn, uv_saved [K + M]} of one forward on W[K][M].  old_u: the mutant sigma = u_old . (W v)"""
    e = f32(eps)
    K = w.shape[0]
    W = _d(w).reshape(K, -1)
    ud, vd = _d(u).reshape(-1), _d(v).reshape(-1)
    if training:
        t = W.t() @ ud
        v2, Mv = _normalise(t, W.abs().t() @ ud.abs(), e)
        s = W @ v2
        Ms = W.abs() @ (v2.abs() + Mv)
        u2, Mu = _normalise(s, Ms, e)
        if old_u:
            u2 = ud
        sigma = (u2 * s).sum()
        Msig = (Mu * s.abs() + u2.abs() * Ms + (u2 * s).abs()).sum()
        ru, rv = Ref(u2, Mu, "sn"), Ref(v2, Mv, "sn")
        saved = Ref(torch.cat([u2, v2]), torch.cat([Mu, Mv]), "sn")
    else:
        s = W @ vd
        Ms = W.abs() @ vd.abs() * 2.0
        sigma = (ud * s).sum()
        Msig = (ud.abs() * Ms + (ud * s).abs()).sum()
        ru, rv, saved = exact(ud), exact(vd), exact(torch.cat([ud, vd]))
    inv = 1.0 / sigma
    Minv = Msig / (sigma * sigma) + inv.abs()
    wsn = W * inv
    return {"u": ru, "v": rv, "sigma": Ref(torch.stack([sigma, inv]), torch.stack([Msig, Minv]), "sn"),
            "w_sn": Ref(wsn.reshape(w.shape), (W.abs() * Minv + wsn.abs()).reshape(w.shape), "sn"), "uv_saved": saved}


def spectral_norm_bwd(dwsn, wsn, u, v, sigma, dw_old=None):
    """dW (+)= (dWsn - (sum dWsn Wsn) u v^T) * sigma[1]"""
    K = wsn.shape[0]
    G, Wn = _d(dwsn).reshape(K, -1), _d(wsn).reshape(K, -1)
    c = (G * Wn).sum()
    Mc = (G * Wn).abs().sum()
    uv = torch.outer(_d(u).reshape(-1), _d(v).reshape(-1))
    inv = float(sigma[1])
    val = (G - c * uv) * inv
    M = (G.abs() + (c.abs() + Mc) * uv.abs()) * abs(inv) + val.abs()
    if dw_old is not None:
        val = val + _d(dw_old).reshape(K, -1)
        M = M + _d(dw_old).reshape(K, -1).abs() + val.abs()
    return Ref(val.reshape(wsn.shape), M.reshape(wsn.shape), "sn_bwd")


# ---- bgemm.hip -----------------------------------------------------------------------------------------------------------------
def bgemm(A, B, C, M, N, K, a_str, b_str, c_str, batch, a_b, b_b, c_b, alpha, beta, variant=None):
    """alpha * A B + beta * C over arbitrary element strides; A, B, C are the base buffers (flat).  With beta == 0 C is not
    read.  Elements of C no (b0, b1, m, n) addresses keep their value (M = 0).  variant: mutants 'beta_on_sum' (beta *
    (alpha acc + C)) and 'drop_last_k' (the last k tile missing)"""
    al, be = f32(alpha), f32(beta)
    Af, Bf = _d(A).reshape(-1), _d(B).reshape(-1)
    out = _d(C).reshape(-1).clone()
    Mo = torch.zeros_like(out)
    m, n, k = torch.arange(M), torch.arange(N), torch.arange(K)
    if variant == "drop_last_k":
        k = k[:(cdiv(K, TK) - 1) * TK]
    for b0 in range(batch[0]):
        for b1 in range(batch[1]):
            Am = Af[b0 * a_b[0] + b1 * a_b[1] + m[:, None] * a_str[0] + k[None, :] * a_str[1]]
            Bm = Bf[b0 * b_b[0] + b1 * b_b[1] + k[:, None] * b_str[0] + n[None, :] * b_str[1]]
            ci = b0 * c_b[0] + b1 * c_b[1] + m[:, None] * c_str[0] + n[None, :] * c_str[1]
            acc, Ma = Am @ Bm, Am.abs() @ Bm.abs()
            if be != 0.0:
                old = out[ci]
                val = be * (al * acc + old) if variant == "beta_on_sum" else al * acc + be * old
                out[ci], Mo[ci] = val, abs(al) * Ma + (be * old).abs()
            else:
                out[ci], Mo[ci] = al * acc, abs(al) * Ma
    return Ref(out.reshape(C.shape), Mo.reshape(C.shape), "gemm")


def softmax_fwd(x, scale):
    z = _d(x) * f32(scale)
    mx = z.max(1, keepdim=True).values
    p = torch.softmax(z, 1)
    c = z.abs() + (z - mx).abs()
    return Ref(p, p * (3.0 + c + (p * c).sum(1, keepdim=True)), "softmax")


def softmax_bwd(p, dp, scale, no_scale=False):
    """ds = scale p (dp - sum p dp) from the p it is handed.  no_scale: the mutant without `scale`"""
    sc = 1.0 if no_scale else f32(scale)
    pd, gd = _d(p), _d(dp)
    dot = (pd * gd).sum(1, keepdim=True)
    Md = (pd * gd).abs().sum(1, keepdim=True)
    v = sc * pd * (gd - dot)
    return Ref(v, abs(sc) * pd * (gd.abs() + dot.abs() + Md) + 2.0 * v.abs(), "softmax_bwd")


# ---- resize.hip ----------------------------------------------------------------------------------------------------------------
CUBIC_A = -0.75


def _c1(x):
    return ((CUBIC_A + 2.0) * x - (CUBIC_A + 3.0)) * x * x + 1.0


def _c2(x):
    return ((CUBIC_A * x - 5.0 * CUBIC_A) * x + 8.0 * CUBIC_A) * x - 4.0 * CUBIC_A


def _e1(x, R):
    return ((CUBIC_A + 2.0) * x + (CUBIC_A + 3.0)) * x * x + 1.0 + ((3.0 * (CUBIC_A + 2.0) * x - 2.0 * (CUBIC_A + 3.0)) * x).abs() * R


def _e2(x, R):
    a = abs(CUBIC_A)
    return ((a * x + 5.0 * a) * x + 8.0 * a) * x + 4.0 * a + ((3.0 * CUBIC_A * x - 10.0 * CUBIC_A) * x + 8.0 * CUBIC_A).abs() * R


def cubic_axis(n_in, n_out, drop_clamped=False):
    """(A, E) [n_out, n_in]: the weights with which output o reads input i along one axis (clamped taps added up) and their
    error proxy.  The source coordinate and its floor are float32: scale = float(n_in) / float(n_out), scale * (o + 0.5f) -
    0.5f; the polynomials are fp64.  drop_clamped: the mutant that drops a tap clamped at the border"""
    scale = _s32(n_in) / _s32(n_out)
    o = torch.arange(n_out, dtype=torch.float32)
    r = scale * (o + 0.5) - 0.5
    fl = torch.floor(r)
    t = (r - fl).double()
    i0 = fl.long()
    R = r.double().abs() + 2.0
    coef = [_c2(t + 1.0), _c1(t), _c1(1.0 - t), _c2(2.0 - t)]
    err = [_e2(t + 1.0, R), _e1(t, R), _e1(1.0 - t, R), _e2(2.0 - t, R)]
    A = torch.zeros(n_out, n_in, dtype=torch.float64)
    E = torch.zeros_like(A)
    rows = torch.arange(n_out)
    for a in range(4):
        raw = i0 - 1 + a
        idx = raw.clamp(0, n_in - 1)
        keep = (raw == idx) | (not drop_clamped)
        A.index_put_((rows, idx), torch.where(keep, coef[a], torch.zeros_like(t)), accumulate=True)
        E.index_put_((rows, idx), err[a], accumulate=True)
    return A, E


def _axes(H, W, OH, OW, drop_clamped=False):
    if OH == H and OW == W:                                # the copy path of both kernels
        return (torch.eye(H, dtype=torch.float64), torch.zeros(H, H, dtype=torch.float64),
                torch.eye(W, dtype=torch.float64), torch.zeros(W, W, dtype=torch.float64))
    return cubic_axis(H, OH, drop_clamped) + cubic_axis(W, OW)


def bicubic_fwd(x, OH, OW, mean=None, std=None, drop_clamped=False):
    H, W = x.shape[2:]
    Ay, Ey, Ax, Ex = _axes(H, W, OH, OW, drop_clamped)
    xd = _d(x)
    v = torch.einsum("oh,nchw,pw->ncop", Ay, xd, Ax)
    M = torch.einsum("oh,nchw,pw->ncop", 2.0 * Ay.abs() + Ey, xd.abs(), Ax.abs()) + torch.einsum("oh,nchw,pw->ncop", Ay.abs(), xd.abs(), Ex)
    if OH == H and OW == W and mean is None:
        return exact(x)
    if mean is not None:
        mu, sd = _d(mean).reshape(1, -1, 1, 1), _d(std).reshape(1, -1, 1, 1)
        out = (v - mu) / sd
        M = (M + v.abs() + mu.abs()) / sd.abs() + out.abs()
        v = out
    return Ref(v, M, "bicubic")


def bicubic_bwd(dy, H, W, std=None):
    """the exact adjoint, from the two per-axis weight matrices"""
    OH, OW = dy.shape[2:]
    Ay, Ey, Ax, Ex = _axes(H, W, OH, OW)
    g = _d(dy)
    if OH == H and OW == W and std is None:
        return exact(dy)
    v = torch.einsum("oh,ncop,pw->nchw", Ay, g, Ax)
    M = torch.einsum("oh,ncop,pw->nchw", 2.0 * Ay.abs() + Ey, g.abs(), Ax.abs()) + torch.einsum("oh,ncop,pw->nchw", Ay.abs(), g.abs(), Ex)
    if std is not None:
        sd = _d(std).reshape(1, -1, 1, 1)
        v = v / sd
        M = M / sd.abs() + v.abs()
    return Ref(v, M, "bicubic")


# ---- retrieval.hip -------------------------------------------------------------------------------------------------------------
def topk_rows(s, k, high_index=False):
    """(idx, val) in faiss order: value descending, index ascending; -0.0 == 0.0.  high_index: the mutant that resolves a tie
    to the higher index"""
    sd = _d(s)
    cols = s.shape[1]
    if high_index:
        val, idx = torch.sort(sd.flip(1), dim=1, descending=True, stable=True)
        idx = cols - 1 - idx
    else:
        val, idx = torch.sort(sd, dim=1, descending=True, stable=True)
    return exact(idx[:, :k]), exact(val[:, :k])


def row_sqsum(x):
    s = _d(x).pow(2).sum(1)
    return Ref(s, s.clone(), "sum")


def add_outer_terms(m, rowv, colv, alpha, a, b):
    v = f32(alpha) * _d(m)
    M = v.abs()
    if rowv is not None:
        t = f32(a) * _d(rowv).reshape(-1, 1)
        v, M = v + t, M + t.abs()
    if colv is not None:
        t = f32(b) * _d(colv).reshape(1, -1)
        v, M = v + t, M + t.abs()
    return Ref(v, M, "ew")


def segment_mean(x, order, offsets):
    """mean of the listed rows.  M = (sum |x_j| + sum_j |S_j|) / n, S_j the partial sums in list order: a sum over a list of
    any length rounds each addition relative to the partial sum it produces, not to the term it adds"""
    xd = _d(x)
    v, M = [], []
    for s in range(offsets.numel() - 1):
        rows = xd[order[int(offsets[s]):int(offsets[s + 1])]]
        v.append(rows.mean(0))
        M.append((rows.abs().sum(0) + rows.cumsum(0).abs().sum(0)) / rows.shape[0])
    return Ref(torch.stack(v), torch.stack(M), "sum")


def segment_mean_f32(x, order, offsets):
    """the float32 model of the contract `members added in list order`: serial float32 additions from 0.0f, then one product
    with the rounded 1.f / n — exact"""
    out = []
    for s in range(offsets.numel() - 1):
        idx = order[int(offsets[s]):int(offsets[s + 1])]
        acc = torch.zeros(x.shape[1], dtype=torch.float32)
        for j in idx:
            acc = acc + x[j]
        out.append(acc * (_s32(1.0) / _s32(idx.numel())))
    return exact(torch.stack(out))


# ---- case lists, built from the launch regimes ---------------------------------------------------------------------------------
SLOPE = 0.2
VEC_BIG = 4 * GRID_CAP["eltwise"] * 256 + 7                          # second float4 trip, n % 4 == 3
VEC_N = [1, 3, 4, 5, 6, 7, 1027, VEC_BIG]
ELT_BIG = GRID_CAP["eltwise"] * 256 + 3                              # the scalar grid-stride kernels of eltwise.hip
GAN_BIG = GRID_CAP["gan"] * 256                                      # strictly more than this many elements: second trip
PLANTED = [0.0, -0.0, 1e-40, -1e-40, float("inf"), float("-inf"), -3.0, 2.5]


def act_input(n, fam, seed=0, planted=True):
    x = family((n,), fam, gen(11 * n % 1000003 + seed))
    if planted:
        m = min(n, len(PLANTED))
        x[torch.arange(m) * max(1, n // m) % n] = torch.tensor(PLANTED[:m])
        if n > 8:
            x[n - 1] = -0.0                                          # a planted value in the tail
    return x


def act_bwd_input(n, act, seed=0):
    """(dy, y): y is the rounded forward output with exact 0.0 and -0.0, and for tanh values next to +-1"""
    x = family((n,), "plain", gen(5 * n % 1000003 + seed))
    y = act_fwd(x, act, SLOPE).value.float()
    plant = [0.0, -0.0, 1.0, -1.0, 1.0 - 2.0 ** -24, -1.0 + 2.0 ** -24] if act == ACT_TANH else [0.0, -0.0]
    m = min(n, len(plant))
    y[torch.arange(m) * max(1, n // m) % n] = torch.tensor(plant[:m])
    dy = family((n,), "scales", gen(n % 1000003 + 77 + seed))
    return dy, y


PAIR_CAT = [(3, 5), (3, 8), (2, 1027), (1, 4 * 1024 * 1024 + 4)]     # (B, per): scalar, vector one chunk, scalar 2 chunks, cap
DROPOUT_P = [0.0, 0.2, 0.5, 0.999]
DROPOUT_SEEDS = [0, 12345, (1 << 63) + 0x1234567]
DROPOUT_CLOCKS = [0, 1, (1 << 32) + 5]
DROPOUT_N = [1, 1027, ELT_BIG]

L2R_D = [1, 255, 256, 257, 2051]
L2_EPS = [0.5, 1e-12]


def l2rows_input(D, eps, fam="plain"):
    """rows: 0 zero, 1 norm < eps, 2 norm == eps exactly (one non-zero element equal to float32(eps)), 3 of scale 1e3, 4 and
    5 of the family"""
    e = float(_s32(eps))
    x = family((6, D), fam, gen(D + 1))
    x[0] = 0.0
    x[1] = x[1] / float(x[1].norm()) * e * 0.01 if fam != "constant" else e * 0.01 / D
    x[2] = 0.0
    x[2, D // 2] = -e
    x[3] = x[3] * 1e3
    return x.contiguous()


L2C = [(2, 3, 5), (3, 37, 49), (16, 5, 4093), (15, 5, 4093)]          # (N, C, HW)


def l2chan_input(N, C, HW, eps):
    """pixel 0 of every image: zero norm; pixel 1: norm == eps exactly; pixel 2: norm < eps"""
    e = float(_s32(eps))
    x = family((16, C, HW), "plain", gen(C * HW))[:N].clone()          # images n < 15 are the same data for N = 15 and 16
    x[:, :, 0] = 0.0
    x[:, :, 1] = 0.0
    x[:, C // 2, 1] = e
    x[:, :, 2] = x[:, :, 2] * e * 1e-3
    return x.contiguous()


COPY_CH = [(2, 3, 5, 7, 2, 9, 4), (1, 2, 33, 2, 0, 5, 3), (3, 1367, 257, 1400, 20, 1380, 11)]   # (N, Cc, HW, Cs, sc0, Cd, dc0)
MIX = [(4, 6, 1, 1.0), (4, 6, 257, 0.3), (5, 3, 257, 0.0), (6, 5, 209717, 0.3)]                   # (rows_src, rows_out, len, lam)


def mix_indices(rows_src, rows_out):
    """repeated indices, ia[j] == ib[j] at j = 1, and source row rows_src - 1 read by nobody (rows_src > 1)"""
    m = max(1, rows_src - 1)
    ia = torch.tensor([(2 * j) % m for j in range(rows_out)], dtype=torch.int64)
    ib = torch.tensor([(j + 1) % m if j != 1 else (2 * j) % m for j in range(rows_out)], dtype=torch.int64)
    return ia, ib


AVGPOOL = [(2, 3, 4, 6, 2), (1, 5, 5, 7, 2), (2, 2, 2, 2, 2), (1, 3, 9, 6, 3), (2, 1, 7, 8, 3), (1, 2, 3, 3, 3)]  # (N, C, H, W, k)
AVGPOOL_BIG = (1, 9, 483, 484, 2)                                     # the backward's N C H W > 8192 * 256


def pad_geoms():
    """[(N, C, H, W, pad)]: pad 0..4, H in pad + 1, 2, 3, 9, W in 8, 12, 20 (vector route unless pad == 4) and 6, 9 (scalar)"""
    out = []
    for pad in range(5):
        for i, Hh in enumerate(sorted(set([pad + 1, 2, 3, 9]))):
            if Hh <= pad:
                continue
            for j, W in enumerate([8, 12, 20, 6, 9]):
                if W > pad and ((i + j + pad) % 2 == 0 or (pad == 4 and W == 12) or Hh == pad + 1):
                    out.append((2, 3, Hh, W, pad))
    return out


PAD_BIG = (1, 61, 186, 186, 1)                                        # scalar route, N C OH OW = 61 * 188 * 188 > 8192 * 256

SN_SHAPES = [(1, 1), (3, 27), (17, 65), (128, 2048), (1024, 64), (8, 12288)]
SN_BWD_SHAPES = [(4, 4096), (5, 3277), (3, 27)]
SN_MULTI = [(3, 27), (17, 65), (1, 1), (64, 576), (8, 12288), (128, 2048), (2, 5)] * 3                # 17 of them are used


def sn_input(K, M, scale=1.0, seed=0):
    g = gen(K * 31 + M + seed)
    w = (torch.randn(K, M, generator=g) * scale).float()
    u = torch.nn.functional.normalize(torch.randn(K, generator=g).double(), dim=0).float()
    v = torch.nn.functional.normalize(torch.randn(M, generator=g).double(), dim=0).float()
    return w, u, v


def bgemm_cases():
    """[(M, N, K, a_rc, b_rc, c_t, batch, alpha, beta, nan_c)]: every M, N of 1, 31, 33, 64, 65, 130, every K of 1, 15, 16, 17,
    33, every ragged M with every ragged K, the four load-mapping pairs, a transposed C, two batch levels, the three (alpha,
    beta) settings"""
    out = []
    Ms, Ks = [1, 31, 33, 64, 65, 130], [1, 15, 16, 17, 33]
    ab = [(1.0, 0.0, False), (0.5, 2.0, False), (1.0, 0.0, True)]
    i = 0
    for mi, M in enumerate(Ms):
        for ki, K in enumerate(Ks):
            if M == 64 and K not in (16, 33):
                continue
            N = Ms[(mi + 2 * ki + 1) % 6]
            out.append((M, N, K, bool(i & 1), bool(i & 2), i % 5 == 3, (3, 2) if i % 7 == 2 else (1, 1)) + ab[i % 3])
            i += 1
    return out


def bgemm_operands(M, N, K, a_rc, b_rc, c_t, batch, fam, seed=0):
    """flat base buffers and strides.  Batched: batch0 images of [heads * rows] channel-major maps, heads as channel offsets
    (the strides of the attention blocks); else plain matrices, transposed where the unit stride runs along the row"""
    g = gen(1000 * seed + 7 * M + 3 * N + K)
    nb = batch[0] * batch[1]
    A = family((nb * M * K,), fam, g)
    B = family((nb * K * N,), fam if fam != "constant" else "plain", g)
    C = family((nb * M * N,), "plain", g)
    a_str = (1, M) if a_rc else (K, 1)
    b_str = (N, 1) if b_rc else (1, K)
    c_str = (1, M) if c_t else (N, 1)
    a_b = (batch[1] * M * K, M * K)
    b_b = (batch[1] * K * N, K * N)
    c_b = (batch[1] * M * N, M * N)
    return A, B, C, a_str, b_str, c_str, a_b, b_b, c_b


SOFTMAX_COLS = [1, 63, 64, 65, 200]
SOFTMAX_ROWS = [1, 5]
SOFTMAX_SCALES = [0.125, -1.5, 0.0]


def softmax_input(rows, cols, fam):
    """row 0 of five: equal values; row 1: logits of +-80"""
    x = family((rows, cols), fam, gen(rows * 1000 + cols), limit=30.0)
    if rows > 1:
        x[0] = 1.25
        x[1] = torch.where(torch.arange(cols) % 2 == 0, torch.tensor(80.0), torch.tensor(-80.0))
    return x


BICUBIC = [((4, 4), (8, 8)), ((5, 3), (11, 7)), ((1, 1), (3, 5)), ((8, 6), (8, 6)), ((9, 7), (4, 3)), ((2, 2), (2, 5))]
BICUBIC_BIG_FWD = (1, 3, (64, 32), (1024, 700))                     # output 3 * 1024 * 700 > 8192 * 256
BICUBIC_BIG_BWD = (12000, 3, (9, 7), (4, 3))                        # input 36000 * 63 > 8192 * 256: the backward's loop
BICUBIC_MEAN, BICUBIC_STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]

TOPK_COLS = [1, 255, 257, 1000]


def topk_input(cols):
    """rows: 0 distinct values, 1 duplicated values, 2 all equal, 3 with +-inf and 0.0 beside -0.0, 4 duplicates and inf"""
    g = gen(cols)
    x = torch.randn(5, cols, generator=g)
    x[1] = torch.randint(0, 4, (cols,), generator=g).float()
    x[2] = 0.7
    x[3] = torch.where(torch.arange(cols) % 2 == 0, torch.tensor(0.0), torch.tensor(-0.0))
    if cols > 4:
        x[3, 1], x[3, cols - 1], x[3, 3] = float("inf"), float("-inf"), float("inf")
    x[4] = torch.randint(-1, 2, (cols,), generator=g).float()
    if cols > 4:
        x[4, cols // 2] = float("-inf")
    return x.contiguous()


def topk_ks(cols):
    return sorted(set(k for k in (1, 7, cols) if k <= cols))


SQSUM_D = [1, 63, 65, 2048]
SQSUM_ROWS = [1, 6]
OUTER = [(3, 5), (7, 300), (699, 3001)]                               # 699 * 3001 > 8192 * 256, cols no power of two
SEG_D = [1, 256, 300]
SEG_SIZES = [1, 2, 300]


def segment_input(D):
    """x [40, D]; order: non-monotone with repeats; segments of 1, 2 and 300 members"""
    x = family((40, D), "plain", gen(D))
    total = sum(SEG_SIZES)
    order = (torch.arange(total) * 17 + 5) % 40
    offsets = torch.tensor([0, 1, 3, total], dtype=torch.int64)
    return x, order.to(torch.int64), offsets
