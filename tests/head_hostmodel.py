"""Host model of the four units that close a training step — csrc/pool.hip, csrc/loss.hip, csrc/cm.hip, csrc/optim.hip — the
comparison partner of tests/test_head_elementwise_gpu.py, tied to float32 torch by tests/test_head_hostmodel_cpu.py.  No tests
and no GPU here.

Three parts:

  dispatch mirrors   partial_grid, the three grid_for caps, the Adam float4 split, the max-pool backward kernel choice, the
                     cm.hip register limit and the wave-per-plane launches: the host arithmetic that shapes a launch, a few
                     lines each, so that the case lists below are BUILT from the launch regimes.
  fp64 references    every entry point of the four files, taking the float32 tensors the C ABI takes.  Each backward takes the
                     forward outputs it is handed (lse, argmax, GeM y, out2), so nothing has to be left out of a comparison.
  error budgets      every reference is Ref(value, M, kind); an element passes when
                         |got - value| <= C_KIND[kind] * 2^-24 * M
                     with M the fp64 sum of the absolute values of the terms THAT element is made of (never a tensor-wide
                     maximum), plus the condition term where the formula is ill-conditioned, plus 2^-102 for every budgeted
                     kind (2^-24 of it is the smallest normal float32: below that a result may be flushed or lose bits):
                         sum       mean / sum of |term|; a squared difference (x - t)^2 counts d^2 + 2 |d| (|x| + |t|), an
                                   affine term |a| + |b x|, 1 / count its own value
                         grad      |factor| times the |operands| of the one difference it multiplies (|x| + |t| for mse), else
                                   |value|: a short chain of products
                         bce       t (|log s| + 1) + (1 - t) (|log(1 - s)| + 1 + s / (1 - s)): each log carries the relative
                                   rounding of its argument, and the argument 1 - s carries the rounding of s, s / (1 - s)
                         bce_bwd   |g| (|s| + |t|)                      (the two torch formulas cancel to g (s - t))
                         ce        lse: |lse| + max |scale z| + 1; loss: that + |scale z_y|  (the argument of exp carries
                                   |scale z| + |lse|)
                         ce_bwd    |g| (p (1 + |scale z| + |lse|) + onehot), p = exp(scale z - lse)
                         gp        pen: |scale| ((n - c)^2 + 2 |n - c| (n + |c|)); v: 2 |scale| (n + |c|) / n |g + 1e-16|
                         gem       y (1 + (mean(xc^p (1 + p |log2 xc|)) / m + |log2 m|) / p): p |log2 x| on each power
                         gem_bwd   dx: |dx| (3 + p |log2 y| + |p - 1| |log2 xc|); dp: per plane |g| y ((|ln m| + cm) / p^2 +
                                   mean(xc^p |ln xc|) / (p m) (cm + cx)), cm = 1 + p |log2 y|, cx = 1 + p max |log2 xc|
                         cm        one term per link of a label's chain: E' = (m E + |m f| + |(1 - m) x|) / n + |f'| (2 + the
                                   relative term of the norm); normalize_listed_rows is one such link with E = 0
                         adam      m: |b1 m| + (1 - b1) Mg; v: |b2 v| + (1 - b2) (g^2 + 2 |g| Mg); p: |p| + step_size
                                   (|m / denom| (1 + Mv / (2 v')) + Mm / denom), Mg = |g scale| + |wd p|
                         sgd       buf: |mom buf| + Mg; p: |p| + lr Mbuf
                         exact     M = 0: a copy, a selection or one correctly rounded product — max-pool y and argmax, max-pool
                                   backward (a float32 model that adds in the kernel's documented order), rows and elements an
                                   entry point must not touch, an ignored cross-entropy row, the saturated BCE gradient

The constants C_KIND are NOT taken from the kernels.  tests/test_head_hostmodel_cpu.py evaluates every case of the lists below
with plain float32 torch on the CPU (F.max_pool2d, F.binary_cross_entropy(torch.sigmoid(x), ...), F.l1_loss, F.mse_loss,
F.cross_entropy, float32 autograd, torch.optim.Adam / SGD with foreach=False, the reference's Python loops for the memory), records
max err / (2^-24 M) per kind, and C_KIND = max(8, 4 x that ratio): 4 for another summation order and the hardware exp / log /
rsqrt, the floor of 8 so that a lucky CPU run cannot make a budget tighter than two roundings per term.  Measured (torch 2.10,
CPU, one thread):

    kind       float32 torch ratio    C_KIND
    sum        5.29                   21.18
    grad       2.65                   10.6
    bce        3.21                   12.86
    bce_bwd    5.66                   22.64
    ce         0.71                   8
    ce_bwd     1.97                   8
    gp         13.35                  53.4
    gem        0.57                   8
    gem_bwd    1.18                   8
    cm         1.09                   8
    adam       2.51                   10.03
    sgd        2.21                   8.84
    exact      0                      0

The larger ratios are torch's own summation order, not the formulas: `sum` and `bce` are driven by the `constant` family (a
serial float32 sum of equal terms rounds the same way every time), `gp` by the all-zero row at D = 1027 (1027 equal squares of
1e-16), `bce_bwd` by the four-operation chain of torch's two backward formulas.
"""
import collections
import math

import torch

U24 = 2.0 ** -24
FILL = -7777.0                      # guard / untouched-output fill value of the device tests

C_KIND = {"sum": 21.18, "grad": 10.6, "bce": 12.86, "bce_bwd": 22.64, "ce": 8.0, "ce_bwd": 8.0, "gp": 53.4, "gem": 8.0,
          "gem_bwd": 8.0, "cm": 8.0, "adam": 10.03, "sgd": 8.84, "exact": 0.0}

Ref = collections.namedtuple("Ref", "value M kind")
TINY_M = 2.0 ** -102                # 2^-24 * TINY_M = 2^-126, the smallest normal float32: below it a result may be flushed or lose bits


def f32(v):
    """the float32 the C ABI receives for a Python float, as a double"""
    return float(torch.tensor(float(v), dtype=torch.float32))


# ---- dispatch mirrors --------------------------------------------------------------------------------------------------------
def cdiv(a, b):
    return -(-a // b)


MAX_PARTIALS = 1024                 # kMaxPartials, loss.hip
GRID_CAP = {"loss": 4096, "pool": 8192, "optim": 8192}
CM_MAX_D = 256 * 16                 # kMaxPerThread = 16, cm.hip
WAVES_PER_WG = 4                    # gap, GeM, normalize_listed_rows: one wave per plane / listed row


def partial_grid(n):
    """partial_grid(), loss.hip: workgroups of the first stage of a two-stage sum"""
    return max(1, min(cdiv(n, 2048), MAX_PARTIALS))


def grid_for(unit, items):
    """grid_for() of loss.hip / pool.hip / optim.hip: workgroups of 256 threads of a grid-stride loop"""
    return max(1, min(cdiv(items, 256), GRID_CAP[unit]))


def trips(unit, items):
    """most trips a thread makes through the grid-stride loop"""
    return cdiv(items, grid_for(unit, items) * 256)


def sum_trips(n):
    return cdiv(n, partial_grid(n) * 256)


def adam_split(n):
    """adam_kernel: (float4 units, scalar tail elements, workgroups)"""
    return n >> 2, n & 3, grid_for("optim", n // 4 + 1)


def maxpool_bwd_kernel(KH, KW, SH, SW, PH, PW, W, dx_addr):
    """rg_maxpool2d_bwd: 'four' = the four-pixels-per-thread kernel of the 3x3 / 2 / pad 1 pool, else 'gather'"""
    if (KH, KW, SH, SW, PH, PW) == (3, 3, 2, 2, 1, 1) and W % 4 == 0 and dx_addr % 16 == 0:
        return "four"
    return "gather"


def wave_workgroups(planes):
    """(workgroups, waves of the last one that have a plane)"""
    return cdiv(planes, WAVES_PER_WG), (planes - 1) % WAVES_PER_WG + 1


def pool_out(H, W, KH, KW, SH, SW, PH, PW):
    return (H + 2 * PH - KH) // SH + 1, (W + 2 * PW - KW) // SW + 1


# ---- the comparator ----------------------------------------------------------------------------------------------------------
Worst = collections.namedtuple("Worst", "ok index err budget ratio")


def _d(t):
    return None if t is None else t.detach().double()


def exact(v):
    v = _d(v)
    return Ref(v, torch.zeros_like(v), "exact")


def compare(got, ref, table=None):
    """per-element check of `got` against ref = Ref(value, M, kind); every element takes part.  An element whose reference is
    NaN or infinite passes only with the same NaN / infinity; a non-finite `got` anywhere else fails.  table: the constants
    per kind (default C_KIND; another host model brings its own kinds)"""
    table = C_KIND if table is None else table
    g = got.detach().double().cpu().reshape(-1)
    v, M = ref.value.reshape(-1), ref.M.reshape(-1)
    assert g.numel() == v.numel(), ("shape", tuple(got.shape), tuple(ref.value.shape))
    same = (g == v) | (torch.isnan(g) & torch.isnan(v))
    err = torch.where(same, torch.zeros_like(g), (g - v).abs())
    err = torch.where(torch.isfinite(err), err, torch.full_like(err, float("inf")))
    if ref.kind != "exact":
        M = M + TINY_M
    bud = table[ref.kind] * U24 * M
    over = err - bud
    i = int(torch.argmax(over)) if over.numel() else 0
    ratio = torch.where(err > 0, err / (U24 * M).clamp_min(1e-300), torch.zeros_like(err))
    idx = tuple(int(k) for k in torch.unravel_index(torch.tensor(i), tuple(ref.value.shape))) if ref.value.dim() else ()
    return Worst(bool((err <= bud).all()), idx, float(err[i]), float(bud[i]), float(ratio.max()) if ratio.numel() else 0.0)


def check(got, ref, what):
    w = compare(got, ref)
    assert w.ok, "%s: worst element %s err %.3e > budget %.3e (%s, max err/(2^-24 M) = %.2f)" % (
        what, w.index, w.err, w.budget, ref.kind, w.ratio)
    return w.ratio


# ---- input families ----------------------------------------------------------------------------------------------------------
FAMILIES = ("plain", "scales", "offset", "constant")          # `planted` values are added per operation


def gen(seed):
    return torch.Generator().manual_seed(seed)


def family(shape, fam, g, limit=None):
    """float32 tensor: plain randn * 1.7 + 0.3; scales sign * 10^U(-4, 3) within one tensor; offset randn + 300 (a sum that
    cancels against a target near it); constant 0.7.  limit: |x| bound (BCE's budgeted families stay at |x| <= 12)"""
    if fam == "plain":
        x = torch.randn(shape, generator=g) * 1.7 + 0.3
    elif fam == "scales":
        hi = 3.0 if limit is None else math.log10(limit)
        x = torch.sign(torch.randn(shape, generator=g)) * 10.0 ** (torch.rand(shape, generator=g) * (hi + 4.0) - 4.0)
    elif fam == "offset":
        x = torch.randn(shape, generator=g) + (300.0 if limit is None else 0.75 * limit)
    elif fam == "constant":
        x = torch.full(shape, 0.7)
    else:
        raise ValueError(fam)
    if limit is not None:
        x = x.clamp(-limit, limit)
    return x.float().contiguous()


KINK_ULPS = 64.0


def kink_margin(diff, mag):
    """smallest |diff| / (64 * 2^-24 * mag) over the elements that are not exactly zero; the `plain` hinge / L1 cases and the
    CM-hard gaps keep it above 1 (asserted in tests/test_head_hostmodel_cpu.py)"""
    nz = diff != 0
    if not bool(nz.any()):
        return float("inf")
    return float((diff[nz].abs() / (KINK_ULPS * U24 * mag[nz])).min())


def off_kink(x, a, b):
    """move the elements of x whose a + b x is within 1e-3 of zero away from it"""
    v = a + b * x.double()
    return torch.where(v.abs() < 1e-3, x + 0.0625, x).float()


# ---- loss.hip: two-stage sums ----------------------------------------------------------------------------------------------------
def sigmoid32(x, chain=False):
    """s as the float32 tensor the op sees: the rounded fp64 sigmoid, or (chain, the saturated family) float32 arithmetic
    1 / (1 + exp(-x)), where 1 + e rounds to 1 from x = 17 on and exp(-x) overflows at x = -100"""
    if chain:
        return 1.0 / (1.0 + torch.exp(-x.float()))
    return torch.sigmoid(x.double()).float()


def sum_terms(op, x, par, chain=False):
    """per-element (term, M) in fp64 of the two-stage sums; par: bce / mse target, affine (a, b, clamp)"""
    xd = _d(x)
    if op == "bce":
        t = f32(par)
        s = sigmoid32(x, chain).double()
        l1 = torch.log(s).clamp_min(-100.0)
        l0 = torch.log(1.0 - s).clamp_min(-100.0)
        M = t * (l1.abs() + 1.0) + (1.0 - t) * (l0.abs() + 1.0 + torch.where(s < 1, s / (1.0 - s).clamp_min(1e-300), s))
        return -(t * l1 + (1.0 - t) * l0), M
    if op == "mse":
        t = f32(par)
        d = xd - t
        return d * d, d * d + 2.0 * d.abs() * (xd.abs() + abs(t))
    if op == "affine":
        a, b, clamp = f32(par[0]), f32(par[1]), par[2]
        v = a + b * xd
        return (v.clamp_min(0.0) if clamp else v), abs(a) + (b * xd).abs()
    raise ValueError(op)


def two_stage(op, x, par, chain=False):
    term, M = sum_terms(op, x, par, chain)
    kind = "bce" if op == "bce" else "sum"
    return Ref(term.mean(), M.mean(), kind)


def sum_bwd(op, x, par, gout, gscale, chain=False):
    """dx of the mean: gout (None = 1) * gscale / n * d term / dx"""
    xd = _d(x)
    n = x.numel()
    g = (1.0 if gout is None else float(gout)) * f32(gscale) / n
    if op == "bce":
        t = f32(par)
        s = sigmoid32(x, chain).double()
        ss = s * (1.0 - s)
        v = g * (s - t) / ss.clamp_min(f32(1e-12)) * ss
        if chain:
            return Ref(v, torch.where(ss == 0, torch.zeros_like(v), abs(g) * (s + t)), "bce_bwd")
        return Ref(v, abs(g) * (s + t), "bce_bwd")
    if op == "mse":
        t = f32(par)
        return Ref(2.0 * g * (xd - t), 2.0 * abs(g) * (xd.abs() + abs(t)), "grad")
    a, b, clamp = f32(par[0]), f32(par[1]), par[2]
    v = torch.where((a + b * xd > 0) | (not clamp), torch.full_like(xd, g * b), torch.zeros_like(xd))
    return Ref(v, v.abs(), "grad")


def l1_fwd(a, b, labels):
    """out2 = [mean |a - b| over the rows with label 1 (None: all rows), 1 / (selected rows * inner)]; nothing selected: NaN,
    inf as the float32 division gives them"""
    rows = a.shape[0]
    ad, bd = _d(a).reshape(rows, -1), _d(b).reshape(rows, -1)
    sel = torch.ones(rows, dtype=torch.bool) if labels is None else labels == 1
    cnt = float(sel.sum()) * ad.shape[1]
    s = (ad - bd).abs()[sel].sum()
    if cnt == 0:
        return Ref(torch.tensor([float("nan"), float("inf")], dtype=torch.float64), torch.zeros(2, dtype=torch.float64), "exact")
    return Ref(torch.stack([s / cnt, torch.tensor(1.0 / cnt, dtype=torch.float64)]),
               torch.stack([s / cnt, torch.tensor(1.0 / cnt, dtype=torch.float64)]), "sum")


def l1_bwd(a, b, labels, gout, out2, gscale):
    """da = sign(a - b) * gout * gscale * out2[1] on the selected rows, 0 elsewhere and at a == b; db = -da"""
    rows = a.shape[0]
    ad, bd = _d(a).reshape(rows, -1), _d(b).reshape(rows, -1)
    g = (1.0 if gout is None else float(gout)) * f32(gscale) * float(out2[1])
    sel = torch.ones(rows, dtype=torch.bool) if labels is None else labels == 1
    v = torch.sign(ad - bd) * g * sel.double().reshape(rows, 1)
    v = v.reshape(a.shape)
    return Ref(v, v.abs(), "grad"), Ref(-v, v.abs(), "grad")


def rows_fwd(op, a, b_or_c):
    """l1_rows: mean_i |a - b| per row; mse_rows: mean_i (x - c)^2 per row"""
    rows = a.shape[0]
    ad = _d(a).reshape(rows, -1)
    if op == "l1_rows":
        t = (ad - _d(b_or_c).reshape(rows, -1)).abs()
        return Ref(t.mean(1), t.mean(1), "sum")
    c = f32(b_or_c)
    d = ad - c
    return Ref((d * d).mean(1), (d * d + 2.0 * d.abs() * (ad.abs() + abs(c))).mean(1), "sum")


def rows_bwd(op, a, b_or_c, grow):
    rows = a.shape[0]
    ad = _d(a).reshape(rows, -1)
    inner = ad.shape[1]
    g = _d(grow).reshape(rows, 1)
    if op == "l1_rows":
        v = (torch.sign(ad - _d(b_or_c).reshape(rows, -1)) * g / inner).reshape(a.shape)
        return Ref(v, v.abs(), "grad"), Ref(-v, v.abs(), "grad")
    c = f32(b_or_c)
    return Ref(((ad - c) * g * 2.0 / inner).reshape(a.shape), ((ad.abs() + abs(c)) * g.abs() * 2.0 / inner).reshape(a.shape), "grad")


def grad_penalty_rows(g, c, scale):
    """pen[r] = scale (|g_r + 1e-16| - c)^2 and v[r] = d pen[r] / d g_r; the 1e-16 is inside the norm"""
    c, scale = f32(c), f32(scale)
    t = _d(g) + f32(1e-16)
    n = t.pow(2).sum(1, keepdim=True).sqrt()
    pen = scale * (n - c) ** 2
    Mp = abs(scale) * ((n - c) ** 2 + 2.0 * (n - c).abs() * (n + abs(c)))
    v = scale * 2.0 * (n - c) / n * t
    return Ref(pen.reshape(-1), Mp.reshape(-1), "gp"), Ref(v, 2.0 * abs(scale) * (n + abs(c)) / n * t.abs(), "gp")


def in_range(labels, K):
    return (labels >= 0) & (labels < K)


def softmax_ce_fwd(z, labels, scale):
    """loss[b] = lse(scale z_b) - scale z_b[y_b], 0 for a label outside [0, K) (ignore_index); lse[b] for every row"""
    B, K = z.shape
    zs = _d(z) * f32(scale)
    lse = torch.logsumexp(zs, 1)
    ok = in_range(labels, K)
    zy = zs.gather(1, labels.clamp(0, K - 1).reshape(B, 1)).reshape(B)
    Ml = lse.abs() + zs.abs().max(1).values + 1.0
    loss = torch.where(ok, lse - zy, torch.zeros_like(lse))
    return {"loss": Ref(loss, torch.where(ok, Ml + zy.abs(), torch.zeros_like(Ml)), "ce"), "lse": Ref(lse, Ml, "ce")}


def softmax_ce_bwd(z, labels, lse, grow, scale, gscale):
    """dz[b] = grow[b] gscale scale (softmax - onehot) from the lse it is handed; an ignored row is exactly zero"""
    B, K = z.shape
    zs = _d(z) * f32(scale)
    l = _d(lse).reshape(B, 1)
    g = (torch.ones(B, dtype=torch.float64) if grow is None else _d(grow)).reshape(B, 1) * f32(gscale) * f32(scale)
    p = torch.exp(zs - l)
    ok = in_range(labels, K).reshape(B, 1)
    onehot = torch.zeros(B, K, dtype=torch.float64).scatter_(1, labels.clamp(0, K - 1).reshape(B, 1), 1.0)
    v = torch.where(ok, g * (p - onehot), torch.zeros_like(p))
    M = torch.where(ok, g.abs() * (p * (1.0 + zs.abs() + l.abs()) + onehot), torch.zeros_like(p))
    return Ref(v, M, "ce_bwd")


def weighted_sum_fwd(x, w, scale):
    t = _d(x) if w is None else _d(x) * _d(w)
    return Ref(t.sum() * f32(scale), t.abs().sum() * abs(f32(scale)), "sum")


def weighted_sum_bwd(gout, w, n, scale):
    g = (1.0 if gout is None else float(gout)) * f32(scale)
    v = torch.full((n,), g, dtype=torch.float64) if w is None else g * _d(w)
    return Ref(v, v.abs(), "grad")


# ---- pool.hip ------------------------------------------------------------------------------------------------------------------
def maxpool_fwd(x, KH, KW, SH, SW, PH, PW, last=False):
    """(y, argmax): the FIRST maximum in scan order over the in-bounds window elements, index r * KW + s relative to the window;
    a NaN wins, and a later NaN wins over an earlier one (torch's `val > max || isnan(val)`).  last: the mutant that takes
    the last of equal maxima"""
    N, C, H, W = x.shape
    P, Q = pool_out(H, W, KH, KW, SH, SW, PH, PW)
    xd = _d(x)
    best = torch.full((N, C, P, Q), float("-inf"), dtype=torch.float64)
    bi = torch.full((N, C, P, Q), -1, dtype=torch.int64)
    hp, wq = torch.arange(P) * SH - PH, torch.arange(Q) * SW - PW
    for r in range(KH):
        for s in range(KW):
            h, w = hp + r, wq + s
            valid = ((h >= 0) & (h < H)).reshape(P, 1) & ((w >= 0) & (w < W)).reshape(1, Q)
            v = xd[:, :, h.clamp(0, H - 1)][:, :, :, w.clamp(0, W - 1)]
            first = valid & (bi < 0)
            bi = torch.where(first, torch.full_like(bi, r * KW + s), bi)
            take = valid & (((v >= best) if last else (v > best)) | torch.isnan(v))
            best = torch.where(take, v, best)
            bi = torch.where(take, torch.full_like(bi, r * KW + s), bi)
    return exact(best), exact(bi)


def maxpool_bwd(dy, arg, x_shape, KH, KW, SH, SW, PH, PW):
    """float32 model: every input pixel adds the dy of the windows that selected it, window rows ascending, then columns,
    starting from 0.0f — the order both kernels document, so the comparison is exact"""
    N, C, H, W = x_shape
    P, Q = dy.shape[2], dy.shape[3]
    dx = torch.zeros(N * C, H * W, dtype=torch.float32)
    d, a = dy.reshape(N * C, P, Q).float(), arg.reshape(N * C, P, Q).long()
    rows = torch.arange(N * C)
    for p in range(P):
        for q in range(Q):
            h = p * SH - PH + a[:, p, q] // KW
            w = q * SW - PW + a[:, p, q] % KW
            dx[rows, h * W + w] = dx[rows, h * W + w] + d[:, p, q]
    return exact(dx.reshape(N, C, H, W))


def gap_fwd(x):
    N, C = x.shape[:2]
    xd = _d(x).reshape(N, C, -1)
    return Ref(xd.mean(2), xd.abs().mean(2), "sum")


def gap_bwd(dy, x_shape):
    N, C = x_shape[:2]
    HW = 1
    for s in x_shape[2:]:
        HW *= s
    v = (_d(dy).reshape(N, C, 1) / HW).expand(N, C, HW).reshape(x_shape)
    return Ref(v, v.abs(), "grad")


def gem_fwd(x, p, eps=1e-6):
    """y = mean(clamp(x, float32(eps))^p)^(1/p) per plane"""
    N, C = x.shape[:2]
    p, eps = float(p.double()), f32(eps)
    xc = _d(x).reshape(N, C, -1).clamp_min(eps)
    pw = xc ** p
    m = pw.mean(2)
    y = m ** (1.0 / p)
    Mm = (pw * (1.0 + p * torch.log2(xc).abs())).mean(2)
    return Ref(y, y * (1.0 + (Mm / m + torch.log2(m).abs()) / p), "gem")


def gem_bwd(x, p, y, dy, eps=1e-6, drop_log_m=False):
    """from the y it is handed (m = y^p): dx = dy y / (m HW) xc^(p - 1) [x >= eps];
    dp = sum_planes dy y (-ln(m) / p^2 + mean(xc^p ln xc) / (p m)).  drop_log_m: the mutant without the first term"""
    N, C = x.shape[:2]
    p, eps = float(p.double()), f32(eps)
    xd = _d(x).reshape(N, C, -1)
    HW = xd.shape[2]
    xc = xd.clamp_min(eps)
    yv, g = _d(y).reshape(N, C, 1), _d(dy).reshape(N, C, 1)
    m = yv ** p
    l2y, l2x = torch.log2(yv).abs(), torch.log2(xc).abs()
    dx = torch.where(xd >= eps, g * yv / (m * HW) * xc ** (p - 1.0), torch.zeros_like(xd))
    Mdx = dx.abs() * (3.0 + p * l2y + abs(p - 1.0) * l2x)
    pw = xc ** p
    A = torch.zeros_like(m) if drop_log_m else -torch.log(m) / (p * p)
    Bm = (pw * torch.log(xc)).mean(2, keepdim=True) / (p * m)
    Ba = (pw * torch.log(xc).abs()).mean(2, keepdim=True) / (p * m)
    cm_, cx = 1.0 + p * l2y, 1.0 + p * l2x.max(2, keepdim=True).values
    part = g * yv * (A + Bm)
    Mpart = g.abs() * yv * ((torch.log(m).abs() + cm_) / (p * p) + Ba * (cm_ + cx))
    return Ref(dx.reshape(x.shape), Mdx.reshape(x.shape), "gem_bwd"), Ref(part.sum().reshape(1), Mpart.sum().reshape(1), "gem_bwd")


# ---- cm.hip --------------------------------------------------------------------------------------------------------------------
def _link(f, E, x, mom, eps_floor):
    """one link: f' = (mom f + (1 - mom) x) / max(|.|, floor) and its error proxy"""
    v = mom * f + (1.0 - mom) * x
    Ev = mom * E + (mom * f).abs() + ((1.0 - mom) * x).abs()
    nr = v.pow(2).sum().sqrt()
    if eps_floor is not None:
        nr = nr.clamp_min(eps_floor)
    if float(nr) == 0.0:
        return v / nr, Ev                                   # 0 / 0: NaN, as the reference's plain division gives
    f2 = v / nr
    rel = float((Ev * v.abs()).sum() / (nr * nr))
    return f2, Ev / nr + f2.abs() * (2.0 + rel)


def cm_update(x, y, feats, mom, normalize_eps, once_per_label=False):
    """the reference's loop in batch order: per sample features[y] = mom features[y] + (1 - mom) x, then normalised (by the
    plain norm, or max(norm, 1e-12) with normalize_eps); labels outside [0, K) are skipped; rows no valid label names come
    back exact.  once_per_label: the mutant that normalises after a label's last sample only"""
    K = feats.shape[0]
    mom = f32(mom)
    f, E = _d(feats).clone(), torch.zeros(feats.shape, dtype=torch.float64)
    floor = f32(1e-12) if normalize_eps else None
    yl = [int(v) for v in y]
    for j, lab in enumerate(yl):
        if lab < 0 or lab >= K:
            continue
        if once_per_label and lab in yl[j + 1:]:
            f[lab] = mom * f[lab] + (1.0 - mom) * _d(x[j])
            continue
        f[lab], E[lab] = _link(f[lab], E[lab], _d(x[j]), mom, floor)
    return Ref(f, E, "cm")


def cm_dots(x, y, feats):
    """{label: [(batch position, fp64 dot with the pre-update centroid, sum |f_d x_d|)]}"""
    K = feats.shape[0]
    out = collections.OrderedDict()
    for j, lab in enumerate(int(v) for v in y):
        if 0 <= lab < K:
            t = _d(feats[lab]) * _d(x[j])
            out.setdefault(lab, []).append((j, float(t.sum()), float(t.abs().sum())))
    return out


def cm_update_hard(x, y, feats, mom, last=False):
    """per distinct label one link with the sample of the smallest dot product against the pre-update centroid, the first such
    sample in batch order (np.argmin).  last: the mutant that takes the last of tied minima"""
    mom = f32(mom)
    f, E = _d(feats).clone(), torch.zeros(feats.shape, dtype=torch.float64)
    for lab, lst in cm_dots(x, y, feats).items():
        best = min(d for _, d, _ in lst)
        js = [j for j, d, _ in lst if d == best]
        j = js[-1] if last else js[0]
        f[lab], E[lab] = _link(f[lab], E[lab], _d(x[j]), mom, None)
    return Ref(f, E, "cm")


def normalize_listed_rows(g, ids, eps):
    """g[id] /= |g[id]| + eps once per distinct valid id"""
    rows = g.shape[0]
    v, E = _d(g).clone(), torch.zeros(g.shape, dtype=torch.float64)
    seen = set()
    for i in (int(t) for t in ids):
        if i < 0 or i >= rows or i in seen:
            continue
        seen.add(i)
        v[i] = v[i] / (v[i].pow(2).sum().sqrt() + f32(eps))
        E[i] = 3.0 * v[i].abs()
    return Ref(v, E, "cm")


# ---- optim.hip -----------------------------------------------------------------------------------------------------------------
def adam_step(p, g, m, v, lr, b1, b2, eps, wd, step, gscale, variant=None):
    """torch.optim.Adam, L2 form: step_size = lr / bc1, denom = sqrt(v') / sqrt(bc2) + eps; hyper-parameters are the float32
    values the ABI carries.  variant: mutants 'eps_inside' (sqrt(v' / bc2 + eps)) and 'step_off' (bias correction of step - 1)"""
    lr, b1, b2, eps, wd, gs = f32(lr), f32(b1), f32(b2), f32(eps), f32(wd), f32(gscale)
    pd, gd, md, vd = _d(p), _d(g), _d(m), _d(v)
    k = step - 1 if variant == "step_off" else step
    bc1, bc2 = 1.0 - b1 ** k, 1.0 - b2 ** k
    gg = gd * gs + wd * pd
    Mg = (gd * gs).abs() + (wd * pd).abs()
    m2 = b1 * md + (1.0 - b1) * gg
    Mm = (b1 * md).abs() + (1.0 - b1) * Mg
    v2 = b2 * vd + (1.0 - b2) * gg * gg
    Mv = (b2 * vd).abs() + (1.0 - b2) * (gg * gg + 2.0 * gg.abs() * Mg)
    denom = (v2 / bc2 + eps).sqrt() if variant == "eps_inside" else v2.sqrt() / math.sqrt(bc2) + eps
    ss = lr / bc1
    p2 = pd - ss * (m2 / denom)
    relv = torch.where(v2 > 0, Mv / (2.0 * v2.clamp_min(1e-300)), torch.zeros_like(v2))
    Mp = pd.abs() + ss * ((m2 / denom).abs() * (1.0 + relv) + Mm / denom)
    return {"p": Ref(p2, Mp, "adam"), "m": Ref(m2, Mm, "adam"), "v": Ref(v2, Mv, "adam")}


def sgd_step(p, g, buf, lr, mom, wd, first, gscale, read_buf_first=False):
    """torch.optim.SGD: the first step sets buf = g (the old buffer is not read); buf None with momentum 0"""
    lr, mom, wd, gs = f32(lr), f32(mom), f32(wd), f32(gscale)
    pd, gd = _d(p), _d(g)
    gg = gd * gs + wd * pd
    Mg = (gd * gs).abs() + (wd * pd).abs()
    out = {}
    if mom != 0.0:
        if first and not read_buf_first:
            b, Mb = gg, Mg
        else:
            b, Mb = mom * _d(buf) + gg, (mom * _d(buf)).abs() + Mg
        out["buf"] = Ref(b, Mb, "sgd")
        gg, Mg = b, Mb
    elif buf is not None:
        out["buf"] = exact(buf)
    out["p"] = Ref(pd - lr * gg, pd.abs() + lr * Mg, "sgd")
    return out


def adam_clock(k, b1, b2):
    """{step, beta1^k, beta2^k} of k applications of rg_adam_advance to {0, 1, 1}: the same k products in Python doubles"""
    b1, b2 = f32(b1), f32(b2)
    st = [0.0, 1.0, 1.0]
    for _ in range(k):
        st = [st[0] + 1.0, st[1] * b1, st[2] * b2]
    return st


# ---- case lists, built from the launch regimes ---------------------------------------------------------------------------------
SUM_N = [1, 255, 256, 257, 2048, 2049, 70001, MAX_PARTIALS * 2048 + 2049]         # 70001: 35 partials, strictly inside
BWD_N = [1, 257, GRID_CAP["loss"] * 256 + 257]
TARGETS = [1.0, 0.0, 0.83]
AFFINE = [(1.0, -1.0, 1), (1.0, 1.0, 1), (0.0, -1.0, 0), (0.5, 2.0, 0)]           # hinge D real / fake, generator, plain
BCE_LIMIT = 12.0
SATURATED = [17.0, -17.0, 40.0, -40.0, 100.0, -100.0]
ROWS_INNER = [1, 255, 256, 257, 1027]
ROWS = [1, 5]
CE_K = [1, 63, 256, 257, 2049]
CE_B = [1, 5]
CE_SCALES = [1.0, 20.0]
WSUM_N = [1, 257, 2051]


def sum_cases():
    """[(op, par, n, family)]: every op at every n, the families and targets going round so that each n meets each of them
    for some op; the capped-grid size runs all three targets"""
    out = []
    for i, n in enumerate(SUM_N):
        for j, t in enumerate(TARGETS):
            if n == SUM_N[-1] or (i + j) % 2 == 0 or n <= 257:
                out.append(("bce", t, n, FAMILIES[(i + j) % 4]))
                out.append(("mse", t, n, FAMILIES[(i + j + 1) % 4]))
        for j, par in enumerate(AFFINE):
            out.append(("affine", par, n, FAMILIES[(i + j + 2) % 4]))
    return out


def sum_input(op, par, n, fam, planted=False):
    """x of a two-stage case.  The last element of the capped-grid case is 64 times the typical magnitude (one dropped
    typical term of 2.1 M lies below the resolution of a float32 sum; this one does not).  `planted` (affine): exact kink
    values a + b x == 0 in fused and unfused evaluation, every 5th element, the last included"""
    g = gen(17 * n + 3 * FAMILIES.index(fam) + len(op))
    x = family((n,), fam, g, BCE_LIMIT if op == "bce" else None)
    if op == "affine" and par[2]:
        x = off_kink(x, f32(par[0]), f32(par[1]))
        if planted:
            x[::5] = -par[0] / par[1]
            x[-1] = -par[0] / par[1]
    if n == SUM_N[-1] and not planted:
        big = 64.0 * float(x.abs().mean())
        x[-1] = -12.0 if op == "bce" else (math.copysign(big, par[1]) if op == "affine" else big)
    return x


def ce_labels(B, K):
    """labels 0, K-1, then the ignored -100, -1 and K (B = 5); B = 1 takes the one at position K % 5"""
    lab = [0, K - 1, -100, -1, K]
    return torch.tensor(lab if B == 5 else [lab[K % 5]], dtype=torch.int64)


def ce_input(B, K, fam, seed=0):
    g = gen(1000 * seed + 31 * K + B)
    if fam == "cosine":
        return (torch.rand(B, K, generator=g) * 2.0 - 1.0).float()
    return family((B, K), fam, g)


def ce_cases():
    """[(B, K, scale, family, grad_rows given)]"""
    out = []
    for i, K in enumerate(CE_K):
        for j, B in enumerate(CE_B):
            for k, sc in enumerate(CE_SCALES):
                # scale 20 on the scales family would put 2e4 into exp's argument: the recipe's logits are cosines
                out.append((B, K, sc, "cosine" if (sc != 1.0 or (i + j) % 2 == 0) else "scales", (i + j + k) % 2 == 0))
    return out


# max-pool (H, W, KH, KW, SH, SW, PH, PW)
POOL_GEOM = [(H, W, 3, 3, 2, 2, 1, 1) for H, W in [(1, 1), (2, 3), (7, 8), (17, 9), (18, 12)]] + [
    (7, 8, 2, 2, 2, 2, 0, 0), (6, 9, 3, 3, 1, 1, 1, 1), (9, 11, 3, 2, 2, 3, 1, 0)]
POOL_FAMILIES = ("relu", "ties", "signed_zero", "nan", "two_nan", "neg_inf")
POOL_NC = [(1, 1), (2, 5), (1, 7)]                                  # N C = 1; 10 and 7 planes: no multiple of anything in the launch
POOL_BIG = (1, 60000, 12, 12, 3, 3, 2, 2, 1, 1)                     # N C P Q = 60000 * 36 > 8192 * 256: the second trip


def pool_input(N, C, H, W, fam, seed=0):
    """relu: post-ReLU zeros; ties: values from {0, 1, 2}, equal maxima in most windows; signed_zero: only -0.0 and 0.0;
    nan: relu with a NaN every 7th element; two_nan: every 2nd; neg_inf: planes 0 all -inf, the rest relu"""
    g = gen(100 * seed + 7 * H + W + N * C)
    x = torch.randn(N, C, H, W, generator=g).relu()
    if fam == "ties":
        x = torch.randint(0, 3, (N, C, H, W), generator=g).float()
    elif fam == "signed_zero":
        x = torch.where(torch.rand(N, C, H, W, generator=g) < 0.5, torch.tensor(-0.0), torch.tensor(0.0))
    elif fam in ("nan", "two_nan"):
        x.reshape(-1)[::7 if fam == "nan" else 2] = float("nan")
    elif fam == "neg_inf":
        x[0, 0] = float("-inf")
    return x.contiguous()


def pool_cases():
    """[(N, C, geometry, family)]: every geometry meets every family over the list"""
    out = []
    for i, geo in enumerate(POOL_GEOM):
        for j, fam in enumerate(POOL_FAMILIES):
            if (i + j) % 2 == 0 or fam in ("relu", "ties"):
                out.append(POOL_NC[(i + j) % 3] + (geo, fam))
    return out


GAP_HW = [1, 63, 64, 65, 128, 4097]
GAP_PLANES = [(1, 1), (1, 4), (1, 5)]
GEM_P = [1.0, 3.0, 6.5]


def gem_input(N, C, HW, seed=0):
    """|randn| with values below, at and above float32(1e-6), negatives, and plane 0 entirely clamped (when there is another)"""
    g = gen(50 * seed + HW + N * C)
    x = torch.randn(N, C, HW, generator=g).abs() + 0.05
    e = torch.tensor(1e-6, dtype=torch.float32)
    vals = torch.stack([e, e * 0.5, torch.nextafter(e, torch.tensor(1.0)), torch.tensor(-0.3), torch.tensor(0.0)])
    flat = x.reshape(-1)
    idx = torch.arange(0, flat.numel(), 6)
    flat[idx] = vals[torch.arange(idx.numel()) % 5]
    if N * C > 1:
        x[0, 0] = torch.tensor([-1.0, 0.0, 5e-7])[torch.arange(HW) % 3]
    return x.contiguous()


CM_D = [1, 64, 255, 256, 257, 2048, 4095, 4096]
CM_B = [1, 8, 24]
CM_K = 11
CM_MOM = [0.0, 0.2, 1.0]
CM_MIXED = [3, 3, 7, 3, 9, 7, 7, 3]                                  # the pattern of tests/test_ops_gpu.py


def cm_labels(pattern, B):
    if pattern == "distinct":
        return torch.arange(B) % CM_K if B <= CM_K else torch.arange(B) % CM_K       # B = 24: chains of 2 or 3 links
    if pattern == "equal":
        return torch.full((B,), 4, dtype=torch.int64)
    if pattern == "mixed":
        return torch.tensor((CM_MIXED * 3)[:B])
    if pattern == "ends":
        return torch.tensor(([0, CM_K - 1] * B)[:B])
    if pattern == "skipped":
        return torch.tensor(([-1, 2, CM_K, 2, -1, 5] * B)[:B])
    raise ValueError(pattern)


CM_PATTERNS = ("distinct", "equal", "mixed", "ends", "skipped")


def cm_input(B, D, seed=0, tie=False):
    """unit rows (the bank and the batch are normalised features); D = 1 rows are +-1.  tie: sample 3 repeats sample 1 bit for
    bit (both carry label 3 in the mixed pattern)"""
    g = gen(10 * seed + 3 * D + B)
    feats = torch.nn.functional.normalize(torch.randn(CM_K, D, generator=g).double(), dim=1).float()
    x = torch.nn.functional.normalize(torch.randn(B, D, generator=g).double(), dim=1).float()
    if tie and B > 3:
        x[3] = x[1]
    return x.contiguous(), feats.contiguous()


def cm_cases():
    """[(B, D, pattern, momentum, normalize_eps)]: every D with every B, patterns and momenta going round"""
    out = []
    i = 0
    for D in CM_D:
        for B in CM_B:
            out.append((B, D, CM_PATTERNS[i % 5], CM_MOM[(i // 2) % 3] if i % 4 == 3 else 0.2, i % 2))
            i += 1
    out += [(8, 257, pat, mom, 0) for pat in CM_PATTERNS for mom in CM_MOM]
    return out


NLR_N = [1, 4, 5]
NLR_D = [1, 63, 64, 65, 2048]

ADAM_N = [1, 2, 3, 4, 5, 7, 1003]
ADAM_BIG = 4 * GRID_CAP["optim"] * 256 + 7                          # second trip of the float4 loop plus a tail
DEV_BIG = GRID_CAP["optim"] * 256 + 3                                # rg_adam_step_dev and rg_sgd_step
ADAM_STEPS = [1, 2, 1000]
ADAM_BETAS = [(0.5, 0.999), (0.9, 0.999)]
ADAM_WD = [0.0, 5e-4]
GSCALES = [1.0, 0.125]


def optim_input(n, fam, seed=0):
    """p, g, m, v; fam 'scales': v over ten decades.  Element 0 has g = m = v = 0 (with weight_decay 0: p unchanged, no NaN)"""
    gg = gen(7 * seed + n % 100003)
    p, g, m = torch.randn(n, generator=gg), torch.randn(n, generator=gg), torch.randn(n, generator=gg) * 0.1
    v = torch.rand(n, generator=gg) * 0.01 + 1e-4
    if fam == "scales":
        v = 10.0 ** (torch.rand(n, generator=gg) * 10.0 - 8.0)
    g[0], m[0], v[0] = 0.0, 0.0, 0.0
    return p.float(), g.float(), m.float(), v.float()


def adam_cases():
    """[(n, step, betas, weight_decay, grad_scale, family)]"""
    out = []
    for i, n in enumerate(ADAM_N + [ADAM_BIG]):
        for j, step in enumerate(ADAM_STEPS):
            if n == ADAM_BIG and j:
                continue
            out.append((n, step, ADAM_BETAS[(i + j) % 2], ADAM_WD[(i + j // 2) % 2], GSCALES[(i + j) % 2], "scales" if (i + j) % 3 == 0 else "plain"))
    return out
