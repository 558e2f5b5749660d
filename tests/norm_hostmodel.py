"""Host model of the normalisation units csrc/norm_bn.hip, norm_instnorm.hip and norm_fold.hip — the comparison partner of
tests/test_norm_elementwise_gpu.py, tied to float32 torch by tests/test_norm_hostmodel_cpu.py.  No tests and no GPU here.

Three parts:

  dispatch mirrors   bn_reg_units, in_lanes / in_regime, pick_slices, bn_train_fused_ok, channel_sum_ok: the host arithmetic that
                     picks a kernel, a few lines each, so that the case lists below are BUILT from the launch regimes.
  fp64 references    closed forms of every entry point (forward, running statistics, backward in train and frozen-statistics form,
                     the sums and the fold helpers).  The backward takes the mask from the y_act it is handed — the kernel's
                     contract — so no element ever has to be left out of a comparison.
  error budgets      every reference tensor comes as Ref(value, M, kind); an element passes when
                         |got - value| <= C_KIND[kind] * 2^-24 * M
                     with M the fp64 sum of the absolute values of the terms THAT element is made of (never a tensor-wide maximum).
                     K = 1 + |mean| * invstd is the condition of the channel / instance:
                         y             (K + |xhat|) |gamma| + |beta| + |residual|
                         mean          mean |x|
                         invstd        invstd                                   (relative)
                         running_mean  (1 - m) |old| + m * M_mean
                         running_var   (1 - m) old + m * var_unbiased           (relative)
                         sums          sum |term|
                         sum_g_xhat    sum |g| (|xhat| + K)
                         dx (train)    |gamma| invstd K (|g| + sum|g| / cnt + (|xhat| + 1) sum(|g| (|xhat| + K)) / cnt)
                         dx (frozen)   |gamma| invstd |g|                       (two products behind one rsqrt)
                         dres, g       exact (dy times 1, 0 or slope, the correctly rounded float32 product): M = 0
                         fold          scale, invstd relative; shift |beta| + |mean scale|
                         scale_rows    |w scale|                                (one rounding)

The constants C_KIND are NOT taken from the kernels.  tests/test_norm_hostmodel_cpu.py evaluates every case of the lists below with
plain float32 torch on the CPU (F.batch_norm / F.instance_norm, float32 autograd fed the reference's mask, float32 sums), records
max err / (2^-24 M) per kind, and C_KIND = max(8, 4 x that ratio): 4 for another summation order and the hardware rsqrt, the
floor of 8 so that a lucky CPU run cannot make the budget tighter than two roundings per term.  Measured (torch 2.10, CPU):

    kind           float32 torch ratio    C_KIND
    y              2.30                   9.2
    mean           2.86                   11.44
    invstd         1.69                   8
    running_mean   1.50                   8
    running_var    1.97                   8
    sum            1.56                   8
    sum_g_xhat     0.44                   8
    dx             2.46                   9.84
    fold           3.28                   13.14
    scale_rows     1.00                   8
    exact          0                      0
"""
import collections

import torch
import torch.nn.functional as F

U24 = 2.0 ** -24
ACT_NONE, ACT_RELU, ACT_LEAKY = 0, 1, 2
FILL = -7777.0                      # guard / untouched-output fill value of the device tests

C_KIND = {"y": 9.2, "mean": 11.44, "invstd": 8.0, "running_mean": 8.0, "running_var": 8.0, "sum": 8.0, "sum_g_xhat": 8.0,
          "dx": 9.84, "fold": 13.14, "scale_rows": 8.0, "exact": 0.0}

Ref = collections.namedtuple("Ref", "value M kind")


# ---- dispatch mirrors --------------------------------------------------------------------------------------------------------
def bn_reg_units(N, C, HW):
    """bn_reg_units(): float4 units per thread of bn_train_*_reg_kernel<U>, 0 = the loop kernels"""
    if (HW & 3) or N * C * HW * 4 >= (1 << 31):
        return 0
    per = (N * (HW >> 2) + 255) // 256
    if per > 16:
        return 0
    return 1 if per <= 1 else 2 if per <= 2 else 4 if per <= 4 else 8 if per <= 8 else 16


def bn_per(N, HW):
    """`per` of bn_reg_units(): float4 units per thread before rounding up to U"""
    return (N * (HW >> 2) + 255) // 256


def in_lanes(HW):
    """in_lanes(): lanes per instance"""
    if HW > 2048:
        return 256
    units = HW if (HW & 3) else HW >> 2
    return 16 if units <= 32 else 32 if units <= 64 else 64


def in_regime(N, C, HW):
    """rg_instnorm_fwd / rg_instnorm_bwd: (LANES, U) of the register kernel, U = 0 for the loop kernel instnorm_*_kernel<LANES>"""
    lanes = in_lanes(HW)
    per = 0 if (HW & 3) else ((HW >> 2) + lanes - 1) // lanes
    if 1 <= per <= 8 and N * C * HW * 4 < (1 << 31):
        return lanes, (1 if per <= 1 else 2 if per <= 2 else 4 if per <= 4 else 8)
    return lanes, 0


def in_per(HW):
    lanes = in_lanes(HW)
    return ((HW >> 2) + lanes - 1) // lanes


IN_SWITCH = [(16, 1), (16, 2), (32, 1), (32, 2), (64, 1), (64, 2), (64, 4), (64, 8), (256, 1), (256, 2), (256, 4), (256, 8)]


def in_reachable(limit=1 << 16):
    """every (LANES, U) that in_regime can select (HW % 4 == 0 up to `limit`)"""
    return sorted(set(in_regime(1, 1, hw) for hw in range(4, limit, 4)) - set((l, 0) for l in (16, 32, 64, 256)))


def pick_slices(N, C, HW):
    """pick_slices(): (S, L) — S slices of L elements (a multiple of 4) over the N*HW values of a channel"""
    total = N * HW
    S = min(-(-2048 // C), -(-total // 4096))
    S = max(S, 1)
    L = (-(-total // S) + 3) & ~3
    return -(-total // L), L


def bn_train_fused_ok(N, C, HW):
    """rg_bn_train_fused_ok()"""
    return N * HW <= 16384 and C >= 128


def channel_sum_ok(N, C, HW):
    """rg_channel_sum_ok()"""
    return N * HW <= 32768 and N * C * HW * 4 < (1 << 31)


# ---- fp64 references ---------------------------------------------------------------------------------------------------------
def _d(t):
    return None if t is None else t.detach().double()


def _pc(v, C):
    """per-channel vector -> [1][C][1]"""
    return None if v is None else _d(v).reshape(1, C, 1)


def act_grad(y_act, act, slope):
    """act'(y) from the forward OUTPUT: y > 0 is positive; 0.0 and -0.0 are not (torch's convention)"""
    y = _d(y_act)
    if act == ACT_RELU:
        return (y > 0).double()
    if act == ACT_LEAKY:
        return torch.where(y > 0, torch.ones_like(y), torch.full_like(y, float(slope)))
    return torch.ones_like(y)


def apply_act(z, act, slope):
    if act == ACT_RELU:
        return torch.where(z > 0, z, torch.zeros_like(z))
    if act == ACT_LEAKY:
        return torch.where(z > 0, z, z * float(slope))
    return z


def _masked(dy, y_act, act, slope):
    """g = dy * act'(y_act) as float32 arithmetic gives it: the product of two floats is exact in fp64, and rounding it to float32
    is the correctly rounded float32 product (slope is the float32 the kernel receives) — so g, dres are compared EXACTLY"""
    if act == ACT_NONE:
        return dy
    fac = act_grad(y_act, act, float(torch.tensor(slope, dtype=torch.float32)))
    return (dy * fac).float().double()


def _dims(kind):
    return (0, 2) if kind == "bn" else (2,)


def forward(kind, x, gamma=None, beta=None, residual=None, eps=1e-5, act=ACT_NONE, slope=0.0, running_mean=None,
            running_var=None, momentum=0.1, frozen=None, stat_is_var=True):
    """kind 'bn' (statistics over n and the pixels) or 'in' (per instance) on x[N][C][HW].  frozen = (mean[C], stat[C]): normalise
    with these instead of the batch statistics; stat is a variance (eval mode) or, with stat_is_var False, an invstd taken as it
    is.  -> dict of Ref; statistics are [C] ('bn') or [N*C] ('in')."""
    N, C, HW = x.shape
    xd = _d(x)
    dims = _dims(kind)
    cnt = float(N * HW if kind == "bn" else HW)
    out = {}
    if frozen is None:
        mean = xd.mean(dims, keepdim=True)
        var = ((xd - mean) ** 2).mean(dims, keepdim=True)
        out["mean"] = Ref(mean.reshape(-1), xd.abs().mean(dims).reshape(-1), "mean")
    else:
        mean, var = _pc(frozen[0], C), _pc(frozen[1], C)
    invstd = (var + eps).rsqrt() if stat_is_var or frozen is None else var
    out["invstd"] = Ref(invstd.reshape(-1), invstd.reshape(-1), "invstd")
    K = 1.0 + mean.abs() * invstd
    xhat = (xd - mean) * invstd
    g_, b_, r_ = _pc(gamma, C), _pc(beta, C), _d(residual)
    z = xhat if g_ is None else xhat * g_
    M = (K + xhat.abs()) * (1.0 if g_ is None else g_.abs())
    if b_ is not None:
        z, M = z + b_, M + b_.abs()
    if r_ is not None:
        z, M = z + r_, M + r_.abs()
    out["y"] = Ref(apply_act(z, act, slope), M, "y")
    if kind == "bn" and frozen is None and running_mean is not None:
        rm = _d(running_mean)
        out["running_mean"] = Ref((1 - momentum) * rm + momentum * out["mean"].value,
                                  (1 - momentum) * rm.abs() + momentum * out["mean"].M, "running_mean")
    if kind == "bn" and frozen is None and running_var is not None:
        unb = var.reshape(-1) * (cnt / (cnt - 1.0)) if cnt > 1 else var.reshape(-1)
        rv = (1 - momentum) * _d(running_var) + momentum * unb
        out["running_var"] = Ref(rv, rv, "running_var")
    return out


def backward(kind, x, dy, y_act, mean, invstd, gamma=None, act=ACT_NONE, slope=0.0, train=True):
    """closed-form backward from the tensors the kernel is handed: g = dy * act'(y_act); sum_g, sum_g_xhat; dres = g;
    dx = gamma invstd (g - train (sum_g / cnt + xhat sum_g_xhat / cnt)).  mean / invstd: [C] ('bn') or [N*C] ('in'), the
    normalising statistics (batch or frozen).  'in' also returns sum_dx, the per-instance sum of the reference dx."""
    N, C, HW = x.shape
    xd, g = _d(x), _d(dy)
    dims = _dims(kind)
    cnt = float(N * HW if kind == "bn" else HW)
    shp = (1, C, 1) if kind == "bn" else (N, C, 1)
    mu, is_ = _d(mean).reshape(shp), _d(invstd).reshape(shp)
    g = _masked(g, y_act, act, slope)
    ga = g.abs()
    K = 1.0 + mu.abs() * is_
    xhat = (xd - mu) * is_
    s1, s2 = g.sum(dims, keepdim=True), (g * xhat).sum(dims, keepdim=True)
    m1, m2 = ga.sum(dims, keepdim=True), (ga * (xhat.abs() + K)).sum(dims, keepdim=True)
    gs = is_ if gamma is None else _pc(gamma, C) * is_
    out = {"dres": Ref(g, torch.zeros_like(g), "exact"),
           "sum_g": Ref(s1.reshape(-1), m1.reshape(-1), "sum"),
           "sum_g_xhat": Ref(s2.reshape(-1), m2.reshape(-1), "sum_g_xhat")}
    if train:
        out["dx"] = Ref(gs * (g - s1 / cnt - xhat * s2 / cnt),
                        gs.abs() * K * (ga + m1 / cnt + (xhat.abs() + 1.0) * m2 / cnt), "dx")
    else:
        out["dx"] = Ref(gs * g, gs.abs() * ga, "dx")
    if kind == "in":
        out["sum_dx"] = Ref(out["dx"].value.sum(2).reshape(-1), out["dx"].M.sum(2).reshape(-1), "sum")
    return out


def channel_sum(dy):
    d = _d(dy)
    return Ref(d.sum((0, 2)), d.abs().sum((0, 2)), "sum")


def rows_sum(a):
    d = _d(a)
    return Ref(d.sum(0), d.abs().sum(0), "sum")


def bn_fold(gamma, beta, mean, var, eps):
    is_ = (_d(var) + eps).rsqrt()
    sc = is_ if gamma is None else _d(gamma) * is_
    sh = -_d(mean) * sc
    M = sh.abs()
    if beta is not None:
        sh, M = sh + _d(beta), M + _d(beta).abs()
    return {"scale": Ref(sc, sc.abs(), "fold"), "shift": Ref(sh, M, "fold"), "invstd": Ref(is_, is_, "fold")}


def scale_rows(w, scale):
    K = w.shape[0]
    v = _d(w).reshape(K, -1) * _d(scale).reshape(K, 1)
    return Ref(v.reshape(w.shape), v.abs().reshape(w.shape), "scale_rows")


def act_bwd(dy, y_act, act, slope):
    """g = dy * act'(y_act) (exact) and its channel sums"""
    g = _masked(_d(dy), y_act, act, slope)
    return {"g": Ref(g, torch.zeros_like(g), "exact"), "sum_g": Ref(g.sum((0, 2)), g.abs().sum((0, 2)), "sum")}


def bn_fold_wgrad(w, G, scale, invstd, mean, sum_g):
    """dgamma[k] = invstd (sum_m w G - mean sum_g), dW = scale G; w, G [K][M], sum_g the channel sums the kernel is handed"""
    wd, Gd = _d(w), _d(G)
    K = wd.shape[0]
    t, ta = (wd * Gd).reshape(K, -1).sum(1), (wd * Gd).abs().reshape(K, -1).sum(1)
    sg = _d(sum_g)
    dW = Gd * _d(scale).reshape(K, *([1] * (Gd.dim() - 1)))
    return {"dgamma": Ref(_d(invstd) * (t - _d(mean) * sg), _d(invstd) * (ta + (_d(mean) * sg).abs()), "sum"),
            "dW": Ref(dW, dW.abs(), "scale_rows")}


# ---- the comparator ----------------------------------------------------------------------------------------------------------
Worst = collections.namedtuple("Worst", "ok index err budget ratio")


def compare(got, ref):
    """per-element check of `got` (any float tensor) against ref = Ref(value, M, kind); every element takes part.
    -> Worst(ok, index of the worst element, its error, its budget, max err / (2^-24 M) over the tensor)."""
    g = got.detach().double().cpu().reshape(-1)
    v, M = ref.value.reshape(-1), ref.M.reshape(-1)
    assert g.numel() == v.numel(), ("shape", tuple(got.shape), tuple(ref.value.shape))
    err = (g - v).abs()
    err = torch.where(torch.isfinite(g), err, torch.full_like(err, float("inf")))
    bud = C_KIND[ref.kind] * U24 * M
    over = err - bud
    i = int(torch.argmax(torch.where(torch.isnan(over), torch.full_like(over, float("inf")), over)))
    unit = U24 * M
    ratio = torch.where(err > 0, err / unit.clamp_min(1e-300), torch.zeros_like(err))
    idx = tuple(int(k) for k in torch.unravel_index(torch.tensor(i), tuple(ref.value.shape))) if ref.value.dim() else ()
    return Worst(bool((err <= bud).all()), idx, float(err[i]), float(bud[i]), float(ratio.max()) if ratio.numel() else 0.0)


def check(got, ref, what):
    """assert with the entry point / case / output in `what`, the worst index, its error and its budget"""
    w = compare(got, ref)
    assert w.ok, "%s: worst element %s err %.3e > budget %.3e (%s, max err/(2^-24 M) = %.2f)" % (
        what, w.index, w.err, w.budget, ref.kind, w.ratio)
    return w.ratio


# ---- input families ----------------------------------------------------------------------------------------------------------
FAMILIES = ("plain", "scales", "offset", "constant", "masked")
Inputs = collections.namedtuple("Inputs", "x gamma beta residual dy running_mean running_var")


def make_inputs(kind, N, C, HW, family, seed=0):
    """float32 CPU tensors x, residual, dy [N][C][HW]; gamma, beta, running_mean, running_var [C].  The family is applied per
    channel:
      plain     randn * 1.7 + 0.3 in every channel
      scales    channel c times 10^linspace(-3, 3, C), gamma and dy divided by it
      offset    unit-variance channels at mean/std +30, -300, +30, ... (a post-ReLU tensor entering a norm)
      constant  plain, with channel 0 ('bn') / instance (0, 0) ('in') constant: xhat = 0, invstd = eps^-1/2
      masked    plain; masked_y_act() then plants 0.0 / -0.0 / denormals in the y_act of the backward"""
    assert family in FAMILIES
    g = torch.Generator().manual_seed(1000 * seed + 7 * N + 131 * C + HW)
    x = torch.randn(N, C, HW, generator=g) * 1.7 + 0.3
    res = torch.randn(N, C, HW, generator=g)
    dy = torch.randn(N, C, HW, generator=g)
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g)
    gamma = gamma * (1 - 2 * (torch.arange(C) % 2 == 1).float())            # both signs
    rm, rv = torch.randn(C, generator=g) * 0.1, torch.rand(C, generator=g) + 0.5
    if family == "scales":
        s = (10.0 ** torch.linspace(-3, 3, C)).reshape(1, C, 1)
        x, gamma, dy = x * s, gamma / s.reshape(C), dy / s
    elif family == "offset":
        m = torch.tensor([30.0, -300.0])[torch.arange(C) % 2].reshape(1, C, 1)
        x = (x - 0.3) / 1.7 + m
    elif family == "constant":
        if kind == "bn":
            x[:, 0, :] = 0.7
        else:
            x[0, 0, :] = 0.7
    return Inputs(x.contiguous(), gamma, beta, res, dy.contiguous(), rm, rv)


def masked_y_act(y_act):
    """plant exact 0.0, -0.0 and denormal-sized positive / negative entries in a copy of y_act (float32), every 3rd element in
    turn, the last four elements of the tensor included (the last float4 of the last row)"""
    y = y_act.detach().float().clone().reshape(-1)
    vals = torch.tensor([0.0, -0.0, 1e-40, -1e-40], dtype=torch.float32)
    idx = torch.arange(0, y.numel(), 3)
    y[idx] = vals[torch.arange(idx.numel()) % 4]
    n = y.numel()
    if n >= 4:
        y[n - 4:] = vals
    return y.reshape(y_act.shape)


# ---- case lists, built from the launch regimes ---------------------------------------------------------------------------------
# rg_bn_train_*_fused, (N, HW): per = ceil(N * HW / 4 / 256) float4 units per thread, rounded up to U
BN_ONE_LAUNCH = [
    (2, 64), (4, 256),             # U = 1: 32 units (ragged: 224 idle threads), 256 units (full)
    (3, 344), (2, 1024),           # U = 2: 258 units (ragged), 512 (full)
    (3, 1028), (4, 1024),          # U = 4: per = 4 with a ragged last unit row (771 units), full
    (5, 820), (8, 1024),           # U = 8: per = 5 (1025 units: three unit rows of sentinels), full
    (3, 2732), (16, 1024),         # U = 16: per = 9 (2049 units), full = the largest one-launch geometry
    (1, 16388),                    # per = 17: loop kernel on float4 rows
    (5, 21), (3, 5462),            # scalar rows: loop kernel
]
BN_C = [3, 4, 5, 6, 7, 3, 4, 5, 6, 3, 7, 5, 4]
BN_WIDE = (4, 130, 36)             # C >= 128: the geometry the module-level bn_train_fused_ok route accepts (ragged U = 1)

# rg_instnorm_*, HW -> (LANES, U); N * C of 5, 6, 17 leave a partly empty last workgroup at 16, 8 and 4 instances per workgroup
IN_HW = [36, 64, 68, 128, 132, 256, 260, 512, 516, 1024, 1028, 2048, 2052, 4096, 4100, 8192, 8196, 9, 63, 130, 2050]
IN_NC = [(1, 5), (2, 3), (1, 17)]

# two-stage / eval kernels (N, C, HW) by pick_slices
SLICE_CASES = [
    (2, 3, 64),                    # S = 1, float4 rows, fewer units than threads
    (5, 4, 21),                    # S = 1, scalar rows, 105 elements for 256 threads
    (16, 3, 1024),                 # S = 4 slices of exactly 4096
    (3, 3, 4100),                  # S = 4, L = 3076: boundaries mid-row, ragged last slice (3072)
    (3, 5, 5462),                  # scalar rows, S = 5, L = 3280: boundaries mid-row, ragged last slice
]


ACTS = [(ACT_RELU, 0.0), (ACT_LEAKY, 0.2), (ACT_NONE, 0.0)]


def case_act(i, family):
    """(act, slope) of case number i: the three in turn; a `masked` case always has a mask"""
    return ACTS[i % 2] if family == "masked" else ACTS[i % 3]


# rg_channel_sum (N, C, HW): both vector forms; N * HW of 1, 255 and 32768 (the one-launch limit); a single float4
CHANNEL_SUM_CASES = [(1, 3, 1), (3, 5, 85), (16384, 3, 2), (1, 4, 4), (8, 3, 4096)]


def bn_cases():
    """[(N, C, HW, family)]: the families go round the ragged and the full regimes separately, so each meets both"""
    out = []
    for i, ((N, HW), C) in enumerate(zip(BN_ONE_LAUNCH, BN_C)):
        out.append((N, C, HW, FAMILIES[(i // 2 + (i % 2) * 2) % 5] if i < 10 else FAMILIES[i % 5]))
    return out


def in_cases():
    out = []
    for i, HW in enumerate(IN_HW):
        N, C = IN_NC[i % 3]
        out.append((N, C, HW, FAMILIES[(i // 2 + (i % 2) * 2) % 5] if i < 16 else FAMILIES[i % 5]))
    return out


def slice_cases():
    return [(N, C, HW, FAMILIES[i % 5]) for i, (N, C, HW) in enumerate(SLICE_CASES)]


# ---- the same operations in plain float32 torch (the budget's yardstick, CPU) --------------------------------------------------
def torch32(kind, inp, eps, act, slope, y_act, momentum=0.1, frozen=None):
    """float32 F.batch_norm / F.instance_norm and float32 autograd of case `inp`; the backward's mask is taken from y_act (the
    tensor the kernels are handed), so that forward rounding cannot move an element across zero.  -> dict name -> float32 tensor"""
    N, C, HW = inp.x.shape
    x = inp.x.clone().requires_grad_(True)
    res = inp.residual.clone().requires_grad_(True)
    rm, rv = inp.running_mean.clone(), inp.running_var.clone()
    out = {}
    if kind == "bn":
        w, b = inp.gamma.clone().requires_grad_(True), inp.beta.clone().requires_grad_(True)
        if frozen is None:
            z = F.batch_norm(x, rm, rv, w, b, True, momentum, eps)
            out["running_mean"], out["running_var"] = rm, rv
            out["mean"] = inp.x.mean((0, 2))
            out["invstd"] = torch.rsqrt(inp.x.var((0, 2), unbiased=False) + eps)
        else:
            z = F.batch_norm(x, frozen[0].clone(), frozen[1].clone(), w, b, False, momentum, eps)
            out["invstd"] = torch.rsqrt(frozen[1] + eps)
    else:
        # instance_norm IS batch_norm on [1][N*C][HW] (torch implements it so); written out here so that the affine gradients
        # arrive per instance, as rg_instnorm_bwd produces them
        w, b = inp.gamma.repeat(N).requires_grad_(True), inp.beta.repeat(N).requires_grad_(True)
        z = F.batch_norm(x.reshape(1, N * C, HW), None, None, w, b, True, 0.0, eps).reshape(N, C, HW)
        out["y_instance_norm"] = F.instance_norm(inp.x, weight=inp.gamma, bias=inp.beta, eps=eps) + inp.residual
        out["mean"] = inp.x.mean(2).reshape(-1)
        out["invstd"] = torch.rsqrt(inp.x.var(2, unbiased=False) + eps).reshape(-1)
    z = z + res
    fwd = {ACT_NONE: lambda t: t, ACT_RELU: F.relu, ACT_LEAKY: lambda t: F.leaky_relu(t, slope)}[act]
    out["y"] = fwd(z.detach())
    if "y_instance_norm" in out:
        out["y_instance_norm"] = fwd(out["y_instance_norm"])
    y = z * act_grad(y_act, act, slope).float() if act != ACT_NONE else z      # backward: y = z * act'(y_act), a constant mask
    y.backward(inp.dy)
    out["dx"], out["dres"], out["sum_g"], out["sum_g_xhat"] = x.grad, res.grad, b.grad, w.grad
    if kind == "in":
        out["sum_dx"] = x.grad.sum(2).reshape(-1)
    return out
