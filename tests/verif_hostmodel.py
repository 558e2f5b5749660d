"""Host model of the fused verification head (csrc/verif_head.hip: rg_verif_head_fwd / rg_verif_head_bwd) — the comparison partner of
tests/test_verif_head_gpu.py, tied to float64 torch autograd, to values recorded from the reference's own modules
(tests/golden/reference_siamese.npz) and to float32 torch by tests/test_verif_hostmodel_cpu.py.  No tests and no GPU here.

    d = (x1 - x2)^2,  z = gamma (d - mean) invstd + beta,  logits = z W^T + bias,
    loss_b = logsumexp(logits_b) - logits_b[y_b],  loss = mean_b loss_b,  correct = #{b: argmax logits_b == y_b}  (lowest index on a tie)

`evaluate(inp, train, dtype)` is the arithmetic in plain torch of `dtype`; `head_fwd` / `head_bwd` put the float64 values together
with per-element error budgets in the Ref(value, M, kind) scheme of tests/head_hostmodel.py: an element passes when
    |got - value| <= C_KIND[kind] * 2^-24 * (M + 2^-102).

Budgets of the forward, every M the sum of the absolute terms that element is made of (in units of one rounding):
    d             E_d = 3 d                            (one rounding of x1 - x2, squared, one of the product)
    mean          mean_b (d + E_d)
    invstd        invstd (1 + S / (var + eps)),  S = mean_b |d - mean| (E_d + M_mean): what the roundings of d move the variance by
    running_mean  (1 - m) |old| + m M_mean;   running_var  (1 - m) old + m B / (B - 1) (var + 2 S)
    xhat          (d + E_d + M_mean) invstd + |xhat| M_invstd / invstd
    z             M_z = M_xhat |gamma| + |gamma xhat| + |beta|
    logits        M_l = sum_ch (|W| M_z + |W z|) + |bias| + |logit|
    loss_rows     sum_k p_k M_l[k] + M_l[y] + |lse| + |l_y| + 1;   loss: mean_b of that + |loss|
    dlogits       (p_k (M_l[k] + sum_j p_j M_l[j] + |l_k| + |lse| + 1) + onehot) / B
    correct / B   exact
A label outside [0, C) gives an exact 0 loss and an exact zero dlogits row.
Budgets of the backward.  It is handed the float32 xhat, invstd and dlogits of the forward reference and recomputes z from xhat:
    dl            g dlogits + up:  E_dl = |g dlogits| + |dl|
    z             E_z = |gamma xhat| + |beta|
    dz            sum_k dl_k W_k:  E_dz = sum_k (E_dl |W| + |dl W|)
    dW[k]         sum_b (E_dl |z| + |dl| E_z + |dl z|);     dbias[k]  sum_b (E_dl + |dl|)
    dbeta = s1    sum_b (E_dz + |dz|);     dgamma = s2   sum_b (E_dz |xhat| + |dz xhat|)
    dd            k (dz - s1 / B - xhat s2 / B), k = gamma invstd (train; eval: k dz):
                  M_dd = |k| (E_dz + |dz| + (E_s1 + |s1|) / B + |xhat| (E_s2 + 2 |s2|) / B) + |dd|
    dx1 = -dx2    2 (x1 - x2) dd:  2 |x1 - x2| M_dd + 2 |dx1|

The constants C_KIND are NOT taken from the kernels.  tests/test_verif_hostmodel_cpu.py evaluates every case of cases() with
`evaluate(..., torch.float32)` on the CPU (torch's own reductions, one thread), records max err / (2^-24 M) per kind, and
C_KIND = max(8, 4 x that ratio), the ratio first raised by 0.05 and rounded up to one decimal so that another torch build's last
digit does not fail the calibration test: 4 for another summation order and the hardware rsqrt / exp / log, the floor of 8 so that
a lucky CPU run cannot make a budget tighter than two roundings per term.  Measured (torch 2.10, CPU, one thread):

    kind           float32 torch ratio    C_KIND
    mean           0.93                   8
    invstd         1.71                   8
    running_mean   1.70                   8
    running_var    1.37                   8
    xhat           3.10 -> 3.2            12.8
    logits         0.75                   8
    ce             1.10                   8
    ce_bwd         1.13                   8
    dsum           1.10                   8
    dx             0.66                   8
"""
import collections

import torch

from tests.head_hostmodel import FAMILIES, FILL, TINY_M, U24, Ref, compare, exact, family, gen  # noqa: F401  (one scheme, one comparator)

C_KIND = {"mean": 8.0, "invstd": 8.0, "running_mean": 8.0, "running_var": 8.0, "xhat": 12.8, "logits": 8.0, "ce": 8.0, "ce_bwd": 8.0,
          "dsum": 8.0, "dx": 8.0, "exact": 0.0}

KCG = 16                            # kCG, verif_head.hip: channels per workgroup of the column phase (16 row slices each)
MAX_C = 16
EPS, MOM = 1e-5, 0.1                # BatchNorm1d's defaults, what EltwiseSubEmbed builds
# the smallest shapes at which the launch arithmetic changes: B around the 16 row slices, D around the 16-channel group, plus the
# stage-I problem itself; each axis is swept with the others small
SWEEP_B = [2, 15, 16, 17, 33, 256]
SWEEP_D = [1, 15, 16, 17, 100, 2048]
SWEEP_C = [1, 2, 3, 16]
STAGE1 = (256, 2048, 2)
PLANTED = ("identical", "bigmean", "ties", "ignored")
DEFECTS = ("biased_running_var", "no_1_over_B", "dx2_sign", "bn_bwd_no_mean", "dbias_axis", "tie_high")


def workspace_bytes(B, D, C):
    return (-(-D // KCG)) * B * C * 4


def _f32(v):
    return float(torch.tensor(float(v), dtype=torch.float32))


def make_input(B, D, C, fam="plain", seed=0, planted=None, bias=True, labels=True):
    """float32 inputs of one case as a dict.  planted: 'identical' — channels 0 and D - 1 have x1 == x2 (d == 0, a zero-variance
    channel, invstd = 1 / sqrt(eps)); 'bigmean' — channel 0 has d near 1e6 with a spread of a few units; 'ties' — integer-valued
    inputs and the last two rows of W equal, bias too: every row ties those two logits exactly; 'ignored' — labels -100 and C"""
    g = gen(100003 * seed + 1009 * B + 31 * D + C + 7 * FAMILIES.index(fam))
    x1, x2 = family((B, D), fam, g), family((B, D), fam, g)
    if fam == "constant":
        x2 = x1.clone()
    W = (torch.randn(C, D, generator=g) * 0.05).float()
    bs = (torch.randn(C, generator=g) * 0.1).float()
    gamma = ((torch.rand(D, generator=g) * 0.6 + 0.2) * torch.sign(torch.randn(D, generator=g))).float()
    beta = (torch.randn(D, generator=g) * 0.1).float()
    d = (x1.double() - x2.double()) ** 2
    rm = (d.mean(0) * (1.0 + 0.1 * torch.randn(D, generator=g).double())).float()
    rv = ((torch.rand(D, generator=g).double() * 0.4 + 0.8) * d.var(0, unbiased=False).clamp_min(1e-3)).float()
    y = torch.randint(0, C, (B,), generator=g)
    if planted == "identical":
        x2[:, 0], x2[:, D - 1] = x1[:, 0], x1[:, D - 1]
    elif planted == "bigmean":
        x1[:, 0] = 1000.0 + torch.randn(B, generator=g) * 1e-3
        x2[:, 0] = 0.0
    elif planted == "ties":
        x1 = torch.randint(-3, 4, (B, D), generator=g).float()
        x2 = torch.randint(-3, 4, (B, D), generator=g).float()
        W = torch.randint(-2, 3, (C, D), generator=g).float() * 0.25
        if C >= 2:
            W[C - 1], bs[C - 1] = W[C - 2], bs[C - 2]
    elif planted == "ignored":
        y[0], y[B - 1] = -100, C
    elif planted is not None:
        raise ValueError(planted)
    return {"x1": x1.contiguous(), "x2": x2.contiguous(), "gamma": gamma, "beta": beta, "rm": rm, "rv": rv, "W": W.contiguous(),
            "bias": bs if bias else None, "labels": y if labels else None, "eps": EPS, "mom": MOM}


def argmax_low(l):
    """index of the maximum of each row, the LOWEST index on a tie (written out: torch.argmax documents no tie rule)"""
    C = l.shape[1]
    idx = torch.arange(C).reshape(1, C).expand_as(l)
    return torch.where(l == l.max(1, keepdim=True).values, idx, torch.full_like(idx, C)).min(1).values


def argmax_high(l):
    C = l.shape[1]
    idx = torch.arange(C).reshape(1, C).expand_as(l)
    return torch.where(l == l.max(1, keepdim=True).values, idx, torch.full_like(idx, -1)).max(1).values


def evaluate(inp, train, dtype=torch.float64, defect=None):
    """the forward in tensors of `dtype` -> dict of plain tensors (logits, xhat, mean, invstd, running_mean, running_var and, with
    labels, loss_rows, out2, dlogits, correct).  defect: one of DEFECTS that touches the forward"""
    c = lambda t: None if t is None else t.detach().to(dtype)      # noqa: E731
    x1, x2, ga, be, W, bs = c(inp["x1"]), c(inp["x2"]), c(inp["gamma"]), c(inp["beta"]), c(inp["W"]), c(inp["bias"])
    rm, rv = c(inp["rm"]), c(inp["rv"])
    eps, m = _f32(inp["eps"]), _f32(inp["mom"])
    B, D = x1.shape
    C = W.shape[0]
    d = (x1 - x2) ** 2
    if train:
        mean = d.mean(0)
        var = ((d - mean) ** 2).mean(0)
        unb = var if defect == "biased_running_var" else var * (B / (B - 1.0))
        rm2, rv2 = (1 - m) * rm + m * mean, (1 - m) * rv + m * unb
    else:
        mean, var, rm2, rv2 = rm, rv, rm, rv
    invstd = (var + eps).rsqrt()
    xhat = (d - mean) * invstd
    z = xhat * ga + be
    logits = z @ W.t()
    if bs is not None:
        logits = logits + bs
    out = {"logits": logits, "xhat": xhat, "mean": mean, "invstd": invstd, "running_mean": rm2, "running_var": rv2, "d": d, "z": z,
           "var": var}
    y = inp["labels"]
    if y is not None:
        ok = (y >= 0) & (y < C)
        yc = y.clamp(0, C - 1).reshape(B, 1)
        lse = torch.logsumexp(logits, 1)
        ly = logits.gather(1, yc).reshape(B)
        rows = torch.where(ok, lse - ly, torch.zeros_like(lse))
        onehot = torch.zeros(B, C, dtype=dtype).scatter_(1, yc, 1.0)
        p = torch.exp(logits - lse.reshape(B, 1))
        scale = 1.0 if defect == "no_1_over_B" else 1.0 / B
        dl = torch.where(ok.reshape(B, 1), (p - onehot) * scale, torch.zeros_like(p))
        arg = argmax_high(logits) if defect == "tie_high" else argmax_low(logits)
        correct = int(((arg == y) & ok).sum())
        out.update({"loss_rows": rows, "out2": torch.stack([rows.sum() * scale, torch.tensor(correct / B, dtype=dtype)]),
                    "dlogits": dl, "correct": correct, "p": p, "lse": lse, "ly": ly, "ok": ok, "onehot": onehot})
    return out


def head_fwd(inp, train):
    """-> dict of Ref: logits, xhat, mean, invstd, running_mean, running_var and, with labels, loss_rows, out2, dlogits;
    plus 'correct' (the plain count)"""
    v = evaluate(inp, train)
    B, D = inp["x1"].shape
    C = inp["W"].shape[0]
    ga, be, W = inp["gamma"].double(), inp["beta"].double(), inp["W"].double()
    eps, m = _f32(inp["eps"]), _f32(inp["mom"])
    d, mean, var, invstd, xhat, z, logits = v["d"], v["mean"], v["var"], v["invstd"], v["xhat"], v["z"], v["logits"]
    Ed = 3.0 * d
    zero = torch.zeros(D, dtype=torch.float64)
    if train:
        Mmean = (d + Ed).mean(0)
        S = ((d - mean).abs() * (Ed + Mmean)).mean(0)
        Minv = invstd * (1.0 + S / (var + eps))
        Mrm = (1 - m) * inp["rm"].double().abs() + m * Mmean
        Mrv = (1 - m) * inp["rv"].double() + m * (B / (B - 1.0)) * (var + 2.0 * S)
    else:
        Mmean, Minv, Mrm, Mrv = zero, invstd, zero, zero
    Mxhat = (d + Ed + Mmean) * invstd + xhat.abs() * (Minv / invstd)
    Mz = Mxhat * ga.abs() + (ga * xhat).abs() + be.abs()
    Ml = Mz @ W.abs().t() + z.abs() @ W.abs().t() + logits.abs()
    if inp["bias"] is not None:
        Ml = Ml + inp["bias"].double().abs()
    out = {"logits": Ref(logits, Ml, "logits"), "xhat": Ref(xhat, Mxhat, "xhat"),
           "mean": Ref(mean, Mmean, "mean" if train else "exact"), "invstd": Ref(invstd, Minv, "invstd"),
           "running_mean": Ref(v["running_mean"], Mrm, "running_mean" if train else "exact"),
           "running_var": Ref(v["running_var"], Mrv, "running_var" if train else "exact")}
    if inp["labels"] is not None:
        p, lse, ly, ok, onehot = v["p"], v["lse"], v["ly"], v["ok"], v["onehot"]
        Ely = Ml.gather(1, inp["labels"].clamp(0, C - 1).reshape(B, 1)).reshape(B)
        Else = (p * Ml).sum(1)
        Mrows = torch.where(ok, Else + Ely + lse.abs() + ly.abs() + 1.0, torch.zeros_like(lse))
        loss = v["out2"][0]
        Mdl = torch.where(ok.reshape(B, 1), (p * (Ml + Else.reshape(B, 1) + logits.abs() + lse.abs().reshape(B, 1) + 1.0) + onehot) / B,
                          torch.zeros_like(p))
        out["loss_rows"] = Ref(v["loss_rows"], Mrows, "ce")
        out["loss"] = Ref(loss.reshape(1), (Mrows.mean() + loss.abs()).reshape(1), "ce")
        # the count times float32(1 / B), one float32 product, as `correct_k.mul_(1. / batch_size)` of the reference's `accuracy`
        out["prec"] = exact((torch.tensor([float(v["correct"])]) * torch.tensor(1.0 / B, dtype=torch.float32)))
        out["dlogits"] = Ref(v["dlogits"], Mdl, "ce_bwd")
        out["correct"] = v["correct"]
    return out


def bwd_terms(inp, xhat, invstd, dlogits, grad_loss, dlogits_up, train, dtype=torch.float64, defect=None):
    """the backward in tensors of `dtype` from the handed forward tensors -> dict of tensors (dx1, dx2, dW, dbias, dgamma, dbeta)
    and, in float64, their budgets under 'M'"""
    c = lambda t: None if t is None else t.detach().to(dtype)      # noqa: E731
    x1, x2, ga, be, W = c(inp["x1"]), c(inp["x2"]), c(inp["gamma"]), c(inp["beta"]), c(inp["W"])
    xh, iv = c(xhat), c(invstd)
    B, D = x1.shape
    C = W.shape[0]
    zero = torch.zeros(B, C, dtype=dtype)
    gl = 1.0 if grad_loss is None else float(c(grad_loss).reshape(-1)[0])
    a = zero if dlogits is None else gl * c(dlogits)
    up = zero if dlogits_up is None else c(dlogits_up)
    dl = a + up
    z = xh * ga + be
    dz = dl @ W
    s1, s2 = dz.sum(0), (dz * xh).sum(0)
    k = ga * iv
    m1 = 0.0 if defect == "bn_bwd_no_mean" else s1 / B
    dd = k * (dz - m1 - xh * s2 / B) if train else k * dz
    t = x1 - x2
    dx1 = 2.0 * t * dd
    out = {"dx1": dx1, "dx2": dx1 if defect == "dx2_sign" else -dx1, "dW": dl.t() @ z,
           "dbias": dl.sum(1)[:C] if (defect == "dbias_axis" and B >= C) else dl.sum(0), "dgamma": s2, "dbeta": s1}
    if dtype == torch.float64:
        Edl = a.abs() + dl.abs()
        Ez = (ga * xh).abs() + be.abs()
        Edz = Edl @ W.abs() + dl.abs() @ W.abs()
        Es1, Es2 = (Edz + dz.abs()).sum(0), (Edz * xh.abs() + (dz * xh).abs()).sum(0)
        if train:
            Mdd = k.abs() * (Edz + dz.abs() + (Es1 + s1.abs()) / B + xh.abs() * (Es2 + 2.0 * s2.abs()) / B) + dd.abs()
        else:
            Mdd = k.abs() * (Edz + dz.abs()) + dd.abs()
        Mdx = 2.0 * t.abs() * Mdd + 2.0 * dx1.abs()
        out["M"] = {"dx1": Mdx, "dx2": Mdx, "dW": Edl.t() @ z.abs() + dl.abs().t() @ Ez + dl.abs().t() @ z.abs(),
                    "dbias": (Edl + dl.abs()).sum(0), "dgamma": Es2, "dbeta": Es1}
    return out


def head_bwd(inp, xhat, invstd, dlogits, grad_loss, dlogits_up, train):
    """-> dict of Ref: dx1, dx2 ('dx'), dW, dbias, dgamma, dbeta ('dsum')"""
    t = bwd_terms(inp, xhat, invstd, dlogits, grad_loss, dlogits_up, train)
    return {k: Ref(t[k], t["M"][k], "dx" if k in ("dx1", "dx2") else "dsum") for k in ("dx1", "dx2", "dW", "dbias", "dgamma", "dbeta")}


def check(got, ref, what):
    w = compare(got, ref, C_KIND)
    assert w.ok, "%s: worst element %s err %.3e > budget %.3e (%s, max err/(2^-24 M) = %.2f)" % (
        what, w.index, w.err, w.budget, ref.kind, w.ratio)
    return w.ratio


Case = collections.namedtuple("Case", "B D C fam train planted bias labels")


SWEEP_FAMILIES = ("plain", "scales", "offset")      # `constant` (x1 == x2: d == 0 everywhere, xhat == 0) checks no statistic: extra cases only


def cases():
    """every axis swept with the others small, every sweep point in TRAIN mode (the column phase: 16 row slices, 16-channel groups,
    per-class partials) and in eval mode, on a non-degenerate family (plain / scales / offset going round so that each axis meets
    each); then the planted rows, NULL bias, NULL labels and the stage-I problem in both modes; then the `constant` family, whose
    d == 0 everywhere, as extra cases at the edges of the D sweep"""
    out, i = [], 0

    def add(B, D, C, train, fam="plain", planted=None, bias=True, labels=True):
        out.append(Case(B, D, C, fam, train, planted, bias, labels))
    for train in (1, 0):
        for B in SWEEP_B:
            add(B, 17, 2, train, SWEEP_FAMILIES[i % 3])
            i += 1
        i += 1
        for D in SWEEP_D:
            add(5, D, 2, train, SWEEP_FAMILIES[i % 3])
            i += 1
        i += 1
        for C in SWEEP_C:
            add(17, 33, C, train, SWEEP_FAMILIES[i % 3])
            i += 1
    for train in (1, 0):
        for pl in PLANTED:
            add(17, 33, 3, train, planted=pl)
        add(33, 100, 2, train, bias=False)
        add(33, 100, 2, train, labels=False)
        add(*STAGE1, train)
    add(16, 16, 16, 1, planted="ties")
    for train, (B, D, C) in ((1, (5, 15, 2)), (1, (17, 2048, 2)), (0, (17, 17, 16))):
        add(B, D, C, train, "constant")
    return out


def case_input(case, seed=0):
    return make_input(case.B, case.D, case.C, case.fam, seed, case.planted, case.bias, case.labels)


def case_upstream(case, seed=0):
    """(grad_loss, dlogits_up) of the case's backward: labels None — the upstream gradient alone; every third case — a grad_loss
    other than 1 together with an upstream gradient; else the plain loss.backward()"""
    g = gen(77 * seed + case.B + case.D + case.C)
    up = (torch.randn(case.B, case.C, generator=g) * 0.1).float()
    if not case.labels:
        return None, up
    if (case.B + case.D + case.C) % 3 == 0:
        return torch.tensor([0.37]), up
    return None, None
