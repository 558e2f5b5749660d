"""Host model of the second stage of the cascade evaluation (csrc/cascade.hip: rg_pair_score / rg_cascade_merge) — the comparison
partner of tests/test_cascade_gpu.py, tied to oracle.ref_torch (OEltwiseSubEmbed, o_cascade_second_stage) and to float32 torch
by tests/test_cascade_hostmodel_cpu.py.  No tests and no GPU here.

Pair (q, j) is probe row q against gallery row idx[q, j]:
    d = (probe_q - g)^2,  z = gamma (d - running_mean) rsqrt(running_var + eps) + beta,  logits = z W^T + bias,
    score = softmax(logits)[0]
which is `verif_hostmodel.evaluate(..., train=False)` on the expanded pairs.  References are Ref(value, M, kind) in the scheme of
tests/head_hostmodel.py: an element passes when |got - value| <= C_KIND[kind] * 2^-24 * (M + 2^-102).

Budgets.
    logits   the forward budget of verif_hostmodel in eval mode, unchanged:
                 M_l = sum_ch (|W| M_z + |W z|) + |bias| + |logit|,  M_z = |gamma| (4 d invstd + |xhat|) + |gamma xhat| + |beta|
             The kernel folds a = gamma invstd, t_c = W_c a and K_c = sum_ch beta W_c + bias_c and sums t_c (d - running_mean).
             That association has the same number of roundings per product as the unfolded chain ((d - mean) invstd, gamma xhat
             + beta, W z: three; gamma invstd, W a, t (d - mean): three), carried by the terms |W gamma xhat| and 4 |W gamma|
             d invstd that M_l holds twice and four times; the beta terms have one rounding each under |W| |beta|.  No extra term
             is needed, and none is added.  The budget does not police the ORDER of the subtraction: the expanded form A d + b
             (pair_values(defect='expanded_form'), the same value in exact arithmetic) evaluated in float32 on the planted
             `bigmean` channel reaches 0.36 of 2^-24 M_l against 0.15 for the mean-first form (D 2048; 0.34 against 0.13 at D
             65) — worse, and inside the budget, because d itself is only known to |t| d 2^-24 there and M_l counts that four
             times.  Subtracting the mean first is the kernel's contract (its source says so); the planted defect that the
             comparison must catch is the wrong VALUE, `mean_after_scale`.
    score    s = e_0 / sum_j e_j, e_j = exp(l_j - m), m = max_j l_j (the same float for every class, so its own error drops out):
             the argument of e_j carries the logit's error and one rounding of the difference, exp one rounding, the sum C - 1,
             the division one:
                 M_s = s (M_l[0] + |l_0 - m| + 1 + sum_j p_j (M_l[j] + |l_j - m| + 1) + C)
             The logit errors enter as C_KIND['logits'] 2^-24 M_l, so C_KIND['score'] >= C_KIND['logits'] is required (asserted).

C_KIND follows the project's rule, max(8, 4 x the float32-torch ratio on the CPU), the ratio first raised by 0.05 and rounded up to
one decimal; it is never taken from the kernels.  Measured (torch 2.10, CPU, one thread) over every case of pair_cases():

    kind      float32 torch ratio    C_KIND
    logits    0.50 (verif_hostmodel's constant, kept)    8
    score     0.39 -> 0.5                                8

The merge is a float32 numpy model in exactly the kernel's documented order (merge_model): its result is compared bit for bit.

Ordering.  A query row is DECIDED when every adjacent pair of its k sorted fp64 scores differs by more than the sum of the two
score budgets; on decided rows the stable order of the device scores must equal the model's.  At most one row in eight of a case
may be undecided (asserted for the model alone on the CPU).
"""
import collections
import math

import numpy as np
import torch

from tests import verif_hostmodel as vh
from tests.head_hostmodel import TINY_M, U24, Ref, compare, gen  # noqa: F401  (one scheme, one comparator)

C_KIND = {"logits": vh.C_KIND["logits"], "score": 8.0, "exact": 0.0}
EPS = vh.EPS

# ---- dispatch mirror (pair_plan, csrc/cascade.hip) -------------------------------------------------------------------------------
K_ROWS, NUM_CU = 4, 256
VEC4, SPLIT_K = 1, 2


def cdiv(a, b):
    return -(-a // b)


def regime(Q, k, D, C, aligned=True):
    """bits of rg_pair_score_regime"""
    vec = D % 4 == 0 and aligned
    s = min(cdiv(k, K_ROWS), cdiv(2 * NUM_CU, Q)) if Q < NUM_CU else 1
    per = cdiv(cdiv(k, s), K_ROWS) * K_ROWS
    return (VEC4 if vec else 0) | (SPLIT_K if cdiv(k, per) > 1 else 0)


# ---- inputs ----------------------------------------------------------------------------------------------------------------------
PLANTED = ("var0", "bigmean", "ties", "far_low", "far_high")
PairCase = collections.namedtuple("PairCase", "Q G k D C planted bias")


def weight_std(D):
    """std of the classifier weights: 0.05 at D <= 64, scaled by sqrt(64 / D) above so that the softmax does not saturate"""
    return 0.05 * math.sqrt(64.0 / max(D, 64))


def make_idx(Q, G, k, g):
    """int32 [Q, k], distinct within a row (what a top-k yields).  Gallery row 0 is listed first by EVERY query (one row under
    several queries, index 0), row G - 1 closes query 0's list (k >= 2) or is query Q - 1's only entry (k == 1, Q >= 2)"""
    idx = torch.empty((Q, k), dtype=torch.int64)
    for q in range(Q):
        rest = (torch.randperm(G - 1, generator=g) + 1).tolist()
        row = [0] + rest
        if q == 0 and 2 <= k < G:
            row.remove(G - 1)
            row.insert(k - 1, G - 1)
        if k == 1 and Q >= 2 and q == Q - 1:
            row = [G - 1]
        idx[q] = torch.tensor(row[:k])
    return idx.to(torch.int32)


def make_input(Q, G, k, D, C, seed=0, planted=None, bias=True):
    """float32 inputs of one case.  The last query EQUALS gallery row 0, which it lists first (k >= 2 or Q == 1): d == 0 there.
    planted: 'var0' — running_var == 0 in channels 0 and D - 1 (invstd = 1 / sqrt(eps)); 'bigmean' — channel 0 has d near 1e4
    with a spread of about 1 and running_mean 1e4; 'ties' — integer-valued inputs, every row of W and every bias equal: all
    logits of a pair are the same float, score exactly 1 / C; 'far_low' / 'far_high' — bias[0] = -200 / +200: logits 200 apart"""
    g = gen(900001 * seed + 7919 * Q + 131 * G + 17 * k + 3 * D + C)
    probe, gallery = torch.randn(Q, D, generator=g), torch.randn(G, D, generator=g)
    idx = make_idx(Q, G, k, g)
    if int(idx[Q - 1, 0]) == 0:
        probe[Q - 1] = gallery[0]
    W = torch.randn(C, D, generator=g) * weight_std(D)
    bs = torch.randn(C, generator=g) * 0.1
    gamma = (torch.rand(D, generator=g) * 0.6 + 0.2) * torch.sign(torch.randn(D, generator=g))
    beta = torch.randn(D, generator=g) * 0.1
    rm = 2.0 * (1.0 + 0.1 * torch.randn(D, generator=g))              # d = (x1 - x2)^2 of unit normals: mean 2, variance 8
    rv = 8.0 * (torch.rand(D, generator=g) * 0.4 + 0.8)
    if planted == "var0":
        rv[0], rv[D - 1] = 0.0, 0.0
        W[:, 0] *= 1e-2                                                  # invstd is 316 there: keep the channel's share comparable
        W[:, D - 1] *= 1e-2
    elif planted == "bigmean":
        probe[:, 0] = 100.0 + 0.005 * torch.randn(Q, generator=g)
        gallery[:, 0] = 0.0
        rm[0], rv[0] = 1e4, 1.0
    elif planted == "ties":
        probe = torch.randint(-3, 4, (Q, D), generator=g).float()
        gallery = torch.randint(-3, 4, (G, D), generator=g).float()
        W = (torch.randint(-2, 3, (1, D), generator=g).float() * 0.25).expand(C, D).clone()
        bs = torch.full((C,), 0.375)
    elif planted == "far_low":
        bs[0] = -200.0
    elif planted == "far_high":
        bs[0] = 200.0
    elif planted is not None:
        raise ValueError(planted)
    f = lambda t: t.float().contiguous()         # noqa: E731
    return {"probe": f(probe), "gallery": f(gallery), "idx": idx.contiguous(), "gamma": f(gamma), "beta": f(beta), "rm": f(rm),
            "rv": f(rv), "W": f(W), "bias": f(bs) if bias else None, "eps": EPS}


def case_input(case, seed=0):
    return make_input(case.Q, case.G, case.k, case.D, case.C, seed, case.planted, case.bias)


def expanded(inp):
    """the head's input dict (tests/verif_hostmodel.py) of the Q * k pairs: x1 = the probe rows repeated, x2 = the gathered rows"""
    Q, k = inp["idx"].shape
    D = inp["probe"].shape[1]
    x1 = inp["probe"].view(Q, 1, D).expand(Q, k, D).reshape(Q * k, D).contiguous()
    x2 = inp["gallery"].index_select(0, inp["idx"].reshape(-1).long()).contiguous()
    return {"x1": x1, "x2": x2, "gamma": inp["gamma"], "beta": inp["beta"], "rm": inp["rm"], "rv": inp["rv"], "W": inp["W"],
            "bias": inp["bias"], "labels": None, "eps": inp["eps"], "mom": vh.MOM}


DEFECTS = ("mean_after_scale", "no_eps", "class1")                       # of the pair scores; the merge has its own two


def pair_values(inp, dtype=torch.float64, defect=None):
    """(logits [Q, k, C], score [Q, k]) in tensors of `dtype`.  defect: 'mean_after_scale' — z = gamma (d invstd - running_mean)
    + beta (the mean is not subtracted before the scaling); 'expanded_form' — the same VALUE as the sound form written as A d + b
    with A = gamma invstd, b = beta - A running_mean (differs in float32 only: what the kernel's contract rules out); 'no_eps' —
    invstd = rsqrt(running_var); 'class1' — the score of class 1 (class 0 when there is one class only)"""
    e = expanded(inp)
    Q, k = inp["idx"].shape
    if defect in ("mean_after_scale", "expanded_form", "no_eps"):
        c = lambda t: None if t is None else t.detach().to(dtype)      # noqa: E731
        d = (c(e["x1"]) - c(e["x2"])) ** 2
        invstd = (c(e["rv"]) + (0.0 if defect == "no_eps" else vh._f32(e["eps"]))).rsqrt()
        A = c(e["gamma"]) * invstd
        if defect == "mean_after_scale":
            z = (d * invstd - c(e["rm"])) * c(e["gamma"]) + c(e["beta"])
        elif defect == "expanded_form":
            z = d * A + (c(e["beta"]) - A * c(e["rm"]))
        else:
            z = (d - c(e["rm"])) * A + c(e["beta"])
        logits = z @ c(e["W"]).t()
        if e["bias"] is not None:
            logits = logits + c(e["bias"])
    else:
        logits = vh.evaluate(e, False, dtype)["logits"]
    p = torch.softmax(logits, 1)
    score = p[:, 1 if (defect == "class1" and p.shape[1] > 1) else 0]
    return logits.reshape(Q, k, -1), score.reshape(Q, k)


def pair_refs(inp):
    """-> {"logits": Ref [Q, k, C], "score": Ref [Q, k]} in float64 with the budgets of the module docstring"""
    e = expanded(inp)
    Q, k = inp["idx"].shape
    ref = vh.head_fwd(e, False)["logits"]
    l, Ml = ref.value, ref.M
    C = l.shape[1]
    m = l.max(1, keepdim=True).values
    p = torch.softmax(l, 1)
    arg = Ml + (l - m).abs() + 1.0
    Ms = p[:, 0] * (arg[:, 0] + (p * arg).sum(1) + C)
    return {"logits": Ref(l.reshape(Q, k, C), Ml.reshape(Q, k, C), "logits"), "score": Ref(p[:, 0].reshape(Q, k), Ms.reshape(Q, k), "score")}


def check(got, ref, what):
    w = compare(got, ref, C_KIND)
    assert w.ok, "%s: worst element %s err %.3e > budget %.3e (%s, max err/(2^-24 M) = %.2f)" % (
        what, w.index, w.err, w.budget, ref.kind, w.ratio)
    return w.ratio


# ---- case tables -------------------------------------------------------------------------------------------------------------------
SWEEP_D = [1, 3, 4, 63, 64, 65, 255, 256, 257, 1000, 2048]              # at Q 3, G 9, k 5, C 2
SWEEP_K = [1, 3, 4, 5, 8, 9]                                            # 9 == G
SWEEP_C = [1, 2, 3, 16]
SWEEP_Q = [1, 2, 300]                                                   # at G 40, k 6, D 64: k split over workgroups, or one per query
BIG = (5, 64, 16, 2048, 2)
# (Q, G, k, D, C) -> the regime bits the shape must take; together they cover the four combinations, with 2, 4 and 16 as the
# compile-time class bound
REGIME_SHAPES = {
    (3, 9, 5, 64, 2): VEC4 | SPLIT_K,
    (300, 40, 6, 64, 2): VEC4,
    (3, 9, 5, 65, 2): SPLIT_K,
    (300, 40, 6, 63, 2): 0,
    (3, 9, 5, 1000, 16): VEC4 | SPLIT_K,
    (260, 9, 3, 1000, 16): VEC4,
    (3, 9, 5, 1001, 16): SPLIT_K,
    (260, 9, 3, 1001, 16): 0,
    (260, 9, 3, 257, 3): 0,
    BIG: VEC4 | SPLIT_K,
    (2, 128, 100, 33, 2): SPLIT_K,                                      # large k goes with small D
}


def pair_cases():
    out = []

    def add(Q, G, k, D, C, planted=None, bias=True):
        c = PairCase(Q, G, k, D, C, planted, bias)
        if c not in out:
            out.append(c)
    for D in SWEEP_D:
        add(3, 9, 5, D, 2)
    for k in SWEEP_K:
        add(3, 9, k, 64, 2)
    for C in SWEEP_C:
        add(3, 9, 5, 64, C)
    for Q in SWEEP_Q:
        add(Q, 40, 6, 64, 2)
    for shape in REGIME_SHAPES:
        add(*shape)
    for pl in PLANTED:
        add(3, 9, 5, 65, 3, planted=pl)
        add(3, 9, 5, 256, 2, planted=pl)
    add(3, 9, 5, 64, 1, planted="ties")
    add(3, 9, 5, 64, 16, planted="ties")
    add(3, 9, 5, 65, 3, bias=False)
    add(3, 9, 5, 256, 2, bias=False)
    return out


# ---- ordering inside the top-k -------------------------------------------------------------------------------------------------------
ORDER_CASES = [(7, 40, 6, 64, 2), (5, 33, 4, 100, 2), (9, 64, 16, 2048, 2)]          # (Q, G, k, D, C)
UNDECIDED_CAP = 8                                                                    # at most one row in eight


def decided_rows(ref):
    """bool [Q]: every adjacent pair of the row's sorted fp64 scores is further apart than the sum of its two budgets"""
    s, bud = ref.value, C_KIND[ref.kind] * U24 * (ref.M + TINY_M)
    order = torch.argsort(s, dim=1, stable=True)
    ss, bs = s.gather(1, order), bud.gather(1, order)
    if s.shape[1] < 2:
        return torch.ones(s.shape[0], dtype=torch.bool)
    return ((ss[:, 1:] - ss[:, :-1]) > (bs[:, 1:] + bs[:, :-1])).all(1)


def check_order(got, ref, what):
    """on decided rows the stable order of `got` [Q, k] equals the model's; -> number of undecided rows (capped)"""
    dec = decided_rows(ref)
    und = int((~dec).sum())
    assert und * UNDECIDED_CAP <= dec.numel(), "%s: %d of %d rows undecided" % (what, und, dec.numel())
    want = torch.argsort(ref.value, dim=1, stable=True)
    have = torch.argsort(got.detach().double().cpu(), dim=1, stable=True)
    bad = [q for q in range(dec.numel()) if bool(dec[q]) and not torch.equal(want[q], have[q])]
    assert not bad, "%s: order differs on decided rows %s" % (what, bad)
    return und


# ---- the merge ---------------------------------------------------------------------------------------------------------------------
MERGE_SHAPES = [(1, 2, 1), (3, 33, 4), (4, 12, 12), (5, 1000, 75), (2, 70000, 100)]      # (Q, G, k)
MERGE_DEFECTS = ("gap_inside", "nxt_after")


def merge_model(dist, idx, score, defect=None):
    """float32 numpy model of rg_cascade_merge, every operation a float32 operation in the documented order; dist [Q, G], idx
    [Q, k] (distinct per row), score [Q, k] -> the merged copy.  defect: 'gap_inside' — the gap is added to the top-k columns
    too; 'nxt_after' — nxt is read after the overwrite, as the (k + 1)-th smallest entry of the overwritten row"""
    out = np.array(dist, dtype=np.float32, copy=True)
    idx, score = np.asarray(idx).astype(np.int64), np.asarray(score, dtype=np.float32)
    Q, G = out.shape
    k = idx.shape[1]
    one = np.float32(1.0)
    for q in range(Q):
        inside = np.zeros(G, dtype=bool)
        inside[idx[q]] = True
        if k >= G:
            out[q, idx[q]] = score[q]
            continue
        nxt = out[q][~inside].min()
        bar = score[q].max()
        out[q, idx[q]] = score[q]
        if defect == "nxt_after":
            nxt = np.sort(out[q], kind="stable")[k]
        gap = np.maximum(np.float32(np.float32(bar + one) - nxt), np.float32(0.0))
        if gap > 0:
            sel = np.ones(G, dtype=bool) if defect == "gap_inside" else ~inside
            out[q, sel] = out[q, sel] + gap
    return out


def merge_input(Q, G, k, seed=0, planted=None):
    """(dist [Q, G] float32 numpy, idx int32 [Q, k] = the stable top-k of dist, score [Q, k]).  planted: 'gap0' — scores far
    below every distance (the gap is exactly 0); 'inf' — +inf in some columns outside the top-k; 'descending' — the top-k
    columns listed in descending column order"""
    rng = np.random.RandomState(1000 * seed + 7 * Q + G + k)
    dist = (rng.rand(Q, G).astype(np.float32) * 3.0 + 0.5).astype(np.float32)
    score = rng.rand(Q, k).astype(np.float32)
    idx = np.argsort(dist, axis=1, kind="stable")[:, :k]
    if planted == "gap0":
        score = (score - 50.0).astype(np.float32)
    elif planted == "inf":
        for q in range(Q):
            outside = np.setdiff1d(np.arange(G), idx[q])
            dist[q, outside[::3]] = np.inf
    elif planted == "descending":
        idx = -np.sort(-idx, axis=1)
    elif planted is not None:
        raise ValueError(planted)
    return dist, np.ascontiguousarray(idx.astype(np.int32)), score
