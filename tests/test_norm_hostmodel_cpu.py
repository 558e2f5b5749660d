"""CPU: the host model of the normalisation unit (tests/norm_hostmodel.py) is one a correct float32 implementation meets and a
subtly wrong one does not.

  * plain float32 torch, on every case of the device tests, stays inside the per-element budget — and its ratios are the source
    of the constants (C_KIND = max(8, 4 x ratio));
  * the comparator rejects seven small mutations of the rounded fp64 reference; the global comparator of tests/test_ops_gpu.py
    accepts two of them (the gap this host model closes);
  * the case lists reach every reachable branch of the mirrored dispatch arithmetic, each with a full and a ragged geometry.

Run as a script (python -m tests.test_norm_hostmodel_cpu) it prints the ratio table of the host model's docstring."""
import functools

import torch

from tests import norm_hostmodel as H
from tests.test_ops_gpu import _close

EPS = 1e-5


def _case(kind, N, C, HW, family, i, frozen=False):
    """reference and float32 torch of one case -> [(name, float32 tensor, Ref)]"""
    act, slope = H.case_act(i, family)
    inp = H.make_inputs(kind, N, C, HW, family, seed=i)
    fz = (inp.running_mean, inp.running_var) if frozen else None
    f = H.forward(kind, inp.x, inp.gamma, inp.beta, inp.residual, EPS, act, slope, inp.running_mean, inp.running_var, 0.1, fz)
    y_act = f["y"].value.float()
    if family == "masked":
        y_act = H.masked_y_act(y_act)
    mean = f["mean"].value if not frozen else inp.running_mean
    b = H.backward(kind, inp.x, inp.dy, y_act, mean, f["invstd"].value, inp.gamma, act, slope, train=not frozen)
    t = H.torch32(kind, inp, EPS, act, slope, y_act, 0.1, fz)
    out = [(k, t[k], f[k]) for k in f if k in t] + [(k, t[k], b[k]) for k in b]
    if kind == "in":
        out.append(("y", t["y_instance_norm"], f["y"]))
    return out


def _all_cases():
    i = 0
    for N, C, HW, fam in H.bn_cases() + [H.BN_WIDE + ("plain",)]:
        yield "bn %s %s" % ((N, C, HW), fam), _case("bn", N, C, HW, fam, i)
        i += 1
    for N, C, HW, fam in H.in_cases():
        yield "in %s %s" % ((N, C, HW), fam), _case("in", N, C, HW, fam, i)
        i += 1
    for N, C, HW, fam in H.slice_cases():
        yield "bn two-stage %s %s" % ((N, C, HW), fam), _case("bn", N, C, HW, fam, i)
        yield "bn frozen %s %s" % ((N, C, HW), fam), _case("bn", N, C, HW, fam, i, frozen=True)
        i += 1
    yield "helpers", _helper_cases()


def _helper_cases():
    out = []
    g = torch.Generator().manual_seed(77)
    for N, C, HW in H.CHANNEL_SUM_CASES:
        for family in ("plain", "scales", "offset"):
            dy = H.make_inputs("bn", N, C, HW, family, seed=4).x
            # torch's sum of a channel gathered into one row (its strided reduction over n adds serially: not the yardstick)
            out.append(("channel_sum", dy.transpose(0, 1).reshape(C, -1).sum(1), H.channel_sum(dy)))
    for N, C in [(1, 1), (15, 16), (33, 17)]:
        a = torch.randn(N, C, generator=g)
        out.append(("rows_sum", a.sum(0), H.rows_sum(a)))
    for M in (1, 3, 4, 147, 4608):
        ga, be, mu, var = torch.rand(M, generator=g) + 0.5, torch.randn(M, generator=g), torch.randn(M, generator=g) * 30, \
            torch.rand(M, generator=g) + 0.01
        is_ = torch.rsqrt(var + EPS)
        ref = H.bn_fold(ga, be, mu, var, EPS)
        out += [("scale", ga * is_, ref["scale"]), ("shift", be - mu * (ga * is_), ref["shift"]), ("fold invstd", is_, ref["invstd"])]
        w = torch.randn(5, M, generator=g)
        sc = torch.randn(5, generator=g)
        out.append(("scale_rows", w * sc.reshape(5, 1), H.scale_rows(w, sc)))
        G, sg = torch.randn(5, M, generator=g), torch.randn(5, generator=g) * 10
        ref = H.bn_fold_wgrad(w, G, sc, is_[:1].expand(5), mu[:1].expand(5), sg)
        out += [("dgamma", is_[0] * ((w * G).sum(1) - mu[0] * sg), ref["dgamma"]), ("dW", G * sc.reshape(5, 1), ref["dW"])]
    return out


@functools.lru_cache(maxsize=None)
def _ratios():
    worst, bad = {}, []
    for name, outs in _all_cases():
        for k, got, ref in outs:
            w = H.compare(got, ref)
            if ref.kind != "exact":
                worst[ref.kind] = max(worst.get(ref.kind, 0.0), w.ratio)
            if not w.ok:
                bad.append("%s %s: worst %s err %.3e budget %.3e" % (name, k, w.index, w.err, w.budget))
    return worst, bad


def test_float32_torch_meets_the_budget_on_every_case():
    worst, bad = _ratios()
    print({k: round(v, 2) for k, v in sorted(worst.items())})
    assert not bad, "\n".join(bad)
    assert set(worst) == set(H.C_KIND) - {"exact"}


def test_constants_follow_the_rule():
    """C_KIND = max(8, 4 x float32-torch ratio) as measured where the table was made; torch's summation order differs between
    hosts (threads, vector width), hence a quarter of slack here instead of equality."""
    worst, _ = _ratios()
    for k, r in worst.items():
        assert H.C_KIND[k] >= 8.0 and 4.0 * r <= 1.25 * H.C_KIND[k], (k, r, H.C_KIND[k])
    assert H.C_KIND["exact"] == 0.0


# ---- mutations ---------------------------------------------------------------------------------------------------------------
def _bn(N, C, HW, family, act=H.ACT_RELU, slope=0.0, seed=3):
    inp = H.make_inputs("bn", N, C, HW, family, seed=seed)
    f = H.forward("bn", inp.x, inp.gamma, inp.beta, inp.residual, EPS, act, slope, inp.running_mean, inp.running_var, 0.1)
    return inp, f


def _accepted_by_old(got, ref, tol=2e-5):
    try:
        _close(got, ref.value, tol=tol)
    except AssertionError:
        return False
    return True


def test_mutation_one_element_of_the_smallest_channel():
    inp, f = _bn(4, 5, 256, "scales")
    y = f["y"]
    good = y.value.float()
    assert H.compare(good, y).ok
    c = int(y.M.mean((0, 2)).argmin())
    n, p = 2, int(y.M[2, c].argmax())
    bad = good.clone()
    bad[n, c, p] = float(y.value[n, c, p] + 4 * H.C_KIND["y"] * H.U24 * y.M[n, c, p])
    w = H.compare(bad, y)
    assert not w.ok and w.index == (n, c, p)
    assert _accepted_by_old(bad, y), "the global comparator was expected to miss this"


def test_mutation_last_float4_left_at_the_fill_value():
    inp, f = _bn(3, 4, 344, "plain")
    bad = f["y"].value.float()
    bad[-1, -1, -4:] = H.FILL
    w = H.compare(bad, f["y"])
    assert not w.ok and w.index[:2] == (2, 3) and w.index[2] >= 340


def test_mutation_invstd_from_the_unbiased_variance():
    N, C, HW = 16, 3, 1024                                   # N * HW = 16384: a relative 3e-5 on invstd
    inp, f = _bn(N, C, HW, "plain")
    xd = inp.x.double()
    is_unb = (xd.var((0, 2), unbiased=True) + EPS).rsqrt()
    assert H.compare(f["invstd"].value.float(), f["invstd"]).ok
    assert not H.compare(is_unb.float(), f["invstd"]).ok
    # what the old suite would have seen of it: y and dx formed with that invstd.  The global comparator accepts dx at the 5e-5 the
    # old tests give it; y (2e-5) sits at its edge — max err 2.0e-4 against 1.6e-4 allowed here — and invstd itself was never
    # compared with a reference.
    m = H.forward("bn", inp.x, inp.gamma, inp.beta, inp.residual, EPS, H.ACT_RELU, 0.0,
                  frozen=(f["mean"].value, 1.0 / is_unb ** 2 - EPS))["y"].value.float()
    assert H.compare(f["y"].value.float(), f["y"]).ok
    assert not H.compare(m, f["y"]).ok
    y_act = f["y"].value.float()
    b = H.backward("bn", inp.x, inp.dy, y_act, f["mean"].value, f["invstd"].value, inp.gamma, H.ACT_RELU, 0.0)
    bm = H.backward("bn", inp.x, inp.dy, y_act, f["mean"].value, is_unb, inp.gamma, H.ACT_RELU, 0.0)
    assert H.compare(b["dx"].value.float(), b["dx"]).ok
    assert not H.compare(bm["dx"].value.float(), b["dx"]).ok
    assert _accepted_by_old(bm["dx"].value.float(), b["dx"], tol=5e-5), "the global comparator was expected to miss this"


def test_mutation_running_var_from_the_biased_variance():
    inp, f = _bn(16, 3, 1024, "plain")
    biased = 0.9 * inp.running_var.double() + 0.1 * inp.x.double().var((0, 2), unbiased=False)
    assert H.compare(f["running_var"].value.float(), f["running_var"]).ok
    assert not H.compare(biased.float(), f["running_var"]).ok


def test_mutation_relu_mask_at_greater_or_equal():
    inp, f = _bn(3, 4, 344, "masked")
    y_act = H.masked_y_act(f["y"].value.float())
    b = H.backward("bn", inp.x, inp.dy, y_act, f["mean"].value, f["invstd"].value, inp.gamma, H.ACT_RELU, 0.0)
    assert H.compare(b["dres"].value.float(), b["dres"]).ok
    g_ge = inp.dy * (y_act >= 0).float()
    assert not H.compare(g_ge, b["dres"]).ok
    assert not H.compare(g_ge.double().sum((0, 2)).float(), b["sum_g"]).ok
    # leaky: 0.0 / -0.0 take the slope
    bl = H.backward("bn", inp.x, inp.dy, y_act, f["mean"].value, f["invstd"].value, inp.gamma, H.ACT_LEAKY, 0.2)
    g_ge = inp.dy * torch.where(y_act >= 0, torch.tensor(1.0), torch.tensor(0.2))
    assert not H.compare(g_ge, bl["dres"]).ok


def test_mutation_channel_sum_without_its_final_element():
    g = torch.Generator().manual_seed(5)
    dy = torch.randn(8, 3, 4096, generator=g)                # 32768 values per channel
    ref = H.channel_sum(dy)
    good = dy.double().sum((0, 2))
    assert H.compare(good.float(), ref).ok
    bad = good.clone()
    bad[-1] -= float(dy[-1, -1, -1])
    assert abs(float(dy[-1, -1, -1])) > 0.1
    assert not H.compare(bad.float(), ref).ok


def test_mutation_dx_without_the_xhat_term_in_one_channel():
    inp, f = _bn(4, 5, 256, "plain", act=H.ACT_NONE)
    b = H.backward("bn", inp.x, inp.dy, None, f["mean"].value, f["invstd"].value, inp.gamma)
    good = b["dx"].value.float()
    assert H.compare(good, b["dx"]).ok
    gs = (inp.gamma.double() * f["invstd"].value)[3]
    bad = good.clone()
    bad[:, 3] = (gs * (inp.dy.double()[:, 3] - b["sum_g"].value[3] / (4 * 256))).float()
    w = H.compare(bad, b["dx"])
    assert not w.ok and w.index[1] == 3


# ---- dispatch coverage -------------------------------------------------------------------------------------------------------
def test_bn_cases_reach_every_unit_count_full_and_ragged():
    seen = {}
    for N, C, HW, _ in H.bn_cases():
        U = H.bn_reg_units(N, C, HW)
        if U:
            total = N * (HW >> 2)
            ragged = H.bn_per(N, HW) < U or total % 256 != 0
            seen.setdefault(U, set()).add("ragged" if ragged else "full")
        else:
            seen.setdefault(0, set()).add("scalar" if HW & 3 else "float4")
    assert seen == {1: {"full", "ragged"}, 2: {"full", "ragged"}, 4: {"full", "ragged"}, 8: {"full", "ragged"},
                    16: {"full", "ragged"}, 0: {"scalar", "float4"}}
    # per = 3, 5, 9 round up to U = 4, 8, 16 (whole unit rows of sentinel offsets); the first geometry past 16 units
    pers = set(H.bn_per(N, HW) for N, C, HW, _ in H.bn_cases() if HW % 4 == 0)
    assert {5, 9, 17} <= pers and H.bn_per(3, 1028) == 4 and H.bn_reg_units(16, 3, 1024) == 16
    assert H.bn_reg_units(1, 3, 16388) == 0 and H.bn_per(1, 16388) == 17
    assert H.bn_train_fused_ok(*H.BN_WIDE) and not H.bn_train_fused_ok(4, 127, 36) and not H.bn_train_fused_ok(1, 130, 16388)
    assert H.bn_train_fused_ok(16, 128, 1024)


def test_in_cases_reach_every_reachable_pair_full_and_ragged():
    reach = H.in_reachable()
    seen, scalar, loop4 = {}, set(), set()
    for N, C, HW, _ in H.in_cases():
        lanes, U = H.in_regime(N, C, HW)
        if U:
            ragged = (HW >> 2) % lanes != 0 or H.in_per(HW) < U
            seen.setdefault((lanes, U), set()).add("ragged" if ragged else "full")
        elif HW & 3:
            scalar.add(lanes)
        else:
            loop4.add(lanes)
    assert sorted(seen) == reach
    assert all(v == {"full", "ragged"} for v in seen.values()), seen
    assert scalar == {16, 32, 64, 256} and loop4 == {256}
    # pairs of the switch that the arithmetic never selects
    assert sorted(set(H.IN_SWITCH) - set(reach)) == [(32, 1), (64, 1), (256, 1), (256, 2)]
    # a partly empty last workgroup at 16, 8 and 4 instances per workgroup
    for lanes in (16, 32, 64):
        assert any(H.in_lanes(HW) == lanes and (N * C) % (256 // lanes) for N, C, HW, _ in H.in_cases())


def test_slice_cases_reach_every_pick_slices_regime():
    kinds = set()
    for N, C, HW, _ in H.slice_cases():
        S, L = H.pick_slices(N, C, HW)
        total = N * HW
        assert L % 4 == 0 and (S - 1) * L < total <= S * L
        if S == 1:
            kinds.add("one")
            if total < 256:
                kinds.add("fewer elements than threads")
        else:
            if total % L:
                kinds.add("ragged last slice")
            if HW & 3 and L % HW:
                kinds.add("mid-row scalar")
            if not (HW & 3) and L % HW:
                kinds.add("mid-row float4")
    assert kinds == {"one", "fewer elements than threads", "ragged last slice", "mid-row scalar", "mid-row float4"}
    assert H.pick_slices(16, 3, 1024) == (4, 4096) and H.pick_slices(3, 3, 4100) == (4, 3076)


def test_channel_sum_mirror():
    assert H.channel_sum_ok(8, 3, 4096) and not H.channel_sum_ok(8, 3, 4097) and not H.channel_sum_ok(1, 1 << 15, 1 << 14)


if __name__ == "__main__":
    worst, bad = _ratios()
    for k in sorted(worst):
        print("%-14s %-8.2f %g" % (k, worst[k], max(8.0, 4 * worst[k])))
    print("\n".join(bad))
