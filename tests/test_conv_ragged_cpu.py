"""CPU: the references, the bound and the case tables of tests/test_conv_ragged_gpu.py, without a GPU.

  * the extended fp64 references of tests/conv_sweep.py (every epilogue, row sums, BatchNorm fold, the ConvTranspose2d roles) equal
    torch's fp64 CPU conv2d / conv_transpose2d / autograd to 1e-12 relative;
  * the bound can fail: for every case of the GPU tables an honest kernel passes at ratio <= 1 and five subtly wrong ones do not.
    THE STAND-IN KERNEL IS TORCH'S OWN fp32 CPU CONVOLUTION (conv2d, conv_transpose2d, torch.nn.grad.conv2d_weight) with the
    epilogue in fp32 torch ops — not the code under test, which needs the GPU.  What this shows is that the chosen inputs and the
    per-element bound notice a wrong tail element, not that the HIP kernels are right;
  * the tables: every geometry is valid, every tensor is far below 4 MB, every case is dispatched where its table says, and the
    regimes the GPU file declares are all reached by some case according to the host model of the dispatch."""
import math
import os

import pytest
import torch
import torch.nn.functional as F

from tests import conv_sweep as S
from tests import test_conv_ragged_gpu as R

FOUR_MB = 4 << 20


def _inputs(fam, geom, seed):
    N, C, H, W, K, KH, KW, SH, SW, PH, PW = geom
    P, Q = R.out_hw(geom)
    g = torch.Generator().manual_seed(seed)
    t = {"x": torch.randn(N, C, H, W, generator=g), "dy": torch.randn(N, K, P, Q, generator=g),
         "w": torch.randn(K, C, KH, KW, generator=g) / math.sqrt((K if fam == "dgrad" else C) * KH * KW)}
    if fam == "wgrad":
        t["dy"] = t["dy"] / math.sqrt(N * P * Q)
    M = C if fam == "dgrad" else K
    oshape = {"fwd": (N, K, P, Q), "dgrad": (N, C, H, W), "wgrad": (K, C, KH, KW)}[fam]
    t["scale"] = torch.rand(M, generator=g) + 0.5
    t["shift"] = torch.randn(M, generator=g) * 0.1
    t["res"] = torch.randn(oshape, generator=g)
    t["mask"] = torch.randn(oshape, generator=g)
    t["invstd"] = torch.rand(K, generator=g) + 0.5
    t["mean"] = torch.randn(K, generator=g) * 0.3
    t["partials"] = torch.randn(K, 8, generator=g)
    t["sum_g"] = torch.randn(K, generator=g)
    return t


def _acc64(fam, geom, t):
    N, C, H, W, K, KH, KW, SH, SW, PH, PW = geom
    if fam == "fwd":
        return S.ref_fwd(t["x"].double(), t["w"].double(), (SH, SW), (PH, PW))
    if fam == "dgrad":
        return S.ref_dgrad(t["dy"].double(), t["w"].double(), (H, W), (SH, SW), (PH, PW))
    return S.ref_wgrad(t["x"].double(), t["dy"].double(), (KH, KW), (SH, SW), (PH, PW))


def _torch_conv(fam, geom, x, w, dy):
    """torch's own convolution of the family, in the dtype of its operands"""
    N, C, H, W, K, KH, KW, SH, SW, PH, PW = geom
    P, Q = R.out_hw(geom)
    if fam == "fwd":
        return F.conv2d(x, w, stride=(SH, SW), padding=(PH, PW))
    if fam == "dgrad":
        op = (H - ((P - 1) * SH - 2 * PH + KH), W - ((Q - 1) * SW - 2 * PW + KW))
        return F.conv_transpose2d(dy, w, stride=(SH, SW), padding=(PH, PW), output_padding=op)
    return torch.nn.grad.conv2d_weight(x, (K, C, KH, KW), dy, stride=(SH, SW), padding=(PH, PW))


def _epilogues(fam, case):
    """[(name, keyword arguments of S.ref_epilogue as tensor names)]"""
    if fam == "fwd":
        return [(e, dict(zip(("scale", "shift", "res"), R.EPI_F[e][:3])), R.EPI_F[e][3], False) for e in case[2]]
    if fam == "dgrad":
        return [(e, dict(zip(("scale", "shift", "res", "mask"), R.EPI_D[e][:4])), R.EPI_D[e][5], bool(R.EPI_D[e][4])) for e in case[2]]
    return [("fold %d" % f, {}, f, False) for f in case[1]]


def _apply(fam, acc, acc_abs, t, use, act, dtype, shift_plus_one=False):
    """the epilogue in `dtype`: fp64 with the absolute contraction gives (ref, tol); fp32 on a kernel's accumulators gives its output"""
    def pick(name):
        if not use.get(name):
            return None
        v = t[name].to(dtype if name != "mask" else torch.float32)
        if shift_plus_one and name == ("scale" if fam == "wgrad" else "shift"):       # indexed by m + 1; past the end reads 0
            v = torch.cat([v[1:], v.new_zeros(1)])
        return v
    return S.ref_epilogue(acc, acc_abs, pick("scale"), pick("shift"), pick("res"), act, mask=pick("mask"))


def _outputs(fam, acc, acc_abs, t, use, act, dtype, shift_plus_one=False):
    """{output name: (value, tol)} of one call"""
    if fam != "wgrad":
        ref, tol = _apply(fam, acc, acc_abs, t, use, act, dtype, shift_plus_one)
        return {fam: (ref, tol)}
    if not act:                 # (wgrad: `act` carries the fold variant)
        return {"wgrad": (acc, acc_abs * S.TOL + S.TINY)}
    scale = t["scale"].to(dtype)
    if shift_plus_one:
        scale = torch.cat([scale[1:], scale.new_zeros(1)])
    return S.ref_fold(acc, acc_abs, t["w"].to(dtype), scale, t["invstd"].to(dtype), t["mean"].to(dtype),
                      partials=t["partials"].to(dtype) if act == 1 else None, sum_g=t["sum_g"].to(dtype) if act == 2 else None)


def _ratio(got, ref, tol):
    return float(((got.double() - ref).abs() / tol).max())


# ---- the mutants: delta (fp64) to add to the honest accumulators ----
def _taps(geom, p, q):
    """the in-bounds (r, s, h, w) of output pixel (p, q), in reduction order"""
    N, C, H, W, K, KH, KW, SH, SW, PH, PW = geom
    return [(r, s, p * SH - PH + r, q * SW - PW + s) for r in range(KH) for s in range(KW)
            if 0 <= p * SH - PH + r < H and 0 <= q * SW - PW + s < W]


def _dropped_term(fam, geom, t, shape):
    """minus the LAST in-bounds term of the reduction of the last output element that has one (the depth tail of the last tile)"""
    N, C, H, W, K, KH, KW, SH, SW, PH, PW = geom
    P, Q = R.out_hw(geom)
    x, w, dy = t["x"].double(), t["w"].double(), t["dy"].double()
    d = torch.zeros(shape, dtype=torch.float64)
    if fam == "fwd":
        r, s, h, ww = _taps(geom, P - 1, Q - 1)[-1]
        d[N - 1, K - 1, P - 1, Q - 1] = -x[N - 1, C - 1, h, ww] * w[K - 1, C - 1, r, s]
        return d
    if fam == "wgrad":
        for p in range(P - 1, -1, -1):
            for q in range(Q - 1, -1, -1):
                taps = _taps(geom, p, q)
                if taps:
                    r, s, h, ww = taps[-1]
                    d[K - 1, C - 1, r, s] = -dy[N - 1, K - 1, p, q] * x[N - 1, C - 1, h, ww]
                    return d
    for h in range(H - 1, -1, -1):
        for ww in range(W - 1, -1, -1):
            for p in range(P - 1, -1, -1):
                for q in range(Q - 1, -1, -1):
                    hit = [(r, s) for r, s, hh, wv in _taps(geom, p, q) if hh == h and wv == ww]
                    if hit:
                        r, s = hit[-1]
                        d[N - 1, C - 1, h, ww] = -dy[N - 1, K - 1, p, q] * w[K - 1, C - 1, r, s]
                        return d
    raise AssertionError("no term")


def _copied_column(fam, acc):
    """the last column of the GEMM (the last column of its last tile) takes its neighbour's values"""
    if fam == "wgrad":
        m = acc.reshape(acc.shape[0], -1)
        d = torch.zeros_like(m)
        d[:, -1] = m[:, -2] - m[:, -1]
        return d.view(acc.shape)
    n, c, hh, ww = acc.shape
    m = acc.permute(0, 2, 3, 1).reshape(-1, c)           # [pixel][row]
    d = torch.zeros_like(m)
    d[-1] = m[-2] - m[-1]
    return d.view(n, hh, ww, c).permute(0, 3, 1, 2).contiguous()


def _unpadded_border(fam, geom, t, acc):
    """the top border row of the last image (weight gradient: the contribution of the top output row) as if PH were 0"""
    N, C, H, W, K, KH, KW, SH, SW, PH, PW = geom
    P, Q = R.out_hw(geom)
    if PH == 0:
        return None
    x, w, dy = t["x"].double(), t["w"].double(), t["dy"].double()
    d = torch.zeros_like(acc)
    if fam == "fwd":
        row = F.conv2d(x[N - 1:, :, :KH], w, stride=(SH, SW), padding=(0, PW))[:, :, 0]
        d[N - 1, :, 0] = row[0] - acc[N - 1, :, 0]
    elif fam == "dgrad":
        full = F.conv_transpose2d(dy[N - 1:], w, stride=(SH, SW), padding=(0, PW))
        wide = min(W, full.shape[3])
        d[N - 1, :, 0, :wide] = full[0, :, 0, :wide] - acc[N - 1, :, 0, :wide]
    else:
        xp = F.pad(x, (0, 0, PH, PH))
        good = torch.nn.grad.conv2d_weight(xp[:, :, :KH].contiguous(), w.shape, dy[:, :, :1].contiguous(), stride=(SH, SW), padding=(0, PW))
        bad = torch.nn.grad.conv2d_weight(xp[:, :, PH:PH + KH].contiguous(), w.shape, dy[:, :, :1].contiguous(), stride=(SH, SW),
                                          padding=(0, PW))
        d = bad - good
    return d


def _doubled_split(fam, geom, t):
    """the partial of the last of five splits of the reduction, once more"""
    N, C, H, W, K, KH, KW, SH, SW, PH, PW = geom
    x, w, dy = t["x"].double(), t["w"].double(), t["dy"].double()
    if fam == "fwd":
        c0 = C - max(1, C // 5)
        return _torch_conv(fam, geom, x[:, c0:], w[:, c0:], None)
    if fam == "dgrad":
        k0 = K - max(1, K // 5)
        return _torch_conv(fam, geom, None, w[k0:], dy[:, k0:])
    n0 = N - max(1, N // 5)
    g = list(geom)
    g[0] = N - n0
    return _torch_conv(fam, tuple(g), x[n0:].contiguous(), None, dy[n0:].contiguous())


MUTANTS = ("one reduction term dropped", "last column copied from its neighbour", "a padded border row as if unpadded",
           "one split's partial added twice", "epilogue shift indexed by k + 1")


def _all_cases():
    for fam, groups in (("fwd", R.FWD_GROUPS), ("dgrad", R.DGRAD_GROUPS), ("wgrad", R.WGRAD_GROUPS)):
        for group, cases in groups:
            for case in cases:
                yield fam, group, case


CASE_IDS = ["%s-%s-%s" % (fam, group, "x".join(str(v) for v in case[0])) for fam, group, case in _all_cases()]


@pytest.mark.parametrize("fam,group,case", list(_all_cases()), ids=CASE_IDS)
def test_bound_passes_torch_fp32_and_fails_every_mutant(fam, group, case):
    """torch's fp32 CPU convolution (the stand-in for an honest kernel, NOT the code under test) passes every epilogue of the case
    at ratio <= 1; each applicable mutant of it exceeds the bound on at least one element"""
    geom = case[0]
    PH = geom[9]
    t = _inputs(fam, geom, 99 + sum(geom))
    acc, acc_abs = _acc64(fam, geom, t)
    honest = _torch_conv(fam, geom, t["x"], t["w"], t["dy"])                   # fp32
    deltas = {MUTANTS[0]: _dropped_term(fam, geom, t, acc.shape), MUTANTS[1]: _copied_column(fam, acc),
              MUTANTS[2]: _unpadded_border(fam, geom, t, acc), MUTANTS[3]: _doubled_split(fam, geom, t)}
    caught = {m: None for m in MUTANTS}
    worst = 0.0
    for name, use, act, _ in _epilogues(fam, case):
        want = _outputs(fam, acc, acc_abs, t, use, act, torch.float64)

        def ratios(acc32, shift_plus_one=False):
            got = _outputs(fam, acc32, acc32.abs(), t, use, act, torch.float32, shift_plus_one)
            return {n: _ratio(got[n][0], want[n][0], want[n][1]) for n in want}

        r = ratios(honest)
        worst = max(worst, max(r.values()))
        assert max(r.values()) <= 1.0, ("torch fp32", name, r)
        for m in MUTANTS[:4]:
            if deltas[m] is None:
                continue
            rm = ratios((honest.double() + deltas[m]).float())
            caught[m] = bool(caught[m]) or rm[fam] > 1.0
        has_shift = bool(act) if fam == "wgrad" else bool(use.get("shift"))
        if has_shift and honest.shape[0 if fam == "wgrad" else 1] >= 1:
            caught[MUTANTS[4]] = bool(caught[MUTANTS[4]]) or ratios(honest, True)[fam] > 1.0
    print("%s %s %s: torch fp32 worst ratio %.3f; mutants %s" % (fam, group, geom, worst, caught))
    missed = [m for m, c in caught.items() if c is False]
    assert not missed, (geom, missed)
    # what does not apply to a case: an unpadded border without padding, a shift without an epilogue that has one
    assert (caught[MUTANTS[2]] is None) == (PH == 0)
    assert all(caught[m] for m in (MUTANTS[0], MUTANTS[1], MUTANTS[3]))


def test_every_mutant_applies_to_some_case_of_every_family():
    for fam, groups in (("fwd", R.FWD_GROUPS), ("dgrad", R.DGRAD_GROUPS), ("wgrad", R.WGRAD_GROUPS)):
        cases = [c for _, cs in groups for c in cs]
        assert any(c[0][9] > 0 for c in cases) and any(c[0][9] == 0 for c in cases), fam
        if fam == "wgrad":
            assert any(any(f for f in c[1]) for c in cases)
        else:
            table = R.EPI_F if fam == "fwd" else R.EPI_D
            assert all(any(table[e][1] for e in c[2]) for c in cases), "%s: a case without a shift epilogue" % fam


# ---- the references against torch's own fp64 operators ----
REF_GEOMS = [(2, 5, 7, 6, 4, 3, 3, 1, 1, 1, 1), (3, 4, 10, 9, 6, 4, 4, 2, 2, 1, 1), (2, 8, 5, 3, 7, 1, 1, 1, 1, 0, 0),
             (2, 6, 10, 8, 5, 3, 3, 2, 2, 1, 1),           # 3x3 / 2 with the P, Q of a ConvTranspose2d with output padding 1
             (2, 3, 9, 7, 5, 1, 1, 2, 2, 0, 0),            # 1x1 / 2: pixels no output touches
             (2, 6, 8, 4, 5, 8, 4, 1, 1, 0, 0)]


def _rel(got, ref):
    return float((got - ref).abs().max()) / max(float(ref.abs().max()), 1e-300)


@pytest.mark.parametrize("geom", REF_GEOMS)
def test_extended_references_match_torch_fp64(geom):
    N, C, H, W, K, KH, KW, SH, SW, PH, PW = geom
    P, Q = R.out_hw(geom)
    slope = S.SLOPE
    acts = {S.ACT_NONE: lambda v: v, S.ACT_RELU: torch.relu, S.ACT_LEAKY: lambda v: F.leaky_relu(v, slope), S.ACT_TANH: torch.tanh}
    for fam in ("fwd", "dgrad"):
        t = {k: v.double() for k, v in _inputs(fam, geom, 5 + sum(geom)).items()}
        acc, acc_abs = _acc64(fam, geom, t)
        M = acc.shape[1]
        for act, fn in acts.items():
            for use_scale, use_res, use_mask in ((1, 1, 1), (0, 0, 0), (1, 0, 0), (0, 1, 1)):
                ref, tol = S.ref_epilogue(acc, acc_abs, t["scale"] if use_scale else None, t["shift"], t["res"] if use_res else None, act,
                                          mask=t["mask"] if use_mask else None)
                # torch: the convolution (for the data gradient: ConvTranspose2d with its bias) of the scaled filters
                ws = t["w"] * (t["scale"].view(-1, 1, 1, 1) if fam == "fwd" else t["scale"].view(1, -1, 1, 1)) if use_scale else t["w"]
                if fam == "fwd":
                    z = F.conv2d(t["x"], ws, bias=t["shift"], stride=(SH, SW), padding=(PH, PW))
                else:
                    op = (H - ((P - 1) * SH - 2 * PH + KH), W - ((Q - 1) * SW - 2 * PW + KW))
                    z = F.conv_transpose2d(t["dy"], ws, bias=t["shift"], stride=(SH, SW), padding=(PH, PW), output_padding=op)
                if use_res:
                    z = z + t["res"]
                want = fn(z)
                if use_mask:
                    want = torch.where(t["mask"] > 0, want, torch.zeros_like(want))
                assert ref.shape == want.shape
                assert _rel(ref, want) <= 1e-12, (fam, act, use_scale, use_res, use_mask, _rel(ref, want))
                assert bool((tol > 0).all()) and tol.shape == ref.shape
                if use_mask:
                    assert float(tol[t["mask"] <= 0].max()) <= 2 * S.TINY and float(ref[t["mask"] <= 0].abs().max()) == 0.0
                rs, rs_tol = S.ref_rowsum(ref, tol)
                assert rs.shape == (M,) and _rel(rs, want.transpose(0, 1).reshape(M, -1).sum(1)) <= 1e-12
                assert _rel(rs_tol, tol.transpose(0, 1).reshape(M, -1).sum(1)) <= 1e-12
        assert not torch.equal(acc, torch.zeros_like(acc))
    # the absolute contraction: the same operator on absolute operands, plus the absolute epilogue operands
    t = {k: v.double() for k, v in _inputs("fwd", geom, 6).items()}
    acc, acc_abs = _acc64("fwd", geom, t)
    _, tol = S.ref_epilogue(acc, acc_abs, -t["scale"], t["shift"], t["res"], S.ACT_LEAKY)
    mag = F.conv2d(t["x"].abs(), t["w"].abs(), stride=(SH, SW), padding=(PH, PW)) * t["scale"].view(1, -1, 1, 1) + \
        t["shift"].abs().view(1, -1, 1, 1) + t["res"].abs()
    assert _rel(tol, mag * S.TOL + S.TINY) <= 1e-12
    # tanh adds the tanh term of tests/body_hostmodel.py on top of the carried bound
    ref, tol_t = S.ref_epilogue(acc, acc_abs, None, t["shift"], None, S.ACT_TANH)
    z = acc + t["shift"].view(1, -1, 1, 1)
    carried = (acc_abs + t["shift"].abs().view(1, -1, 1, 1)) * S.TOL
    assert _rel(tol_t, carried + S.C_KIND["tanh"] * 2.0 ** -24 * (ref.abs() + z.abs() * (1 - ref * ref)) + S.TINY) <= 1e-12


@pytest.mark.parametrize("geom", REF_GEOMS)
def test_fold_and_transposed_roles_match_torch_autograd(geom):
    """the BatchNorm fold behind the weight gradient against autograd through conv2d -> frozen-statistics BatchNorm, and the weight
    gradient in the ConvTranspose2d roles (x and dy swapped) against autograd through conv_transpose2d"""
    N, C, H, W, K, KH, KW, SH, SW, PH, PW = geom
    P, Q = R.out_hw(geom)
    t = {k: v.double() for k, v in _inputs("wgrad", geom, 17 + sum(geom)).items()}
    G, G_abs = _acc64("wgrad", geom, t)
    # y = conv(x, w * scale) + beta with scale = gamma * invstd, beta' = beta - gamma invstd mean: d/dgamma = invstd (sum w G - mean sum_g)
    gamma = (t["scale"] / t["invstd"]).clone().requires_grad_(True)
    beta = torch.zeros(K, dtype=torch.float64, requires_grad=True)
    wf = t["w"].clone().requires_grad_(True)
    x = t["x"]
    y = F.conv2d(x, wf * (gamma * t["invstd"]).view(-1, 1, 1, 1), stride=(SH, SW), padding=(PH, PW)) + \
        (beta - gamma * t["invstd"] * t["mean"]).view(1, -1, 1, 1)
    y.backward(t["dy"])
    sum_g = t["dy"].sum((0, 2, 3))
    parts = torch.stack([sum_g * f for f in (0.5, 0.25, 0.125, 0.125, 0.0, 0.5, -0.25, -0.25)], 1)       # slices that add up to sum_g
    for kw in (dict(partials=parts), dict(sum_g=sum_g)):
        out = S.ref_fold(G, G_abs, t["w"], t["scale"], t["invstd"], t["mean"], **kw)
        assert _rel(out["wgrad"][0], wf.grad) <= 1e-12
        assert _rel(out["wgrad fold dgamma"][0], gamma.grad) <= 1e-11
        if "partials" in kw:
            assert _rel(out["wgrad fold dbeta"][0], beta.grad) <= 1e-12
        else:
            assert "wgrad fold dbeta" not in out
        assert all(bool((tol > 0).all()) for _, tol in out.values())
    # ConvTranspose2d(K -> C) with weight [K][C][KH][KW]: input a = our dy, output b = our dx; its weight gradient for an upstream
    # gradient gb is the conv weight gradient with x := gb, dy := a; its forward is the data gradient
    a = t["dy"].clone()
    wt = t["w"].clone().requires_grad_(True)
    op = (H - ((P - 1) * SH - 2 * PH + KH), W - ((Q - 1) * SW - 2 * PW + KW))
    b = F.conv_transpose2d(a, wt, stride=(SH, SW), padding=(PH, PW), output_padding=op)
    gb = t["x"]
    b.backward(gb)
    got, _ = S.ref_wgrad(gb, a, (KH, KW), (SH, SW), (PH, PW))
    assert _rel(got, wt.grad) <= 1e-12
    fwd, _ = S.ref_dgrad(a, t["w"], (H, W), (SH, SW), (PH, PW))
    assert _rel(fwd, b.detach()) <= 1e-12


# ---- the case tables ----
def test_case_geometries_are_valid_and_small():
    seen = set()
    for fam, group, case in _all_cases():
        geom = case[0]
        N, C, H, W, K, KH, KW, SH, SW, PH, PW = geom
        P, Q = R.out_hw(geom)
        assert P >= 1 and Q >= 1, geom
        assert (P, Q) == ((H + 2 * PH - KH) // SH + 1, (W + 2 * PW - KW) // SW + 1)
        assert (P - 1) * SH - PH < H and (Q - 1) * SW - PW < W and PH < KH and PW < KW, geom          # every tap row meets the input
        for numel in (N * C * H * W, K * C * KH * KW, N * K * P * Q):
            assert numel * 4 < FOUR_MB // 4, (geom, numel)
        if fam == "dgrad":
            assert SH <= 2 and SW <= 2
        assert (fam, group, geom) not in seen, "a case twice"
        seen.add((fam, group, geom))
    bench = set()
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "conv_choices_mi355x.txt")) as f:
        for ln in f:
            v = [int(s) for s in ln.split()]
            if v:
                bench.add(tuple(v[1:12]))
    assert not bench & {c[0] for _, _, c in _all_cases()}, "a case copies a bench geometry"


def test_cases_are_dispatched_where_their_table_says():
    for group, cases in R.FWD_GROUPS:
        want = {"thin": "thin", "tap reuse": "tap reuse"}.get(group, "generic")
        for geom, plans, epis in cases:
            assert R.fwd_route(geom) == want, (group, geom)
            assert set(epis) <= set(R.EPI_F) and "none" in epis
            if group.startswith("cross"):
                assert set(R.CROSS) <= set(plans) and tuple(epis) == R.ALL_F
    for group, cases in R.DGRAD_GROUPS:
        for geom, plans, epis in cases:
            route = R.dgrad_route(geom)
            assert route == {"tap reuse": "tap reuse"}.get(group, "generic") or (group == "small C" and route.startswith("small C"))
            assert set(epis) <= set(R.EPI_D) and "none" in epis
            if group.startswith("cross"):
                assert set(R.CROSS) <= set(plans) and tuple(epis) == R.ALL_D
    assert len(R.FWD_CROSS) >= 8, "the full cross product on at least eight designated forward shapes"
    for group, cases in R.WGRAD_GROUPS:
        for geom, folds in cases:
            assert R.wgrad_route(geom) == group, (group, geom)
    # the regimes the tables name in their comments
    assert {R.fwd_route(c[0]) for c in R.FWD_THIN} == {"thin"}
    assert {c[0][4] for c in R.FWD_THIN if c[0][5] == 3} == {1, 2, 3, 4} and any(c[0][5] == 4 for c in R.FWD_THIN)
    halos = {R.halo_geom(c[0][2], c[0][3]) for c in R.FWD_HALO}
    assert 288 in halos and 264 in halos and {c[0][3] for c in R.FWD_HALO} == {4, 8, 16, 32, 64}
    assert {c[0][4] for c in R.FWD_HALO} >= {64, 80, 96, 160}
    assert {R.dgrad_route(c[0]) for c in R.DGRAD_SMALLC} == {"small C four-pixel", "small C plain"}
    assert {c[0][1] for c in R.DGRAD_SMALLC if R.dgrad_route(c[0]) == "small C four-pixel"} == {1, 2, 3}
    assert {c[0][1] for c in R.DGRAD_HALO} == {64, 68, 128}
    forms = {(c[0][4], R.wgrad_thin_form(c[0])[0]) for c in R.WGRAD_THIN}
    assert forms >= {(k, f) for k in (1, 2, 3, 4) for f in ("four-pixel", "scalar")}, forms
    slices = {(R.wgrad_thin_form(c[0])[0], min(2, R.wgrad_thin_form(c[0])[1])) for c in R.WGRAD_THIN}
    assert slices == {("four-pixel", 1), ("four-pixel", 2), ("scalar", 1), ("scalar", 2)}, slices
    # empty parity classes, an untouched column, an empty trailing split
    assert any(sum(1 for c in R.dgrad_classes(g[0]) if c[1] == 0) == 3 for g in R.DGRAD_MODEL)
    key, tile, splits = R.wgrad_regime((2, 20, 97, 16, 40, 3, 3, 1, 1, 1, 1))
    nk = R.cdiv(2 * 97 * 16, 16)
    assert (key, tile, splits) == (7, 2, 16) and (splits - 1) * R.cdiv(nk, splits) >= nk


def test_every_declared_regime_has_a_case():
    modelled = R.modelled_regimes()
    missing = sorted(R.DECLARED - modelled, key=str)
    assert not missing, "%d declared regimes without a case: %s" % (len(missing), missing[:20])
    fams = {r[0] for r in R.DECLARED}
    assert fams == {"fwd", "dgrad", "wgrad", "fwd path", "dgrad path"}
