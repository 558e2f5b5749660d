"""CPU: the host model of the pooling / loss / cluster-memory / optimizer units (tests/head_hostmodel.py) is one a correct
float32 implementation meets and a subtly wrong one does not.

  * plain float32 torch, on every case of the device tests, stays inside the per-element budget — and its ratios are the source
    of the constants (C_KIND = max(8, 4 x ratio));
  * the case lists reach every regime of the mirrored dispatch arithmetic (asserted from the mirrors);
  * the comparator rejects eleven small mutations of the reference;
  * the discrete outcomes (CM-hard minima, hinge / L1 kinks) are decided by a margin in every case, or by an exact tie.

Run as a script (python -m tests.test_head_hostmodel_cpu) it prints the ratio table of the host model's docstring."""
import functools

import torch
import torch.nn.functional as F

from tests import head_hostmodel as H

f32 = H.f32


# ---- float32 torch of every case ---------------------------------------------------------------------------------------------
def _sum32(op, x, par, gout, gscale):
    x = x.clone().requires_grad_(True)
    if op == "bce":
        loss = F.binary_cross_entropy(torch.sigmoid(x), torch.full_like(x, par))
    elif op == "mse":
        loss = F.mse_loss(x, torch.full_like(x, par))
    else:
        v = par[0] + par[1] * x
        loss = (v.relu() if par[2] else v).mean()
    (loss * (1.0 if gout is None else float(gout)) * gscale).backward()
    return loss.detach(), x.grad


def _sum_outputs():
    for i, (op, par, n, fam) in enumerate(H.sum_cases()):
        x = H.sum_input(op, par, n, fam)
        loss, _ = _sum32(op, x, par, None, 1.0)
        yield "%s n %d %s %s" % (op, n, par, fam), loss, H.two_stage(op, x, par)
    for op, par in [("bce", 0.83), ("bce", 1.0), ("bce", 0.0), ("mse", 0.83), ("affine", H.AFFINE[0]), ("affine", H.AFFINE[1]),
                    ("affine", H.AFFINE[3])]:
        for n in H.BWD_N:
            for fam in (H.FAMILIES if n < 1000 else H.FAMILIES[:2]):
                for gout, gs in ((None, 1.0), (torch.tensor(0.5), 0.3)):
                    x = H.sum_input(op, par, n, fam)
                    _, dx = _sum32(op, x, par, gout, gs)
                    yield "%s bwd n %d %s" % (op, n, fam), dx, H.sum_bwd(op, x, par, gout, gs)
    xs = torch.tensor(H.SATURATED * 3)
    for t in H.TARGETS:
        loss, dx = _sum32("bce", xs, t, None, 1.0)
        yield "bce saturated %s" % t, loss, H.two_stage("bce", xs, t, chain=True)
        yield "bce bwd saturated %s" % t, dx, H.sum_bwd("bce", xs, t, None, 1.0, chain=True)
    for n in (5, 257):                                   # planted kinks: exact zeros of a + b x
        for par in H.AFFINE[:2]:
            x = H.sum_input("affine", par, n, "plain", planted=True)
            loss, dx = _sum32("affine", x, par, None, 1.0)
            yield "affine planted", loss, H.two_stage("affine", x, par)
            yield "affine bwd planted", dx, H.sum_bwd("affine", x, par, None, 1.0)


def l1_pair(rows, inner, fam, seed=0, planted=True):
    g = H.gen(1000 * seed + 13 * rows + inner)
    a, b = H.family((rows, inner), fam, g), H.family((rows, inner), "plain" if fam == "constant" else fam, g)
    b = torch.where((a - b).abs() < 1e-3 + 128 * H.U24 * (a.abs() + b.abs()), b + 0.0625, b)      # off the kink of |a - b|
    if planted:
        b.reshape(-1)[::5] = a.reshape(-1)[::5]          # a == b: sign 0
        b.reshape(-1)[-1] = a.reshape(-1)[-1]
    return a.contiguous(), b.contiguous()


L1_CASES = [(1, 1), (1, 255), (1, 257), (1, 2048), (1, 2049), (6, 100), (5, 2049), (3, 23334), (7, (H.MAX_PARTIALS * 2048 + 2049) // 7 + 1)]


def l1_labels(rows, mode):
    if mode == "none":
        return None
    if mode == "mixed":
        return (torch.arange(rows) + 1) % 3               # 1, 2, 0, 1, ...: only 1 selects (row 0 does)
    return torch.zeros(rows, dtype=torch.int64)           # nothing selected


def _l1_outputs():
    for i, (rows, inner) in enumerate(L1_CASES):
        fam = H.FAMILIES[i % 4]
        a, b = l1_pair(rows, inner, fam, planted=i % 2 == 0)
        for mode in ("none", "mixed", "nothing"):
            lab = l1_labels(rows, mode)
            sel = torch.ones(rows, dtype=torch.bool) if lab is None else lab == 1
            ar, br = a.clone().requires_grad_(True), b.clone().requires_grad_(True)
            loss = F.l1_loss(ar[sel], br[sel])
            cnt = float(sel.sum()) * inner
            ref = H.l1_fwd(a, b, lab)
            out2 = torch.stack([loss.detach(), torch.tensor(1.0) / torch.tensor(cnt)])
            yield "l1 %s %s %s" % ((rows, inner), fam, mode), out2, ref
            if cnt:
                (loss * 10.0 * 0.25).backward()
                da, db = H.l1_bwd(a, b, lab, torch.tensor(10.0), ref.value.float(), 0.25)
                yield "l1 da", ar.grad, da
                yield "l1 db", br.grad, db


def _rows_outputs():
    for rows in H.ROWS:
        for i, inner in enumerate(H.ROWS_INNER):
            fam = H.FAMILIES[(i + rows) % 4]
            a, b = l1_pair(rows, inner, fam, seed=1)
            grow = torch.randn(rows, generator=H.gen(inner))
            ar, br = a.clone().requires_grad_(True), b.clone().requires_grad_(True)
            out = (ar - br).abs().flatten(1).mean(-1)
            (out * grow).sum().backward()
            da, db = H.rows_bwd("l1_rows", a, b, grow)
            yield "l1_rows %s" % ((rows, inner),), out.detach(), H.rows_fwd("l1_rows", a, b)
            yield "l1_rows da", ar.grad, da
            yield "l1_rows db", br.grad, db
            for c in (1.0, 0.0, 0.83):
                xr = a.clone().requires_grad_(True)
                out = ((xr - c) ** 2).flatten(1).mean(-1)
                (out * grow).sum().backward()
                yield "mse_rows %s c %s %s" % ((rows, inner), c, fam), out.detach(), H.rows_fwd("mse_rows", a, c)
                yield "mse_rows dx", xr.grad, H.rows_bwd("mse_rows", a, c, grow)
            for gfam in ("plain", "scales", "zero_row", "const0", "const1"):
                gr = gp_input(rows, inner, gfam)
                t = gr.clone().requires_grad_(True)
                n = (t + 1e-16).norm(2, dim=1)
                pen = 10.0 * (n - 1.0) ** 2
                pen.sum().backward()
                rp, rv = H.grad_penalty_rows(gr, 1.0, 10.0)
                yield "gp pen %s %s" % ((rows, inner), gfam), pen.detach(), rp
                yield "gp v %s %s" % ((rows, inner), gfam), t.grad, rv


def gp_input(rows, D, fam):
    g = H.gen(3 * rows + D)
    if fam in ("plain", "scales"):
        return H.family((rows, D), fam, g)
    if fam == "zero_row":
        x = H.family((rows, D), "plain", g)
        x[0] = 0.0
        return x
    return torch.full((rows, D), 0.0 if fam == "const0" else 1.0)


def _ce_outputs():
    for i, (B, K, sc, fam, given) in enumerate(H.ce_cases()):
        z, lab = H.ce_input(B, K, fam, seed=i), H.ce_labels(B, K)
        ign = torch.where(H.in_range(lab, K), lab, torch.full_like(lab, -100))
        grow = torch.rand(B, generator=H.gen(i)) + 0.5 if given else None
        zr = z.clone().requires_grad_(True)
        loss = F.cross_entropy(zr * sc, ign, reduction="none", ignore_index=-100)
        (loss * (1.0 if grow is None else grow) * 0.7).sum().backward()
        f = H.softmax_ce_fwd(z, lab, sc)
        tag = "ce B %d K %d scale %s %s" % (B, K, sc, fam)
        yield tag + " loss", loss.detach(), f["loss"]
        yield tag + " lse", torch.logsumexp(z * sc, 1), f["lse"]
        yield tag + " dz", zr.grad, H.softmax_ce_bwd(z, lab, f["lse"].value.float(), grow, sc, 0.7)
    for n in H.WSUM_N:
        for fam in H.FAMILIES:
            g = H.gen(n)
            x, w = H.family((n,), fam, g), torch.rand(n, generator=g)
            yield "wsum %d %s" % (n, fam), (x * w).sum() * 0.125, H.weighted_sum_fwd(x, w, 0.125)
            yield "wsum no w", x.sum() * 0.125, H.weighted_sum_fwd(x, None, 0.125)
            yield "wsum bwd", torch.tensor(0.5) * 0.125 * w, H.weighted_sum_bwd(torch.tensor(0.5), w, n, 0.125)


def torch_maxpool(x, geo):
    """F.max_pool2d with its flat plane indices turned into window-relative ones"""
    H_, W, KH, KW, SH, SW, PH, PW = geo
    y, idx = F.max_pool2d(x, (KH, KW), (SH, SW), (PH, PW), return_indices=True)
    P, Q = y.shape[2:]
    r = idx // W - (torch.arange(P) * SH - PH).reshape(1, 1, P, 1)
    s = idx % W - (torch.arange(Q) * SW - PW).reshape(1, 1, 1, Q)
    return y, r * KW + s


def _pool_outputs():
    for i, (N, C, geo, fam) in enumerate(H.pool_cases() + [H.POOL_BIG[:2] + (H.POOL_BIG[2:], "ties")]):
        x = H.pool_input(N, C, geo[0], geo[1], fam, seed=i)
        ry, ra = H.maxpool_fwd(x, *geo[2:])
        xr = x.clone().requires_grad_(True)
        y, arg = torch_maxpool(xr, geo)
        tag = "maxpool %s %s %s" % ((N, C), geo, fam)
        yield tag + " y", y.detach(), ry
        yield tag + " argmax", arg, ra
        dy = torch.randn(y.shape, generator=H.gen(i))
        y.backward(dy)
        yield tag + " dx", xr.grad, H.maxpool_bwd(dy, ra.value, x.shape, *geo[2:])
    for HW in H.GAP_HW:
        for j, (N, C) in enumerate(H.GAP_PLANES):
            fam = H.FAMILIES[(HW + j) % 4]
            x = H.family((N, C, HW), fam, H.gen(HW + j))
            dy = torch.randn(N, C, generator=H.gen(HW))
            yield "gap %s %s" % ((N, C, HW), fam), x.mean(2), H.gap_fwd(x)
            yield "gap bwd", (dy / HW).reshape(N, C, 1).expand(N, C, HW), H.gap_bwd(dy, x.shape)
            for p in H.GEM_P:
                x = H.gem_input(N, C, HW, seed=j)
                xr, pr = x.clone().requires_grad_(True), torch.tensor([p], requires_grad=True)
                y = xr.clamp(min=1e-6).pow(pr).mean(2).pow(1.0 / pr)
                y.backward(dy)
                ry = H.gem_fwd(x, pr.detach())
                rdx, rdp = H.gem_bwd(x, pr.detach(), ry.value.float(), dy)
                tag = "gem %s p %s" % ((N, C, HW), p)
                yield tag + " y", y.detach(), ry
                yield tag + " dx", xr.grad, rdx
                yield tag + " dp", pr.grad, rdp


def _cm_loop32(x, y, feats, mom, normalize_eps):
    f = feats.clone()
    for xi, yi in zip(x, y.tolist()):
        if yi < 0 or yi >= f.shape[0]:
            continue
        f[yi] = mom * f[yi] + (1.0 - mom) * xi
        f[yi] = F.normalize(f[yi], dim=0) if normalize_eps else f[yi] / f[yi].norm()
    return f


def _cm_hard32(x, y, feats, mom):
    f = feats.clone()
    for lab in sorted(set(v for v in y.tolist() if 0 <= v < f.shape[0])):
        idx = (y == lab).nonzero().flatten()
        j = idx[(x[idx] @ feats[lab]).argmin()]
        f[lab] = f[lab] * mom + (1.0 - mom) * x[j]
        f[lab] /= f[lab].norm()
    return f


def nlr_input(n_ids, D, rows=9):
    g = H.gen(n_ids * 100 + D)
    gm = H.family((rows, D), "scales", g)
    gm[2] = 0.0                                              # a zero row: 0 / (0 + eps) = 0
    ids = torch.tensor(([2, 7, 2, -1, rows][:n_ids]) if n_ids > 1 else [rows - 1])
    return gm, ids


def _cm_outputs():
    for i, (B, D, pat, mom, ne) in enumerate(H.cm_cases()):
        x, feats = H.cm_input(B, D, seed=i)
        y = H.cm_labels(pat, B)
        tag = "cm B %d D %d %s mom %s eps %d" % (B, D, pat, mom, ne)
        yield tag, _cm_loop32(x, y, feats, mom, ne), H.cm_update(x, y, feats, mom, ne)
        for tie in (False, True):
            x, feats = H.cm_input(B, D, seed=i, tie=tie)
            yield tag + " hard", _cm_hard32(x, y, feats, mom), H.cm_update_hard(x, y, feats, mom)
    x, feats = H.cm_input(4, 64)
    x[:] = 0.0
    y = torch.tensor([1, 1, 2, 3])
    yield "cm zero vector", _cm_loop32(x, y, feats, 0.0, 1), H.cm_update(x, y, feats, 0.0, 1)
    for n_ids in H.NLR_N:
        for D in H.NLR_D:
            gm, ids = nlr_input(n_ids, D)
            g32 = gm.clone()
            for t in sorted(set(v for v in ids.tolist() if 0 <= v < gm.shape[0])):
                g32[t] /= g32[t].norm() + 1e-16
            yield "normalize_listed_rows %d %d" % (n_ids, D), g32, H.normalize_listed_rows(gm, ids, 1e-16)


LR, EPS = 3.5e-4, 1e-8
SGD_CASES = [(n, mom, first) for n in (1, 5, 1003) for mom, first in ((0.9, True), (0.9, False), (0.0, True))] + [(H.DEV_BIG, 0.9, False)]


def _adam32(p, g, m, v, step, betas, wd, gs):
    pr = p.clone().requires_grad_(True)
    opt = torch.optim.Adam([pr], lr=f32(LR), betas=(f32(betas[0]), f32(betas[1])), eps=f32(EPS), weight_decay=f32(wd), foreach=False)
    opt.state[pr] = {"step": torch.tensor(float(step - 1)), "exp_avg": m.clone(), "exp_avg_sq": v.clone()}
    pr.grad = g * gs
    opt.step()
    st = opt.state[pr]
    return {"p": pr.detach(), "m": st["exp_avg"], "v": st["exp_avg_sq"]}


def _optim_outputs():
    for i, (n, step, betas, wd, gs, fam) in enumerate(H.adam_cases()):
        p, g, m, v = H.optim_input(n, fam, seed=i)
        got = _adam32(p, g, m, v, step, betas, wd, gs)
        ref = H.adam_step(p, g, m, v, LR, betas[0], betas[1], EPS, wd, step, gs)
        for k in ("p", "m", "v"):
            yield "adam n %d step %d %s wd %s %s %s" % (n, step, betas, wd, fam, k), got[k], ref[k]
    for i, (n, mom, first) in enumerate(SGD_CASES):
        p, g, buf, _ = H.optim_input(n, "plain", seed=50 + i)
        for wd, gs in ((1e-4, 1.0), (0.0, 0.125)):
            pr = p.clone().requires_grad_(True)
            opt = torch.optim.SGD([pr], lr=f32(0.01), momentum=f32(mom), weight_decay=f32(wd), foreach=False)
            if not first:
                opt.state[pr] = {"momentum_buffer": buf.clone()}
            pr.grad = g * gs
            opt.step()
            ref = H.sgd_step(p, g, buf if mom else None, 0.01, mom, wd, first, gs)
            yield "sgd n %d mom %s first %s p" % (n, mom, first), pr.detach(), ref["p"]
            if mom:
                yield "sgd buf", opt.state[pr]["momentum_buffer"], ref["buf"]


def _all_outputs():
    for gen_ in (_sum_outputs, _l1_outputs, _rows_outputs, _ce_outputs, _pool_outputs, _cm_outputs, _optim_outputs):
        for item in gen_():
            yield item


@functools.lru_cache(maxsize=None)
def _ratios():
    """one thread: torch splits a long sum among its threads, and the yardstick should not depend on how many a host has"""
    worst, bad, count = {}, [], 0
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        for name, got, ref in _all_outputs():
            w = H.compare(got, ref)
            count += 1
            if ref.kind != "exact":
                worst[ref.kind] = max(worst.get(ref.kind, 0.0), w.ratio)
            if not w.ok:
                bad.append("%s: worst %s err %.3e budget %.3e ratio %.2f" % (name, w.index, w.err, w.budget, w.ratio))
    finally:
        torch.set_num_threads(threads)
    return worst, bad, count


def test_float32_torch_meets_the_budget_on_every_case():
    worst, bad, count = _ratios()
    print({k: round(v, 2) for k, v in sorted(worst.items())}, count, "outputs")
    assert not bad, "\n".join(bad[:40])
    assert set(worst) == set(H.C_KIND) - {"exact"}


def test_constants_follow_the_rule():
    """C_KIND = max(8, 4 x float32-torch ratio) as measured where the table was made; torch's summation order differs between
    hosts (threads, vector width), hence a quarter of slack here instead of equality."""
    worst, _, _ = _ratios()
    for k, r in worst.items():
        assert H.C_KIND[k] >= 8.0 and 4.0 * r <= 1.25 * H.C_KIND[k], (k, r, H.C_KIND[k])
    assert H.C_KIND["exact"] == 0.0


# ---- reach: asserted from the mirrors ------------------------------------------------------------------------------------------
def test_case_lists_reach_every_regime():
    grids = set(H.partial_grid(n) for n in H.SUM_N)
    assert 1 in grids and H.MAX_PARTIALS in grids and any(1 < g < H.MAX_PARTIALS for g in grids)
    assert H.partial_grid(2048) == 1 and H.partial_grid(2049) == 2
    assert H.sum_trips(H.SUM_N[-1]) == 9 and H.SUM_N[-1] % (H.MAX_PARTIALS * 256) != 0       # some threads make an extra trip
    for op in ("bce", "mse", "affine"):
        ns = set(n for o, _, n, _ in H.sum_cases() if o == op)
        assert ns == set(H.SUM_N), op
        assert set(f for o, _, n, f in H.sum_cases() if o == op) == set(H.FAMILIES)
    for t in H.TARGETS:
        assert any(o == "bce" and p == t and n == H.SUM_N[-1] for o, p, n, _ in H.sum_cases())
    assert set(H.partial_grid(r * i) for r, i in L1_CASES) >= {1, 2, H.MAX_PARTIALS} and any(i % 256 for _, i in L1_CASES)
    assert [H.trips("loss", n) for n in H.BWD_N] == [1, 1, 2]
    assert H.trips("loss", 5 * 1027) == 1 and H.trips("loss", ROWS_BWD_BIG[0] * ROWS_BWD_BIG[1]) == 2
    # pooling: both backward kernels at the same geometry; the second trip; partly empty last workgroups
    w4 = [g for g in H.POOL_GEOM if H.maxpool_bwd_kernel(*g[2:], W=g[1], dx_addr=0) == "four"]
    assert len(w4) >= 2 and all(H.maxpool_bwd_kernel(*g[2:], W=g[1], dx_addr=4) == "gather" for g in w4)
    assert any(H.maxpool_bwd_kernel(*g[2:], W=g[1], dx_addr=0) == "gather" and g[2:] == (3, 3, 2, 2, 1, 1) for g in H.POOL_GEOM)
    N, C, Hh, W = H.POOL_BIG[:4]
    P, Q = H.pool_out(Hh, W, *H.POOL_BIG[4:])
    assert H.trips("pool", N * C * P * Q) == 2 and N * C <= 65535
    for geo in H.POOL_GEOM:
        assert set(f for _, _, g, f in H.pool_cases() if g == geo) >= {"relu", "ties"}
    assert set(f for _, _, _, f in H.pool_cases()) == set(H.POOL_FAMILIES)
    assert set(N * C for N, C, _, _ in H.pool_cases()) == {1, 10, 7}
    assert [H.wave_workgroups(n * c) for n, c in H.GAP_PLANES] == [(1, 1), (1, 4), (2, 1)]
    assert H.trips("pool", GAP_BWD_BIG[0] * GAP_BWD_BIG[1] * GAP_BWD_BIG[2]) == 2
    # cluster memory: the register limit on both sides, every chain length
    assert max(H.CM_D) == H.CM_MAX_D and H.CM_MAX_D - 1 in H.CM_D
    assert set((B, D) for B, D, _, _, _ in H.cm_cases()) >= set((B, D) for B in H.CM_B for D in H.CM_D)
    assert set(p for _, _, p, _, _ in H.cm_cases()) == set(H.CM_PATTERNS) and set(m for _, _, _, m, _ in H.cm_cases()) == set(H.CM_MOM)
    assert set(e for _, _, _, _, e in H.cm_cases()) == {0, 1}
    assert [H.wave_workgroups(n) for n in H.NLR_N] == [(1, 1), (1, 4), (2, 1)]
    # optimizers: nv == 0, every n % 4, the second float4 trip with a tail
    splits = [H.adam_split(n) for n, *_ in H.adam_cases()]
    assert any(nv == 0 for nv, _, _ in splits) and set(t for _, t, _ in splits) == {0, 1, 2, 3}
    nv, tail, grid = H.adam_split(H.ADAM_BIG)
    assert grid == H.GRID_CAP["optim"] and H.cdiv(nv, grid * 256) == 2 and tail == 3
    assert H.trips("optim", H.DEV_BIG) == 2
    assert set(s for _, s, *_ in H.adam_cases()) == set(H.ADAM_STEPS)
    assert set(c[2] for c in H.adam_cases()) == set(H.ADAM_BETAS) and set(c[3] for c in H.adam_cases()) == set(H.ADAM_WD)
    assert set(c[4] for c in H.adam_cases()) == set(H.GSCALES) and set(c[5] for c in H.adam_cases()) == {"plain", "scales"}


ROWS_BWD_BIG = (5, 209767)                                # rows * inner = 4096 * 256 + 259: *_rows_bwd past the grid cap
GAP_BWD_BIG = (1, 5, 419431)                              # 5 * 419431 = 8192 * 256 + 3: gap_bwd past its cap


# ---- mutations: the host check must reject each ----------------------------------------------------------------------------------
def _rejects(got, ref):
    return not H.compare(got, ref).ok


def test_mutation_1_last_element_left_at_the_fill_value():
    x = H.sum_input("mse", 0.83, 257, "plain")
    ref = H.sum_bwd("mse", x, 0.83, None, 1.0)
    got = ref.value.float()
    assert not _rejects(got, ref)
    got[-1] = H.FILL
    assert _rejects(got, ref)
    p, g, m, v = H.optim_input(1003, "plain")
    ref = H.adam_step(p, g, m, v, LR, 0.9, 0.999, EPS, 0.0, 2, 1.0)
    for k in ("p", "m", "v"):
        got = ref[k].value.float()
        assert not _rejects(got, ref[k])
        got[1000 - 4:1000] = H.FILL                      # the last float4
        assert _rejects(got, ref[k])


def test_mutation_2_sum_without_its_last_term():
    for op, par in (("bce", 0.83), ("mse", 0.0), ("affine", H.AFFINE[0])):
        for n in (H.SUM_N[1], H.SUM_N[-1]):
            fam = [f for o, p, nn, f in H.sum_cases() if o == op and nn == n][0]
            x = H.sum_input(op, par, n, fam)
            term, _ = H.sum_terms(op, x, par)
            ref = H.two_stage(op, x, par)
            assert not _rejects(ref.value.float(), ref)
            assert _rejects(((term.sum() - term[-1]) / n).float(), ref), (op, n, fam)
    x = torch.tensor([0.3])                               # the smallest case: the only term
    assert _rejects(torch.tensor(0.0), H.two_stage("mse", x, 0.83))


def test_mutation_3_sign_at_a_tie_taken_as_greater_or_equal():
    a, b = l1_pair(5, 257, "plain", planted=True)
    out2 = H.l1_fwd(a, b, None).value.float()
    da, _ = H.l1_bwd(a, b, None, None, out2, 1.0)
    g = float(out2[1])
    mut = torch.where(a.double() - b.double() >= 0, g, -g)
    assert bool((a == b).any()) and _rejects(mut.float(), da) and not _rejects(da.value.float(), da)
    par = H.AFFINE[0]
    x = H.sum_input("affine", par, 257, "plain", planted=True)
    ref = H.sum_bwd("affine", x, par, None, 1.0)
    v = par[0] + par[1] * x.double()
    assert bool((v == 0).any())
    mut = torch.where(v >= 0, torch.full_like(v, par[1] / 257.0), torch.zeros_like(v))
    assert _rejects(mut.float(), ref) and not _rejects(ref.value.float(), ref)


def test_mutation_4_argmax_takes_the_last_of_equal_maxima():
    geo = H.POOL_GEOM[2]
    x = H.pool_input(2, 5, geo[0], geo[1], "ties")
    _, ra = H.maxpool_fwd(x, *geo[2:])
    _, mut = H.maxpool_fwd(x, *geo[2:], last=True)
    assert _rejects(mut.value, ra) and not _rejects(ra.value, ra)


def test_mutation_5_gradient_in_an_ignored_row():
    z, lab = H.ce_input(5, 63, "cosine"), H.ce_labels(5, 63)
    lse = H.softmax_ce_fwd(z, lab, 20.0)["lse"].value.float()
    ref = H.softmax_ce_bwd(z, lab, lse, None, 20.0, 1.0)
    mut = 20.0 * torch.exp(z.double() * 20.0 - lse.double().reshape(5, 1))            # g * softmax in the ignored rows
    got = torch.where(H.in_range(lab, 63).reshape(5, 1), ref.value, mut)
    assert _rejects(got.float(), ref) and not _rejects(ref.value.float(), ref)
    assert bool((ref.value[2:] == 0).all()) and bool((ref.M[2:] == 0).all())


def test_mutation_6_adam_eps_inside_the_root_or_bias_correction_off_by_one():
    tried = {"eps_inside": 0, "step_off": 0}
    for n, step, betas, wd, gs, fam in [c for c in H.adam_cases() if c[0] == 1003]:
        p, g, m, v = H.optim_input(n, fam)
        ref = H.adam_step(p, g, m, v, LR, betas[0], betas[1], EPS, wd, step, gs)["p"]
        assert not _rejects(ref.value.float(), ref)
        # eps inside the root shows where sqrt(v') is not far above sqrt(eps): the `scales` family carries such elements
        if fam == "scales":
            assert _rejects(H.adam_step(p, g, m, v, LR, betas[0], betas[1], EPS, wd, step, gs, "eps_inside")["p"].value.float(), ref)
            tried["eps_inside"] += 1
        if step > 1:
            assert _rejects(H.adam_step(p, g, m, v, LR, betas[0], betas[1], EPS, wd, step, gs, "step_off")["p"].value.float(), ref), step
            tried["step_off"] += 1
    assert tried["eps_inside"] >= 1 and tried["step_off"] >= 2, tried


def test_mutation_7_sgd_reads_the_buffer_on_the_first_step():
    p, g, buf, _ = H.optim_input(1003, "plain")
    ref = H.sgd_step(p, g, buf, 0.01, 0.9, 1e-4, True, 1.0)
    mut = H.sgd_step(p, g, buf, 0.01, 0.9, 1e-4, True, 1.0, read_buf_first=True)
    for k in ("p", "buf"):
        assert _rejects(mut[k].value.float(), ref[k]) and not _rejects(ref[k].value.float(), ref[k])


def test_mutation_8_cm_update_normalises_once_per_label():
    x, feats = H.cm_input(8, 257)
    y = H.cm_labels("mixed", 8)
    ref = H.cm_update(x, y, feats, 0.2, 0)
    mut = H.cm_update(x, y, feats, 0.2, 0, once_per_label=True)
    assert _rejects(mut.value.float(), ref) and not _rejects(ref.value.float(), ref)


def test_mutation_9_cm_hard_takes_the_last_of_tied_minima():
    """bit-identical rows give the same update whichever is taken, so the later twin differs from the earlier one in one
    coordinate that does not enter the dot product: a zero of the centroid.  The pair (samples 1 and 3 of label 3) is the
    minimum of its label: the label's other samples are the centroid itself"""
    x, feats = H.cm_input(8, 257, tie=True)
    y = H.cm_labels("mixed", 8)
    for j in (0, 7):
        x[j] = feats[3]
    f2 = feats.clone()
    f2[3, 0] = 0.0
    x3 = x.clone()
    x3[3, 0] = x[1, 0] + 0.5
    lst = H.cm_dots(x3, y, f2)[3]
    assert lst[1][1] == lst[2][1] == min(d for _, d, _ in lst)
    ref = H.cm_update_hard(x3, y, f2, 0.2)
    mut = H.cm_update_hard(x3, y, f2, 0.2, last=True)
    assert _rejects(mut.value.float(), ref) and not _rejects(ref.value.float(), ref)


def test_mutation_10_gem_dp_without_the_log_m_term():
    x = H.gem_input(1, 5, 65)
    p = torch.tensor([3.0])
    y = H.gem_fwd(x, p).value.float()
    dy = torch.randn(1, 5, generator=H.gen(1))
    _, rdp = H.gem_bwd(x, p, y, dy)
    _, mut = H.gem_bwd(x, p, y, dy, drop_log_m=True)
    assert _rejects(mut.value.float(), rdp) and not _rejects(rdp.value.float(), rdp)


def test_mutation_11_l1_denominator_counts_all_rows():
    a, b = l1_pair(6, 100, "plain")
    lab = l1_labels(6, "mixed")
    ref = H.l1_fwd(a, b, lab)
    sel = lab == 1
    s = (a.double() - b.double()).abs()[sel].sum()
    mut = torch.stack([s / 600.0, torch.tensor(1.0 / 600.0, dtype=torch.float64)])
    assert _rejects(mut.float(), ref) and not _rejects(ref.value.float(), ref)


# ---- discrete outcomes are decided by a margin, or by an exact tie -------------------------------------------------------------------
def test_cm_hard_minima_are_decided():
    """in EVERY CM-hard case the fp64 gap between the smallest and the second-smallest dot product of a label is at least
    64 * 2^-24 * sum |f_d x_d|, or the two are an exact tie of bit-identical rows"""
    seen_tie = 0
    for i, (B, D, pat, mom, ne) in enumerate(H.cm_cases()):
        y = H.cm_labels(pat, B)
        for tie in (False, True):
            x, feats = H.cm_input(B, D, seed=i, tie=tie)
            for lab, lst in H.cm_dots(x, y, feats).items():
                ds = sorted(lst, key=lambda t: t[1])
                for (j0, d0, m0), (j1, d1, m1) in zip(ds, ds[1:]):
                    if torch.equal(x[j0], x[j1]):
                        assert d0 == d1
                        seen_tie += 1
                    else:
                        assert d1 - d0 >= H.KINK_ULPS * H.U24 * max(m0, m1), (B, D, pat, lab, j0, j1, d1 - d0)
                    break                                 # the smallest pair decides
    assert seen_tie > 0


def test_plain_hinge_and_l1_cases_keep_off_the_kink():
    for op, par, n, fam in H.sum_cases():
        if op == "affine" and par[2]:
            x = H.sum_input(op, par, n, fam).double()
            v = f32(par[0]) + f32(par[1]) * x
            assert bool((v != 0).all()) and H.kink_margin(v, abs(par[0]) + (par[1] * x).abs()) >= 1.0, (par, n, fam)
    for i, (rows, inner) in enumerate(L1_CASES):
        a, b = l1_pair(rows, inner, H.FAMILIES[i % 4], planted=i % 2 == 0)
        d = a.double() - b.double()
        assert H.kink_margin(d, a.double().abs() + b.double().abs()) >= 1.0
        assert bool((d == 0).any()) == (i % 2 == 0)        # zeros only where planted, exact by construction (b = a)
    for par in H.AFFINE[:2]:
        x = H.sum_input("affine", par, 257, "plain", planted=True)
        fused = torch.tensor(par[0], dtype=torch.float64) + par[1] * x.double()
        unfused = torch.tensor(par[0]) + (torch.tensor(par[1]) * x)
        assert bool(((fused == 0) == (unfused == 0)).all()) and bool((fused == 0).any())


if __name__ == "__main__":
    worst, bad, count = _ratios()
    print("\n".join(bad))
    print("    kind       float32 torch ratio    C_KIND")
    for k in H.C_KIND:
        r = worst.get(k, 0.0)
        print("    %-10s %-22s %s" % (k, "%.2f" % r, "%g" % (0.0 if k == "exact" else max(8.0, round(4.0 * r, 2)))))
    print(count, "outputs")
