"""GPU: the part pooling kernels (csrc/pool.hip, rg_part_pool_fwd / rg_part_pool_bwd) and the fused multi-part head
(csrc/part_head.hip, rg_mp_head_fwd / rg_mp_head_bwd) per element against fp64, every element compared, every output between two
rows of guard values, and two runs of every kernel byte-equal.

A part pool is the existing pool on a contiguous sub-range of each plane, so its references and error budgets are
tests/head_hostmodel.py's gap_fwd / gap_bwd / gem_fwd / gem_bwd applied to x[:, :, lo:hi]; dp is the sum of the two parts' Refs.
The head is checked against tests/mp_hostmodel.py (budgets derived there); its backward is handed the rounded reference forward.

Each check prints `RATIO <entry point> <output> <family> <max err / (2^-24 M)>` (pytest -s shows them;
profiles/mp_elementwise_ratios.txt keeps the worst per entry point and output)."""
import pytest
import torch

from tests import head_hostmodel as HH
from tests import mp_hostmodel as H
from tests.test_head_elementwise_gpu import _Out, _lib, _ptr, _st, _to

pytestmark = pytest.mark.gpu

# (H, W, split_row): what the launch arithmetic distinguishes (one wave per plane, 64 lanes, float4 units between a scalar head / tail)
PART_GEOM = [
    (16, 8, 8),       # the recipe's case: 64 + 64, one trip per lane
    (4, 2, 2),        # parts shorter than a wave
    (5, 2, 2),        # unequal parts, odd HW: every second plane base is off 16-byte alignment
    (14, 14, 7),      # boundary at element 98: misaligned start of part 1, second loop trip
    (3, 1, 1),        # a 1-element part
    (24, 12, 12),     # parts above 128 elements
]
PART_PLANES = [(2, 4), (1, 5)]          # N C a multiple of 4, and N C % 4 == 1: a ragged last workgroup


def _check(out, ref, what, fam, table=None):
    out.guards(what)
    w = HH.compare(out.t, ref, table)
    assert w.ok, "%s: worst element %s err %.3e > budget %.3e (%s, max err/(2^-24 M) = %.2f)" % (
        what, w.index, w.err, w.budget, ref.kind, w.ratio)
    print("RATIO %s %s %.3f" % (what.split(" | ")[0], fam, w.ratio))


def _cat_parts(refs, dim):
    return HH.Ref(torch.cat([r.value for r in refs], dim), torch.cat([r.M for r in refs], dim), refs[0].kind)


def _stack_parts(refs):
    return HH.Ref(torch.stack([r.value for r in refs]), torch.stack([r.M for r in refs]), refs[0].kind)


@pytest.mark.parametrize("geom", PART_GEOM, ids=lambda g: "%dx%d_%d" % g)
def test_part_average_pool(dev, geom):
    lib = _lib()
    Hh, W, split = geom
    HW, n0 = Hh * W, split * W
    for j, (N, C) in enumerate(PART_PLANES):
        for fam in HH.FAMILIES:
            x = HH.family((N, C, HW), fam, HH.gen(HW + 11 * j))
            dy = torch.randn(2, N, C, generator=HH.gen(HW + j))
            xd, dyd = _to(dev, x, dy)
            tag = "%s planes %s %s" % (geom, (N, C), fam)
            y = _Out((2, N, C), dev)
            lib.rg_part_pool_fwd(xd.data_ptr(), None, y.ptr, N, C, Hh, W, split, 0.0, _st())
            _check(y, _stack_parts([HH.gap_fwd(x[:, :, :n0]), HH.gap_fwd(x[:, :, n0:])]), "rg_part_pool_fwd y(avg) | " + tag, fam)
            y2 = _Out((2, N, C), dev)
            lib.rg_part_pool_fwd(xd.data_ptr(), None, y2.ptr, N, C, Hh, W, split, 0.0, _st())
            assert torch.equal(y.buf, y2.buf), "rg_part_pool_fwd (avg): two runs differ | " + tag
            ref = _cat_parts([HH.gap_bwd(dy[0], (N, C, n0)), HH.gap_bwd(dy[1], (N, C, HW - n0))], 2)
            for shift in (0, 1):                        # dx planes on and off the alignment the float4 units need
                dx = _Out((N, C, HW), dev, shift=shift)
                lib.rg_part_pool_bwd(None, None, None, dyd.data_ptr(), dx.ptr, None, N, C, Hh, W, split, 0.0, None, 0, _st())
                _check(dx, ref, "rg_part_pool_bwd dx(avg) | %s shift %d" % (tag, shift), fam)


@pytest.mark.parametrize("geom", PART_GEOM, ids=lambda g: "%dx%d_%d" % g)
def test_part_gem_pool(dev, geom):
    """GeM p of 1, 3, 6.5 on values below, at and above eps, negatives and an entirely clamped plane (the zero-gradient branch of
    the clamp); dp given and NULL; the workspace exactly 4 N C bytes"""
    lib = _lib()
    Hh, W, split = geom
    HW, n0 = Hh * W, split * W
    for j, (N, C) in enumerate(PART_PLANES):
        x = HH.gem_input(N, C, HW, seed=j)
        dy = torch.randn(2, N, C, generator=HH.gen(HW + j))
        for p in HH.GEM_P:
            pt = torch.tensor([p])
            xd, dyd, pd = _to(dev, x, dy, pt)
            tag = "%s planes %s p %s" % (geom, (N, C), p)
            y = _Out((2, N, C), dev)
            lib.rg_part_pool_fwd(xd.data_ptr(), pd.data_ptr(), y.ptr, N, C, Hh, W, split, 1e-6, _st())
            ry = [HH.gem_fwd(x[:, :, :n0], pt), HH.gem_fwd(x[:, :, n0:], pt)]
            _check(y, _stack_parts(ry), "rg_part_pool_fwd y(gem) | " + tag, "planted")
            y2 = _Out((2, N, C), dev)
            lib.rg_part_pool_fwd(xd.data_ptr(), pd.data_ptr(), y2.ptr, N, C, Hh, W, split, 1e-6, _st())
            assert torch.equal(y.buf, y2.buf), "rg_part_pool_fwd (gem): two runs differ | " + tag
            y32 = torch.stack([r.value for r in ry]).float()            # the backward is handed the rounded reference forward
            yd, = _to(dev, y32)
            r0, p0 = HH.gem_bwd(x[:, :, :n0], pt, y32[0], dy[0])
            r1, p1 = HH.gem_bwd(x[:, :, n0:], pt, y32[1], dy[1])
            rdx, rdp = _cat_parts([r0, r1], 2), HH.Ref(p0.value + p1.value, p0.M + p1.M, p0.kind)
            prev = None
            for need_dp, shift in ((True, 0), (False, 0), (True, 1), (True, 0)):
                ws = _Out((N * C,), dev)
                dx = _Out((N, C, HW), dev, shift=shift)
                dp = _Out((1,), dev) if need_dp else None
                lib.rg_part_pool_bwd(xd.data_ptr(), pd.data_ptr(), yd.data_ptr(), dyd.data_ptr(), dx.ptr, _ptr(dp), N, C, Hh, W, split,
                                     1e-6, ws.ptr if need_dp else None, 4 * N * C if need_dp else 0, _st())
                _check(dx, rdx, "rg_part_pool_bwd dx(gem) | %s dp %s shift %d" % (tag, need_dp, shift), "planted")
                ws.guards("rg_part_pool_bwd workspace")
                if need_dp:
                    _check(dp, rdp, "rg_part_pool_bwd dp | " + tag, "planted")
                else:
                    ws.untouched("rg_part_pool_bwd workspace without dp")
                if need_dp and shift == 0:
                    if prev is not None:
                        assert torch.equal(prev[0], dx.buf) and torch.equal(prev[1], dp.buf), "rg_part_pool_bwd: two runs differ | " + tag
                    prev = (dx.buf, dp.buf)
        ws, dx, dp = _Out((N * C,), dev), _Out((N, C, HW), dev), _Out((1,), dev)
        with pytest.raises(RuntimeError, match="workspace too small"):
            lib.rg_part_pool_bwd(xd.data_ptr(), pd.data_ptr(), yd.data_ptr(), dyd.data_ptr(), dx.ptr, dp.ptr, N, C, Hh, W, split, 1e-6,
                                 ws.ptr, 4 * N * C - 1, _st())
        dx.untouched("rg_part_pool_bwd dx after the workspace error")
        dp.untouched("rg_part_pool_bwd dp after the workspace error")


def test_part_pool_through_the_ops_wrappers(dev):
    from rg_hip import ops
    N, C, Hh, W, split = 1, 5, 5, 2, 2
    n0 = split * W
    x = HH.gem_input(N, C, Hh * W).reshape(N, C, Hh, W)
    xf = x.reshape(N, C, -1)
    pt, dy = torch.tensor([3.0]), torch.randn(2, N, C, generator=HH.gen(9))
    y = ops.part_pool_fwd(x.to(dev), split, pt.to(dev))
    ry = [HH.gem_fwd(xf[:, :, :n0], pt), HH.gem_fwd(xf[:, :, n0:], pt)]
    HH.check(y, _stack_parts(ry), "ops.part_pool_fwd")
    y32 = torch.stack([r.value for r in ry]).float()
    dx, dp = ops.part_pool_bwd(x.to(dev), split, dy.to(dev), pt.to(dev), y32.to(dev))
    r0, p0 = HH.gem_bwd(xf[:, :, :n0], pt, y32[0], dy[0])
    r1, p1 = HH.gem_bwd(xf[:, :, n0:], pt, y32[1], dy[1])
    HH.check(dx.reshape(N, C, -1), _cat_parts([r0, r1], 2), "ops.part_pool_bwd dx")
    HH.check(dp, HH.Ref(p0.value + p1.value, p0.M + p1.M, p0.kind), "ops.part_pool_bwd dp")
    ya = ops.part_pool_fwd(x.to(dev), split)
    HH.check(ya, _stack_parts([HH.gap_fwd(xf[:, :, :n0]), HH.gap_fwd(xf[:, :, n0:])]), "ops.part_pool_fwd avg")
    dxa, none = ops.part_pool_bwd(tuple(x.shape), split, dy.to(dev))
    assert none is None
    HH.check(dxa.reshape(N, C, -1), _cat_parts([HH.gap_bwd(dy[0], (N, C, n0)), HH.gap_bwd(dy[1], (N, C, Hh * W - n0))], 2),
             "ops.part_pool_bwd avg")


# ---- the fused head --------------------------------------------------------------------------------------------------------------
HEAD_PARAMS = list(enumerate(H.head_cases()))


def _head_forward(dev, lib, args, B, D, train, fusion):
    """one rg_mp_head_fwd between guards -> the outputs (dict of _Out) and the workspace"""
    xs, gammas, betas, rms, rvs, epss, moms = args
    dv = _to(dev, *(xs + gammas + betas))
    o = {"out": _Out((4, B, D), dev), "xhat": _Out((3, B, D), dev), "mean": _Out((3, D), dev), "invstd": _Out((3, D), dev),
         "norms": _Out((4, B), dev), "running_mean": _Out((3, D), dev, init=torch.stack(rms)),
         "running_var": _Out((3, D), dev, init=torch.stack(rvs))}
    nbytes = lib.rg_mp_head_workspace(B, D)
    assert nbytes == H.head_workspace(B, D)
    ws = _Out((nbytes // 4,), dev)
    rm, rv = o["running_mean"].t, o["running_var"].t
    lib.rg_mp_head_fwd(*[t.data_ptr() for t in dv], *[rm[j].data_ptr() for j in range(3)], *[rv[j].data_ptr() for j in range(3)],
                       o["out"].ptr, o["xhat"].ptr, o["mean"].ptr, o["invstd"].ptr, o["norms"].ptr, B, D, train, fusion, *epss, *moms,
                       ws.ptr if train else None, nbytes if train else 0, _st())
    return o, ws, dv


@pytest.mark.parametrize("i,case", HEAD_PARAMS, ids=lambda v: str(v) if isinstance(v, int) else "B%d_D%d_%s_%s_f%d_%s_%s" % (
    v[0], v[1], v[2], "train" if v[3] else "eval", v[4], v[5], "z%s" % v[6]))
def test_mp_head(dev, i, case):
    lib = _lib()
    B, D, fam, train, fusion, pat, zero = case
    args = H.head_input(B, D, fam, zero_branch=zero)
    tag = "B %d D %d %s fusion %d zero %s" % (B, D, "train" if train else "eval", fusion, zero)
    ref = H.head_fwd(*args, train, fusion)
    o, ws, dv = _head_forward(dev, lib, args, B, D, train, fusion)
    for k, r in ref.items():
        _check(o[k], r, "rg_mp_head_fwd %s | %s" % (k, tag), fam, H.C_KIND)
    if train:
        ws.guards("rg_mp_head_fwd workspace")
    else:
        ws.untouched("rg_mp_head_fwd workspace in eval mode")
    o2, _, _ = _head_forward(dev, lib, args, B, D, train, fusion)
    for k in o:
        assert torch.equal(o[k].buf, o2[k].buf), "rg_mp_head_fwd %s: two runs differ | %s" % (k, tag)
    # backward, handed the rounded reference forward
    xhat, invstd, norms = ref["xhat"].value.float(), ref["invstd"].value.float(), ref["norms"].value.float()
    dys = H.head_dys(B, D, pat)
    rb = H.head_bwd(dys, xhat, invstd, norms, args[1], args[2], train, fusion)
    sv = _to(dev, xhat, invstd, norms)
    dyd = _to(dev, *dys)
    runs = []
    for want_beta in (False, True, False):
        dx, dg, db = _Out((3, B, D), dev), _Out((3, D), dev), _Out((3, D), dev)
        reach = [rb["dx"][j] is not None for j in range(3)]
        rows = lambda t, on=True: [t.t[j].data_ptr() if (reach[j] and on) else None for j in range(3)]      # noqa: E731
        lib.rg_mp_head_bwd(*[_ptr(d) for d in dyd], None, None, None, *[t.data_ptr() for t in sv], *[t.data_ptr() for t in dv[3:9]],
                           *rows(dx), *rows(dg), *rows(db, want_beta), B, D, train, fusion, _st())
        for name, outp, on in (("dx", dx, True), ("dgamma", dg, True), ("dbeta", db, want_beta)):
            outp.guards("rg_mp_head_bwd " + name)
            for j in range(3):
                if reach[j] and on:
                    w = HH.compare(outp.t[j], rb[name][j], H.C_KIND)
                    assert w.ok, "rg_mp_head_bwd %s[%d] | %s %s: worst element %s err %.3e > budget %.3e (ratio %.2f)" % (
                        name, j, tag, pat, w.index, w.err, w.budget, w.ratio)
                    print("RATIO rg_mp_head_bwd %s %s %.3f" % (name, fam, w.ratio))
                else:
                    assert bool((outp.t[j] == HH.FILL).all()), "rg_mp_head_bwd %s[%d] written without a gradient | %s" % (name, j, tag)
        runs.append((dx.buf, dg.buf))
    assert torch.equal(runs[0][0], runs[2][0]) and torch.equal(runs[0][1], runs[2][1]), "rg_mp_head_bwd: two runs differ | " + tag


def test_mp_head_adds_a_gradient_given_for_the_batchnorm_outputs(dev):
    """dz_j (the 'cat' fusion's path) enters like an upstream gradient of z_j: by linearity the result equals the BatchNorm backward
    of dz alone plus nothing else when every dy is NULL — checked against the fp64 model of that backward"""
    lib = _lib()
    B, D = 16, 100
    args = H.head_input(B, D, "plain")
    ref = H.head_fwd(*args, 1, 0)
    xhat, invstd, norms = ref["xhat"].value.float(), ref["invstd"].value.float(), ref["norms"].value.float()
    dz = [torch.randn(B, D, generator=HH.gen(5 + j)).float() for j in range(3)]
    sv, dzd, par = _to(dev, xhat, invstd, norms), _to(dev, *dz), _to(dev, *(args[1] + args[2]))
    dx, dg = _Out((3, B, D), dev), _Out((3, D), dev)
    lib.rg_mp_head_bwd(None, None, None, None, *[t.data_ptr() for t in dzd], *[t.data_ptr() for t in sv], *[t.data_ptr() for t in par],
                       *[dx.t[j].data_ptr() for j in range(3)], *[dg.t[j].data_ptr() for j in range(3)], None, None, None, B, D, 1, 0,
                       _st())
    for j in range(3):
        g, xh = dz[j].double(), xhat[j].double()
        s1, s2 = g.sum(0), (g * xh).sum(0)
        k = args[1][j].double() * invstd[j].double()
        v = k * (g - s1 / B - xh * s2 / B)
        Es1, Es2 = g.abs().sum(0), (g * xh).abs().sum(0)
        M = k.abs() * (g.abs() + (Es1 + s1.abs()) / B + xh.abs() * (Es2 + 2.0 * s2.abs()) / B) + v.abs()
        w = HH.compare(dx.t[j], H.Ref(v, M, "dx"), H.C_KIND)
        assert w.ok, ("dx", j, w)
        w = HH.compare(dg.t[j], H.Ref(s2, Es2, "dsum"), H.C_KIND)
        assert w.ok, ("dgamma", j, w)
    dx.guards("rg_mp_head_bwd dx"), dg.guards("rg_mp_head_bwd dgamma")


def test_mp_head_through_the_ops_wrappers(dev):
    from rg_hip import ops
    B, D = 3, 100
    args = H.head_input(B, D, "plain")
    xs, gammas, betas, rms, rvs, epss, moms = args
    ref = H.head_fwd(*args, 1, 1)
    dv = [_to(dev, *grp) for grp in (xs, gammas, betas, rms, rvs)]
    out, xhat, mean, invstd, norms = ops.mp_head_fwd(*dv, epss, moms, True, 1)
    for got, k in ((out, "out"), (xhat, "xhat"), (mean, "mean"), (invstd, "invstd"), (norms, "norms"), (torch.stack(dv[3]), "running_mean"),
                   (torch.stack(dv[4]), "running_var")):
        assert HH.compare(got, ref[k], H.C_KIND).ok, k
    dys = H.head_dys(B, D, "g")
    rb = H.head_bwd(dys, xhat.cpu(), invstd.cpu(), norms.cpu(), gammas, betas, 1, 1)
    dx, dgamma, dbeta, reached = ops.mp_head_bwd(_to(dev, *dys), xhat, invstd, norms, dv[1], dv[2], True, 1)
    assert reached == [True, False, False] and dbeta is None
    assert HH.compare(dx[0], rb["dx"][0], H.C_KIND).ok and HH.compare(dgamma[0], rb["dgamma"][0], H.C_KIND).ok
