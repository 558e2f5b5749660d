"""GPU: every entry point of csrc/norm_bn.hip, norm_instnorm.hip and norm_fold.hip, per element against the fp64 host model
(tests/norm_hostmodel.py) with its per-element error budgets, at geometries built from the dispatch arithmetic: every value of
bn_reg_units and every reachable (LANES, U) of InstanceNorm with a full and a ragged geometry, the scalar and the loop routes,
every pick_slices regime — with the optional arguments given and NULL, the input families plain / scales / offset / constant /
masked, every output between two rows of guard floats, and no element left out of any comparison.

The C ABI is called the way rg_hip.ops calls it (ops allocates its outputs itself, so it cannot put them between guards and
cannot pass `neither dx nor dres`); the module-level route through ops.bn_train_fused_ok has a case of its own.

Each check prints `RATIO <entry point> <output> <family> <max err / (2^-24 M)>` (pytest -s shows them).

Why a subtly wrong kernel fails here — (a) the last float4 / last unit of a ragged row dropped, (b) unbiased variance in invstd or
biased in running_var, (c) the ReLU mask taken at y >= 0:
  bn_train_fwd_reg<U>, bn_train_bwd_reg<U>   U = 1, 2, 4, 8, 16 each run ragged and full; outputs start at the fill value, so (a)
      leaves -7777 in y / dx / dres and moves mean, invstd and both sums; (b) is 1 / (2 N HW) >= 3e-5 relative on invstd against a
      budget of 8 * 2^-24 (running_var: momentum / (N HW) relative, same budget; the N HW = 16384 case is the smallest change);
      (c) every `masked` case plants 0.0 / -0.0 in y_act, the last four elements included, and dres is compared exactly.
  bn_train_*_fused (loops)   the float4 case (1, 16388), the scalar cases, and every register case again under RG_BN_REG=0.
  instnorm_*_reg<LANES, U>   all eight reachable pairs, ragged and full, N * C leaving a partly empty last workgroup; (b) is
      1 / (2 HW) relative; sum_dx is compared with the reference's own dx sum.  Loop kernels: HW = 8196, four scalar HW (one per
      lane count), and the child run.
  bn_stats / bn_apply_fwd / bn_bwd_reduce / bn_bwd_apply / bn_eval_bwd / act_bwd_sum   the five pick_slices regimes, float4 and
      scalar, with a ragged last slice and mid-row boundaries: (a) at a slice end changes the sums by one float4 of terms, far above
      8 * 2^-24 of sum |term| only when that unit is not small — the fill value in dx / dres / g catches it regardless; (b), (c) as above
      (the `masked` regime is the scalar five-slice case, `constant` and `offset` are float4 ones).
  channel_sum_small<VEC>   both forms at 1, 255 and 32768 values per channel; rows_sum_pair, bn_fold, scale_rows,
      bn_fold_wgrad   every size class of their loops (below, at and above 16 rows / 256 threads)."""
import os
import subprocess
import sys

import pytest
import torch

from tests import norm_hostmodel as H

pytestmark = pytest.mark.gpu

EPS, MOM = 1e-5, 0.1
GUARD = 64
ACTS = H.ACTS
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ops():
    from rg_hip import ops
    return ops


def _lib():
    from rg_hip.lib import lib
    return lib


class _Out(object):
    """an output tensor between two rows of 64 guard floats; unwritten elements keep the fill value.  init: start contents
    (in-place outputs)"""

    def __init__(self, shape, dev, init=None):
        n = 1
        for d in shape:
            n *= d
        self.n = n
        self.buf = torch.full((n + 2 * GUARD,), H.FILL, dtype=torch.float32, device=dev)
        self.t = self.buf[GUARD:GUARD + n].view(shape)
        if init is not None:
            self.t.copy_(init.reshape(shape))
        assert self.t.data_ptr() % 16 == 0

    @property
    def ptr(self):
        return self.t.data_ptr()

    def guards(self, what):
        b = self.buf.cpu()
        assert bool((b[:GUARD] == H.FILL).all()) and bool((b[GUARD + self.n:] == H.FILL).all()), "%s: guard floats written" % what

    def check(self, ref, what, family):
        self.guards(what)
        r = H.check(self.t, ref, what)
        print("RATIO %s %s %.3f" % (what.split(" | ")[0], family, r))


def _ptr(o):
    return None if o is None else (o.ptr if isinstance(o, _Out) else o.data_ptr())


def _to(dev, *ts):
    return [None if t is None else t.contiguous().to(dev) for t in ts]


def _variant_args(inp, variant, i, family):
    """-> (gamma, beta, residual, running_mean, running_var, act, slope, need_dx, need_dres)"""
    if variant == "null":
        return None, None, None, None, None, H.ACT_NONE, 0.0, True, False
    act, slope = H.case_act(i, family)
    need = {"full": (True, True), "dx_only": (True, False), "dres_only": (False, True), "neither": (False, False)}[variant]
    return (inp.gamma, inp.beta, inp.residual, inp.running_mean, inp.running_var, act, slope) + need


def _one_launch(dev, kind, N, C, HW, family, variant, i):
    """rg_bn_train_fwd_fused / _bwd_fused ('bn') or rg_instnorm_fwd / _bwd ('in') on one case"""
    ops, lib = _ops(), _lib()
    inp = H.make_inputs(kind, N, C, HW, family, seed=i)
    gamma, beta, res, rm, rv, act, slope, need_dx, need_dres = _variant_args(inp, variant, i, family)
    nstat = C if kind == "bn" else N * C
    tag = "%s %s %s act %d" % ((N, C, HW), family, variant, act)
    f = H.forward(kind, inp.x, gamma, beta, res, EPS, act, slope, rm, rv, MOM)
    x, dy, gd, bd, rd = _to(dev, inp.x, inp.dy, gamma, beta, res)
    y, mean, invstd = _Out((N, C, HW), dev), _Out((nstat,), dev), _Out((nstat,), dev)
    if kind == "bn":
        fwd = "rg_bn_train_fwd_fused"
        rmo = _Out((C,), dev, rm) if rm is not None else None
        rvo = _Out((C,), dev, rv) if rv is not None else None
        lib.rg_bn_train_fwd_fused(x.data_ptr(), _ptr(gd), _ptr(bd), _ptr(rd), y.ptr, mean.ptr, invstd.ptr, _ptr(rmo), _ptr(rvo),
                                  N, C, HW, EPS, MOM, act, slope, ops._stream())
        if rmo is not None:
            rmo.check(f["running_mean"], "%s running_mean | %s" % (fwd, tag), family)
            rvo.check(f["running_var"], "%s running_var | %s" % (fwd, tag), family)
    else:
        fwd = "rg_instnorm_fwd"
        lib.rg_instnorm_fwd(x.data_ptr(), _ptr(gd), _ptr(bd), _ptr(rd), y.ptr, mean.ptr, invstd.ptr, N, C, HW, EPS, act, slope,
                            ops._stream())
    y.check(f["y"], "%s y | %s" % (fwd, tag), family)
    mean.check(f["mean"], "%s mean | %s" % (fwd, tag), family)
    invstd.check(f["invstd"], "%s invstd | %s" % (fwd, tag), family)

    # backward: handed the rounded reference statistics and forward output, not the kernel's own
    y_act = f["y"].value.float()
    if family == "masked":
        y_act = H.masked_y_act(y_act)
    mean32, invstd32 = f["mean"].value.float(), f["invstd"].value.float()
    b = H.backward(kind, inp.x, inp.dy, y_act if act != H.ACT_NONE else None, mean32, invstd32, gamma, act, slope)
    ya, md, isd = _to(dev, y_act if act != H.ACT_NONE else None, mean32, invstd32)
    dx = _Out((N, C, HW), dev) if need_dx else None
    dres = _Out((N, C, HW), dev) if need_dres else None
    s1, s2 = _Out((nstat,), dev), _Out((nstat,), dev)
    if kind == "bn":
        bwd = "rg_bn_train_bwd_fused"
        lib.rg_bn_train_bwd_fused(x.data_ptr(), dy.data_ptr(), _ptr(ya), md.data_ptr(), isd.data_ptr(), _ptr(gd), _ptr(dx),
                                  _ptr(dres), s1.ptr, s2.ptr, N, C, HW, act, slope, ops._stream())
    else:
        bwd = "rg_instnorm_bwd"
        sdx = _Out((nstat,), dev) if need_dx else None
        lib.rg_instnorm_bwd(x.data_ptr(), dy.data_ptr(), _ptr(ya), md.data_ptr(), isd.data_ptr(), _ptr(gd), _ptr(dx), _ptr(dres),
                            s1.ptr, s2.ptr, _ptr(sdx), N, C, HW, act, slope, ops._stream())
        if sdx is not None:
            sdx.check(b["sum_dx"], "%s sum_dx | %s" % (bwd, tag), family)
    s1.check(b["sum_g"], "%s sum_g | %s" % (bwd, tag), family)
    s2.check(b["sum_g_xhat"], "%s sum_g_xhat | %s" % (bwd, tag), family)
    if dx is not None:
        dx.check(b["dx"], "%s dx | %s" % (bwd, tag), family)
    if dres is not None:
        dres.check(b["dres"], "%s dres | %s" % (bwd, tag), family)


def _with_variants(cases, extra):
    """every case in the full and the all-NULL form; `extra` {case index: variant} adds the remaining forms"""
    out = []
    for i, c in enumerate(cases):
        out += [(i, c, "full"), (i, c, "null")]
        for v in extra.get(i, ()):
            out.append((i, c, v))
    return out


def _id(p):
    i, (N, C, HW, fam), v = p
    return "%dx%dx%d-%s-%s" % (N, C, HW, fam, v)


BN_PARAMS = _with_variants(H.bn_cases() + [H.BN_WIDE + ("plain",)],
                           {0: ("dres_only",), 2: ("dx_only", "neither"), 5: ("dres_only",), 6: ("neither",), 9: ("dx_only",),
                            10: ("dres_only", "neither"), 11: ("dx_only",), 12: ("dres_only",)})
IN_PARAMS = _with_variants(H.in_cases(),
                           {0: ("dres_only",), 3: ("dx_only", "neither"), 4: ("dres_only",), 9: ("dx_only",), 10: ("neither",),
                            12: ("dres_only",), 15: ("dx_only",), 16: ("dres_only", "neither"), 17: ("dx_only",), 20: ("dres_only",)})


@pytest.mark.parametrize("p", BN_PARAMS, ids=_id)
def test_bn_one_launch(dev, p):
    i, (N, C, HW, fam), variant = p
    _one_launch(dev, "bn", N, C, HW, fam, variant, i)


@pytest.mark.parametrize("p", IN_PARAMS, ids=_id)
def test_in_one_launch(dev, p):
    i, (N, C, HW, fam), variant = p
    _one_launch(dev, "in", N, C, HW, fam, variant, 100 + i)


def test_bn_one_launch_through_the_module_route(dev):
    """C = 130: the geometry rg_hip.ops.bn_train_fused_ok accepts, through the ops wrappers the modules call"""
    ops = _ops()
    N, C, HW = H.BN_WIDE
    assert H.bn_train_fused_ok(N, C, HW)
    inp = H.make_inputs("bn", N, C, HW, "offset", seed=9)
    act, slope = H.ACT_LEAKY, 0.2
    x, dy, gd, bd, rd, rmd, rvd = _to(dev, inp.x, inp.dy, inp.gamma, inp.beta, inp.residual, inp.running_mean, inp.running_var)
    assert ops.bn_train_fused_ok(x) and not ops.bn_train_fused_ok(x[:, :127].contiguous())
    f = H.forward("bn", inp.x, inp.gamma, inp.beta, inp.residual, EPS, act, slope, inp.running_mean, inp.running_var, MOM)
    y, mean, invstd = ops.bn_train_fwd_fused(x, gd, bd, rd, rmd, rvd, EPS, MOM, act, slope)
    for k, t in (("y", y), ("mean", mean), ("invstd", invstd), ("running_mean", rmd), ("running_var", rvd)):
        H.check(t, f[k], "ops.bn_train_fwd_fused %s" % k)
    y_act = f["y"].value.float()
    mean32, invstd32 = f["mean"].value.float(), f["invstd"].value.float()
    b = H.backward("bn", inp.x, inp.dy, y_act, mean32, invstd32, inp.gamma, act, slope)
    dx, dres, s1, s2 = ops.bn_train_bwd_fused(x, dy, y_act.to(dev), mean32.to(dev), invstd32.to(dev), gd, act, slope, need_dx=True,
                                              need_dres=True)
    for k, t in (("dx", dx), ("dres", dres), ("sum_g", s1), ("sum_g_xhat", s2)):
        H.check(t, b[k], "ops.bn_train_bwd_fused %s" % k)


# ---- two-stage and eval kernels on the pick_slices regimes ----------------------------------------------------------------------
def _ws(dev, N, C, HW):
    ops = _ops()
    ws = ops.workspace(ops._ws_query("rg_bn_workspace", N, C, HW), dev)
    return ws.data_ptr(), ws.numel()


SLICE_PARAMS = _with_variants(H.slice_cases(), {1: ("dx_only",), 3: ("dres_only",)})


@pytest.mark.parametrize("p", SLICE_PARAMS, ids=_id)
def test_bn_two_stage_train(dev, p):
    """rg_bn_stats, rg_bn_apply_fwd (stat = invstd), rg_bn_bwd_reduce, rg_bn_bwd_apply (train)"""
    ops, lib = _ops(), _lib()
    i, (N, C, HW, family), variant = p
    assert lib.rg_bn_slices(N, C, HW) == H.pick_slices(N, C, HW)[0]
    inp = H.make_inputs("bn", N, C, HW, family, seed=200 + i)
    gamma, beta, res, rm, rv, act, slope, need_dx, need_dres = _variant_args(inp, variant, i, family)
    tag = "%s %s %s act %d" % ((N, C, HW), family, variant, act)
    wsp, wsn = _ws(dev, N, C, HW)
    x, dy, gd, bd, rd = _to(dev, inp.x, inp.dy, gamma, beta, res)
    f = H.forward("bn", inp.x, gamma, beta, res, EPS, act, slope, rm, rv, MOM)
    mean, invstd = _Out((C,), dev), _Out((C,), dev)
    rmo = _Out((C,), dev, rm) if rm is not None else None
    rvo = _Out((C,), dev, rv) if rv is not None else None
    lib.rg_bn_stats(x.data_ptr(), mean.ptr, invstd.ptr, _ptr(rmo), _ptr(rvo), N, C, HW, EPS, MOM, wsp, wsn, ops._stream())
    mean.check(f["mean"], "rg_bn_stats mean | " + tag, family)
    invstd.check(f["invstd"], "rg_bn_stats invstd | " + tag, family)
    if rmo is not None:
        rmo.check(f["running_mean"], "rg_bn_stats running_mean | " + tag, family)
        rvo.check(f["running_var"], "rg_bn_stats running_var | " + tag, family)
    # apply: the statistics it is handed are the rounded reference ones
    mean32, invstd32 = f["mean"].value.float(), f["invstd"].value.float()
    fa = H.forward("bn", inp.x, gamma, beta, res, EPS, act, slope, frozen=(mean32, invstd32), stat_is_var=False)
    md, isd = _to(dev, mean32, invstd32)
    y = _Out((N, C, HW), dev)
    lib.rg_bn_apply_fwd(x.data_ptr(), md.data_ptr(), isd.data_ptr(), _ptr(gd), _ptr(bd), _ptr(rd), y.ptr, N, C, HW, 0, EPS, act,
                        slope, ops._stream())
    y.check(fa["y"], "rg_bn_apply_fwd y | " + tag, family)
    y_act = f["y"].value.float()
    if family == "masked":
        y_act = H.masked_y_act(y_act)
    y_act = y_act if act != H.ACT_NONE else None
    b = H.backward("bn", inp.x, inp.dy, y_act, mean32, invstd32, gamma, act, slope)
    ya, = _to(dev, y_act)
    s1, s2 = _Out((C,), dev), _Out((C,), dev)
    lib.rg_bn_bwd_reduce(x.data_ptr(), dy.data_ptr(), _ptr(ya), md.data_ptr(), isd.data_ptr(), s1.ptr, s2.ptr, N, C, HW, 0, EPS, act,
                         slope, wsp, wsn, ops._stream())
    s1.check(b["sum_g"], "rg_bn_bwd_reduce sum_g | " + tag, family)
    s2.check(b["sum_g_xhat"], "rg_bn_bwd_reduce sum_g_xhat | " + tag, family)
    if not (need_dx or need_dres):
        return
    dx = _Out((N, C, HW), dev) if need_dx else None
    dres = _Out((N, C, HW), dev) if need_dres else None
    s1d, s2d = _to(dev, b["sum_g"].value.float(), b["sum_g_xhat"].value.float())
    lib.rg_bn_bwd_apply(x.data_ptr(), dy.data_ptr(), _ptr(ya), md.data_ptr(), isd.data_ptr(), _ptr(gd), s1d.data_ptr(),
                        s2d.data_ptr(), _ptr(dx), _ptr(dres), N, C, HW, 1, 0, EPS, act, slope, ops._stream())
    if dx is not None:
        dx.check(b["dx"], "rg_bn_bwd_apply(train) dx | " + tag, family)
    if dres is not None:
        dres.check(b["dres"], "rg_bn_bwd_apply(train) dres | " + tag, family)


@pytest.mark.parametrize("p", SLICE_PARAMS + [(0, H.slice_cases()[0], "sums_only"), (3, H.slice_cases()[3], "sums_only"),
                                              (2, H.slice_cases()[2], "dx_no_x"), (4, H.slice_cases()[4], "dx_no_x")], ids=_id)
def test_bn_frozen_statistics(dev, p):
    """rg_bn_apply_fwd (stat = running variance), rg_bn_bwd_reduce / rg_bn_bwd_apply (eval), rg_bn_eval_bwd — also sums only and
    dx only without x"""
    ops, lib = _ops(), _lib()
    i, (N, C, HW, family), variant = p
    inp = H.make_inputs("bn", N, C, HW, family, seed=300 + i)
    base = {"sums_only": "neither", "dx_no_x": "dx_only"}.get(variant, variant)
    gamma, beta, res, _, _, act, slope, need_dx, need_dres = _variant_args(inp, base, i + 1, family)
    # running statistics near the batch's, so that every family keeps its condition
    xd = inp.x.double()
    rm = (xd.mean((0, 2)) * 1.01 + 0.01).float()
    rv = (xd.var((0, 2), unbiased=False) * 1.1 + 1e-6).float()
    tag = "%s %s %s act %d" % ((N, C, HW), family, variant, act)
    wsp, wsn = _ws(dev, N, C, HW)
    x, dy, gd, bd, rd, rmd, rvd = _to(dev, inp.x, inp.dy, gamma, beta, res, rm, rv)
    f = H.forward("bn", inp.x, gamma, beta, res, EPS, act, slope, frozen=(rm, rv))
    y = _Out((N, C, HW), dev)
    lib.rg_bn_apply_fwd(x.data_ptr(), rmd.data_ptr(), rvd.data_ptr(), _ptr(gd), _ptr(bd), _ptr(rd), y.ptr, N, C, HW, 1, EPS, act,
                        slope, ops._stream())
    y.check(f["y"], "rg_bn_apply_fwd(var) y | " + tag, family)
    y_act = f["y"].value.float()
    if family == "masked":
        y_act = H.masked_y_act(y_act)
    y_act = y_act if act != H.ACT_NONE else None
    ya, = _to(dev, y_act)
    # the kernels form invstd = rsqrt(var + eps) themselves: the reference keeps the exact one and the budget's relative term
    b = H.backward("bn", inp.x, inp.dy, y_act, rm, f["invstd"].value, gamma, act, slope, train=False)
    want_sums = variant != "dx_no_x"
    if variant not in ("sums_only", "dx_no_x"):
        s1, s2 = _Out((C,), dev), _Out((C,), dev)
        lib.rg_bn_bwd_reduce(x.data_ptr(), dy.data_ptr(), _ptr(ya), rmd.data_ptr(), rvd.data_ptr(), s1.ptr, s2.ptr, N, C, HW, 1,
                             EPS, act, slope, wsp, wsn, ops._stream())
        s1.check(b["sum_g"], "rg_bn_bwd_reduce(var) sum_g | " + tag, family)
        s2.check(b["sum_g_xhat"], "rg_bn_bwd_reduce(var) sum_g_xhat | " + tag, family)
        dx = _Out((N, C, HW), dev) if need_dx else None
        dres = _Out((N, C, HW), dev) if need_dres else None
        lib.rg_bn_bwd_apply(None, dy.data_ptr(), _ptr(ya), rmd.data_ptr(), rvd.data_ptr(), _ptr(gd), None, None, _ptr(dx),
                            _ptr(dres), N, C, HW, 0, 1, EPS, act, slope, ops._stream())
        if dx is not None:
            dx.check(b["dx"], "rg_bn_bwd_apply(eval) dx | " + tag, family)
        if dres is not None:
            dres.check(b["dres"], "rg_bn_bwd_apply(eval) dres | " + tag, family)
    dx = _Out((N, C, HW), dev) if need_dx else None
    dres = _Out((N, C, HW), dev) if need_dres else None
    s1 = _Out((C,), dev) if want_sums else None
    s2 = _Out((C,), dev) if want_sums else None
    lib.rg_bn_eval_bwd(x.data_ptr() if want_sums else None, dy.data_ptr(), _ptr(ya), rmd.data_ptr(), rvd.data_ptr(), _ptr(gd),
                       _ptr(dx), _ptr(dres), _ptr(s1), _ptr(s2), N, C, HW, EPS, act, slope, wsp, wsn, ops._stream())
    if want_sums:
        s1.check(b["sum_g"], "rg_bn_eval_bwd sum_g | " + tag, family)
        s2.check(b["sum_g_xhat"], "rg_bn_eval_bwd sum_g_xhat | " + tag, family)
    if dx is not None:
        dx.check(b["dx"], "rg_bn_eval_bwd dx | " + tag, family)
    if dres is not None:
        dres.check(b["dres"], "rg_bn_eval_bwd dres | " + tag, family)


# ---- the remaining entry points --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", H.CHANNEL_SUM_CASES, ids=lambda s: "%dx%dx%d" % s)
def test_channel_sum(dev, shape):
    """both vector forms; N * HW of 1, 255, 32768 (the one-launch limit) and a single float4"""
    ops, lib = _ops(), _lib()
    N, C, HW = shape
    assert H.channel_sum_ok(N, C, HW) and lib.rg_channel_sum_ok(N, C, HW) == 1
    for family in ("plain", "scales", "offset"):
        dy = H.make_inputs("bn", N, C, HW, family, seed=4).x
        out = _Out((C,), dev)
        dyd, = _to(dev, dy)                                          # held: a temporary's block may be handed out again
        lib.rg_channel_sum(dyd.data_ptr(), out.ptr, N, C, HW, ops._stream())
        out.check(H.channel_sum(dy), "rg_channel_sum out | %s %s" % (shape, family), family)


def test_rows_sum_pair(dev):
    ops, lib = _ops(), _lib()
    g = torch.Generator().manual_seed(12)
    for N in (1, 15, 16, 17, 33):
        for C in (1, 15, 16, 17):
            a = torch.randn(N, C, generator=g) * (10.0 ** torch.linspace(-3, 3, C))
            b = torch.randn(N, C, generator=g) + 30.0
            ad, bd = a.to(dev), b.to(dev)
            for mode in ("a", "b", "ab"):
                oa = _Out((C,), dev) if "a" in mode else None
                ob = _Out((C,), dev) if "b" in mode else None
                lib.rg_rows_sum_pair(ad.data_ptr() if oa else None, bd.data_ptr() if ob else None, _ptr(oa), _ptr(ob), N, C,
                                     ops._stream())
                tag = "N %d C %d %s" % (N, C, mode)
                if oa:
                    oa.check(H.rows_sum(a), "rg_rows_sum_pair out_a | " + tag, "scales")
                if ob:
                    ob.check(H.rows_sum(b), "rg_rows_sum_pair out_b | " + tag, "offset")


@pytest.mark.parametrize("M", [1, 3, 4, 147, 4608])
def test_bn_fold_and_scale_rows(dev, M):
    ops, lib = _ops(), _lib()
    g = torch.Generator().manual_seed(M)
    ga, be = (torch.rand(M, generator=g) + 0.5) * (1 - 2 * (torch.arange(M) % 2).float()), torch.randn(M, generator=g)
    mu = torch.randn(M, generator=g) * 30
    var = (torch.rand(M, generator=g) + 0.01) * (10.0 ** torch.linspace(-6, 6, M))
    var[0] = 0.0                                                    # a constant channel: invstd = eps^-1/2
    mud, vard = _to(dev, mu, var)
    for gam, bet in ((ga, be), (None, None), (ga, None)):
        gd, bd = _to(dev, gam, bet)
        sc, sh, is_ = _Out((M,), dev), _Out((M,), dev), _Out((M,), dev)
        lib.rg_bn_fold(_ptr(gd), _ptr(bd), mud.data_ptr(), vard.data_ptr(), EPS, sc.ptr, sh.ptr, is_.ptr, M, ops._stream())
        ref = H.bn_fold(gam, bet, mu, var, EPS)
        tag = "C %d gamma %s beta %s" % (M, gam is not None, bet is not None)
        sc.check(ref["scale"], "rg_bn_fold scale | " + tag, "scales")
        sh.check(ref["shift"], "rg_bn_fold shift | " + tag, "scales")
        is_.check(ref["invstd"], "rg_bn_fold invstd | " + tag, "scales")
    for K in (1, 5):
        w = torch.randn(K, M, generator=g)
        s = torch.randn(K, generator=g) * (10.0 ** torch.linspace(-3, 3, K))
        out = _Out((K, M), dev)
        wd, sd = _to(dev, w, s)
        lib.rg_scale_rows(wd.data_ptr(), sd.data_ptr(), out.ptr, K, M, ops._stream())
        out.check(H.scale_rows(w, s), "rg_scale_rows out | K %d M %d" % (K, M), "scales")


@pytest.mark.parametrize("p", [(i, c, "full") for i, c in enumerate(H.slice_cases())], ids=_id)
def test_act_bwd_sum_and_partial(dev, p):
    ops, lib = _ops(), _lib()
    i, (N, C, HW, family), _ = p
    inp = H.make_inputs("bn", N, C, HW, family, seed=400 + i)
    S = lib.rg_bn_slices(N, C, HW)
    assert S == H.pick_slices(N, C, HW)[0]
    wsp, wsn = _ws(dev, N, C, HW)
    y_act = H.masked_y_act(inp.x) if family == "masked" else inp.x
    dy, ya = _to(dev, inp.dy, y_act)
    for act, slope in ACTS:
        ref = H.act_bwd(inp.dy, y_act, act, slope)
        yp = ya.data_ptr() if act != H.ACT_NONE else None
        for need_g in (True, False):
            tag = "%s %s act %d need_g %s" % ((N, C, HW), family, act, need_g)
            g = _Out((N, C, HW), dev) if need_g else None
            sg = _Out((C,), dev)
            lib.rg_act_bwd_sum(dy.data_ptr(), yp, _ptr(g), sg.ptr, N, C, HW, act, slope, wsp, wsn, ops._stream())
            sg.check(ref["sum_g"], "rg_act_bwd_sum sum_g | " + tag, family)
            if g is not None:
                g.check(ref["g"], "rg_act_bwd_sum g | " + tag, family)
            g = _Out((N, C, HW), dev) if need_g else None
            part = _Out((C, S), dev)
            lib.rg_act_bwd_partial(dy.data_ptr(), yp, _ptr(g), part.ptr, N, C, HW, act, slope, ops._stream())
            cols = _Out((C,), dev, part.t.double().sum(1).float())      # column sum of the partials in fp64, one rounding
            part.guards("rg_act_bwd_partial partials | " + tag)
            cols.check(ref["sum_g"], "rg_act_bwd_partial sum of partials | " + tag, family)
            if g is not None:
                g.check(ref["g"], "rg_act_bwd_partial g | " + tag, family)
    gq = _Out((N, C, HW), dev)
    lib.rg_act_bwd_sum(dy.data_ptr(), ya.data_ptr(), gq.ptr, None, N, C, HW, H.ACT_RELU, 0.0, None, 0, ops._stream())
    gq.check(H.act_bwd(inp.dy, y_act, H.ACT_RELU, 0.0)["g"], "rg_act_bwd_sum g without the sum | %s" % ((N, C, HW),), family)


@pytest.mark.parametrize("K", [1, 5])
@pytest.mark.parametrize("M", [9, 147, 576])
def test_bn_fold_wgrad(dev, K, M):
    ops, lib = _ops(), _lib()
    g = torch.Generator().manual_seed(K * 1000 + M)
    w, G = torch.randn(K, M, generator=g), torch.randn(K, M, generator=g)
    sc = torch.randn(K, generator=g) * (10.0 ** torch.linspace(-2, 2, K))
    is_, mu = torch.rand(K, generator=g) + 0.5, torch.randn(K, generator=g) * 30
    wd, scd, isd, mud = _to(dev, w, sc, is_, mu)
    for S in (0, 3, 300):                                            # 0: fed sum_g; else slice partials [K][S]
        for want_dgamma in (True, False):
            tag = "K %d M %d S %d dgamma %s" % (K, M, S, want_dgamma)
            if S:
                part = torch.randn(K, S, generator=g)
                sum_g, ref_beta = part.double().sum(1), H.rows_sum(part.t())
            else:
                part, sum_g = None, (torch.randn(K, generator=g) * 10)
            ref = H.bn_fold_wgrad(w, G, sc, is_, mu, sum_g)
            Gd = _Out((K, M), dev, G)
            dgam = _Out((K,), dev) if want_dgamma else None
            dbeta = _Out((K,), dev) if S else None
            pd, sgd = _to(dev, part, None if S else sum_g)
            lib.rg_bn_fold_wgrad(wd.data_ptr(), Gd.ptr, scd.data_ptr(), isd.data_ptr(), mud.data_ptr(), _ptr(sgd), _ptr(pd), S,
                                 _ptr(dbeta), _ptr(dgam), K, M, ops._stream())
            Gd.check(ref["dW"], "rg_bn_fold_wgrad dW | " + tag, "scales")
            if dgam is not None:
                dgam.check(ref["dgamma"], "rg_bn_fold_wgrad dgamma | " + tag, "offset")
            if dbeta is not None:
                dbeta.check(ref_beta, "rg_bn_fold_wgrad dbeta | " + tag, "plain")


# ---- the one-launch cases again on the loop kernels -----------------------------------------------------------------------------
def test_register_cases_on_the_loop_kernels(dev):
    """RG_BN_REG=0 (read once at library load) keeps the loop kernels at the register-eligible geometries: the one-launch
    BatchNorm and InstanceNorm cases above, in one fresh interpreter"""
    if os.environ.get("RG_BN_REG") == "0":
        return                                                       # this IS the child (or the whole run is on the loop kernels)
    env = dict(os.environ)
    env["RG_BN_REG"] = "0"
    cmd = [sys.executable, "-m", "pytest", "-q", "-x", "-p", "no:cacheprovider", os.path.abspath(__file__), "-k", "one_launch"]
    res = subprocess.run(cmd, cwd=REPO, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True,
                         timeout=600)
    assert res.returncode == 0, "child exited %d:\n%s" % (res.returncode, res.stdout[-4000:])
