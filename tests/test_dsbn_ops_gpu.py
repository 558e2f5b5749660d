"""GPU: rg_dsbn_fwd / rg_dsbn_bwd per element against the fp64 host model (tests/dsbn_hostmodel.py: norm_hostmodel's closed forms
on each half, its budgets C_KIND * 2^-24 * M unchanged), called through the C ABI as tests/test_norm_elementwise_gpu.py does:
every output sits between two rows of guard floats and starts at the fill value, no element is left out of any comparison, dres
and the masked gradients are compared exactly, and each check prints `RATIO <entry point> <output> <family> <max err / (2^-24 M)>`
(collected in profiles/dsbn_elementwise_ratios.txt).

Cases come from the dispatch mirror (dsbn_hostmodel.one_launch_cases / slice_cases, which assert the route of every case):
  one launch     every register unit count U = 1, 2, 4, 8, 16 ragged and full, the loop route on scalar rows (odd HW), h = 1, HW = 1 with
                 h = 3 (the 1d layer), C = 3 .. 130 — the layer has no channel threshold, so C far below the 128 channels
                 rg_bn_train_fused_ok asks of a BatchNorm take this route too — most of them no multiple of 64; the loop route on
                 float4 rows is reachable only with RG_BN_REG=0 (per-domain extents above 16 units per thread leave the one-launch
                 regime), so the one-launch cases run once more in a child interpreter with that switch
  slice regime   per-domain extents just above the one-launch limit and beyond: S = 4 (set by the channel count), 5 and 6 slices per
                 domain on float4 and scalar rows, h = 1, 2, 3, 5; in every case the per-domain extent is no multiple of the slice
                 length, so slices laid over the whole batch would straddle sample h
  arguments      full (residual, running statistics, activation), all optional arguments NULL, dx only, dres only, neither;
                 the three activations in turn, the `masked` family with planted 0.0 / -0.0 / denormals in y_act

Input family `two domains` (dsbn_hostmodel.two_domains): source half x ~ N(0.3, 1.7) (norm_hostmodel's families), target half
3 x + 4 of its own draw; |gamma_t| in 2..3 with the sign opposite to gamma_s (|gamma_s| in 0.5..1.5), beta_t ~ N(5, 1) against
N(0, 1), running_mean_t ~ 4 against ~0, running_var_t in 8.5..9.5 against 0.5..1.5.  Why a wrong kernel is orders of magnitude
above the budget, on paper (plain family; n = h HW values per virtual channel, at most 20500 in these cases):
  one sample counted in the wrong domain   HW of the n source values come from the target half: the source mean moves by about
      (4.9 - 0.3) / h >= 4.6 / 16 = 0.29 (h <= 16 here) against a budget of 11.44 * 2^-24 * mean|x| ~ 1e-6;
  N HW for h HW   in dx the two correction terms are halved, an error of |gamma| invstd (|mean g| + |xhat| |mean g xhat|) / 2, of
      the order of dx itself, against 9.84 * 2^-24 of its terms: this is what catches the mistake with orders of magnitude to spare.
      In the unbiased variance var n / (n - 1) becomes var 2n / (2n - 1), a relative change of running_var of
      momentum * (var / new running_var) / (2n) >= 0.5 * (2.9 / 2.2) / 41000 = 1.6e-5 (momentum 0.5 / 0.6 here; source half:
      var = 1.7^2, the updated running_var at most 0.5 * 1.5 + 1.45) against 8 * 2^-24 = 4.8e-7: a factor 33 at the largest extent
      n = 20500 and 20500 / n times more below it (more than 100 below n = 6700) — a thinner margin than the others, and none in the
      constant channel of the `constant` family, whose variance is 0;
  swapped parameter sets   y moves by |gamma_s - gamma_t| |xhat| + |beta_s - beta_t| >= 2.5 |xhat| + ~5 against 9.2 * 2^-24 * O(10);
      dx by the factor gamma_t / gamma_s <= -4/3;
  the wrong domain's running statistics updated   running_mean_s would receive momentum * 4.9 where momentum * 0.3 belongs, and
      running_mean_t (~4) would stay an untouched 4 instead of moving towards 4.9: both O(0.5) against 8 * 2^-24 * O(1).
Two runs of every `full` case are compared bit for bit, and the workspace handed over is exactly rg_dsbn_workspace bytes between
guard floats."""
import os
import subprocess
import sys

import pytest
import torch

from tests import dsbn_hostmodel as D
from tests import norm_hostmodel as H
from tests.test_norm_elementwise_gpu import _Out, _lib, _ops, _ptr, _to

pytestmark = pytest.mark.gpu

EPS, MOM = (1e-5, 2e-5), (0.5, 0.6)
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VARIANTS = {"full": (True, True), "null": (True, False), "dx_only": (True, False), "dres_only": (False, True), "neither": (False, False)}


def _workspace(dev, N, C, HW):
    nbytes = _lib().rg_dsbn_workspace(N, C, HW)
    assert nbytes == D.workspace_bytes(N, C, HW)
    return _Out((nbytes // 4,), dev), nbytes


def _launch(dev, inp, N, C, HW, variant, act, slope, tag, family, check=True):
    """one forward and one backward through the C ABI -> every output tensor (for the bit-for-bit repeat)"""
    ops, lib = _ops(), _lib()
    null = variant == "null"
    need_dx, need_dres = VARIANTS[variant]
    s, t = (D.NOSET, D.NOSET) if null else (inp.s, inp.t)
    res = None if null else inp.residual
    f = D.forward(inp.x, s, t, res, EPS, act, slope, MOM)
    x, dy, rd = _to(dev, inp.x, inp.dy, res)
    gs, bs, gt, bt = _to(dev, s.gamma, s.beta, t.gamma, t.beta)
    y, mean, invstd = _Out((N, C, HW), dev), _Out((2 * C,), dev), _Out((2 * C,), dev)
    run = {k: (None if null else _Out((C,), dev, v)) for k, v in (("running_mean_s", s.running_mean), ("running_var_s", s.running_var),
                                                                ("running_mean_t", t.running_mean), ("running_var_t", t.running_var))}
    ws, nbytes = _workspace(dev, N, C, HW)
    lib.rg_dsbn_fwd(x.data_ptr(), _ptr(gs), _ptr(bs), _ptr(gt), _ptr(bt), _ptr(rd), y.ptr, mean.ptr, invstd.ptr,
                    _ptr(run["running_mean_s"]), _ptr(run["running_var_s"]), _ptr(run["running_mean_t"]), _ptr(run["running_var_t"]),
                    N, C, HW, EPS[0], EPS[1], MOM[0], MOM[1], act, slope, ws.ptr, nbytes, ops._stream())
    outs = [y, mean, invstd] + [o for o in run.values() if o is not None]
    if check:
        ws.guards("rg_dsbn_fwd workspace | " + tag)
        y.check(f["y"], "rg_dsbn_fwd y | " + tag, family)
        mean.check(f["mean"], "rg_dsbn_fwd mean | " + tag, family)
        invstd.check(f["invstd"], "rg_dsbn_fwd invstd | " + tag, family)
        for k, o in run.items():
            if o is not None:
                o.check(f[k], "rg_dsbn_fwd %s | %s" % (k, tag), family)

    # backward: handed the rounded reference statistics and forward output, not the kernel's own
    y_act = f["y"].value.float()
    if family == "masked":
        y_act = H.masked_y_act(y_act)
    y_act = y_act if act != H.ACT_NONE else None
    mean32, invstd32 = f["mean"].value.float(), f["invstd"].value.float()
    b = D.backward(inp.x, inp.dy, y_act, mean32, invstd32, s.gamma, t.gamma, act, slope)
    ya, md, isd = _to(dev, y_act, mean32, invstd32)
    dx = _Out((N, C, HW), dev) if need_dx else None
    dres = _Out((N, C, HW), dev) if need_dres else None
    grads = {k: _Out((C,), dev) for k in ("d_gamma_s", "d_beta_s", "d_gamma_t", "d_beta_t")}
    ws2, nbytes = _workspace(dev, N, C, HW)
    lib.rg_dsbn_bwd(x.data_ptr(), dy.data_ptr(), _ptr(ya), md.data_ptr(), isd.data_ptr(), _ptr(gs), _ptr(gt), _ptr(dx), _ptr(dres),
                    grads["d_gamma_s"].ptr, grads["d_beta_s"].ptr, grads["d_gamma_t"].ptr, grads["d_beta_t"].ptr, N, C, HW, act, slope,
                    ws2.ptr, nbytes, ops._stream())
    if check:
        ws2.guards("rg_dsbn_bwd workspace | " + tag)
        for k, o in grads.items():
            o.check(b[k], "rg_dsbn_bwd %s | %s" % (k, tag), family)
        if dx is not None:
            dx.check(b["dx"], "rg_dsbn_bwd dx | " + tag, family)
        if dres is not None:
            dres.check(b["dres"], "rg_dsbn_bwd dres | " + tag, family)
    return outs + list(grads.values()) + [o for o in (dx, dres) if o is not None]


def _case(dev, p, seed0):
    i, (N, C, HW, family), variant = p
    inp = D.two_domains(N, C, HW, family, seed=seed0 + i)
    act, slope = (H.ACT_NONE, 0.0) if variant == "null" else H.case_act(i, family)
    tag = "%s %s %s %s act %d" % ((N, C, HW), D.dsbn_regime(N, C, HW), family, variant, act)
    first = _launch(dev, inp, N, C, HW, variant, act, slope, tag, family)
    if variant == "full":                                            # no float atomics: a second run gives the same bits
        again = _launch(dev, inp, N, C, HW, variant, act, slope, tag, family, check=False)
        for a, b in zip(first, again):
            assert torch.equal(a.buf, b.buf), "two runs differ | " + tag


def _with_variants(cases, extra):
    out = []
    for i, c in enumerate(cases):
        out += [(i, c, "full"), (i, c, "null")]
        for v in extra.get(i, ()):
            out.append((i, c, v))
    return out


def _id(p):
    i, (N, C, HW, fam), v = p
    return "%dx%dx%d-%s-%s" % (N, C, HW, fam, v)


ONE_PARAMS = _with_variants(D.one_launch_cases(), {0: ("dres_only",), 2: ("dx_only", "neither"), 5: ("dres_only",), 8: ("dx_only",),
                                                  10: ("dres_only", "neither"), 12: ("dx_only",), 13: ("dres_only",)})
SLICE_PARAMS = _with_variants(D.slice_cases(), {0: ("dx_only",), 1: ("dres_only",), 2: ("dres_only", "neither"), 4: ("dx_only",)})


@pytest.mark.parametrize("p", ONE_PARAMS, ids=_id)
def test_dsbn_one_launch(dev, p):
    N, C, HW = p[1][:3]
    assert _lib().rg_dsbn_one_launch(N, C, HW) == 1
    # the kernel form this run really takes: the library's own answer, which knows RG_BN_REG (the mirror does not)
    want = 0 if os.environ.get("RG_BN_REG") == "0" else H.bn_reg_units(N // 2, C, HW)
    assert _lib().rg_bn_reg_units(N // 2, C, HW) == want, "register units %d, expected %d" % (_lib().rg_bn_reg_units(N // 2, C, HW), want)
    _case(dev, p, 300)


@pytest.mark.parametrize("p", SLICE_PARAMS, ids=_id)
def test_dsbn_slice_regime(dev, p):
    N, C, HW = p[1][:3]
    assert _lib().rg_dsbn_one_launch(N, C, HW) == 0 and _lib().rg_dsbn_slices(N, C, HW) == D.dsbn_slices(N, C, HW)[0]
    _case(dev, p, 400)


def test_dsbn_odd_batch_launches_nothing(dev):
    ops, lib = _ops(), _lib()
    N, C, HW = 5, 64, 16
    x = torch.randn(N, C, HW, device=dev)
    y, mean, invstd = _Out((N, C, HW), dev), _Out((2 * C,), dev), _Out((2 * C,), dev)
    ws = _Out((64,), dev)
    with pytest.raises(RuntimeError, match="halves"):
        lib.rg_dsbn_fwd(x.data_ptr(), None, None, None, None, None, y.ptr, mean.ptr, invstd.ptr, None, None, None, None, N, C, HW,
                        1e-5, 1e-5, 0.1, 0.1, 0, 0.0, ws.ptr, 256, ops._stream())
    g = [_Out((C,), dev) for _ in range(4)]
    dx = _Out((N, C, HW), dev)
    with pytest.raises(RuntimeError, match="halves"):
        lib.rg_dsbn_bwd(x.data_ptr(), x.data_ptr(), None, mean.ptr, invstd.ptr, None, None, dx.ptr, None, g[0].ptr, g[1].ptr, g[2].ptr,
                        g[3].ptr, N, C, HW, 0, 0.0, ws.ptr, 256, ops._stream())
    torch.cuda.synchronize()
    for o in [y, mean, invstd, ws, dx] + g:
        assert bool((o.buf == H.FILL).all()), "an odd batch wrote something"


@pytest.mark.parametrize("shape", [(6, 66, 344), (10, 3, 4100)], ids=["one_launch", "slices"])
def test_dsbn_through_the_ops_wrappers(dev, shape):
    """ops.dsbn_fwd / ops.dsbn_bwd, the route the modules take (they allocate their own outputs)"""
    ops = _ops()
    N, C, HW = shape
    inp = D.two_domains(N, C, HW, "plain", seed=9)
    act, slope = H.ACT_RELU, 0.0
    f = D.forward(inp.x, inp.s, inp.t, inp.residual, EPS, act, slope, MOM)
    x, dy, rd = _to(dev, inp.x, inp.dy, inp.residual)
    s, t = D.Set(*_to(dev, *inp.s)), D.Set(*_to(dev, *inp.t))
    y, stats = ops.dsbn_fwd(x, s.gamma, s.beta, t.gamma, t.beta, (s.running_mean, s.running_var), (t.running_mean, t.running_var),
                            EPS, MOM, residual=rd, act=act, slope=slope)
    for k, got in (("y", y), ("mean", stats[0]), ("invstd", stats[1]), ("running_mean_s", s.running_mean),
                   ("running_var_s", s.running_var), ("running_mean_t", t.running_mean), ("running_var_t", t.running_var)):
        H.check(got, f[k], "ops.dsbn_fwd %s %s" % (k, shape))
    y_act = f["y"].value.float()
    st32 = torch.stack((f["mean"].value.float().reshape(2, C), f["invstd"].value.float().reshape(2, C)))
    b = D.backward(inp.x, inp.dy, y_act, st32[0], st32[1], inp.s.gamma, inp.t.gamma, act, slope)
    res = ops.dsbn_bwd(x, dy, y_act.to(dev), st32.to(dev), s.gamma, t.gamma, act, slope, need_dx=True, need_dres=True)
    for k, got in zip(("dx", "dres", "d_gamma_s", "d_beta_s", "d_gamma_t", "d_beta_t"), res):
        H.check(got, b[k], "ops.dsbn_bwd %s %s" % (k, shape))


def test_one_launch_cases_on_the_loop_kernels(dev):
    """RG_BN_REG=0 (read once at library load) keeps the loop form of the one-launch kernels at the register-eligible geometries —
    the only way the float4 loop rows are reached by this layer: the one-launch cases above, in one fresh interpreter.  Each case
    asserts rg_bn_reg_units() == 0 there, so a switch that stopped working fails the child instead of re-testing the register
    kernels."""
    if os.environ.get("RG_BN_REG") == "0":
        return                                                       # this IS the child (or the whole run is on the loop kernels)
    env = dict(os.environ)
    env["RG_BN_REG"] = "0"
    cmd = [sys.executable, "-m", "pytest", "-q", "-x", "-p", "no:cacheprovider", os.path.abspath(__file__), "-k", "test_dsbn_one_launch"]
    res = subprocess.run(cmd, cwd=REPO, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True,
                         timeout=600)
    assert res.returncode == 0, "child exited %d:\n%s" % (res.returncode, res.stdout[-4000:])
