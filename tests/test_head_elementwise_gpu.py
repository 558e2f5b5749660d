"""GPU: every entry point of csrc/pool.hip, csrc/loss.hip, csrc/cm.hip and csrc/optim.hip, per element against the fp64 host
model (tests/head_hostmodel.py) with its per-element error budgets, at geometries built from the launch arithmetic: one, some
and the capped number of partial sums, every grid-stride loop on its second trip, both max-pool backward kernels at the same
geometry, the float4 / tail split of Adam at every n % 4, the register limit of the cluster memory on both sides, partly empty
last workgroups — with every optional pointer given and NULL, every output between two rows of guard values, and no element
left out of any comparison.

The C ABI is called the way rg_hip.ops calls it (ops allocates its outputs itself, so it cannot put them between guards); one
case per unit goes through the ops wrappers.  Each backward is handed the rounded reference forward outputs (lse, argmax,
GeM y, out2), not the kernel's own.

Each check prints `RATIO <entry point> <output> <family> <max err / (2^-24 M)>` (pytest -s shows them).

_Out is a copy of the one in tests/test_norm_elementwise_gpu.py with a dtype, a fill value and an offset inside the guard buffer
(uint8 argmax, the float64 Adam clock, the misaligned dx / p cases)."""
import pytest
import torch

from tests import head_hostmodel as H
from tests import test_head_hostmodel_cpu as T

pytestmark = pytest.mark.gpu

GUARD = 64


def _ops():
    from rg_hip import ops
    return ops


def _lib():
    from rg_hip.lib import lib
    return lib


def _st():
    return _ops()._stream()


class _Out(object):
    """an output tensor between two rows of 64 guard elements; unwritten elements keep the fill value.  init: start contents
    (in-place outputs); shift: elements by which the tensor is moved inside the buffer (misalignment)"""

    def __init__(self, shape, dev, init=None, dtype=torch.float32, fill=H.FILL, shift=0):
        n = 1
        for d in shape:
            n *= d
        self.n, self.fill, self.start = n, fill, GUARD + shift
        self.buf = torch.full((n + 2 * GUARD + 4,), fill, dtype=dtype, device=dev)
        self.t = self.buf[self.start:self.start + n].view(shape)
        if init is not None:
            self.t.copy_(init.reshape(shape))
        assert self.buf.data_ptr() % 16 == 0

    @property
    def ptr(self):
        return self.t.data_ptr()

    def guards(self, what):
        b = self.buf.cpu()
        assert bool((b[:self.start] == self.fill).all()) and bool((b[self.start + self.n:] == self.fill).all()), \
            "%s: guard elements written" % what

    def untouched(self, what):
        self.guards(what)
        assert bool((self.t == self.fill).all()), "%s: output written" % what

    def check(self, ref, what, family):
        self.guards(what)
        r = H.check(self.t, ref, what)
        print("RATIO %s %s %.3f" % (what.split(" | ")[0], family, r))


def _ptr(o):
    return None if o is None else (o.ptr if isinstance(o, _Out) else o.data_ptr())


def _to(dev, *ts):
    return [None if t is None else t.contiguous().to(dev) for t in ts]


def _ws(dev):
    """the loss workspace, exactly rg_loss_workspace() bytes, between guards"""
    nbytes = _lib().rg_loss_workspace()
    assert nbytes == H.MAX_PARTIALS * 4
    return _Out((nbytes // 4,), dev), nbytes


# ---- loss.hip ------------------------------------------------------------------------------------------------------------------
def _sum_fwd(dev, op, x, par, chain, tag, fam):
    lib = _lib()
    ws, nb = _ws(dev)
    xd, = _to(dev, x)
    out = _Out((1,), dev)
    if op == "bce":
        name = "rg_sigmoid_bce_fwd"
        lib.rg_sigmoid_bce_fwd(xd.data_ptr(), out.ptr, x.numel(), par, ws.ptr, nb, _st())
    elif op == "mse":
        name = "rg_mse_const_fwd"
        lib.rg_mse_const_fwd(xd.data_ptr(), out.ptr, x.numel(), par, ws.ptr, nb, _st())
    else:
        name = "rg_affine_relu_mean_fwd"
        lib.rg_affine_relu_mean_fwd(xd.data_ptr(), out.ptr, x.numel(), par[0], par[1], par[2], ws.ptr, nb, _st())
    ref = H.two_stage(op, x, par, chain)
    out.check(H.Ref(ref.value.reshape(1), ref.M.reshape(1), ref.kind), "%s loss | %s" % (name, tag), fam)
    ws.guards(name + " workspace | " + tag)


def _sum_bwd(dev, op, x, par, gout, gs, chain, tag, fam):
    lib = _lib()
    xd, gd = _to(dev, x, gout)
    dx = _Out(tuple(x.shape), dev)
    if op == "bce":
        name = "rg_sigmoid_bce_bwd"
        lib.rg_sigmoid_bce_bwd(xd.data_ptr(), _ptr(gd), dx.ptr, x.numel(), par, gs, _st())
    elif op == "mse":
        name = "rg_mse_const_bwd"
        lib.rg_mse_const_bwd(xd.data_ptr(), _ptr(gd), dx.ptr, x.numel(), par, gs, _st())
    else:
        name = "rg_affine_relu_mean_bwd"
        lib.rg_affine_relu_mean_bwd(xd.data_ptr(), _ptr(gd), dx.ptr, x.numel(), par[0], par[1], par[2], gs, _st())
    dx.check(H.sum_bwd(op, x, par, gout, gs, chain), "%s dx | %s" % (name, tag), fam)


@pytest.mark.parametrize("op", ["bce", "mse", "affine"])
def test_two_stage_sums(dev, op):
    """every n of SUM_N (1 partial, 2, 35, the cap of 1024 with an extra trip for some threads), the targets 1, 0 and 0.83 /
    the four (a, b, clamp), every family; BCE's saturated family and the planted hinge kinks"""
    for o, par, n, fam in H.sum_cases():
        if o == op:
            _sum_fwd(dev, op, H.sum_input(op, par, n, fam), par, False, "n %d par %s %s" % (n, par, fam), fam)
    if op == "bce":
        xs = torch.tensor(H.SATURATED * 3)
        for t in H.TARGETS:
            _sum_fwd(dev, op, xs, t, True, "saturated target %s" % t, "saturated")
    if op == "affine":
        for n in (5, 257):
            for par in H.AFFINE[:2]:
                _sum_fwd(dev, op, H.sum_input(op, par, n, "plain", planted=True), par, False, "n %d par %s planted" % (n, par),
                         "planted")


@pytest.mark.parametrize("op,par", [("bce", 0.83), ("bce", 1.0), ("bce", 0.0), ("mse", 0.83), ("affine", H.AFFINE[0]),
                                    ("affine", H.AFFINE[1]), ("affine", H.AFFINE[3])], ids=str)
def test_sum_backwards(dev, op, par):
    """n of 1, 257 and 4096 * 256 + 257 (second trip); grad_out given and NULL; grad_scale != 1"""
    for n in H.BWD_N:
        for fam in (H.FAMILIES if n < 1000 else H.FAMILIES[:2]):
            for gout, gs in ((None, 1.0), (torch.tensor([0.5]), 0.3)):
                x = H.sum_input(op, par, n, fam)
                _sum_bwd(dev, op, x, par, gout, gs, False, "n %d par %s %s gout %s" % (n, par, fam, gout is not None), fam)
    if op == "bce":
        _sum_bwd(dev, op, torch.tensor(H.SATURATED * 3), par, None, 1.0, True, "saturated target %s" % par, "saturated")
    if op == "affine" and par[2]:
        for n in (5, 257):
            _sum_bwd(dev, op, H.sum_input(op, par, n, "plain", planted=True), par, None, 1.0, False, "planted n %d" % n, "planted")


def test_loss_workspace_too_small(dev):
    lib = _lib()
    ws, nb = _ws(dev)
    x, = _to(dev, torch.randn(300))
    out = _Out((1,), dev)
    with pytest.raises(RuntimeError, match="workspace too small"):
        lib.rg_sigmoid_bce_fwd(x.data_ptr(), out.ptr, 300, 1.0, ws.ptr, nb - 1, _st())
    with pytest.raises(RuntimeError, match="workspace too small"):
        lib.rg_l1_fwd(x.data_ptr(), x.data_ptr(), None, out.ptr, 3, 100, None, nb, _st())
    out.untouched("loss after the workspace error")
    ws.untouched("workspace after the workspace error")


@pytest.mark.parametrize("i", range(len(T.L1_CASES)), ids=lambda i: "%dx%d" % T.L1_CASES[i])
def test_l1(dev, i):
    """labels NULL, mixed 0 / 1 / 2 (only 1 selects), nothing selected (NaN, inf); inner not dividing 256; da only, db only,
    both; planted a == b"""
    lib = _lib()
    rows, inner = T.L1_CASES[i]
    fam = H.FAMILIES[i % 4]
    a, b = T.l1_pair(rows, inner, fam, planted=i % 2 == 0)
    ad, bd = _to(dev, a, b)
    for k, mode in enumerate(("none", "mixed", "nothing")):
        lab = T.l1_labels(rows, mode)
        labd, = _to(dev, lab)
        tag = "%s %s %s" % ((rows, inner), fam, mode)
        ws, nb = _ws(dev)
        out2 = _Out((2,), dev)
        lib.rg_l1_fwd(ad.data_ptr(), bd.data_ptr(), _ptr(labd), out2.ptr, rows, inner, ws.ptr, nb, _st())
        ref = H.l1_fwd(a, b, lab)
        out2.check(ref, "rg_l1_fwd out2 | " + tag, fam)
        ws.guards("rg_l1_fwd workspace")
        if mode == "nothing":
            continue
        o2 = ref.value.float()
        o2d, = _to(dev, o2)
        for gout, gs, need in ((None, 1.0, "ab"), (torch.tensor([10.0]), 0.25, "ab"[(i + k) % 2])):
            gd, = _to(dev, gout)
            da = _Out((rows, inner), dev) if "a" in need else None
            db = _Out((rows, inner), dev) if "b" in need else None
            lib.rg_l1_bwd(ad.data_ptr(), bd.data_ptr(), _ptr(labd), _ptr(gd), o2d.data_ptr(), _ptr(da), _ptr(db), rows, inner, gs,
                          _st())
            ra, rb = H.l1_bwd(a, b, lab, gout, o2, gs)
            if da is not None:
                da.check(ra, "rg_l1_bwd da | %s %s" % (tag, need), fam)
            if db is not None:
                db.check(rb, "rg_l1_bwd db | %s %s" % (tag, need), fam)


def _rows_case(dev, rows, inner, fam, seed, gp=True):
    lib = _lib()
    a, b = T.l1_pair(rows, inner, fam, seed=seed)
    grow = torch.randn(rows, generator=H.gen(inner))
    ad, bd, gd = _to(dev, a, b, grow)
    tag = "%s %s" % ((rows, inner), fam)
    out = _Out((rows,), dev)
    lib.rg_l1_rows_fwd(ad.data_ptr(), bd.data_ptr(), out.ptr, rows, inner, _st())
    out.check(H.rows_fwd("l1_rows", a, b), "rg_l1_rows_fwd out | " + tag, fam)
    ra, rb = H.rows_bwd("l1_rows", a, b, grow)
    for need in ("ab", "a", "b"):
        da = _Out((rows, inner), dev) if "a" in need else None
        db = _Out((rows, inner), dev) if "b" in need else None
        lib.rg_l1_rows_bwd(ad.data_ptr(), bd.data_ptr(), gd.data_ptr(), _ptr(da), _ptr(db), rows, inner, _st())
        if da is not None:
            da.check(ra, "rg_l1_rows_bwd da | %s %s" % (tag, need), fam)
        if db is not None:
            db.check(rb, "rg_l1_rows_bwd db | %s %s" % (tag, need), fam)
    for c in (1.0, 0.0, 0.83):
        out = _Out((rows,), dev)
        lib.rg_mse_const_rows_fwd(ad.data_ptr(), c, out.ptr, rows, inner, _st())
        out.check(H.rows_fwd("mse_rows", a, c), "rg_mse_const_rows_fwd out | %s c %s" % (tag, c), fam)
        dx = _Out((rows, inner), dev)
        lib.rg_mse_const_rows_bwd(ad.data_ptr(), c, gd.data_ptr(), dx.ptr, rows, inner, _st())
        dx.check(H.rows_bwd("mse_rows", a, c, grow), "rg_mse_const_rows_bwd dx | %s c %s" % (tag, c), fam)
    if not gp:
        return
    for gfam in ("plain", "scales", "zero_row", "const0", "const1"):
        g = T.gp_input(rows, inner, gfam)
        gdv, = _to(dev, g)
        pen, v = _Out((rows,), dev), _Out((rows, inner), dev)
        lib.rg_grad_penalty_rows(gdv.data_ptr(), pen.ptr, v.ptr, rows, inner, 1.0, 10.0, _st())
        rp, rv = H.grad_penalty_rows(g, 1.0, 10.0)
        pen.check(rp, "rg_grad_penalty_rows pen | %s %s" % ((rows, inner), gfam), gfam)
        v.check(rv, "rg_grad_penalty_rows v | %s %s" % ((rows, inner), gfam), gfam)


@pytest.mark.parametrize("rows", H.ROWS)
def test_row_losses(dev, rows):
    """l1_rows, mse_const_rows, grad_penalty_rows: one workgroup per row; inner / D of 1, 255, 256, 257, 1027"""
    for i, inner in enumerate(H.ROWS_INNER):
        _rows_case(dev, rows, inner, H.FAMILIES[(i + rows) % 4], 1)


def test_row_loss_backwards_past_the_grid_cap(dev):
    rows, inner = T.ROWS_BWD_BIG
    assert H.trips("loss", rows * inner) == 2
    _rows_case(dev, rows, inner, "plain", 2, gp=False)


def _ce_case(dev, i, B, K, sc, fam, given):
    lib = _lib()
    z, lab = H.ce_input(B, K, fam, seed=i), H.ce_labels(B, K)
    grow = torch.rand(B, generator=H.gen(i)) + 0.5 if given else None
    zd, labd, gd = _to(dev, z, lab, grow)
    tag = "B %d K %d scale %s %s labels %s grad_rows %s" % (B, K, sc, fam, lab.tolist(), given)
    loss, lse = _Out((B,), dev), _Out((B,), dev)
    lib.rg_softmax_ce_fwd(zd.data_ptr(), labd.data_ptr(), loss.ptr, lse.ptr, B, K, sc, _st())
    f = H.softmax_ce_fwd(z, lab, sc)
    loss.check(f["loss"], "rg_softmax_ce_fwd loss | " + tag, fam)
    lse.check(f["lse"], "rg_softmax_ce_fwd lse | " + tag, fam)
    lse32 = f["lse"].value.float()
    ld, = _to(dev, lse32)
    dz = _Out((B, K), dev)
    lib.rg_softmax_ce_bwd(zd.data_ptr(), labd.data_ptr(), ld.data_ptr(), _ptr(gd), dz.ptr, B, K, sc, 0.7, _st())
    dz.check(H.softmax_ce_bwd(z, lab, lse32, grow, sc, 0.7), "rg_softmax_ce_bwd dlogits | " + tag, fam)


CE_PARAMS = list(enumerate(H.ce_cases()))


@pytest.mark.parametrize("p", CE_PARAMS, ids=lambda p: "B%d-K%d-s%g-%s-%s" % (p[1][:4] + (p[1][4],)))
def test_softmax_ce(dev, p):
    """K of 1, 63, 256, 257, 2049; scale 1 and 20; labels 0, K - 1 and the ignored -100, -1 and K, whose rows have loss 0 and
    gradient 0 (the kernel before this suite wrote grad * softmax into them)"""
    i, (B, K, sc, fam, given) = p
    _ce_case(dev, i, B, K, sc, fam, given)


def test_weighted_sum(dev):
    lib = _lib()
    for n in H.WSUM_N:
        for fam in H.FAMILIES:
            g = H.gen(n)
            x, w = H.family((n,), fam, g), torch.rand(n, generator=g)
            xd, wd, gd = _to(dev, x, w, torch.tensor([0.5]))
            for wt, wdv in ((w, wd), (None, None)):
                tag = "n %d %s w %s" % (n, fam, wt is not None)
                out = _Out((1,), dev)
                lib.rg_weighted_sum_fwd(xd.data_ptr(), _ptr(wdv), out.ptr, n, 0.125, _st())
                out.check(H.weighted_sum_fwd(x, wt, 0.125), "rg_weighted_sum_fwd out | " + tag, fam)
                for gout, gdv in ((torch.tensor(0.5), gd), (None, None)):
                    dx = _Out((n,), dev)
                    lib.rg_weighted_sum_bwd(_ptr(gdv), _ptr(wdv), dx.ptr, n, 0.125, _st())
                    dx.check(H.weighted_sum_bwd(gout, wt, n, 0.125), "rg_weighted_sum_bwd dx | %s gout %s" % (tag, gout is not None), fam)


# ---- pool.hip ------------------------------------------------------------------------------------------------------------------
ARG_FILL = 171


def _pool_case(dev, i, N, C, geo, fam):
    lib = _lib()
    Hh, W = geo[:2]
    win = geo[2:]
    P, Q = H.pool_out(*geo)
    x = H.pool_input(N, C, Hh, W, fam, seed=i)
    xd, = _to(dev, x)
    tag = "%s %s %s" % ((N, C), geo, fam)
    y = _Out((N, C, P, Q), dev)
    arg = _Out((N, C, P, Q), dev, dtype=torch.uint8, fill=ARG_FILL)
    lib.rg_maxpool2d_fwd(xd.data_ptr(), y.ptr, arg.ptr, N, C, Hh, W, *win, P, Q, _st())
    ry, ra = H.maxpool_fwd(x, *win)
    y.check(ry, "rg_maxpool2d_fwd y | " + tag, fam)
    arg.check(ra, "rg_maxpool2d_fwd argmax | " + tag, fam)
    yc = y.t.cpu()
    assert torch.equal(torch.signbit(yc), torch.signbit(ry.value.float())), "maxpool y: sign of zero | " + tag
    # backward, handed the reference argmax; the W % 4 == 0 geometries a second time with dx one float off 16 bytes
    dy = torch.randn(N, C, P, Q, generator=H.gen(i))
    dyd, ad = _to(dev, dy, ra.value.to(torch.uint8))
    rdx = H.maxpool_bwd(dy, ra.value, x.shape, *win)
    got = {}
    for shift in (0, 1):
        dx = _Out((N, C, Hh, W), dev, shift=shift)
        kern = H.maxpool_bwd_kernel(*win, W=W, dx_addr=dx.ptr)
        if shift and H.maxpool_bwd_kernel(*win, W=W, dx_addr=0) != "four":
            continue
        assert kern == ("gather" if shift else H.maxpool_bwd_kernel(*win, W=W, dx_addr=0))
        lib.rg_maxpool2d_bwd(dyd.data_ptr(), ad.data_ptr(), dx.ptr, N, C, Hh, W, *win, P, Q, _st())
        dx.check(rdx, "rg_maxpool2d_bwd dx (%s) | %s" % (kern, tag), fam)
        got[kern] = dx.t.cpu().clone()
    if len(got) == 2:
        a, b = got["four"].view(torch.int32), got["gather"].view(torch.int32)
        assert torch.equal(a, b), "maxpool backward: the two kernels differ in bits | " + tag


POOL_PARAMS = list(enumerate(H.pool_cases()))


@pytest.mark.parametrize("p", POOL_PARAMS, ids=lambda p: "%dx%d-%s-%s" % (p[1][0], p[1][1], "x".join(map(str, p[1][2])), p[1][3]))
def test_maxpool(dev, p):
    i, (N, C, geo, fam) = p
    _pool_case(dev, i, N, C, geo, fam)


def test_maxpool_second_trip(dev):
    N, C = H.POOL_BIG[:2]
    geo = H.POOL_BIG[2:]
    P, Q = H.pool_out(*geo)
    assert H.trips("pool", N * C * P * Q) == 2
    _pool_case(dev, len(POOL_PARAMS), N, C, geo, "ties")


@pytest.mark.parametrize("HW", H.GAP_HW)
def test_global_average_and_gem(dev, HW):
    """planes 1, 4, 5 (the last workgroup partly empty); GeM p of 1, 3, 6.5 on values below, at and above eps, negatives and an
    entirely clamped plane; dp given and NULL; the workspace exactly 4 N C bytes, one byte less is the workspace error"""
    lib = _lib()
    for j, (N, C) in enumerate(H.GAP_PLANES):
        fam = H.FAMILIES[(HW + j) % 4]
        x = H.family((N, C, HW), fam, H.gen(HW + j))
        dy = torch.randn(N, C, generator=H.gen(HW))
        xd, dyd = _to(dev, x, dy)
        tag = "%s %s" % ((N, C, HW), fam)
        y = _Out((N, C), dev)
        lib.rg_global_avgpool_fwd(xd.data_ptr(), y.ptr, N, C, HW, _st())
        y.check(H.gap_fwd(x), "rg_global_avgpool_fwd y | " + tag, fam)
        dx = _Out((N, C, HW), dev)
        lib.rg_global_avgpool_bwd(dyd.data_ptr(), dx.ptr, N, C, HW, _st())
        dx.check(H.gap_bwd(dy, x.shape), "rg_global_avgpool_bwd dx | " + tag, fam)
        x = H.gem_input(N, C, HW, seed=j)
        xd, = _to(dev, x)
        for p in H.GEM_P:
            pt = torch.tensor([p])
            pd, = _to(dev, pt)
            tag = "%s p %s" % ((N, C, HW), p)
            y = _Out((N, C), dev)
            lib.rg_gem_pool_fwd(xd.data_ptr(), pd.data_ptr(), y.ptr, N, C, HW, 1e-6, _st())
            ry = H.gem_fwd(x, pt)
            y.check(ry, "rg_gem_pool_fwd y | " + tag, "planted")
            y32 = ry.value.float()
            yd, = _to(dev, y32)
            rdx, rdp = H.gem_bwd(x, pt, y32, dy)
            for need_dp in (True, False):
                ws = _Out((N * C,), dev)
                dx = _Out((N, C, HW), dev)
                dp = _Out((1,), dev) if need_dp else None
                lib.rg_gem_pool_bwd(xd.data_ptr(), pd.data_ptr(), yd.data_ptr(), dyd.data_ptr(), dx.ptr, _ptr(dp), N, C, HW, 1e-6,
                                    ws.ptr if need_dp else None, 4 * N * C if need_dp else 0, _st())
                dx.check(rdx, "rg_gem_pool_bwd dx | %s dp %s" % (tag, need_dp), "planted")
                ws.guards("rg_gem_pool_bwd workspace")
                if need_dp:
                    dp.check(rdp, "rg_gem_pool_bwd dp | " + tag, "planted")
                else:
                    ws.untouched("rg_gem_pool_bwd workspace without dp")
        ws, dx, dp = _Out((N * C,), dev), _Out((N, C, HW), dev), _Out((1,), dev)
        with pytest.raises(RuntimeError, match="workspace too small"):
            lib.rg_gem_pool_bwd(xd.data_ptr(), pd.data_ptr(), yd.data_ptr(), dyd.data_ptr(), dx.ptr, dp.ptr, N, C, HW, 1e-6, ws.ptr,
                                4 * N * C - 1, _st())
        dx.untouched("rg_gem_pool_bwd dx after the workspace error")
        dp.untouched("rg_gem_pool_bwd dp after the workspace error")


def test_gap_bwd_past_the_grid_cap(dev):
    lib = _lib()
    N, C, HW = T.GAP_BWD_BIG
    assert H.trips("pool", N * C * HW) == 2
    dy = torch.randn(N, C, generator=H.gen(3))
    dyd, = _to(dev, dy)
    dx = _Out((N, C, HW), dev)
    lib.rg_global_avgpool_bwd(dyd.data_ptr(), dx.ptr, N, C, HW, _st())
    dx.check(H.gap_bwd(dy, (N, C, HW)), "rg_global_avgpool_bwd dx | %s" % ((N, C, HW),), "plain")


# ---- cm.hip --------------------------------------------------------------------------------------------------------------------
CM_PARAMS = list(enumerate(H.cm_cases()))


@pytest.mark.parametrize("p", CM_PARAMS, ids=lambda p: "B%d-D%d-%s-m%g-e%d" % p[1])
def test_cm_update(dev, p):
    """rg_cm_update (normalize_eps as the case says) and rg_cm_update_hard (without and with a bit-identical tied pair); the
    whole bank is compared: rows no valid label names have M = 0"""
    lib = _lib()
    i, (B, D, pat, mom, ne) = p
    y = H.cm_labels(pat, B)
    tag = "B %d D %d %s mom %s" % (B, D, pat, mom)
    x, feats = H.cm_input(B, D, seed=i)
    xd, yd = _to(dev, x, y)
    bank = _Out((H.CM_K, D), dev, feats)
    lib.rg_cm_update(xd.data_ptr(), yd.data_ptr(), bank.ptr, B, D, H.CM_K, mom, ne, _st())
    bank.check(H.cm_update(x, y, feats, mom, ne), "rg_cm_update(eps %d) features | %s" % (ne, tag), pat)
    for tie in (False, True):
        x, feats = H.cm_input(B, D, seed=i, tie=tie)
        xd, = _to(dev, x)
        bank = _Out((H.CM_K, D), dev, feats)
        lib.rg_cm_update_hard(xd.data_ptr(), yd.data_ptr(), bank.ptr, B, D, H.CM_K, mom, _st())
        bank.check(H.cm_update_hard(x, y, feats, mom), "rg_cm_update_hard features | %s tie %s" % (tag, tie), pat)


def test_cm_update_edges(dev):
    """D = 4097 is an error that leaves the bank bit for bit unchanged; the zero vector with normalize_eps gives a zero row"""
    lib = _lib()
    D = H.CM_MAX_D + 1
    x, feats = H.cm_input(4, D)
    y = torch.tensor([1, 1, 2, 3])
    xd, yd = _to(dev, x, y)
    for hard in (False, True):
        bank = _Out((H.CM_K, D), dev, feats)
        with pytest.raises(RuntimeError, match="feature dim"):
            if hard:
                lib.rg_cm_update_hard(xd.data_ptr(), yd.data_ptr(), bank.ptr, 4, D, H.CM_K, 0.2, _st())
            else:
                lib.rg_cm_update(xd.data_ptr(), yd.data_ptr(), bank.ptr, 4, D, H.CM_K, 0.2, 0, _st())
        bank.check(H.exact(feats), "bank after the D = 4097 error (hard %s)" % hard, "plain")
    x, feats = H.cm_input(4, 64)
    x[:] = 0.0
    xd, = _to(dev, x)
    bank = _Out((H.CM_K, 64), dev, feats)
    lib.rg_cm_update(xd.data_ptr(), yd.data_ptr(), bank.ptr, 4, 64, H.CM_K, 0.0, 1, _st())
    ref = H.cm_update(x, y, feats, 0.0, 1)
    assert bool((ref.value[1:4] == 0).all())
    bank.check(ref, "rg_cm_update(eps 1) zero vector", "planted")


def test_normalize_listed_rows(dev):
    """n_ids of 1, 4, 5; a repeated id divided once; ids -1 and `rows` skipped; unlisted rows unchanged; a zero row"""
    lib = _lib()
    for n_ids in H.NLR_N:
        for D in H.NLR_D:
            gm, ids = T.nlr_input(n_ids, D)
            idd, = _to(dev, ids)
            g = _Out(tuple(gm.shape), dev, gm)
            lib.rg_normalize_listed_rows(g.ptr, idd.data_ptr(), n_ids, gm.shape[0], D, 1e-16, _st())
            g.check(H.normalize_listed_rows(gm, ids, 1e-16), "rg_normalize_listed_rows g | n_ids %d D %d" % (n_ids, D), "scales")


# ---- optim.hip -----------------------------------------------------------------------------------------------------------------
LR, EPS = T.LR, T.EPS


def _adam_bufs(dev, n, fam, seed):
    p, g, m, v = H.optim_input(n, fam, seed=seed)
    gd, = _to(dev, g)
    assert gd.data_ptr() % 16 == 0
    return (p, g, m, v), gd, [_Out((n,), dev, t) for t in (p, m, v)]


ADAM_PARAMS = list(enumerate(H.adam_cases()))


@pytest.mark.parametrize("p", ADAM_PARAMS, ids=lambda p: "n%d-step%d-b%g-wd%g-gs%g-%s" % (p[1][0], p[1][1], p[1][2][0], p[1][3], p[1][4], p[1][5]))
def test_adam_step(dev, p):
    """one step from given p, m, v: rg_adam_step(step = k), and rg_adam_step_dev on the clock k applications of rg_adam_advance
    leave (the same budget); the clock itself against the same products in Python doubles"""
    lib = _lib()
    i, (n, step, betas, wd, gs, fam) = p
    (p0, g, m, v), gd, (po, mo, vo) = _adam_bufs(dev, n, fam, i)
    ref = H.adam_step(p0, g, m, v, LR, betas[0], betas[1], EPS, wd, step, gs)
    tag = "n %d step %d betas %s wd %s gs %s" % (n, step, betas, wd, gs)
    lib.rg_adam_step(po.ptr, gd.data_ptr(), mo.ptr, vo.ptr, n, LR, betas[0], betas[1], EPS, wd, step, gs, _st())
    for k, o in (("p", po), ("m", mo), ("v", vo)):
        o.check(ref[k], "rg_adam_step %s | %s" % (k, tag), fam)
    if wd == 0.0:
        assert float(po.t[0]) == float(p0[0])                      # g = m = v = 0: p unchanged, no NaN
    if n == H.ADAM_BIG:
        return
    clock = _Out((4,), dev, torch.tensor([0.0, 1.0, 1.0, 0.0], dtype=torch.float64), dtype=torch.float64)
    for _ in range(step):
        lib.rg_adam_advance(clock.ptr, betas[0], betas[1], _st())
    clock.guards("rg_adam_advance state")
    want = H.adam_clock(step, betas[0], betas[1])
    st = clock.t.cpu().tolist()
    assert st[3] == 0.0 and all(abs(a - b) <= 1e-15 * abs(b) for a, b in zip(st[:3], want)), (st, want)
    (p0, g, m, v), gd, (po, mo, vo) = _adam_bufs(dev, n, fam, i)
    lib.rg_adam_step_dev(po.ptr, gd.data_ptr(), mo.ptr, vo.ptr, n, LR, betas[0], betas[1], EPS, wd, clock.ptr, gs, _st())
    for k, o in (("p", po), ("m", mo), ("v", vo)):
        o.check(ref[k], "rg_adam_step_dev %s | %s" % (k, tag), fam)


def test_adam_step_dev_second_trip(dev):
    lib = _lib()
    n = H.DEV_BIG
    (p0, g, m, v), gd, (po, mo, vo) = _adam_bufs(dev, n, "scales", 77)
    step, (b1, b2) = 2, H.ADAM_BETAS[1]
    clock, = _to(dev, torch.tensor(H.adam_clock(step, b1, b2) + [0.0], dtype=torch.float64))
    lib.rg_adam_step_dev(po.ptr, gd.data_ptr(), mo.ptr, vo.ptr, n, LR, b1, b2, EPS, 5e-4, clock.data_ptr(), 0.125, _st())
    ref = H.adam_step(p0, g, m, v, LR, b1, b2, EPS, 5e-4, step, 0.125)
    for k, o in (("p", po), ("m", mo), ("v", vo)):
        o.check(ref[k], "rg_adam_step_dev %s | n %d" % (k, n), "scales")


def test_adam_step_misaligned_buffer(dev):
    """one buffer 4 bytes off 16: the alignment error, and all four buffers unchanged"""
    lib = _lib()
    n = 1003
    p, g, m, v = H.optim_input(n, "plain")
    for which in range(4):
        outs = [_Out((n,), dev, t, shift=1 if k == which else 0) for k, t in enumerate((p, g, m, v))]
        with pytest.raises(RuntimeError, match="16-byte aligned"):
            lib.rg_adam_step(outs[0].ptr, outs[1].ptr, outs[2].ptr, outs[3].ptr, n, LR, 0.9, 0.999, EPS, 0.0, 1, 1.0, _st())
        for o, t in zip(outs, (p, g, m, v)):
            o.check(H.exact(t), "buffer after the alignment error", "plain")


def test_u64_add(dev):
    lib = _lib()
    buf = torch.full((5,), 12345, dtype=torch.int64, device=dev)
    buf[2] = 2 ** 32 - 1
    lib.rg_u64_add(buf[2:].data_ptr(), 1, _st())
    assert buf.cpu().tolist() == [12345, 12345, 2 ** 32, 12345, 12345]              # the carry past 2^32
    lib.rg_u64_add(buf[2:].data_ptr(), 2 ** 40 + 7, _st())
    assert buf.cpu().tolist() == [12345, 12345, 2 ** 32 + 2 ** 40 + 7, 12345, 12345]


@pytest.mark.parametrize("c", T.SGD_CASES, ids=lambda c: "n%d-m%g-first%s" % c)
def test_sgd_step(dev, c):
    """momentum 0.9 and 0 (momentum_buf NULL); a first step with the buffer full of NaN; a later step; n past the grid cap"""
    lib = _lib()
    n, mom, first = c
    i = T.SGD_CASES.index(c)
    p, g, buf, _ = H.optim_input(n, "plain", seed=50 + i)
    gd, = _to(dev, g)
    for wd, gs in ((1e-4, 1.0), (0.0, 0.125)):
        po = _Out((n,), dev, p)
        start = torch.full((n,), float("nan")) if first else buf
        bo = _Out((n,), dev, start) if mom else None
        lib.rg_sgd_step(po.ptr, gd.data_ptr(), _ptr(bo), n, 0.01, mom, wd, int(first), gs, _st())
        ref = H.sgd_step(p, g, buf if mom else None, 0.01, mom, wd, first, gs)
        tag = "n %d mom %s first %s wd %s gs %s" % (n, mom, first, wd, gs)
        po.check(ref["p"], "rg_sgd_step p | " + tag, "plain")
        if bo is not None:
            bo.check(ref["buf"], "rg_sgd_step buf | " + tag, "plain")


# ---- one case per unit through the rg_hip.ops wrappers (their workspace and allocation) -------------------------------------------------
def test_through_the_ops_wrappers(dev):
    ops = _ops()
    # loss
    x = H.sum_input("bce", 0.83, 70001, "plain")
    xd, = _to(dev, x)
    ref = H.two_stage("bce", x, 0.83)
    H.check(ops.sigmoid_bce_fwd(xd, 0.83), ref, "ops.sigmoid_bce_fwd")
    H.check(ops.sigmoid_bce_bwd(xd, None, 0.83, 0.3), H.sum_bwd("bce", x, 0.83, None, 0.3), "ops.sigmoid_bce_bwd")
    z, lab = H.ce_input(5, 257, "cosine"), H.ce_labels(5, 257)
    zd, labd = _to(dev, z, lab)
    f = H.softmax_ce_fwd(z, lab, 20.0)
    loss, lse = ops.softmax_ce_fwd(zd, labd, 20.0)
    H.check(loss, f["loss"], "ops.softmax_ce_fwd loss")
    H.check(lse, f["lse"], "ops.softmax_ce_fwd lse")
    lse32 = f["lse"].value.float()
    H.check(ops.softmax_ce_bwd(zd, labd, lse32.to(dev), None, 20.0, 0.7), H.softmax_ce_bwd(z, lab, lse32, None, 20.0, 0.7),
            "ops.softmax_ce_bwd")
    # pool
    geo = H.POOL_GEOM[4]
    x = H.pool_input(2, 5, geo[0], geo[1], "ties")
    xd, = _to(dev, x)
    ry, ra = H.maxpool_fwd(x, *geo[2:])
    y, arg = ops.maxpool2d_fwd(xd, 3, 2, 1)
    H.check(y, ry, "ops.maxpool2d_fwd y")
    H.check(arg, ra, "ops.maxpool2d_fwd argmax")
    dy = torch.randn(y.shape, generator=H.gen(5))
    H.check(ops.maxpool2d_bwd(dy.to(dev), ra.value.to(torch.uint8).to(dev), x.shape, 3, 2, 1),
            H.maxpool_bwd(dy, ra.value, x.shape, *geo[2:]), "ops.maxpool2d_bwd")
    x = H.gem_input(1, 5, 65).reshape(1, 5, 13, 5)
    pt = torch.tensor([3.0])
    ry = H.gem_fwd(x, pt)
    dyg = torch.randn(1, 5, generator=H.gen(6))
    H.check(ops.gem_pool_fwd(x.to(dev), pt.to(dev)), ry, "ops.gem_pool_fwd")
    y32 = ry.value.float()
    dx, dp = ops.gem_pool_bwd(x.to(dev), pt.to(dev), y32.to(dev), dyg.to(dev))
    rdx, rdp = H.gem_bwd(x, pt, y32, dyg)
    H.check(dx, rdx, "ops.gem_pool_bwd dx")
    H.check(dp, rdp, "ops.gem_pool_bwd dp")
    # cluster memory
    x, feats = H.cm_input(8, 2048)
    y = H.cm_labels("mixed", 8)
    bank = feats.to(dev).clone()
    ops.cm_update(x.to(dev), y.to(dev), bank, 0.2)
    H.check(bank, H.cm_update(x, y, feats, 0.2, 0), "ops.cm_update")
    bank = feats.to(dev).clone()
    ops.cm_update(x.to(dev), y.to(dev), bank, 0.2, hard=True)
    H.check(bank, H.cm_update_hard(x, y, feats, 0.2), "ops.cm_update(hard)")
    gm, ids = T.nlr_input(5, 65)
    H.check(ops.normalize_listed_rows(gm.to(dev), ids.to(dev)), H.normalize_listed_rows(gm, ids, 1e-16), "ops.normalize_listed_rows")
    # optimizers
    p, g, m, v = H.optim_input(1003, "plain")
    pd, gd, md, vd = [torch.zeros(1008, device=dev)[:1003].copy_(t) for t in (p, g, m, v)]
    ops.adam_step(pd, gd, md, vd, LR, 0.9, 0.999, EPS, 5e-4, 2)
    ref = H.adam_step(p, g, m, v, LR, 0.9, 0.999, EPS, 5e-4, 2, 1.0)
    for k, t in (("p", pd), ("m", md), ("v", vd)):
        H.check(t, ref[k], "ops.adam_step " + k)
    pd, gd, bd = _to(dev, p, g, m)
    ops.sgd_step(pd, gd, bd, 0.01, 0.9, 1e-4, False)
    ref = H.sgd_step(p, g, m, 0.01, 0.9, 1e-4, False, 1.0)
    H.check(pd, ref["p"], "ops.sgd_step p")
    H.check(bd, ref["buf"], "ops.sgd_step buf")
