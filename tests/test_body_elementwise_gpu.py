"""GPU: every entry point of csrc/eltwise.hip, csrc/gan_extra.hip, csrc/bgemm.hip, csrc/resize.hip and csrc/retrieval.hip
(except rg_fill and rg_spin_us), per element against the fp64 host model (tests/body_hostmodel.py) with its per-element error
budgets, at geometries built from the launch arithmetic: every grid-stride loop on its second trip, the float4 / tail split at
every n % 4 and with no float4 at all, both instantiations of the channel normalisation at the same per-pixel data, both routes
of the reflection padding at the same geometry (bit for bit), both spectral-norm backward kernels on either side of their
switch, the descriptor batch boundary, ragged GEMM tiles in all four load mappings — with every optional pointer given and NULL,
every output between two rows of guard values, and no element left out of any comparison.

The C ABI is called the way rg_hip.ops calls it (ops allocates its outputs itself, so it cannot put them between guards); one
case per unit goes through the ops wrappers.  Each backward is handed the rounded reference forward outputs (y, norm, p, sigma,
u, v, w_sn), not the kernel's own.

Each check prints `RATIO <entry point> <output> <family> <max err / (2^-24 M)>` (pytest -s shows them).

_Out is a copy of the one in tests/test_head_elementwise_gpu.py."""
import ctypes

import pytest
import torch

from tests import body_hostmodel as B
from tests import test_body_hostmodel_cpu as T

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

    def __init__(self, shape, dev, init=None, dtype=torch.float32, fill=B.FILL, shift=0):
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
        r = B.check(self.t, ref, what)
        print("RATIO %s %s %.3f" % (what.split(" | ")[0], family, r))


def _ptr(o):
    return None if o is None else (o.ptr if isinstance(o, _Out) else o.data_ptr())


def _to(dev, *ts):
    return [None if t is None else t.contiguous().to(dev) for t in ts]


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


# ---- eltwise.hip ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("act", B.ACTS)
def test_activations(dev, act):
    """n of 1, 3 (no float4), 4, 5, 6, 7, 1027 and 4 * 4096 * 256 + 7 (second float4 trip, tail of 3); planted 0.0, -0.0,
    denormals, +-inf; the backward at y == 0, y == -0.0 and |y| next to 1"""
    lib = _lib()
    for n, a, fam in T.act_cases():
        if a != act:
            continue
        tag = "n %d act %d %s" % (n, act, fam)
        x = B.act_input(n, fam, seed=act)
        xd, = _to(dev, x)
        y = _Out((n,), dev)
        lib.rg_act_fwd(xd.data_ptr(), y.ptr, n, act, B.SLOPE, _st())
        y.check(B.act_fwd(x, act, B.SLOPE), "rg_act_fwd y | " + tag, fam)
        dy, yy = B.act_bwd_input(n, act)
        dyd, yd = _to(dev, dy, yy)
        dx = _Out((n,), dev)
        lib.rg_act_bwd(dyd.data_ptr(), yd.data_ptr(), dx.ptr, n, act, B.SLOPE, _st())
        dx.check(B.act_bwd(dy, yy, act, B.SLOPE), "rg_act_bwd dx | " + tag, "planted")
    x = B.act_input(1027, "plain", seed=act)
    xd, = _to(dev, x)
    B.check(_ops().act_fwd(xd, act, B.SLOPE), B.act_fwd(x, act, B.SLOPE), "ops.act_fwd")
    dy, yy = B.act_bwd_input(1027, act)
    B.check(_ops().act_bwd(*_to(dev, dy, yy), act, B.SLOPE), B.act_bwd(dy, yy, act, B.SLOPE), "ops.act_bwd")


def test_axpby(dev):
    lib = _lib()
    for i, n in enumerate(B.VEC_N):
        fam = T.FAMS[i % 4] if n < 10000 else "scales"
        a, b = B.family((n,), fam, B.gen(n % 1000)), B.family((n,), "plain", B.gen(n % 1000 + 1))
        ad, bd = _to(dev, a, b)
        for bb, bdev in ((b, bd), (None, None)):
            y = _Out((n,), dev)
            lib.rg_axpby(ad.data_ptr(), _ptr(bdev), y.ptr, n, 0.7, -1.3, _st())
            y.check(B.axpby(a, bb, 0.7, -1.3), "rg_axpby y | n %d %s b %s" % (n, fam, bb is not None), fam)


def test_sub_square(dev):
    """da NULL only, db NULL only, both given; n = 4096 * 256 + 3 on the second trip"""
    lib = _lib()
    for n, fam in ((1, "plain"), (257, "offset"), (1027, "scales"), (B.ELT_BIG, "plain")):
        a, b, dy = (B.family((n,), fam, B.gen(n % 1000 + k)) for k in range(3))
        ad, bd, gd = _to(dev, a, b, dy)
        tag = "n %d %s" % (n, fam)
        y = _Out((n,), dev)
        lib.rg_sub_square_fwd(ad.data_ptr(), bd.data_ptr(), y.ptr, n, _st())
        y.check(B.sub_square_fwd(a, b), "rg_sub_square_fwd y | " + tag, fam)
        ra, rb = B.sub_square_bwd(a, b, dy)
        for need in ("ab", "a", "b"):
            da = _Out((n,), dev) if "a" in need else None
            db = _Out((n,), dev) if "b" in need else None
            lib.rg_sub_square_bwd(ad.data_ptr(), bd.data_ptr(), gd.data_ptr(), _ptr(da), _ptr(db), n, _st())
            if da is not None:
                da.check(ra, "rg_sub_square_bwd da | %s %s" % (tag, need), fam)
            if db is not None:
                db.check(rb, "rg_sub_square_bwd db | %s %s" % (tag, need), fam)


def test_pair_cat(dev):
    """per % 4 != 0 and == 0, one chunk, two chunks, and the chunk cap of 1024 (B = 1, per / 4 > 1024 * 1024); take_a NULL,
    all ones, mixed"""
    lib = _lib()
    for Bn, per in B.PAIR_CAT:
        a, b = B.family((Bn, per), "plain", B.gen(per % 1000)), B.family((Bn, per), "scales", B.gen(per % 1000 + 1))
        ad, bd = _to(dev, a, b)
        for mode in ("null", "ones", "mixed"):
            take = None if mode == "null" else (torch.ones(Bn, dtype=torch.int64) if mode == "ones" else (torch.arange(Bn) % 2 * 5).to(torch.int64))
            td, = _to(dev, take)
            out = _Out((2 * Bn, per), dev)
            lib.rg_pair_cat(ad.data_ptr(), bd.data_ptr(), _ptr(td), out.ptr, Bn, per, _st())
            out.check(B.pair_cat(a, b, take), "rg_pair_cat out | %s %s" % ((Bn, per), mode), mode)


def _dropout(dev, x, xd, p, seed, clock, tag):
    lib = _lib()
    n = x.numel()
    ys = []
    for _ in range(2):
        y = _Out((n,), dev)
        if clock is None:
            lib.rg_dropout(xd.data_ptr(), y.ptr, n, p, seed, _st())
        else:
            cd = torch.tensor([clock], dtype=torch.int64, device=dev)
            lib.rg_dropout_clocked(xd.data_ptr(), y.ptr, n, p, seed, cd.data_ptr(), _st())
        ys.append(y)
    ref, keep = B.dropout(x, p, seed, clock)
    name = "rg_dropout" if clock is None else "rg_dropout_clocked"
    assert torch.equal((ys[0].t != 0).cpu(), keep), "%s: mask differs from the oracle | %s" % (name, tag)
    ys[0].check(ref, "%s y | %s" % (name, tag), "p %g" % p)
    assert torch.equal(_bits(ys[0].t), _bits(ys[1].t)), "%s: the same call twice differs | %s" % (name, tag)
    ys[1].guards(name)


def test_dropout(dev):
    """the mask bit for bit against oracle.ref_torch.dropout_keep_mask, the kept values as modelled (one rounded reciprocal,
    one rounded product), the same call twice; p of 0, 0.2, 0.5, 0.999; seeds 0, 12345 and >= 2^63; clocks 0, 1 and >= 2^32;
    n = 4096 * 256 + 3 on the second trip; a rate whose threshold equals an element's hash"""
    for n in B.DROPOUT_N:
        x = (torch.rand(n, generator=B.gen(n % 1000)) + 0.5).float()     # no zeros: the mask is y != 0
        xd, = _to(dev, x)
        for i, p in enumerate(B.DROPOUT_P):
            for j, seed in enumerate(B.DROPOUT_SEEDS):
                if n == B.ELT_BIG and (i, j) not in ((1, 2), (3, 0)):
                    continue
                _dropout(dev, x, xd, p, seed, None, "n %d p %g seed %d" % (n, p, seed))
                clock = B.DROPOUT_CLOCKS[(i + j) % 3]
                if n != B.ELT_BIG or j == 2:
                    _dropout(dev, x, xd, p, seed, clock, "n %d p %g seed %d clock %d" % (n, p, seed, clock))
    seed, p, i = T.threshold_case()
    x = torch.ones(4096)
    xd, = _to(dev, x)
    assert bool(B.dropout(x, p, seed)[1][i])
    _dropout(dev, x, xd, p, seed, None, "threshold hit at element %d" % i)
    y = _ops().dropout(xd, 0.5, 12345)                                # the wrapper: the clocked entry point at the step clock
    clock = int(_ops().step_clock(xd.device).cpu()[0])
    B.check(y, B.dropout(x, 0.5, 12345, clock)[0], "ops.dropout")


def test_l2norm_rows(dev):
    """D of 1, 255, 256, 257, 2051; rows planted: zero, norm < eps, norm == eps exactly, scale 1e3; eps 0.5 and float32(1e-12);
    norm NULL in the forward"""
    lib = _lib()
    for D, eps, fam in T.l2rows_cases():
        x = B.l2rows_input(D, eps, fam)
        rows = x.shape[0]
        dy = B.family(x.shape, "plain", B.gen(D))
        ry, rn = B.l2norm_fwd(x, eps)
        xd, gd, yd, nd = _to(dev, x, dy, ry.value.float(), rn.value.float())
        tag = "D %d eps %g %s" % (D, eps, fam)
        for with_norm in (True, False):
            y, nr = _Out((rows, D), dev), _Out((rows,), dev) if with_norm else None
            lib.rg_l2norm_rows_fwd(xd.data_ptr(), y.ptr, _ptr(nr), rows, D, eps, _st())
            y.check(ry, "rg_l2norm_rows_fwd y | %s norm %s" % (tag, with_norm), fam)
            if nr is not None:
                nr.check(rn, "rg_l2norm_rows_fwd norm | " + tag, fam)
        dx = _Out((rows, D), dev)
        lib.rg_l2norm_rows_bwd(yd.data_ptr(), gd.data_ptr(), nd.data_ptr(), dx.ptr, rows, D, eps, _st())
        dx.check(B.l2norm_bwd(ry.value.float(), dy, rn.value.float(), eps), "rg_l2norm_rows_bwd dx | " + tag, fam)
    x = B.l2rows_input(257, 1e-12)
    y, nr = _ops().l2norm_rows_fwd(_to(dev, x)[0])
    ry, rn = B.l2norm_fwd(x, 1e-12)
    B.check(y, ry, "ops.l2norm_rows_fwd y")
    B.check(nr, rn, "ops.l2norm_rows_fwd norm")


def test_l2norm_channels(dev):
    """(2, 3, 5): groups without a channel; (3, 37, 49); (16, 5, 4093) on PX = 64 and (15, 5, 4093) on PX = 16 at the same
    per-pixel data.  The two instantiations do NOT add in the same order (PX = 64: four channel groups, channels g, g + 4, ...
    per group; PX = 16: sixteen groups), so their overlapping images are each compared within the budget, and the number of
    elements that differ in the last bits is printed, not asserted."""
    lib = _lib()
    kept = {}
    for N, C, HW in B.L2C:
        for eps in B.L2_EPS[:1] if HW > 1000 else B.L2_EPS:
            x = B.l2chan_input(N, C, HW, eps)
            dy = B.family(x.shape, "plain", B.gen(HW))
            ry, rn = B.l2norm_fwd(x, eps)
            xd, gd, yd, nd = _to(dev, x, dy, ry.value.float(), rn.value.float())
            tag = "%s eps %g PX %d" % ((N, C, HW), eps, B.l2c_px(N, HW))
            for with_norm in (True, False):
                y, nr = _Out((N, C, HW), dev), _Out((N, HW), dev) if with_norm else None
                lib.rg_l2norm_channels_fwd(xd.data_ptr(), y.ptr, _ptr(nr), N, C, HW, eps, _st())
                y.check(ry, "rg_l2norm_channels_fwd y | %s norm %s" % (tag, with_norm), "planted")
                if nr is not None:
                    nr.check(rn, "rg_l2norm_channels_fwd norm | " + tag, "planted")
                    kept[(N, "y")], kept[(N, "norm")] = y.t.cpu(), nr.t.cpu()
            dx = _Out((N, C, HW), dev)
            lib.rg_l2norm_channels_bwd(yd.data_ptr(), gd.data_ptr(), nd.data_ptr(), dx.ptr, N, C, HW, eps, _st())
            dx.check(B.l2norm_bwd(ry.value.float(), dy, rn.value.float(), eps), "rg_l2norm_channels_bwd dx | " + tag, "planted")
            kept[(N, "dx")] = dx.t.cpu()
    for k in ("y", "norm", "dx"):
        a, b = kept[(16, k)][:15], kept[(15, k)]
        print("PX 64 against PX 16, %s: %d of %d elements differ" % (k, int((_bits(a) != _bits(b)).sum()), a.numel()))
    x = B.l2chan_input(3, 37, 49, 1e-12).reshape(3, 37, 7, 7)
    y, nr = _ops().l2norm_channels_fwd(_to(dev, x)[0])
    B.check(y.reshape(3, 37, 49), B.l2norm_fwd(x.reshape(3, 37, 49), 1e-12)[0], "ops.l2norm_channels_fwd")


def test_copy_channels(dev):
    """accumulate 0 and 1, non-zero sc0 and dc0 with Cs != Cd, channels outside the range untouched, N Cc HW past 4096 * 256"""
    lib = _lib()
    for N, Cc, HW, Cs, sc0, Cd, dc0 in B.COPY_CH:
        src = B.family((N, Cs, HW), "plain", B.gen(HW))
        dst = B.family((N, Cd, HW), "scales", B.gen(HW + 1))
        sd, = _to(dev, src)
        for acc in (0, 1):
            out = _Out((N, Cd, HW), dev, init=dst)
            lib.rg_copy_channels(sd.data_ptr(), out.ptr, N, Cc, HW, Cs, sc0, Cd, dc0, acc, _st())
            out.check(B.copy_channels(src, dst, Cc, sc0, dc0, acc), "rg_copy_channels dst | %s accumulate %d" % ((N, Cc, HW, Cs, sc0, Cd, dc0), acc),
                      "plain")


def test_mix_rows(dev):
    """lam of 0, 0.3, 1; repeated indices, a source row nobody reads, ia[j] == ib[j]; len of 1 and 257; both totals on the
    second trip"""
    lib = _lib()
    for rs, ro, ln, lam in B.MIX:
        src = B.family((rs, ln), "plain", B.gen(ln))
        g = B.family((ro, ln), "scales", B.gen(ln + 1))
        ia, ib = B.mix_indices(rs, ro)
        sd, gd, iad, ibd = _to(dev, src, g, ia, ib)
        tag = "%s" % ((rs, ro, ln, lam),)
        out = _Out((ro, ln), dev)
        lib.rg_mix_rows_fwd(sd.data_ptr(), iad.data_ptr(), ibd.data_ptr(), lam, out.ptr, rs, ro, ln, _st())
        out.check(B.mix_rows_fwd(src, ia, ib, lam), "rg_mix_rows_fwd out | " + tag, "plain")
        ds = _Out((rs, ln), dev)
        lib.rg_mix_rows_bwd(gd.data_ptr(), iad.data_ptr(), ibd.data_ptr(), lam, ds.ptr, rs, ro, ln, _st())
        ds.check(B.mix_rows_bwd(g, ia, ib, lam, rs), "rg_mix_rows_bwd dsrc | " + tag, "scales")
    rs, ro, ln, lam = B.MIX[1]
    src = B.family((rs, ln), "plain", B.gen(ln))
    ia, ib = B.mix_indices(rs, ro)
    B.check(_ops().mix_rows_fwd(*_to(dev, src, ia, ib), lam), B.mix_rows_fwd(src, ia, ib, lam), "ops.mix_rows_fwd")


# ---- gan_extra.hip -------------------------------------------------------------------------------------------------------------
def test_avgpool(dev):
    """k of 2 and 3; H % k and W % k both zero and both non-zero; H == k; the backward past 8192 * 256 with a ragged rim"""
    lib = _lib()
    for N, C, H, W, k in B.AVGPOOL + [B.AVGPOOL_BIG]:
        fam = T.FAMS[(H + W) % 4]
        x = B.family((N, C, H, W), fam, B.gen(H * W))
        dy = B.family((N, C, H // k, W // k), "plain", B.gen(H))
        xd, gd = _to(dev, x, dy)
        tag = "%s" % ((N, C, H, W, k),)
        y = _Out((N, C, H // k, W // k), dev)
        lib.rg_avgpool2d_fwd(xd.data_ptr(), y.ptr, N, C, H, W, k, _st())
        y.check(B.avgpool_fwd(x, k), "rg_avgpool2d_fwd y | " + tag, fam)
        dx = _Out((N, C, H, W), dev)
        lib.rg_avgpool2d_bwd(gd.data_ptr(), dx.ptr, N, C, H, W, k, _st())
        dx.check(B.avgpool_bwd(dy, H, W, k), "rg_avgpool2d_bwd dx | " + tag, "plain")
        P, Q = H // k, W // k
        assert bool((dx.t[:, :, P * k:] == 0).all()) and bool((dx.t[:, :, :, Q * k:] == 0).all()), "non-zero ragged rim | " + tag
    x = B.family((2, 3, 5, 7), "plain", B.gen(1))
    B.check(_ops().avgpool2d_fwd(_to(dev, x)[0], 2), B.avgpool_fwd(x, 2), "ops.avgpool2d_fwd")


def _shifted(dev, t, shift):
    """a device copy of t whose address is `shift` floats past a 16-byte boundary"""
    buf = torch.empty(t.numel() + 8, dtype=torch.float32, device=dev)
    assert buf.data_ptr() % 16 == 0
    v = buf[shift:shift + t.numel()].view(t.shape)
    v.copy_(t)
    return v


def _pad_input(N, C, H, W, pad):
    x = B.act_input(N * C * H * W, "plain", seed=pad).reshape(N, C, H, W)
    return torch.where(torch.isinf(x) & (x > 0), torch.tensor(3.0), x).contiguous()


def _pad_case(dev, N, C, H, W, pad):
    lib = _lib()
    OH, OW = H + 2 * pad, W + 2 * pad
    x = _pad_input(N, C, H, W, pad)
    dy = B.family((N, C, OH, OW), "plain", B.gen(H * W + pad))
    gd, = _to(dev, dy)
    vec = B.pad_vec_route(W, pad, 0)
    tag = "%s" % ((N, C, H, W, pad),)
    outs = {}
    for shift in ((0, 1) if vec else (0,)):
        # shift 1: x (forward) and dx (backward) one float off a 16-byte boundary — the documented way onto the scalar route
        route = "vector" if vec and not shift else "scalar"
        xd = _shifted(dev, x, shift)
        assert B.pad_vec_route(W, pad, xd.data_ptr()) == (route == "vector")
        y = _Out((N, C, OH, OW), dev)
        lib.rg_reflection_pad2d_fwd(xd.data_ptr(), y.ptr, N, C, H, W, pad, B.ACT_NONE, 0.0, _st())
        y.check(B.reflection_pad_fwd(x, pad), "rg_reflection_pad2d_fwd y | %s %s" % (tag, route), route)
        dx = _Out((N, C, H, W), dev, shift=shift)
        assert B.pad_vec_route(W, pad, dx.ptr, 0) == (route == "vector")
        lib.rg_reflection_pad2d_bwd(gd.data_ptr(), None, dx.ptr, N, C, H, W, pad, B.ACT_NONE, 0.0, _st())
        dx.check(B.reflection_pad_bwd(dy, H, W, pad), "rg_reflection_pad2d_bwd dx | %s %s" % (tag, route), route)
        outs[route] = (_bits(y.t), _bits(dx.t))
    if vec:
        assert torch.equal(outs["vector"][0], outs["scalar"][0]), "forward: the two routes differ | " + tag
        assert torch.equal(outs["vector"][1], outs["scalar"][1]), "backward: the two routes do not add in the same order | " + tag
        xd, = _to(dev, x)
        for act in (B.ACT_RELU, B.ACT_LEAKY):
            y = _Out((N, C, OH, OW), dev)
            lib.rg_reflection_pad2d_fwd(xd.data_ptr(), y.ptr, N, C, H, W, pad, act, B.SLOPE, _st())
            y.check(B.reflection_pad_fwd(x, pad, act, B.SLOPE), "rg_reflection_pad2d_fwd y | %s act %d" % (tag, act), "act %d" % act)
            ya = torch.empty_like(xd)
            lib.rg_act_fwd(xd.data_ptr(), ya.data_ptr(), x.numel(), act, B.SLOPE, _st())
            want = ya.cpu()[:, :, B.reflect_index(H, pad)][:, :, :, B.reflect_index(W, pad)]
            assert torch.equal(_bits(y.t), _bits(want)), "not pad(rg_act_fwd(x)) bit for bit, sign of zero included | %s act %d" % (tag, act)
            dx = _Out((N, C, H, W), dev)
            lib.rg_reflection_pad2d_bwd(gd.data_ptr(), xd.data_ptr(), dx.ptr, N, C, H, W, pad, act, B.SLOPE, _st())
            dx.check(B.reflection_pad_bwd(dy, H, W, pad, x, act, B.SLOPE), "rg_reflection_pad2d_bwd dx | %s act %d" % (tag, act), "act %d" % act)


@pytest.mark.parametrize("pad", range(5))
def test_reflection_pad(dev, pad):
    """pad 0..4; H of pad + 1, 2, 3, 9; W of 8, 12, 20 (vector route; pad 4 scalar) and 6, 9 (scalar); every vector geometry
    also on the scalar route through a one-float offset of x / dx, forward and backward bit for bit; ReLU / leaky folded in
    on the vector route with planted -0.0, negatives and -inf: pad(rg_act_fwd(x)) bit for bit"""
    for g in B.pad_geoms():
        if g[4] == pad:
            _pad_case(dev, *g)
    if pad == 1:
        _pad_case(dev, *B.PAD_BIG)                                    # N C OH OW past 8192 * 256
        x = _pad_input(2, 3, 9, 12, 1)
        y = _ops().reflection_pad2d_fwd(_to(dev, x)[0], 1, B.ACT_RELU, 0.0)
        B.check(y, B.reflection_pad_fwd(x, 1, B.ACT_RELU, 0.0), "ops.reflection_pad2d_fwd")


def _sn_call(dev, w, u, v, training, saved=True, eps=1e-12):
    """one rg_spectral_norm_fwd on fresh guarded buffers -> dict of _Out"""
    K, M = w.shape
    wd, = _to(dev, w)
    o = {"u": _Out((K,), dev, init=u), "v": _Out((M,), dev, init=v), "w_sn": _Out((K, M), dev), "sigma": _Out((2,), dev),
         "uv_saved": _Out((K + M,), dev) if saved else None}
    _lib().rg_spectral_norm_fwd(wd.data_ptr(), o["u"].ptr, o["v"].ptr, o["w_sn"].ptr, o["sigma"].ptr, _ptr(o["uv_saved"]), K, M,
                                training, eps, _st())
    return o


@pytest.mark.parametrize("i", range(len(T.sn_cases())), ids=lambda i: "%dx%d-train%d-%g" % T.sn_cases()[i])
def test_spectral_norm_fwd(dev, i):
    """(1, 1), (3, 27), (17, 65): the wave loop's second trip, (128, 2048), (1024, 64) and (8, 12288): the limits; training
    and eval; uv_saved given and NULL; W * 1e-14: both eps clamps bind"""
    K, M, training, scale = T.sn_cases()[i]
    w, u, v = B.sn_input(K, M, scale)
    ref = B.spectral_norm_fwd(w, u, v, training, 1e-12)
    for saved in (True, False):
        o = _sn_call(dev, w, u, v, training, saved)
        tag = "%s training %d scale %g saved %s" % ((K, M), training, scale, saved)
        for k in ("u", "v", "sigma", "w_sn", "uv_saved"):
            if o[k] is not None:
                o[k].check(ref[k], "rg_spectral_norm_fwd %s | %s" % (k, tag), "scale %g" % scale)


def test_spectral_norm_three_successive_forwards(dev):
    """u and v are updated in place: each forward is compared with the reference of the u, v the one before it left"""
    K, M = 17, 65
    w, u, v = B.sn_input(K, M)
    wd, = _to(dev, w)
    ub, vb = _Out((K,), dev, init=u), _Out((M,), dev, init=v)
    for step in range(3):
        ref = B.spectral_norm_fwd(w, u, v, 1, 1e-12)
        wsn, sig = _Out((K, M), dev), _Out((2,), dev)
        _lib().rg_spectral_norm_fwd(wd.data_ptr(), ub.ptr, vb.ptr, wsn.ptr, sig.ptr, None, K, M, 1, 1e-12, _st())
        for o, k in ((ub, "u"), (vb, "v"), (wsn, "w_sn"), (sig, "sigma")):
            o.check(ref[k], "rg_spectral_norm_fwd %s | forward %d of 3" % (k, step + 1), "plain")
        u, v = ub.t.cpu().clone(), vb.t.cpu().clone()
    w_sn, sigma = _ops().spectral_norm_fwd(wd, *_to(dev, *B.sn_input(K, M)[1:]))
    B.check(w_sn, B.spectral_norm_fwd(w, *B.sn_input(K, M)[1:], 1, 1e-12)["w_sn"], "ops.spectral_norm_fwd")


def test_spectral_norm_rejects_what_exceeds_one_workgroup(dev):
    """K = 1025 and M = 12289 return RG_ERR_INVALID before any launch and write nothing"""
    for K, M in ((B.SN_MAX_K + 1, 4), (2, B.SN_MAX_M + 1)):
        wd = torch.zeros(K * M, device=dev)
        o = [_Out((K,), dev), _Out((M,), dev), _Out((K * M,), dev), _Out((2,), dev), _Out((K + M,), dev)]
        with pytest.raises(RuntimeError, match=r"\(-1\)"):
            _lib().rg_spectral_norm_fwd(wd.data_ptr(), o[0].ptr, o[1].ptr, o[2].ptr, o[3].ptr, o[4].ptr, K, M, 1, 1e-12, _st())
        for t in o:
            t.untouched("rg_spectral_norm_fwd %d x %d" % (K, M))


def test_spectral_norm_multi_equals_the_single_calls(dev):
    """17 descriptors of mixed sizes: two batches (RG_SN_MAX_BATCH = 16); every output bit for bit the single call's"""
    ops = _ops()
    shapes = B.SN_MULTI[:B.SN_MAX_BATCH + 1]
    assert len(shapes) == 17
    for training in (1, 0):
        ins = [B.sn_input(K, M, seed=j) for j, (K, M) in enumerate(shapes)]
        single = [_sn_call(dev, w, u, v, training) for w, u, v in ins]
        keep = []
        descs = (ops._SNDesc * len(shapes))()
        multi = []
        for j, (w, u, v) in enumerate(ins):
            K, M = w.shape
            wd, = _to(dev, w)
            keep.append(wd)
            o = {"u": _Out((K,), dev, init=u), "v": _Out((M,), dev, init=v), "w_sn": _Out((K, M), dev), "sigma": _Out((2,), dev),
                 "uv_saved": _Out((K + M,), dev) if j % 2 == 0 else None}
            d = descs[j]
            d.w, d.u, d.v, d.w_sn, d.sigma, d.uv_saved, d.K, d.M = wd.data_ptr(), o["u"].ptr, o["v"].ptr, o["w_sn"].ptr, o["sigma"].ptr, _ptr(o["uv_saved"]), K, M
            multi.append(o)
        _lib().rg_spectral_norm_fwd_multi(ctypes.addressof(descs), len(shapes), training, 1e-12, _st())
        for j, (s, m) in enumerate(zip(single, multi)):
            for k in ("u", "v", "w_sn", "sigma", "uv_saved"):
                if m[k] is None:
                    continue
                m[k].guards("rg_spectral_norm_fwd_multi %s of descriptor %d" % (k, j))
                assert torch.equal(_bits(m[k].t), _bits(s[k].t)), "descriptor %d %s %s training %d: differs from the single call" % (
                    j, shapes[j], k, training)


def test_spectral_norm_bwd(dev):
    """K M = 16384 (one workgroup) and 16385 (slice partials); accumulate 0 and 1; a workspace one byte short"""
    lib = _lib()
    for K, M in B.SN_BWD_SHAPES:
        w, u, v = B.sn_input(K, M)
        f = B.spectral_norm_fwd(w, u, v, 1, 1e-12)
        wsn, sig, un, vn = (f[k].value.float() for k in ("w_sn", "sigma", "u", "v"))
        g = torch.randn(K, M, generator=B.gen(K))
        old = torch.randn(K, M, generator=B.gen(M))
        gd, wd, ud, vd, sd = _to(dev, g, wsn, un, vn, sig)
        nbytes = lib.rg_spectral_norm_bwd_workspace(K, M)
        assert nbytes == B.sn_workspace(K, M)
        for acc in (0, 1):
            ws = _Out((max(nbytes // 4, 1),), dev)
            dw = _Out((K, M), dev, init=old)
            lib.rg_spectral_norm_bwd(gd.data_ptr(), wd.data_ptr(), ud.data_ptr(), vd.data_ptr(), sd.data_ptr(), dw.ptr, K, M, acc,
                                     ws.ptr if nbytes else None, nbytes, _st())
            dw.check(B.spectral_norm_bwd(g, wsn, un, vn, sig, old if acc else None),
                     "rg_spectral_norm_bwd dw | %s %s accumulate %d" % ((K, M), B.sn_bwd_kernel(K, M), acc), "plain")
            ws.guards("rg_spectral_norm_bwd workspace")
        if nbytes:
            ws, dw = _Out((nbytes // 4,), dev), _Out((K, M), dev)
            with pytest.raises(RuntimeError, match=r"\(-3\)"):
                lib.rg_spectral_norm_bwd(gd.data_ptr(), wd.data_ptr(), ud.data_ptr(), vd.data_ptr(), sd.data_ptr(), dw.ptr, K, M, 0,
                                         ws.ptr, nbytes - 1, _st())
            dw.untouched("dw after the workspace error")
            ws.untouched("workspace after the workspace error")


# ---- bgemm.hip -----------------------------------------------------------------------------------------------------------------
def test_bgemm(dev):
    """M, N of 1, 31, 33, 64, 65, 130; K of 1, 15, 16, 17, 33; the four (a_rc, b_rc) load mappings; a transposed C; 3 x 2
    batches; (alpha, beta) of (1, 0), (0.5, 2) and (1, 0) on a C full of NaN, which beta == 0 must not read"""
    lib = _lib()
    for i, (M, N, K, a_rc, b_rc, c_t, batch, alpha, beta, nan_c) in enumerate(B.bgemm_cases()):
        fam = T.FAMS[i % 4]
        A, Bm, C, a_s, b_s, c_s, a_b, b_b, c_b = B.bgemm_operands(M, N, K, a_rc, b_rc, c_t, batch, fam)
        if nan_c:
            C = torch.full_like(C, float("nan"))
        Ad, Bd = _to(dev, A, Bm)
        out = _Out(tuple(C.shape), dev, init=C)
        lib.rg_bgemm(Ad.data_ptr(), Bd.data_ptr(), out.ptr, M, N, K, a_s[0], a_s[1], b_s[0], b_s[1], c_s[0], c_s[1], batch[0], batch[1],
                     a_b[0], a_b[1], b_b[0], b_b[1], c_b[0], c_b[1], alpha, beta, _st())
        ref = B.bgemm(A, Bm, C, M, N, K, a_s, b_s, c_s, batch, a_b, b_b, c_b, alpha, beta)
        assert bool(torch.isfinite(ref.value).all())
        out.check(ref, "rg_bgemm C | %s" % ((M, N, K, a_rc, b_rc, c_t, batch, alpha, beta, nan_c),), fam)
    # heads as channel offsets: [B][heads * dh][L] maps, scores[b][h] = Q_h^T K_h (the strides of the attention blocks)
    Bn, heads, dh, L = 3, 2, 20, 35
    q, k = B.family((Bn * heads * dh * L,), "plain", B.gen(1)), B.family((Bn * heads * dh * L,), "plain", B.gen(2))
    S = torch.zeros(Bn * heads * L * L)
    args = (L, L, dh, (1, L), (L, 1), (L, 1), (Bn, heads), (heads * dh * L, dh * L), (heads * dh * L, dh * L), (heads * L * L, L * L))
    qd, kd = _to(dev, q, k)
    out = _Out((S.numel(),), dev, init=S)
    _ops().bgemm(qd, kd, out.t, *args, alpha=0.25)
    out.check(B.bgemm(q, k, S, *args, 0.25, 0.0), "ops.bgemm scores | heads as channel offsets", "plain")


def test_softmax_rows(dev):
    """cols of 1, 63, 64, 65, 200; rows 1 and 5 (a partly empty second workgroup); scale positive, negative and 0; a row of
    equal values, a row of +-80; in place for both directions"""
    lib = _lib()
    for rows in B.SOFTMAX_ROWS:
        for i, cols in enumerate(B.SOFTMAX_COLS):
            for j, sc in enumerate(B.SOFTMAX_SCALES):
                fam = T.FAMS[(i + j) % 4]
                x = B.softmax_input(rows, cols, fam)
                dp = B.family((rows, cols), "plain", B.gen(cols))
                rp = B.softmax_fwd(x, sc)
                p = rp.value.float()
                rd = B.softmax_bwd(p, dp, sc)
                xd, pd, gd = _to(dev, x, p, dp)
                tag = "%s scale %g %s" % ((rows, cols), sc, fam)
                for inplace in (False, True):
                    y = _Out((rows, cols), dev, init=x if inplace else None)
                    lib.rg_softmax_rows_fwd(y.ptr if inplace else xd.data_ptr(), y.ptr, rows, cols, sc, _st())
                    y.check(rp, "rg_softmax_rows_fwd y | %s in place %s" % (tag, inplace), fam)
                    ds = _Out((rows, cols), dev, init=dp if inplace else None)
                    lib.rg_softmax_rows_bwd(pd.data_ptr(), ds.ptr if inplace else gd.data_ptr(), ds.ptr, rows, cols, sc, _st())
                    ds.check(rd, "rg_softmax_rows_bwd ds | %s in place %s" % (tag, inplace), fam)
    x = B.softmax_input(5, 65, "plain")
    B.check(_ops().softmax_rows_fwd(_to(dev, x)[0], 0.125), B.softmax_fwd(x, 0.125), "ops.softmax_rows_fwd")


# ---- resize.hip ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(T.bicubic_cases())), ids=lambda i: "%d-%d-%s-%s-%s" % T.bicubic_cases()[i])
def test_bicubic_normalize(dev, i):
    """integer and non-integer up-sampling, H = W = 1, the copy path, down-sampling, OH == H with OW != W; mean / std given
    (three different std) and NULL; stdv NULL in the backward; the forward's and the backward's loop on the second trip"""
    lib = _lib()
    N, C, (H, W), (OH, OW), on = T.bicubic_cases()[i]
    fam = "plain" if N > 100 else T.FAMS[(H + OW) % 4]
    x = B.family((N, C, H, W), fam, B.gen(H * OW))
    dy = B.family((N, C, OH, OW), "plain", B.gen(OH))
    mean, std = T.mean_std(C, on)
    xd, gd, md, sd = _to(dev, x, dy, mean, std)
    tag = "%s" % ((N, C, H, W, OH, OW, on),)
    y = _Out((N, C, OH, OW), dev)
    lib.rg_bicubic_normalize_fwd(xd.data_ptr(), y.ptr, N, C, H, W, OH, OW, _ptr(md), _ptr(sd), _st())
    y.check(B.bicubic_fwd(x, OH, OW, mean, std), "rg_bicubic_normalize_fwd y | " + tag, fam)
    dx = _Out((N, C, H, W), dev)
    lib.rg_bicubic_normalize_bwd(gd.data_ptr(), dx.ptr, N, C, H, W, OH, OW, _ptr(sd), _st())
    dx.check(B.bicubic_bwd(dy, H, W, std), "rg_bicubic_normalize_bwd dx | " + tag, "plain")
    if i == 2:
        B.check(_ops().bicubic_normalize_fwd(xd, (OH, OW), md, sd), B.bicubic_fwd(x, OH, OW, mean, std), "ops.bicubic_normalize_fwd")


# ---- retrieval.hip -------------------------------------------------------------------------------------------------------------
def test_topk_rows(dev):
    """cols of 1, 255, 257, 1000; k of 1, 7 and cols; duplicated values, all-equal rows, +-inf, 0.0 beside -0.0: indices and
    values exact, in faiss order"""
    lib = _lib()
    for cols in B.TOPK_COLS:
        x = B.topk_input(cols)
        xd, = _to(dev, x)
        rows = x.shape[0]
        for k in B.topk_ks(cols):
            idx, val = _Out((rows, k), dev, dtype=torch.int32, fill=-7777), _Out((rows, k), dev)
            lib.rg_topk_rows(xd.data_ptr(), rows, cols, k, idx.ptr, val.ptr, _st())
            ri, rv = B.topk_rows(x, k)
            idx.check(ri, "rg_topk_rows idx | cols %d k %d" % (cols, k), "ties")
            val.check(rv, "rg_topk_rows val | cols %d k %d" % (cols, k), "ties")
    x = B.topk_input(257)
    got = _ops().topk_rows(_to(dev, x)[0], 7)
    B.check(got[0], B.topk_rows(x, 7)[0], "ops.topk_rows idx")


def test_row_sqsum_and_outer_terms(dev):
    """D of 1, 63, 65, 2048, rows 1 and 6 (a partly empty workgroup); rowv / colv each given and NULL, alpha 0 and 1, rows x
    cols past 8192 * 256 with cols no power of two"""
    lib = _lib()
    for rows in B.SQSUM_ROWS:
        for i, D in enumerate(B.SQSUM_D):
            fam = T.FAMS[(i + rows) % 4]
            x = B.family((rows, D), fam, B.gen(D))
            out = _Out((rows,), dev)
            lib.rg_row_sqsum(_to(dev, x)[0].data_ptr(), out.ptr, rows, D, _st())
            out.check(B.row_sqsum(x), "rg_row_sqsum out | %s" % ((rows, D),), fam)
    for r, c, rv, cv, al in T.outer_cases():
        m = B.family((r, c), "plain", B.gen(r))
        row = B.family((r,), "scales", B.gen(r + 1)) if rv else None
        col = B.family((c,), "offset", B.gen(c)) if cv else None
        rd, cd = _to(dev, row, col)
        out = _Out((r, c), dev, init=m)
        lib.rg_add_outer_terms(out.ptr, _ptr(rd), _ptr(cd), al, 1.0, -2.0, r, c, _st())
        out.check(B.add_outer_terms(m, row, col, al, 1.0, -2.0), "rg_add_outer_terms m | %s" % ((r, c, rv, cv, al),), "plain")


def test_segment_mean(dev):
    """segments of 1, 2 and 300 members, a non-monotone order with repeats, D of 1, 256, 300; within the budget, and bit for
    bit the float32 sum in list order"""
    lib = _lib()
    for D in B.SEG_D:
        x, order, offsets = B.segment_input(D)
        xd, od, fd = _to(dev, x, order, offsets)
        out = _Out((len(B.SEG_SIZES), D), dev)
        lib.rg_segment_mean(xd.data_ptr(), od.data_ptr(), fd.data_ptr(), out.ptr, len(B.SEG_SIZES), D, _st())
        out.check(B.segment_mean(x, order, offsets), "rg_segment_mean out | D %d" % D, "plain")
        out.check(B.segment_mean_f32(x, order, offsets), "rg_segment_mean out, list order | D %d" % D, "exact")
    x, order, offsets = B.segment_input(256)
    B.check(_ops().segment_mean(*_to(dev, x, order, offsets)), B.segment_mean(x, order, offsets), "ops.segment_mean")
