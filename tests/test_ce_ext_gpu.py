"""GPU: rg_softmax_ce_ext_fwd / rg_softmax_ce_ext_bwd (csrc/loss.hip) per element against the fp64 host model
(tests/ce_ext_hostmodel.py) through the C ABI, every output between two rows of guard values, every element compared, two runs
byte-equal; then the memory the fused path of ClusterMemory_Gradient.forward(ex_f=...) needs.

Shapes: (t, group) in {(1,1), (2,2), (4,4), (3,5), (16,16)} x m in {1, 7, 64, 257, 1500}: with n = t * group the boundary between
the two blocks falls inside a wave, at a wave edge and past the first trip of the 256-thread loop, and the rows of lb (t floats)
start off every vector alignment.  Planted rows: see ce_ext_hostmodel.case.  The backward is handed the rounded reference lse.

Each check prints `RATIO <entry point> <output> <family> <max err / (2^-24 M)>` (pytest -s shows them;
profiles/ce_ext_elementwise_ratios.txt keeps the worst per entry point and output)."""
import pytest
import torch

from tests import ce_ext_hostmodel as H
from tests import head_hostmodel as HH
from tests.test_head_elementwise_gpu import _Out, _lib, _ptr, _st, _to

pytestmark = pytest.mark.gpu


def _check(out, ref, what, fam="planted"):
    out.guards(what)
    w = HH.compare(out.t, ref)
    assert w.ok, "%s: worst element %s err %.3e > budget %.3e (%s, max err/(2^-24 M) = %.2f)" % (
        what, w.index, w.err, w.budget, ref.kind, w.ratio)
    print("RATIO %s %s %.3f" % (what.split(" | ")[0], fam, w.ratio))


def _run_fwd(dev, lad, lbd, yd, n, m, t, group):
    loss, lse = _Out((n,), dev), _Out((n,), dev)
    _lib().rg_softmax_ce_ext_fwd(lad.data_ptr(), lbd.data_ptr(), yd.data_ptr(), loss.ptr, lse.ptr, n, m, t, group, H.MASK, H.SCALE,
                                 _st())
    return loss, lse


def _run_bwd(dev, lad, lbd, yd, ld, gd, gscale, n, m, t, group):
    dla, dlb = _Out((n, m), dev), _Out((n, t), dev)
    _lib().rg_softmax_ce_ext_bwd(lad.data_ptr(), lbd.data_ptr(), yd.data_ptr(), ld.data_ptr(), _ptr(gd), gscale, dla.ptr, dlb.ptr,
                                 n, m, t, group, H.MASK, H.SCALE, _st())
    return dla, dlb


@pytest.mark.parametrize("m", H.MS)
@pytest.mark.parametrize("t,group", H.TG, ids=lambda v: str(v))
def test_ce_ext(dev, t, group, m):
    n = t * group
    la, lb, labels, grow = H.case(t, group, m)
    tag = "t %d group %d m %d" % (t, group, m)
    lad, lbd, yd, gd = _to(dev, la, lb, labels, grow)
    # lb rows off every vector alignment: the block is handed at an odd float offset as well
    lb_off = torch.empty(n * t + 1, device=dev)[1:].view(n, t).copy_(lbd)
    f = H.fwd(la, lb, labels, group, H.MASK, H.SCALE)
    for name, b in (("", lbd), (" (lb + 4 bytes)", lb_off)):
        loss, lse = _run_fwd(dev, lad, b, yd, n, m, t, group)
        _check(loss, f["loss"], "rg_softmax_ce_ext_fwd loss | " + tag + name)
        _check(lse, f["lse"], "rg_softmax_ce_ext_fwd lse | " + tag + name)
        loss2, lse2 = _run_fwd(dev, lad, b, yd, n, m, t, group)
        assert torch.equal(loss.buf, loss2.buf) and torch.equal(lse.buf, lse2.buf), "rg_softmax_ce_ext_fwd: two runs differ | " + tag
    lse32 = f["lse"].value.float()
    ld, = _to(dev, lse32)
    rows = torch.arange(n)
    for g, gt, gscale in ((gd, grow, 0.7), (None, None, 1.0 / n)):          # grad_rows given and NULL
        ra, rb = H.bwd(la, lb, labels, lse32, gt, gscale, group, H.MASK, H.SCALE)
        which = "given" if g is not None else "NULL"
        dla, dlb = _run_bwd(dev, lad, lbd, yd, ld, g, gscale, n, m, t, group)
        _check(dla, ra, "rg_softmax_ce_ext_bwd dla | %s grad_rows %s" % (tag, which))
        _check(dlb, rb, "rg_softmax_ce_ext_bwd dlb | %s grad_rows %s" % (tag, which))
        # the masked column: exactly 0.0f ((x - 10000) * 20 underflows expf), also where it holds the row's largest raw logit
        assert bool((dlb.t[rows, rows // group] == 0).all()), "masked column has a gradient | " + tag
        dla2, dlb2 = _run_bwd(dev, lad, lbd, yd, ld, g, gscale, n, m, t, group)
        assert torch.equal(dla.buf, dla2.buf) and torch.equal(dlb.buf, dlb2.buf), "rg_softmax_ce_ext_bwd: two runs differ | " + tag


def test_ops_wrappers_and_shape_error(dev):
    """the rg_hip.ops wrappers on one shape, and n != t * group refused on the host"""
    from rg_hip import ops
    t, group, m = 3, 5, 257
    la, lb, labels, grow = H.case(t, group, m)
    lad, lbd, yd, gd = _to(dev, la, lb, labels, grow)
    f = H.fwd(la, lb, labels, group, H.MASK, H.SCALE)
    loss, lse = ops.softmax_ce_ext_fwd(lad, lbd, yd, group, H.MASK, H.SCALE)
    HH.check(loss, f["loss"], "ops.softmax_ce_ext_fwd loss")
    HH.check(lse, f["lse"], "ops.softmax_ce_ext_fwd lse")
    lse32 = f["lse"].value.float()
    ra, rb = H.bwd(la, lb, labels, lse32, grow, 0.7, group, H.MASK, H.SCALE)
    dla, dlb = ops.softmax_ce_ext_bwd(lad, lbd, yd, lse32.to(dev), gd, group, H.MASK, H.SCALE, 0.7)
    HH.check(dla, ra, "ops.softmax_ce_ext_bwd dla")
    HH.check(dlb, rb, "ops.softmax_ce_ext_bwd dlb")
    with pytest.raises(ValueError):
        ops.softmax_ce_ext_fwd(lad, lbd, yd, 4, H.MASK, H.SCALE)
    with pytest.raises(RuntimeError, match="t \\* group"):           # the C ABI refuses it too, before any launch
        out = _Out((15,), dev)
        _lib().rg_softmax_ce_ext_fwd(lad.data_ptr(), lbd.data_ptr(), yd.data_ptr(), out.ptr, out.ptr, 15, m, t, 4, H.MASK, H.SCALE,
                                     _st())


def _requested(what):
    """bytes the code asked the allocator for (torch's `requested_bytes`): `allocated_bytes` also counts the unsplit remainder of a
    cached block an allocation is served from — up to 1 MB per large tensor, depending on what ran before in the process"""
    return torch.cuda.memory_stats()["requested_bytes.all." + what]


def test_cluster_memory_gradient_ex_f_allocates_no_mask_and_no_concatenation(dev):
    """forward + backward of ClusterMemory_Gradient.forward(ex_f=...) at n = 256, m = 1500, t = 16: the peak of requested memory
    above the inputs stays below

        the two logit blocks + the two gradient blocks + the [n, D] tensors + 64 KB

    where the [n, D] tensors are the normalised inputs the forward keeps, the two data gradients of the GEMMs, their sum and the
    gradient handed to the caller (5 n D floats) and the 64 KB cover the normalised ex_f [t, D], the O(n) vectors (norms, loss
    rows, lse, row gradients).  D = 64 keeps the [n, D] tensors (64 KB each) far below one
    [n, m + t] buffer (1.55 MB).

    That bound alone separates nothing: autograd frees the first logit block as soon as the concatenation has copied it, and the
    concatenated gradient dies before its slices are all that is left, so the composition this path replaced (eye /
    repeat_interleave / add / cat, two slices in backward) peaks at 3 191 808 bytes, this path at 3 177 480, the bound is
    3 497 984.  What the composition cannot do is the FORWARD in the memory of the two blocks: while it concatenates it holds the
    blocks and their copy.  So the forward alone must stay below the two logit blocks + the normalised inputs + 64 KB (1 683 456
    bytes; the old composition: see profiles/ce_ext_elementwise_ratios.txt)."""
    from clustercontrast.models.cm import ClusterMemory_Gradient
    n, m, t, D = 256, 1500, 16, 64
    g = HH.gen(7)
    mem = ClusterMemory_Gradient(D, m, temp=0.05)
    mem.set_clusters(torch.randn(m, D, generator=g).to(dev), 0.1)
    x = torch.randn(n, D, generator=g).to(dev).requires_grad_(True)
    ex = torch.randn(t, D, generator=g).to(dev)
    labels = torch.randint(0, m, (n,), generator=g).to(dev)
    mem(x, labels, ex_f=ex).backward()               # warm-up: workspaces, the library's lazy state
    x.grad = None
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = _requested("current")
    blocks = 4 * n * (m + t)
    loss = mem(x, labels, ex_f=ex)
    torch.cuda.synchronize()
    fwd_peak = _requested("peak") - base
    fwd_bound = blocks + n * D * 4 + 64 * 1024
    print("ce_ext forward peak above the inputs %d bytes, bound %d" % (fwd_peak, fwd_bound))
    assert fwd_peak < fwd_bound, (fwd_peak, fwd_bound)
    loss.backward()
    torch.cuda.synchronize()
    peak = _requested("peak") - base
    bound = 2 * blocks + 5 * n * D * 4 + 64 * 1024
    print("ce_ext peak above the inputs %d bytes, bound %d, one [n, m + t] buffer %d" % (peak, bound, blocks))
    assert peak < bound, (peak, bound)
    assert x.grad is not None and bool(torch.isfinite(loss))
