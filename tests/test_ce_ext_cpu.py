"""CPU: tests/ce_ext_hostmodel.py against torch's own F.cross_entropy and autograd in fp64 on every shape of the GPU test, and the
new entry points in the public header."""
import pytest
import torch
import torch.nn.functional as F

from tests import ce_ext_hostmodel as H
from tests import head_hostmodel as HH

CASES = [(t, g, m) for t, g in H.TG for m in H.MS]


def _torch_ref(la, lb, labels, grow, group, mask, scale):
    """F.cross_entropy(cat([la, lb + mask_matrix], 1) * scale, reduction='none') in fp64 — the sum lb + mask_matrix is the float32
    addition of the definition — and the gradients of sum(grow * loss) to the two blocks (through the float32 addition: its
    derivative is 1)"""
    n, t = lb.shape
    m = la.shape[1]
    z = torch.cat([la, lb + H.mask_matrix(n, t, group, mask)], 1).double().requires_grad_(True)
    ok = HH.in_range(labels, m + t)
    loss = F.cross_entropy(z * HH.f32(scale), torch.where(ok, labels, torch.full_like(labels, -100)), reduction='none')
    (loss * grow.double()).sum().backward()
    return loss.detach(), z.grad[:, :m], z.grad[:, m:]


@pytest.mark.parametrize("t,group,m", CASES, ids=lambda v: str(v))
def test_host_model_is_torch_cross_entropy_in_fp64(t, group, m):
    la, lb, labels, grow = H.case(t, group, m)
    loss, dla, dlb = _torch_ref(la, lb, labels, grow, group, H.MASK, H.SCALE)
    f = H.fwd(la, lb, labels, group, H.MASK, H.SCALE)
    assert torch.allclose(f["loss"].value, loss, rtol=1e-12, atol=1e-12)
    ra, rb = H.bwd(la, lb, labels, f["lse"].value, grow, 1.0, group, H.MASK, H.SCALE)
    # the model is handed lse and exponentiates z - lse; torch subtracts the maximum first: a few fp64 roundings of |z| ~ 1600
    assert torch.allclose(ra.value, dla, rtol=1e-9, atol=1e-12)
    assert torch.allclose(rb.value, dlb, rtol=1e-9, atol=1e-12)
    # the masked column: probability and gradient exactly zero, in the model as in torch's fp64
    n = t * group
    rows = torch.arange(n)
    assert bool((rb.value[rows, rows // group] == 0).all()) and bool((dlb[rows, rows // group] == 0).all())
    # rows of a label out of range: loss and both gradient rows exactly zero
    out = ~HH.in_range(labels, m + t)
    assert bool((f["loss"].value[out] == 0).all()) and bool((ra.value[out] == 0).all()) and bool((rb.value[out] == 0).all())
    assert bool((f["loss"].M[out] == 0).all()) and bool((ra.M[out] == 0).all())


def test_planted_rows_are_what_they_claim():
    la, lb, labels, _ = H.case(16, 16, 257)
    assert float(la[0].abs().min()) == 80.0 and bool((la[1] == la[1, 0]).all())
    assert 257 <= int(labels[2]) < 257 + 16 and int(labels[2]) - 257 != 2 // 16
    assert int(labels[3]) == 257 + 16 and int(labels[4]) == -1
    assert float(lb[5, 0]) == 3.0 and float(torch.cat([la[5], lb[5]]).max()) == 3.0
    f = H.fwd(la, lb, labels, 16, H.MASK, H.SCALE)
    assert bool(torch.isfinite(f["lse"].value).all())
    # the budget of a row is not widened by its dead masked column
    assert float(f["lse"].M[5]) < 100.0


def test_grad_rows_none_is_ones_and_gscale_multiplies():
    la, lb, labels, grow = H.case(4, 4, 7)
    lse = H.fwd(la, lb, labels, 4, H.MASK, H.SCALE)["lse"].value
    a1, b1 = H.bwd(la, lb, labels, lse, None, 0.7, 4, H.MASK, H.SCALE)
    a2, b2 = H.bwd(la, lb, labels, lse, torch.ones(16), 0.7, 4, H.MASK, H.SCALE)
    assert torch.equal(a1.value, a2.value) and torch.equal(b1.value, b2.value)
    a3, _ = H.bwd(la, lb, labels, lse, None, 1.0, 4, H.MASK, H.SCALE)
    assert torch.allclose(a1.value, a3.value * HH.f32(0.7), rtol=1e-15, atol=0)


def test_entry_points_are_declared():
    from rg_hip.lib import parse_header
    protos = parse_header()
    fwd = [t for t, _ in protos["rg_softmax_ce_ext_fwd"][1]]
    bwd = [t for t, _ in protos["rg_softmax_ce_ext_bwd"][1]]
    assert fwd == ["const float*", "const float*", "const int64_t*", "float*", "float*", "int", "int", "int", "int", "float", "float",
                   "rg_stream_t"]
    assert bwd == ["const float*", "const float*", "const int64_t*", "const float*", "const float*", "float", "float*", "float*",
                   "int", "int", "int", "int", "float", "float", "rg_stream_t"]


def test_wrapper_refuses_rows_that_are_not_whole_groups():
    """n != t * group is a ValueError on the host, before the library is touched (no GPU needed)"""
    from rg_hip.ops.loss import _ce_ext_shape
    assert _ce_ext_shape(torch.zeros(8, 5), torch.zeros(8, 4), 2) == (8, 5, 4)
    for n, t, group in ((6, 2, 4), (8, 4, 0), (8, 3, 2)):
        with pytest.raises(ValueError):
            _ce_ext_shape(torch.zeros(n, 5), torch.zeros(n, t), group)
