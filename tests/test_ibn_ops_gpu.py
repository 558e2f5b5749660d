"""The fused IBN layer (rg_ibn_fwd / rg_ibn_bwd: InstanceNorm on channels [0, half), BatchNorm on [half, C) of one tensor)
against torch in fp64: cat(instance_norm(x[:, :half]), batch_norm(x[:, half:])) — output, saved statistics, dx, the four affine
gradients and the running statistics, for every launch regime of the entry points; the pre-masked-gradient path of the module;
run-to-run bits; and the allocation bound that separates the fused layer (y or dx only) from any slice / cat composition.

Tolerances are those of test_ops_gpu.test_instance_norm_single_launch: 2e-5 of the reference tensor's largest entry for forward
values, 5e-5 for gradients."""
import pytest
import torch
import torch.nn.functional as F

from tests.test_ops_gpu import _close

pytestmark = pytest.mark.gpu

# (N, C, H, W)
SHAPES = [
    (2, 5, 3, 3),        # odd planes: IN 2 / BN 3, HW 9, scalar loads
    (3, 6, 7, 9),        # HW 63, not a multiple of 4
    (1, 8, 4, 2),        # N = 1, HW 8: the layer-3 map of a 64 x 32 crop
    (2, 64, 64, 32),     # layer-1 geometry, small BN extent: one launch in train mode
    (9, 64, 64, 32),     # N*HW = 18 432: beyond the one-launch BN regime, slice-parallel statistics / sums
    (4, 128, 32, 16),    # HW 512
    (4, 256, 16, 8),     # HW 128, 128 BN channels
    (2, 2, 256, 128),    # HW 32 768: one workgroup per row
    # register rows that do not fill their lanes (N*C leaves the last workgroup partly empty)
    (3, 6, 4, 5),        # HW 20 = 5 float4: 16 lanes x 2 units, most lanes empty
    (3, 6, 11, 12),      # HW 132 = 33 float4: 32 lanes x 2 units, the second unit on one lane
    (3, 6, 13, 20),      # HW 260 = 65 float4: 64 lanes x 2 units, ragged
    (3, 6, 12, 43),      # HW 516 = 129 float4: 64 lanes x 8 units, ragged
    (2, 4, 27, 76),      # HW 2052 = 513 float4: 256 lanes x 8 units, ragged, one launch in train mode
    (9, 4, 27, 76),      # the same rows with N*HW = 18 468: slice-parallel statistics, train-mode BN rows in the rows kernel
]
EPS, MOM = 1e-5, 0.1


def _case(shape, seed=33):
    g = torch.Generator().manual_seed(seed)
    N, C = shape[:2]
    half = int(C / 2)
    cb = C - half
    c = dict(half=half,
             x=torch.randn(shape, generator=g) * 1.7 + 0.3,
             dy=torch.randn(shape, generator=g),
             in_w=torch.rand(half, generator=g) + 0.5, in_b=torch.randn(half, generator=g),
             bn_w=torch.rand(cb, generator=g) + 0.5, bn_b=torch.randn(cb, generator=g),
             rm=torch.randn(cb, generator=g) * 0.3, rv=torch.rand(cb, generator=g) * 0.4 + 0.8)
    return c


def _reference(c, train, relu):
    """fp64 torch on the CPU -> dict of every quantity the layer produces"""
    half = c["half"]
    x = c["x"].double().requires_grad_(True)
    p = {k: c[k].double().requires_grad_(True) for k in ("in_w", "in_b", "bn_w", "bn_b")}
    rm, rv = c["rm"].double().clone(), c["rv"].double().clone()
    a = F.instance_norm(x[:, :half], weight=p["in_w"], bias=p["in_b"], eps=EPS)
    b = F.batch_norm(x[:, half:], rm, rv, p["bn_w"], p["bn_b"], training=train, momentum=MOM, eps=EPS)
    y = torch.cat((a, b), 1)
    if relu:
        y = F.relu(y)
    y.backward(c["dy"].double())
    xi, xb = c["x"].double()[:, :half].flatten(2), c["x"].double()[:, half:].transpose(0, 1).flatten(1)
    out = dict(y=y.detach(), dx=x.grad, rm=rm, rv=rv,
               in_mean=xi.mean(2).flatten(), in_invstd=(xi.var(2, unbiased=False) + EPS).rsqrt().flatten(),
               bn_mean=xb.mean(1), bn_invstd=(xb.var(1, unbiased=False) + EPS).rsqrt())
    out.update({"d_" + k: v.grad for k, v in p.items()})
    return out


def _run(ops, c, dev, train, relu):
    d = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in c.items()}
    rm, rv = d["rm"].clone(), d["rv"].clone()
    act = ops.ACT_RELU if relu else ops.ACT_NONE
    y, in_mean, in_invstd, bn_mean, bn_invstd = ops.ibn_fwd(d["x"], d["half"], d["in_w"], d["in_b"], d["bn_w"], d["bn_b"], rm, rv,
                                                            train, EPS, EPS, MOM, act=act)
    stat = (bn_mean, bn_invstd) if train else (rm, rv)
    dx, dgi, dbi, dgb, dbb = ops.ibn_bwd(d["x"], d["dy"], y if relu else None, d["half"], in_mean, in_invstd, stat[0], stat[1],
                                         d["in_w"], d["bn_w"], train, EPS, act)
    return dict(y=y, dx=dx, rm=rm, rv=rv, in_mean=in_mean, in_invstd=in_invstd, bn_mean=bn_mean, bn_invstd=bn_invstd,
                d_in_w=dgi, d_in_b=dbi, d_bn_w=dgb, d_bn_b=dbb)


@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("relu", [False, True], ids=["none", "relu"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_ibn_layer_matches_fp64(dev, shape, relu, train):
    from rg_hip import ops
    c = _case(shape)
    ref = _reference(c, train, relu)
    got = _run(ops, c, dev, train, relu)
    for k in ("y", "in_mean", "in_invstd", "rm", "rv"):
        _close(got[k], ref[k], name=k)
    if train:
        _close(got["bn_mean"], ref["bn_mean"], name="bn_mean")
        _close(got["bn_invstd"], ref["bn_invstd"], name="bn_invstd")
    else:
        assert torch.equal(got["rm"].cpu(), c["rm"]) and torch.equal(got["rv"].cpu(), c["rv"]), "eval mode updated the running statistics"
    for k in ("dx", "d_in_w", "d_in_b", "d_bn_w", "d_bn_b"):
        _close(got[k], ref[k], tol=5e-5, name=k)
    again = _run(ops, c, dev, train, relu)
    for k, v in got.items():
        if v is not None:
            assert torch.equal(v, again[k]), "%s differs between two calls" % k


def test_ibn_rejects_residual_and_bad_split(dev):
    from rg_hip import ops
    c = _case((2, 6, 4, 4))
    d = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in c.items()}
    with pytest.raises(RuntimeError, match="residual"):
        ops.ibn_fwd(d["x"], 3, d["in_w"], d["in_b"], d["bn_w"], d["bn_b"], d["rm"], d["rv"], True, residual=d["dy"])
    with pytest.raises(RuntimeError, match="split"):
        ops.ibn_fwd(d["x"], 6, d["in_w"], d["in_b"], d["bn_w"], d["bn_b"], d["rm"], d["rv"], True)


def _module(dev, planes, c):
    from rg_hip import nn as rnn
    m = rnn.IBN(planes).to(dev)
    with torch.no_grad():
        m.IN.weight.copy_(c["in_w"]), m.IN.bias.copy_(c["in_b"]), m.BN.weight.copy_(c["bn_w"]), m.BN.bias.copy_(c["bn_b"])
        m.BN.running_mean.copy_(c["rm"]), m.BN.running_var.copy_(c["rv"])
    return m


@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("shape", [(3, 6, 7, 9), (9, 64, 64, 32)], ids=lambda s: "x".join(map(str, s)))
def test_ibn_module_premasked_gradient(dev, shape, train):
    """IBN.tb(dy_masked=True): the consumer's dgrad already applied the ReLU mask, so the forward output is not read (it is
    overwritten with NaN here) and the results are those of the unmasked call; gradients arrive through the tape; the BN child
    counts its batches on the host."""
    from rg_hip import ops
    from rg_hip.tape import Tape
    c = _case(shape)
    ref = _reference(c, train, True)
    x, dy = c["x"].to(dev), c["dy"].to(dev)
    outs = []
    for masked in (False, True):
        m = _module(dev, shape[1], c).train(train)
        tape = Tape()
        y = m.tf(tape, x, act=ops.ACT_RELU)
        g = dy
        if masked:
            g = dy * (y > 0).float()
            y.fill_(float("nan"))
        dx = m.tb(tape, g, dy_masked=masked)
        assert not tape.stack
        grads = [tape.grads[id(p)] for p in (m.IN.weight, m.IN.bias, m.BN.weight, m.BN.bias)]
        outs.append([dx] + grads)
        assert int(m.BN.num_batches_tracked) == (1 if train else 0)
        assert sorted(m.state_dict()) == ["BN.bias", "BN.num_batches_tracked", "BN.running_mean", "BN.running_var", "BN.weight",
                                          "IN.bias", "IN.weight"]
    for k, a, b in zip(("dx", "d_in_w", "d_in_b", "d_bn_w", "d_bn_b"), outs[0], outs[1]):
        _close(a, ref[k], tol=5e-5, name=k)
        assert torch.equal(a, b), "%s: pre-masked gradient gives other bits" % k


@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
def test_ibn_allocates_one_activation_per_direction(dev, train):
    """The fused layer writes y (forward) and dx (backward) and nothing else of the activation's size: 1 x the bytes of x plus the
    statistics.  Any composition of slice copies, two norms and a concatenation holds at least 2 x (the halves and the result)."""
    from rg_hip import ops
    from rg_hip.tape import Tape
    shape = (8, 64, 64, 32)
    c = _case(shape)
    m = _module(dev, shape[1], c).train(train)
    x, dy = c["x"].to(dev), c["dy"].to(dev)
    limit = 1.25 * x.numel() * 4

    def one(measure):
        tape = Tape()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        y = m.tf(tape, x, act=ops.ACT_RELU)
        torch.cuda.synchronize()
        fwd = torch.cuda.max_memory_allocated() - base
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        dx = m.tb(tape, dy)
        torch.cuda.synchronize()
        bwd = torch.cuda.max_memory_allocated() - base
        if measure:
            print("IBN %s: forward allocates %.3f x, backward %.3f x the bytes of x" % (shape, fwd / (x.numel() * 4.0), bwd / (x.numel() * 4.0)))
            assert fwd <= limit, "forward peak %d bytes > 1.25 x %d" % (fwd, x.numel() * 4)
            assert bwd <= limit, "backward peak %d bytes > 1.25 x %d" % (bwd, x.numel() * 4)
        del y, dx

    one(False)        # warm-up: the library's workspace is allocated here
    one(True)
