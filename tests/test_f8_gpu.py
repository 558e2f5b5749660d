"""The fp8 convolution family (csrc/conv_f8.hip, rg_hip/lowp.py; BASELINE config 5) on the MI355X.

Three levels:
 1. the quantiser is BIT-EXACT against the CPU emulation (oracle/ref_fp8.py): same bytes in both operand layouts and both
    formats, zero padding, same dequantisation scale, collected amax == max|x|;
 2. the three GEMMs agree with the emulation (exact products of the same fp8 operands) at fp32-accumulation tolerance, 2e-5
    of the output's max norm, over the layer geometries of the dual_gan networks (3x3/1, 4x4/2, 1x1, 3x3/2 transposed
    with output padding), ragged channel counts (39 inputs, 3 outputs), batches that need zero padding, both tile heights;
 3. DECLARED tolerance of the family against fp32 arithmetic (the reference's own type): relative L2 error of a layer's
    output <= 6e-2 with e4m3 x e4m3 operands (forward) and <= 1e-1 when an e5m2 gradient is an operand (data / weight
    gradient) — measured 3.5e-2 to 7e-2 on Gaussian data, independent of the reduction length.
"""
import pytest
import torch
import torch.nn.functional as F

from oracle import ref_fp8 as R

pytestmark = pytest.mark.gpu

TOL_EMU = 1e-4
TOL_FWD_VS_FP32 = 6e-2
TOL_BWD_VS_FP32 = 1e-1


def _states(dev, n=8):
    from rg_hip import lowp
    st = lowp.F8States(dev, capacity=n)
    st.policy = "jit"
    out = [st.new(lowp.E4M3 if i % 2 == 0 else lowp.E5M2) for i in range(n)]
    st.finalize()
    return st, out


def _maxrel(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return (got - ref).abs().max().item() / max(ref.abs().max().item(), 1e-30)


def _l2rel(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return (got - ref).norm().item() / max(ref.norm().item(), 1e-30)


@pytest.mark.parametrize("fmt", [0, 1])
@pytest.mark.parametrize("shape", [(2, 5, 6, 4), (3, 39, 16, 8), (32, 64, 8, 4), (7, 3, 3, 3), (64, 16, 1, 1)])
def test_quantizer_bit_exact(dev, fmt, shape):
    from rg_hip import lowp
    g = torch.Generator().manual_seed(sum(shape) + fmt)
    # wide dynamic range: exercises normals, subnormals and the clamp at the format maximum
    x = torch.randn(shape, generator=g) * torch.exp(torch.randn(shape, generator=g) * 2.0)
    st, states = _states(dev)
    s = states[fmt]                                    # index parity selects the format
    xd = x.to(dev)
    s.prepare(xd)
    qa = lowp.quantize(xd, s, "nhwc")
    qb = lowp.quantize(xd, s, "chwn", qa.scale)
    torch.cuda.synchronize()
    amax = x.abs().max()
    xq, d = R.quantize(x, amax, fmt)
    assert torch.equal(qa.buf.cpu(), R.to_layout(xq, "nhwc")), "nhwc bytes differ"
    assert torch.equal(qb.buf.cpu(), R.to_layout(xq, "chwn")), "chwn bytes differ"
    # the single-pass form (what the layers use): both layouts from one read of the fp32 tensor
    da, db = lowp.quantize_dual(xd, s)
    torch.cuda.synchronize()
    assert torch.equal(da.buf.cpu(), qa.buf.cpu()) and torch.equal(db.buf.cpu(), qb.buf.cpu()), "dual-layout pass differs"
    assert float(da.scale.cpu()) == float(d)
    only_b = lowp.quantize_dual(xd, s, want_a=False)[1]
    assert torch.equal(only_b.buf.cpu(), qb.buf.cpu())
    assert float(qa.scale.cpu()) == float(d)
    state = s.view().cpu()
    assert float(state[0]) == float(amax) and float(state[1]) == float(amax) and float(state[3]) == R.FMAX[fmt]


@pytest.mark.parametrize("act", ["none", "leaky", "relu", "tanh"])
@pytest.mark.parametrize("shape", [(2, 5, 6, 4), (3, 39, 16, 8), (32, 64, 32, 16), (7, 3, 3, 3), (17, 16, 1, 1), (20, 21, 64, 32)])
def test_gradient_quantizer_fuses_activation_backward_and_bias_sum(dev, act, shape):
    """rg_f8_quantize_grad: g = dy * act'(y) quantised (e5m2, both layouts) with the channel sums of g, against the CPU emulation
    applied to the same g: bytes bit-exact (the fused product is the one rg_act_bwd computes), sums at fp32 summation accuracy,
    collected amax == max|g|."""
    from rg_hip import lowp, ops
    g = torch.Generator().manual_seed(sum(shape) + len(act))
    dy = torch.randn(shape, generator=g) * torch.exp(torch.randn(shape, generator=g) * 2.0)
    y = torch.randn(shape, generator=g)
    if act == "tanh":
        y = torch.tanh(y)
    code = {"none": ops.ACT_NONE, "leaky": ops.ACT_LEAKY, "relu": ops.ACT_RELU, "tanh": ops.ACT_TANH}[act]
    slope = 0.2
    dyd, yd = dy.to(dev), y.to(dev)
    # g as the stand-alone activation backward (rg_act_bwd) computes it: the fused pass must form the same fp32 products
    gref = (dyd if act == "none" else ops.act_bwd(dyd, yd, code, slope)).cpu()
    if act == "relu":
        assert torch.equal(gref, dy * (y > 0).float())
    if act == "leaky":
        assert torch.equal(gref, dy * torch.where(y > 0, torch.ones_like(y), torch.full_like(y, slope)))
    st, states = _states(dev)
    s = states[1]                                       # e5m2
    s.prepare(gref.to(dev))                             # the scale the delayed policy would carry over
    a, b, part = lowp.quantize_grad_dual(dyd, s, True, True, y=yd, act=code, slope=slope, want_sum=True)
    torch.cuda.synchronize()
    xq, d = R.quantize(gref, gref.abs().max(), 1)
    assert torch.equal(a.buf.cpu(), R.to_layout(xq, "nhwc")), "nhwc bytes differ"
    assert torch.equal(b.buf.cpu(), R.to_layout(xq, "chwn")), "chwn bytes differ"
    assert float(a.scale.cpu()) == float(d)
    N, C = shape[0], shape[1]
    L = shape[2] * shape[3]
    assert tuple(part.shape) == (((N + 15) // 16) * ((L + 63) // 64), C)
    db = part.double().sum(0).cpu()
    ref = gref.double().sum((0, 2, 3))
    assert (db - ref).abs().max().item() <= 2e-6 * gref.double().abs().sum((0, 2, 3)).max().item()
    assert float(s.view().cpu()[1]) == float(gref.abs().max())
    # sums only / one layout only: same results
    _, b2, p2 = lowp.quantize_grad_dual(dyd, s, False, True, y=yd, act=code, slope=slope, want_sum=True)
    assert torch.equal(b2.buf, b.buf) and torch.equal(p2, part)
    out, _ = ops.rows_sum_pair(part, None, part.shape[0], C)
    assert (out.double().cpu() - ref).abs().max().item() <= 2e-6 * gref.double().abs().sum((0, 2, 3)).max().item()


def test_delayed_scaling_rolls_once_per_step(dev):
    """policy 'delayed': the first use calibrates just in time, later uses quantise with the previous step's amax while
    collecting the next one; values beyond the stale range saturate instead of overflowing."""
    from rg_hip import lowp
    st, states = _states(dev)
    st.policy = "delayed"
    s = states[0]
    x1 = torch.linspace(-2.0, 2.0, 2 * 4 * 8 * 8).view(2, 4, 8, 8).to(dev)
    x2 = x1 * 3.0
    s.prepare(x1)
    q1 = lowp.quantize(x1, s, "nhwc")
    st.roll()
    s.prepare(x2)                                      # calibrated: no new measurement
    q2 = lowp.quantize(x2, s, "nhwc")
    torch.cuda.synchronize()
    assert float(q2.scale.cpu()) == float(q1.scale.cpu())            # still the scale of step 1
    xq, _ = R.quantize(x2.cpu(), 2.0, 0)                             # emulation with the stale amax: saturates at 448
    assert torch.equal(q2.buf.cpu(), R.to_layout(xq, "nhwc"))
    st.roll()
    assert abs(float(s.view().cpu()[0]) - 6.0) < 1e-6                # the maximum collected during step 2 is now in use


GEOMS = [
    # N, C, H, W, K, k, stride, pad
    (2, 16, 12, 8, 32, 3, 1, 1),
    (3, 39, 16, 8, 64, 4, 2, 1),          # first generator layer: 2*18 + 3 input channels
    (2, 64, 8, 4, 3, 3, 1, 0),            # output convolution after reflection padding: 3 output channels
    (4, 128, 6, 5, 160, 1, 1, 0),         # 1x1, more than one 128-row tile
    (32, 64, 8, 4, 128, 3, 1, 1),         # a full batch chunk for the weight gradient
    (2, 24, 9, 7, 40, 3, 2, 1),           # odd sizes, stride 2
]


@pytest.mark.parametrize("geom", GEOMS)
def test_conv_f8_against_emulation_and_fp32(dev, geom):
    from rg_hip import lowp, ops
    N, C, H, W, K, k, s, p = geom
    g = torch.Generator().manual_seed(N * 1000 + C)
    x = torch.randn(N, C, H, W, generator=g)
    w = torch.randn(K, C, k, k, generator=g) / (C * k * k) ** 0.5
    b = torch.randn(K, generator=g) * 0.1
    P, Q = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    res = torch.randn(N, K, P, Q, generator=g) * 0.1
    dy = torch.randn(N, K, P, Q, generator=g) * 1e-3
    st, states = _states(dev)
    sx, sdy, sw = states[0], states[1], states[2]
    xd, wd, dyd = x.to(dev), w.to(dev), dy.to(dev)
    sx.prepare(xd)
    xq = lowp.quantize(xd, sx, "nhwc")
    xqt = lowp.quantize(xd, sx, "chwn", xq.scale)
    sw.prepare(wd)
    wq = lowp.quantize(wd, sw, "krsc")
    wqt = lowp.quantize(wd, sw, "crsk", wq.scale)
    sdy.prepare(dyd)
    dyq = lowp.quantize(dyd, sdy, "nhwc")
    dyqt = lowp.quantize(dyd, sdy, "chwn", dyq.scale)
    gm = (N, C, H, W, K, k, k, s, s, p, p)

    y = lowp.conv_fwd(xq, wq, gm, shift=b.to(dev), residual=res.to(dev), act=ops.ACT_LEAKY, slope=0.1)
    y_emu = R.conv_fwd(x, w, 0, b, res, s, p, "leaky", 0.1)
    assert _maxrel(y, y_emu) <= TOL_EMU, "fwd vs emulation %.3e" % _maxrel(y, y_emu)
    y_plain = lowp.conv_fwd(xq, wq, gm)
    assert _l2rel(y_plain, F.conv2d(x, w, None, s, p)) <= TOL_FWD_VS_FP32

    dx = lowp.conv_dgrad(dyq, wqt, gm, (H, W))
    dx_emu = R.conv_dgrad(dy, w, (H, W), 1, None, None, s, p)
    assert _maxrel(dx, dx_emu) <= TOL_EMU, "dgrad vs emulation %.3e" % _maxrel(dx, dx_emu)
    xr = x.clone().requires_grad_(True)
    wr = w.clone().requires_grad_(True)
    F.conv2d(xr, wr, None, s, p).backward(dy)
    assert _l2rel(dx, xr.grad) <= TOL_BWD_VS_FP32

    dw = lowp.conv_wgrad(xqt, dyqt, gm)
    dw_emu = R.conv_wgrad(x, dy, w.shape, 0, 1, s, p)
    assert _maxrel(dw, dw_emu) <= TOL_EMU, "wgrad vs emulation %.3e" % _maxrel(dw, dw_emu)
    assert _l2rel(dw, wr.grad) <= TOL_BWD_VS_FP32


# N, C, H, W, K, k, stride, pad; splits of the plan; the reducer K*C*k*k selects.  Every geometry of GEOMS has K*C*k*k % 4 == 0
# and at most two splits, so the scalar reducer and the deep loops of both never run there.
WGRAD_SPLIT_GEOMS = [
    ((2, 5, 8, 8, 3, 3, 1, 1), 2),        # 135 outputs: scalar reducer
    ((2, 5, 21, 21, 3, 3, 1, 1), 13),     # scalar, 111 k-tiles in 13 splits of 9: both chains and the tail of lane 0
    ((2, 5, 21, 21, 4, 3, 1, 1), 13),     # 180 outputs: float4 reducer, the four-loads-in-flight loop (k + 12 < splits)
]


@pytest.mark.parametrize("geom,splits", WGRAD_SPLIT_GEOMS)
def test_wgrad_split_k_reducers(dev, geom, splits):
    """The weight gradient alone against the emulation where the split-K slab sum (csrc/conv_reduce.h) has work to do.  Only
    TOL_EMU: the fp32 bands were measured on layers with >= 16 channels."""
    from rg_hip import lowp, ops
    N, C, H, W, K, k, s, p = geom
    P, Q = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    n = K * C * k * k
    assert ops._ws_query("rg_conv2d_f8_wgrad_workspace", N, C, K, k, k, P, Q) == splits * n * 4      # the regime meant
    g = torch.Generator().manual_seed(N * 1000 + C + K)
    x = torch.randn(N, C, H, W, generator=g)
    dy = torch.randn(N, K, P, Q, generator=g) * 1e-3
    st, states = _states(dev)
    sx, sdy = states[0], states[1]
    xd, dyd = x.to(dev), dy.to(dev)
    sx.prepare(xd)
    xqt = lowp.quantize(xd, sx, "chwn")
    sdy.prepare(dyd)
    dyqt = lowp.quantize(dyd, sdy, "chwn")
    dw = lowp.conv_wgrad(xqt, dyqt, (N, C, H, W, K, k, k, s, s, p, p))
    dw_emu = R.conv_wgrad(x, dy, (K, C, k, k), 0, 1, s, p)
    err = _maxrel(dw, dw_emu)
    print("wgrad vs emulation %.3e (n = %d, %d splits)" % (err, n, splits))
    assert err <= TOL_EMU, "wgrad vs emulation %.3e" % err


def test_transposed_conv_roles(dev):
    """ConvTranspose2d(3x3, stride 2, padding 1, output_padding 1) of the generator's decoder blocks: forward = data gradient
    with e4m3 activations, input gradient = forward kernel with an e5m2 operand, filter gradient with swapped roles."""
    from rg_hip import lowp
    from rg_hip import nn as rnn
    from rg_hip.tape import Tape
    torch.manual_seed(5)
    ct = rnn.ConvTranspose2d(32, 24, 3, 2, 1, 1).to(dev)
    ref = torch.nn.ConvTranspose2d(32, 24, 3, 2, 1, 1)
    ref.load_state_dict({k: v.cpu() for k, v in ct.state_dict().items()})
    net = rnn.Sequential(ct)
    lowp.set_conv_dtype(net, "fp8", policy="jit")
    x = torch.randn(4, 32, 8, 4)
    dy = torch.randn(4, 24, 16, 8) * 1e-2
    tape = Tape()
    y = ct.tf(tape, x.to(dev))
    dx = ct.tb(tape, dy.to(dev))
    xr = x.clone().requires_grad_(True)
    yr = ref(xr)
    yr.backward(dy)
    # emulation: forward == dgrad with fmt 0; bias added in the epilogue
    y_emu = R.conv_dgrad(x, ref.weight.detach(), (16, 8), 0, ref.bias.detach(), None, 2, 1)
    assert _maxrel(y, y_emu) <= TOL_EMU
    assert _l2rel(y, yr) <= TOL_FWD_VS_FP32
    assert _l2rel(dx, xr.grad) <= TOL_BWD_VS_FP32
    dw = tape.grads[id(ct.weight)]
    assert _l2rel(dw, ref.weight.grad) <= TOL_BWD_VS_FP32
    assert _l2rel(tape.grads[id(ct.bias)], ref.bias.grad) <= 1e-5        # the bias gradient stays fp32


def test_fp8_needs_the_gpu():
    from rg_hip import lowp
    from rg_hip import nn as rnn
    with pytest.raises(RuntimeError):
        lowp.set_conv_dtype(rnn.Sequential(rnn.Conv2d(4, 4, 3)), "fp8")
