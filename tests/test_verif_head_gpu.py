"""GPU: the fused verification head (csrc/verif_head.hip, rg_verif_head_fwd / rg_verif_head_bwd) through the C ABI, per element
against tests/verif_hostmodel.py: every element of every output compared, every output between two rows of guard values, two runs
byte-equal and a run on a side stream byte-equal to the main stream.  The backward is handed the rounded reference forward.  The
composed path the head replaces (ops.sub_square_fwd -> BatchNorm1d -> Linear -> cross_entropy) goes through the same comparison at
the stage-I shape.

Each check prints `RATIO <entry point> <output> <case> <max err / (2^-24 M)>` (pytest -s shows them;
profiles/verif_elementwise_ratios.txt keeps the worst per entry point and output, fused and composed side by side)."""
import pytest
import torch

from tests import head_hostmodel as HH
from tests import verif_hostmodel as H
from tests.test_head_elementwise_gpu import _Out, _lib, _ptr, _st, _to

pytestmark = pytest.mark.gpu

CASES = H.cases()
FWD_KEYS = ("logits", "xhat", "mean", "invstd", "running_mean", "running_var")
BWD_KEYS = ("dx1", "dx2", "dW", "dbias", "dgamma", "dbeta")


def _id(c):
    return "B%d-D%d-C%d-%s-%s-%s%s%s" % (c.B, c.D, c.C, c.fam, "train" if c.train else "eval", c.planted, "" if c.bias else "-nobias",
                                          "" if c.labels else "-nolabels")


def _check(out, ref, what, tag):
    out.guards(what)
    w = HH.compare(out.t, ref, H.C_KIND)
    assert w.ok, "%s | %s: worst element %s err %.3e > budget %.3e (%s, max err/(2^-24 M) = %.2f)" % (
        what, tag, w.index, w.err, w.budget, ref.kind, w.ratio)
    print("RATIO %s %s %.3f" % (what, tag, w.ratio))


def _out2_ref(f):
    return HH.Ref(torch.cat([f["loss"].value, f["prec"].value.double()]), torch.cat([f["loss"].M, torch.zeros(1, dtype=torch.float64)]), "ce")


class _Fwd(object):
    """one rg_verif_head_fwd call on fresh guarded outputs"""

    def __init__(self, dev, inp, train, ws_bytes=None):
        B, D = inp["x1"].shape
        C = inp["W"].shape[0]
        self.dev_in = dict(zip(("x1", "x2", "gamma", "beta", "W", "bias", "labels"),
                               _to(dev, inp["x1"], inp["x2"], inp["gamma"], inp["beta"], inp["W"], inp["bias"], inp["labels"])))
        o = {"logits": _Out((B, C), dev), "xhat": _Out((B, D), dev), "mean": _Out((D,), dev), "invstd": _Out((D,), dev),
             "running_mean": _Out((D,), dev, init=inp["rm"].to(dev)), "running_var": _Out((D,), dev, init=inp["rv"].to(dev))}
        if inp["labels"] is not None:
            o.update({"loss_rows": _Out((B,), dev), "out2": _Out((2,), dev), "dlogits": _Out((B, C), dev)})
        need = H.workspace_bytes(B, D, C) if ws_bytes is None else ws_bytes
        self.ws = _Out((max(need // 4, 1),), dev) if train else None
        self.out, self.args = o, (B, D, C, 1 if train else 0, inp["eps"], inp["mom"])
        self.need = need

    def run(self):
        d, o = self.dev_in, self.out
        _lib().rg_verif_head_fwd(d["x1"].data_ptr(), d["x2"].data_ptr(), d["gamma"].data_ptr(), d["beta"].data_ptr(),
                                 o["running_mean"].ptr, o["running_var"].ptr, d["W"].data_ptr(), _ptr(d["bias"]), _ptr(d["labels"]),
                                 o["logits"].ptr, o["xhat"].ptr, o["mean"].ptr, o["invstd"].ptr, _ptr(o.get("loss_rows")),
                                 _ptr(o.get("out2")), _ptr(o.get("dlogits")), *self.args, _ptr(self.ws),
                                 self.need if self.ws is not None else 0, _st())
        return self


def _bwd(dev, inp, f, case, gl, up, drop=None):
    """one rg_verif_head_bwd call handed the rounded reference forward -> {name: _Out}; drop: the output passed as NULL"""
    B, D, C = case.B, case.D, case.C
    xh, iv = f["xhat"].value.float(), f["invstd"].value.float()
    dl = f["dlogits"].value.float() if case.labels else None
    d = dict(zip(("x1", "x2", "gamma", "beta", "W", "xhat", "invstd", "dlogits", "gl", "up"),
                 _to(dev, inp["x1"], inp["x2"], inp["gamma"], inp["beta"], inp["W"], xh, iv, dl, gl, up)))
    o = {"dx1": _Out((B, D), dev), "dx2": _Out((B, D), dev), "dW": _Out((C, D), dev), "dbias": _Out((C,), dev), "dgamma": _Out((D,), dev),
         "dbeta": _Out((D,), dev)}
    p = {k: (None if k == drop else v.ptr) for k, v in o.items()}
    _lib().rg_verif_head_bwd(_ptr(d["gl"]), _ptr(d["dlogits"]), _ptr(d["up"]), d["x1"].data_ptr(), d["x2"].data_ptr(), d["xhat"].data_ptr(),
                             d["invstd"].data_ptr(), d["gamma"].data_ptr(), d["beta"].data_ptr(), d["W"].data_ptr(), p["dx1"], p["dx2"],
                             p["dW"], p["dbias"], p["dgamma"], p["dbeta"], B, D, C, case.train, _st())
    return o


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_head_per_element(dev, case):
    inp = H.case_input(case)
    tag = _id(case)
    f = H.head_fwd(inp, case.train)
    run = _Fwd(dev, inp, case.train).run()
    for k in FWD_KEYS:
        _check(run.out[k], f[k], "rg_verif_head_fwd " + k, tag)
    if case.labels:
        _check(run.out["loss_rows"], f["loss_rows"], "rg_verif_head_fwd loss_rows", tag)
        _check(run.out["out2"], _out2_ref(f), "rg_verif_head_fwd out2", tag)
        _check(run.out["dlogits"], f["dlogits"], "rg_verif_head_fwd dlogits", tag)
        got = float(run.out["out2"].t[1]) * case.B
        assert round(got) == f["correct"] and abs(got - round(got)) < 1e-3, "correct: %r, model %d | %s" % (got, f["correct"], tag)
    if run.ws is not None:
        run.ws.guards("rg_verif_head_fwd workspace | " + tag)
    again = _Fwd(dev, inp, case.train).run()
    side = _Fwd(dev, inp, case.train)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        side.run()
    torch.cuda.synchronize()
    for k, o in run.out.items():
        assert torch.equal(o.buf, again.out[k].buf), "rg_verif_head_fwd %s: two runs differ | %s" % (k, tag)
        assert torch.equal(o.buf, side.out[k].buf), "rg_verif_head_fwd %s: the side stream differs | %s" % (k, tag)
    gl, up = H.case_upstream(case)
    b = H.head_bwd(inp, f["xhat"].value.float(), f["invstd"].value.float(), f["dlogits"].value.float() if case.labels else None, gl, up,
                   case.train)
    o1 = _bwd(dev, inp, f, case, gl, up)
    for k in BWD_KEYS:
        _check(o1[k], b[k], "rg_verif_head_bwd " + k, tag)
    o2 = _bwd(dev, inp, f, case, gl, up)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        o3 = _bwd(dev, inp, f, case, gl, up)
    torch.cuda.synchronize()
    for k in BWD_KEYS:
        assert torch.equal(o1[k].buf, o2[k].buf), "rg_verif_head_bwd %s: two runs differ | %s" % (k, tag)
        assert torch.equal(o1[k].buf, o3[k].buf), "rg_verif_head_bwd %s: the side stream differs | %s" % (k, tag)


@pytest.mark.parametrize("train", (1, 0))
def test_each_backward_output_may_be_null(dev, train):
    case = H.Case(17, 33, 3, "plain", train, None, True, True)
    inp = H.case_input(case)
    f = H.head_fwd(inp, train)
    gl, up = torch.tensor([0.37]), H.case_upstream(case)[1]
    if up is None:
        up = (torch.randn(case.B, case.C, generator=HH.gen(5)) * 0.1).float()
    b = H.head_bwd(inp, f["xhat"].value.float(), f["invstd"].value.float(), f["dlogits"].value.float(), gl, up, train)
    for drop in BWD_KEYS:
        o = _bwd(dev, inp, f, case, gl, up, drop=drop)
        for k in BWD_KEYS:
            if k == drop:
                o[k].untouched("rg_verif_head_bwd %s passed as NULL" % k)
            else:
                _check(o[k], b[k], "rg_verif_head_bwd " + k, "without-" + drop)


def test_eval_mode_takes_no_workspace_and_train_mode_checks_it(dev):
    case = H.Case(17, 33, 3, "plain", 0, None, True, True)
    inp = H.case_input(case)
    run = _Fwd(dev, inp, 0).run()                       # _Fwd passes workspace NULL, 0 bytes in eval mode
    assert run.ws is None
    _check(run.out["logits"], H.head_fwd(inp, 0)["logits"], "rg_verif_head_fwd logits", "eval-no-workspace")
    short = _Fwd(dev, inp, 1, ws_bytes=H.workspace_bytes(case.B, case.D, case.C) - 1)
    with pytest.raises(RuntimeError, match="workspace too small"):
        short.run()
    for k, o in short.out.items():
        if k in ("running_mean", "running_var"):
            o.guards(k)
            assert torch.equal(o.t.cpu(), inp["rm" if k == "running_mean" else "rv"]), "%s moved after the workspace error" % k
        else:
            o.untouched("rg_verif_head_fwd %s after the workspace error" % k)


def test_one_row_in_train_mode_is_refused(dev):
    inp = H.make_input(1, 17, 2)
    run = _Fwd(dev, inp, 1)
    with pytest.raises(RuntimeError, match="more than 1 row"):
        run.run()
    run.out["logits"].untouched("rg_verif_head_fwd logits after the refusal")
    _Fwd(dev, inp, 0).run()                             # eval mode takes one row
    from rg_hip import ops
    d = _to(dev, inp["x1"], inp["x2"], inp["gamma"], inp["beta"], inp["rm"], inp["rv"], inp["W"], inp["bias"], inp["labels"])
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        ops.verif_head_fwd(*d, True, H.EPS, H.MOM)


def test_ops_wrappers_against_the_model(dev):
    from rg_hip import ops
    case = H.Case(33, 100, 2, "plain", 1, None, True, True)
    inp = H.case_input(case)
    f = H.head_fwd(inp, 1)
    d = _to(dev, inp["x1"], inp["x2"], inp["gamma"], inp["beta"], inp["rm"], inp["rv"], inp["W"], inp["bias"], inp["labels"])
    logits, xhat, mean, invstd, rows, out2, dl = ops.verif_head_fwd(*d, True, H.EPS, H.MOM)
    for got, k in ((logits, "logits"), (xhat, "xhat"), (mean, "mean"), (invstd, "invstd"), (rows, "loss_rows"), (dl, "dlogits"),
                   (d[4], "running_mean"), (d[5], "running_var")):
        H.check(got, f[k], "ops.verif_head_fwd " + k)
    H.check(out2, _out2_ref(f), "ops.verif_head_fwd out2")
    b = H.head_bwd(inp, xhat.cpu(), invstd.cpu(), dl.cpu(), None, None, 1)
    res = ops.verif_head_bwd(None, dl, None, d[0], d[1], xhat, invstd, d[2], d[3], d[6], True)
    for got, k in zip(res, BWD_KEYS):
        H.check(got, b[k], "ops.verif_head_bwd " + k)
    only = ops.verif_head_bwd(None, dl, None, d[0], d[1], xhat, invstd, d[2], d[3], d[6], True, need_dx=(False, True), need_dweight=False,
                              need_dbeta=False)
    assert only[0] is None and only[2] is None and only[5] is None and torch.equal(only[1], res[1]) and torch.equal(only[4], res[4])


def test_composed_path_at_the_stage1_shape(dev):
    """the layers the head replaces — ops.sub_square_fwd -> rnn.BatchNorm1d -> rnn.Linear (EltwiseSubEmbed's module call) -> torch's
    cross_entropy — through the same comparison.  Its backward starts from its own forward, not from the rounded reference."""
    import torch.nn.functional as F
    from reid.models.embedding import EltwiseSubEmbed
    B, D, C = H.STAGE1
    case = H.Case(B, D, C, "plain", 1, None, True, True)
    inp = H.case_input(case)
    f = H.head_fwd(inp, 1)
    b = H.head_bwd(inp, f["xhat"].value.float(), f["invstd"].value.float(), f["dlogits"].value.float(), None, None, 1)
    m = EltwiseSubEmbed(use_batch_norm=True, use_classifier=True, num_features=D, num_classes=C).to(dev).train()
    with torch.no_grad():
        m.bn.weight.copy_(inp["gamma"]), m.bn.bias.copy_(inp["beta"]), m.bn.running_mean.copy_(inp["rm"]), m.bn.running_var.copy_(inp["rv"])
        m.classifier.weight.copy_(inp["W"]), m.classifier.bias.copy_(inp["bias"])
    x1, x2 = inp["x1"].to(dev).requires_grad_(True), inp["x2"].to(dev).requires_grad_(True)
    logits = m(x1, x2)
    loss = F.cross_entropy(logits, inp["labels"].to(dev))
    loss.backward()
    got = {"logits": logits.detach(), "loss": loss.detach().reshape(1), "running_mean": m.bn.running_mean, "running_var": m.bn.running_var,
           "dx1": x1.grad, "dx2": x2.grad, "dW": m.classifier.weight.grad, "dbias": m.classifier.bias.grad, "dgamma": m.bn.weight.grad,
           "dbeta": m.bn.bias.grad}
    for k, g in got.items():
        ref = f[k] if k in f else b[k]
        w = HH.compare(g, ref, H.C_KIND)
        print("RATIO composed %s %s %.3f" % (k, _id(case), w.ratio))
        assert w.ok, "composed %s: worst element %s err %.3e > budget %.3e (%s, max err/(2^-24 M) = %.2f)" % (
            k, w.index, w.err, w.budget, ref.kind, w.ratio)


def _requested(what):
    return torch.cuda.memory_stats()["requested_bytes.all." + what]


def test_forward_and_backward_keep_one_saved_tensor_of_the_input_size(dev):
    """forward + backward at the stage-I shape allocate xhat and the two input gradients, three [B, D] tensors, plus the small ones
    ([B, C], [C, D], [D] vectors: under 256 KB); the workspace (O(B C D / 16)) is the per-stream scratch buffer, there after the
    warm-up.  A fourth [B, D] tensor (d, z or dz: 2 MB) does not fit under the bound."""
    from rg_hip import ops
    B, D, C = H.STAGE1
    inp = H.make_input(B, D, C)
    d = _to(dev, inp["x1"], inp["x2"], inp["gamma"], inp["beta"], inp["rm"], inp["rv"], inp["W"], inp["bias"], inp["labels"])

    def both():
        logits, xhat, mean, invstd, rows, out2, dl = ops.verif_head_fwd(*d, True, H.EPS, H.MOM)
        return ops.verif_head_bwd(None, dl, None, d[0], d[1], xhat, invstd, d[2], d[3], d[6], True), logits, out2
    both()                                              # warm-up: the workspace, the library's lazy state
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = _requested("current")
    res = both()
    torch.cuda.synchronize()
    peak = _requested("peak") - base
    bound = 3 * B * D * 4 + 256 * 1024
    print("verif head forward + backward peak above the inputs %d bytes, bound %d, one [B, D] tensor %d" % (peak, bound, B * D * 4))
    assert peak < bound, (peak, bound)
    assert H.workspace_bytes(B, D, C) == B * C * (D // 16) * 4 and res[0][0] is not None
