"""The host model of the fused verification head (tests/verif_hostmodel.py) against what it restates: float64 torch autograd over the
oracle's EltwiseSubEmbed + F.cross_entropy, the values recorded from the reference's own modules, float32 torch (the calibration of
the budget constants), and six planted defects that the comparison must catch.  Also the host side of the feature that needs no
GPU: the header's prototypes and `import reid.trainers` without a reference tree."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import ref_torch as O
from tests import verif_hostmodel as H
from tests.golden import cases_siamese as GC

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = H.cases()


def _autograd64(inp, train, grad_loss=None, up=None):
    """float64 autograd over the oracle's module -> values, the six gradients, the running statistics"""
    B, D = inp["x1"].shape
    C = inp["W"].shape[0]
    m = O.OEltwiseSubEmbed(use_batch_norm=True, use_classifier=True, num_features=D, num_classes=C).double()
    m.train(bool(train))
    m.bn.eps, m.bn.momentum = H._f32(inp["eps"]), H._f32(inp["mom"])       # the float32 values the C ABI carries
    with torch.no_grad():
        m.bn.weight.copy_(inp["gamma"]), m.bn.bias.copy_(inp["beta"])
        m.bn.running_mean.copy_(inp["rm"]), m.bn.running_var.copy_(inp["rv"])
        m.classifier.weight.copy_(inp["W"])
        m.classifier.bias.copy_(inp["bias"]) if inp["bias"] is not None else m.classifier.bias.zero_()
    x1, x2 = inp["x1"].double().requires_grad_(True), inp["x2"].double().requires_grad_(True)
    logits = m(x1, x2)
    out = {"logits": logits.detach()}
    obj = 0.0
    if inp["labels"] is not None:
        loss = F.cross_entropy(logits, inp["labels"])
        out["loss"] = loss.detach()
        obj = loss * (1.0 if grad_loss is None else float(grad_loss))
    if up is not None:
        obj = obj + (logits * up.double()).sum()
    obj.backward()
    out.update({"dx1": x1.grad, "dx2": x2.grad, "dW": m.classifier.weight.grad, "dbias": m.classifier.bias.grad,
                "dgamma": m.bn.weight.grad, "dbeta": m.bn.bias.grad, "running_mean": m.bn.running_mean, "running_var": m.bn.running_var})
    return out


def _close(a, b, what, tol=1e-9):
    a, b = torch.as_tensor(a).double().reshape(-1), torch.as_tensor(b).double().reshape(-1)
    err = float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))
    assert err <= tol, "%s: relative distance %.3e" % (what, err)


AUTOGRAD_CASES = [c for c in CASES if c.planted != "ignored" and (c.B, c.D, c.C) != H.STAGE1]      # F.cross_entropy averages over the kept rows only


def _id(c):
    return "B%d-D%d-C%d-%s-%s-%s%s%s" % (c.B, c.D, c.C, c.fam, "train" if c.train else "eval", c.planted, "" if c.bias else "-nobias",
                                          "" if c.labels else "-nolabels")


@pytest.mark.parametrize("case", AUTOGRAD_CASES, ids=_id)
def test_model_is_float64_autograd_over_the_oracle(case):
    inp = H.case_input(case)
    gl, up = H.case_upstream(case)
    ref = _autograd64(inp, case.train, gl, up)
    f = H.head_fwd(inp, case.train)
    b = H.head_bwd(inp, f["xhat"].value, f["invstd"].value, f["dlogits"].value if case.labels else None, gl, up, case.train)
    tol = 1e-6 if case.planted == "bigmean" or case.fam in ("offset", "scales") else 1e-9      # float64 itself cancels there
    _close(f["logits"].value, ref["logits"], "logits", tol)
    if case.labels:
        _close(f["loss"].value, ref["loss"], "loss", tol)
    for k in ("running_mean", "running_var"):
        _close(f[k].value, ref[k], k, tol)
    for k in ("dx1", "dx2", "dW", "dbias", "dgamma", "dbeta"):
        if k == "dbias" and inp["bias"] is None:
            continue
        _close(b[k].value, ref[k], k, max(tol, 1e-7))


@pytest.mark.parametrize("name", sorted(GC.CASES))
def test_model_reproduces_the_values_recorded_from_the_reference(name):
    rec = np.load(os.path.join(REPO, "tests", "golden", "reference_siamese.npz"))
    g = GC.inputs(name)
    inp = {"x1": g["f1"], "x2": g["f2"], "gamma": g["gamma"], "beta": g["beta"], "rm": g["rm"], "rv": g["rv"], "W": g["W"],
           "bias": g["bias"], "labels": g["targets"], "eps": H.EPS, "mom": H.MOM}
    f = H.head_fwd(inp, 1)
    b = H.head_bwd(inp, f["xhat"].value, f["invstd"].value, f["dlogits"].value, None, None, 1)
    got = {"logits": f["logits"], "loss": f["loss"], "prec": f["prec"], "df1": b["dx1"], "df2": b["dx2"], "dW": b["dW"],
           "dbias": b["dbias"], "dgamma": b["dgamma"], "dbeta": b["dbeta"], "running_mean": f["running_mean"],
           "running_var": f["running_var"]}
    assert sorted(got) == sorted(GC.QUANTITIES)
    for k, r in got.items():
        # the recorded values are the reference's float32 results: they lie within the model's own budget of its float64 value
        H.check(torch.from_numpy(rec["%s_%s" % (name, k)]).reshape(r.value.shape), r, "%s %s" % (name, k))


def _f32_ratios(case):
    """max err / (2^-24 M) per kind of the float32 torch evaluation of one case, and whether its argmax agrees on every row"""
    inp = H.case_input(case)
    gl, up = H.case_upstream(case)
    f, v = H.head_fwd(inp, case.train), H.evaluate(inp, case.train, torch.float32)
    worst = {}

    def rec(got, ref):
        w = H.compare(got, ref, H.C_KIND)
        if ref.kind != "exact":
            worst[ref.kind] = max(worst.get(ref.kind, 0.0), w.ratio)
    for k in ("logits", "xhat", "mean", "invstd", "running_mean", "running_var"):
        rec(v[k], f[k])
    agree = True
    if case.labels:
        rec(v["loss_rows"], f["loss_rows"]), rec(v["out2"][0].reshape(1), f["loss"]), rec(v["dlogits"], f["dlogits"])
        agree = v["correct"] == f["correct"] and bool((H.argmax_low(v["logits"]) == H.argmax_low(f["logits"].value)).all())
    xh, iv = f["xhat"].value.float(), f["invstd"].value.float()
    dl = f["dlogits"].value.float() if case.labels else None
    b = H.head_bwd(inp, xh, iv, dl, gl, up, case.train)
    t = H.bwd_terms(inp, xh, iv, dl, gl, up, case.train, torch.float32)
    for k in b:
        rec(t[k], b[k])
    return worst, agree


def test_float32_torch_lies_within_a_quarter_of_every_budget_and_agrees_on_every_argmax():
    """the calibration of C_KIND (its docstring): C_KIND = max(8, 4 x the float32 torch ratio), so the ratio of every kind is at most
    C_KIND / 4; and no row of any case has an argmax that float32 and float64 settle differently, so the device test can ask for
    the exact `correct` count on all of them"""
    torch.set_num_threads(1)                 # the thread count the constants were measured at
    worst = {}
    for case in CASES:
        w, agree = _f32_ratios(case)
        assert agree, "float32 and float64 disagree on an argmax of %s" % (case,)
        for k, r in w.items():
            worst[k] = max(worst.get(k, 0.0), r)
    print("float32 torch ratios:", {k: round(v, 2) for k, v in sorted(worst.items())})
    for k, r in worst.items():
        assert r <= H.C_KIND[k] / 4.0 + 1e-9, "%s: float32 torch ratio %.2f, C_KIND %.2f" % (k, r, H.C_KIND[k])


def test_the_ties_cases_tie_at_the_maximum_and_the_lowest_index_wins():
    for case in CASES:
        if case.planted != "ties":
            continue
        inp = H.case_input(case)
        l = H.evaluate(inp, case.train)["logits"]
        tied = (l == l.max(1, keepdim=True).values).sum(1) > 1
        assert int(tied.sum()) >= 1, "no row ties at its maximum: %s" % (case,)
        assert bool((H.argmax_low(l)[tied] == case.C - 2).all())


DEFECT_OUTPUT = {"biased_running_var": "running_var", "no_1_over_B": "dlogits", "dx2_sign": "dx2", "bn_bwd_no_mean": "dx1",
                 "dbias_axis": "dbias", "tie_high": "correct"}


@pytest.mark.parametrize("defect", H.DEFECTS)
def test_planted_defect_is_caught(defect):
    case = H.Case(17, 33, 3, "plain", 1, "ties" if defect == "tie_high" else None, True, True)
    inp = H.case_input(case)
    f = H.head_fwd(inp, 1)
    xh, iv, dl = f["xhat"].value.float(), f["invstd"].value.float(), f["dlogits"].value.float()
    b = H.head_bwd(inp, xh, iv, dl, None, None, 1)
    bad = H.evaluate(inp, 1, defect=defect)
    bad.update(H.bwd_terms(inp, xh, iv, dl, None, None, 1, defect=defect))
    k = DEFECT_OUTPUT[defect]
    if k == "correct":
        assert bad["correct"] != f["correct"]
        return
    ref = f[k] if k in f else b[k]
    assert not H.compare(bad[k], ref, H.C_KIND).ok, "%s passes the comparison of %s" % (defect, k)
    sound = H.evaluate(inp, 1)
    sound.update(H.bwd_terms(inp, xh, iv, dl, None, None, 1))
    assert H.compare(sound[k], ref, H.C_KIND).ok


def test_header_declares_the_three_entry_points():
    from rg_hip.lib import parse_header
    protos = parse_header()
    for name in ("rg_verif_head_workspace", "rg_verif_head_fwd", "rg_verif_head_bwd"):
        assert name in protos, name
    assert protos["rg_verif_head_workspace"][0] == "int64_t"
    assert [t for t, _ in protos["rg_verif_head_workspace"][1]] == ["int", "int", "int"]
    assert protos["rg_verif_head_fwd"][0] == "int" and protos["rg_verif_head_bwd"][0] == "int"


def test_workspace_query_matches_the_model():
    from rg_hip.lib import lib
    for B, D, C in [(2, 1, 1), (17, 100, 3), H.STAGE1]:
        assert lib.rg_verif_head_workspace(B, D, C) == H.workspace_bytes(B, D, C)
    assert lib.rg_verif_head_workspace(0, 8, 2) == 0


def test_trainers_import_without_a_reference_tree():
    code = ("import reid.trainers as T\n"
            "from reid.evaluation_metrics import accuracy\n"
            "import inspect, torch\n"
            "assert str(inspect.signature(T.BaseTrainer.train)) == '(self, epoch, data_loader, optimizer, base_lr=0.1, print_freq=1)'\n"
            "assert list(inspect.signature(T.SiameseTrainer.__init__).parameters)[:5] == ['self', 'model', 'criterion', 'num_classes', 'num_instances']\n"
            "assert T.SiameseTrainer(None, None).sync_every_step is False\n"
            "p, = accuracy(torch.tensor([[0.1, 0.9], [0.8, 0.2], [0.3, 0.7]]), torch.tensor([1, 0, 0]))\n"
            "assert abs(float(p[0]) - 2.0 / 3.0) < 1e-6\n"
            "print('IMPORT-OK')\n")
    env = dict(os.environ)
    env["PYTHONPATH"] = os.path.join(REPO, "reid-gan_amd")
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "IMPORT-OK" in out.stdout, out.stdout + out.stderr


def test_trainer_refuses_a_world_size_above_one(monkeypatch):
    """stage I under torch.distributed is not built: the refusal comes before the model is called"""
    import torch.distributed as dist
    from torch import nn
    from reid.trainers import SiameseTrainer

    def model(*a):
        raise AssertionError("the model was called")
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda *a, **k: 2)
    trainer = SiameseTrainer(model, nn.CrossEntropyLoss())
    with pytest.raises(NotImplementedError, match="ADVICE.md item 1"):
        trainer.step(None, None, None, None)
