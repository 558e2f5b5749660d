"""IBN-a modules on the MI355X: Bottleneck(ibn=True), resnet_ibn50a / resnet_ibn101a and one cluster-contrast training step,
against the host model (tests/ibn_hostmodel.py) on identical seeded weights and inputs, and against the values recorded from
the reference's own modules (tests/golden/reference_ibn.npz).  Metrics and tolerances are those of tests/test_modules_gpu.py
(forward 1e-3 in the max norm; train-mode gradients anchored on an fp64 run) and tests/test_cc_gpu.py (the training step)."""
import os

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from tests import ibn_hostmodel as H
from tests.golden import cases_ibn as C
from tests.golden.cases import sub
from tests.test_modules_gpu import _check, _check_anchored, _check_grads, _check_grads_anchored, _check_l2

pytestmark = pytest.mark.gpu

GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "reference_ibn.npz"))


def _vs_fixture(got, key, tol, n=None):
    ref = GOLD[key]
    v = got.detach().double().cpu()
    v = sub(v, n)[0] if n else v.numpy()
    err = np.abs(v.reshape(ref.shape) - ref).max() / max(np.abs(ref).max(), 1e-12)
    print("%s: rel err vs the recorded reference %.3e (bound %.1e)" % (key, err, tol))
    assert err <= tol, "%s: %.3e > %.1e" % (key, err, tol)


def _double(m):
    import copy
    return copy.deepcopy(m).double()


@pytest.mark.parametrize("mode", ["train", "eval"])
def test_ibn_bottleneck(dev, mode):
    from rg_hip import nn as rnn
    from rg_hip.resnet_trunk import Bottleneck
    cin, w = C.BLOCK["cin"], C.BLOCK["width"]
    o = H.bottleneck(cin, w, 1, nn.Sequential(nn.Conv2d(cin, 4 * w, 1, 1, bias=False), nn.BatchNorm2d(4 * w)))
    o.load_state_dict(C.fill(o.state_dict(), "ibn_block"))
    r = Bottleneck(cin, w, 1, rnn.Sequential(rnn.Conv2d(cin, 4 * w, 1, bias=False), rnn.BatchNorm2d(4 * w)), ibn=True)
    r.load_state_dict(o.state_dict())
    r.to(dev)
    o64 = _double(o)
    for m in (o, r, o64):
        getattr(m, mode)()
    x, dy = C.block_input()
    xo, x64, xr = x.clone().requires_grad_(True), x.double().requires_grad_(True), x.clone().to(dev).requires_grad_(True)
    yo, y64, yr = o(xo), o64(x64), r(xr)
    _check(yr, yo, 1e-3, "output")
    yo.backward(dy), y64.backward(dy.double()), yr.backward(dy.to(dev))
    if mode == "train":
        _check_anchored(xr.grad, xo.grad, x64.grad, "input grad")
        _check_grads_anchored(r, o, o64, "Bottleneck(ibn) train")
        _vs_fixture(yr, "block_y", 1e-3)
        _vs_fixture(xr.grad, "block_dx", 1e-3)
        sr, so = r.state_dict(), o.state_dict()
        assert list(sr.keys()) == list(so.keys())
        for k in so:
            if "running" in k:
                _check(sr[k], so[k], 1e-3, k)
            if "num_batches_tracked" in k:
                assert int(sr[k]) == int(so[k]) == 1, k
    else:
        _check_l2(xr.grad, xo.grad, 2e-3, "input grad")
        _check_grads(r, o, 2e-3, "Bottleneck(ibn) eval")


@pytest.mark.parametrize("mode", ["train", "eval"])
def test_resnet_ibn50a(dev, mode):
    """against the host model (fp32, fp64 anchor for the train-mode gradients) and against the recorded reference values; the
    bound on the latter is 1e-3 or, where larger, 4 x the reference's own recorded distance from fp64 (see test_ibn_cpu)"""
    import clustercontrast.models as M
    o = H.HResNetIBN(C.MODEL["depth"], **C.MODEL["kw"])
    sd = C.fill(o.state_dict(), "ibn_model")
    o.load_state_dict(sd)
    r = M.create("resnet_ibn50a", pretrained=False, **C.MODEL["kw"])
    r.load_state_dict(sd, strict=True)
    r.to(dev)
    o64 = _double(o)
    for m in (o, r, o64):
        getattr(m, mode)()
    x, dy = C.model_input()
    xo, x64, xr = x.clone().requires_grad_(True), x.double().requires_grad_(True), x.clone().to(dev).requires_grad_(True)
    fo, f64, fr = o(xo), o64(x64), r(xr)
    assert torch.is_tensor(fr) and fr.shape == (4, 2048)              # train mode: bn_x alone, no tuple
    _check(fr, fo, 1e-3, "embedding")
    (fo * dy).sum().backward(), (f64 * dy.double()).sum().backward(), (fr * dy.to(dev)).sum().backward()
    if mode == "train":
        _check_anchored(xr.grad, xo.grad, x64.grad, "input grad")
        _check_grads_anchored(r, o, o64, "resnet_ibn50a train")
    else:
        _check_l2(xr.grad, xo.grad, 2e-3, "input grad")
        _check_grads(r, o, 2e-3, "resnet_ibn50a eval")
    assert r.feat_bn.bias.grad is None
    sr, so = r.state_dict(), o.state_dict()
    for k in so:
        if "running" in k:
            _check(sr[k], so[k], 1e-3, k)
        if "num_batches_tracked" in k:
            assert int(sr[k]) == int(so[k]) == (1 if mode == "train" else 0), k
    params = dict(r.named_parameters())
    rec = {"emb": fr, "dx": xr.grad}
    rec.update({"grad:" + k: params[k].grad for k in C.GRAD_KEYS})
    for k, v in rec.items():
        key = "model_%s_%s" % (mode, k)
        _vs_fixture(v, key, max(1e-3, 4.0 * float(GOLD[key + "_ref_vs_fp64"])), n=2048)
    for k in ("running_mean", "running_var"):
        _vs_fixture(sr[C.STATS_LAYER + k], "model_%s_stat:%s" % (mode, k), 1e-3)


def test_resnet_ibn101a_eval(dev):
    import clustercontrast.models as M
    o = H.HResNetIBN("101a", **C.MODEL["kw"])
    sd = C.fill(o.state_dict(), "ibn_model101")
    o.load_state_dict(sd)
    r = M.create("resnet_ibn101a", pretrained=False, **C.MODEL["kw"])
    r.load_state_dict(sd, strict=True)
    r.to(dev).eval()
    o.eval()
    x, _ = C.model_input(2)
    with torch.no_grad():
        _check(r(x.to(dev)), o(x), 1e-3, "eval embedding")


def test_eval_trunk_with_ibn_folds_its_plain_pairs_in_one_launch(dev, monkeypatch):
    """the FoldGroup of an IBN trunk holds the 40 (conv, BatchNorm) pairs and folds them with ONE launch per weight version; no
    pair falls back to the per-pair fold; the 13 conv1 -> IBN pairs run unfused"""
    import clustercontrast.models as M
    from rg_hip import nn as rnn
    from rg_hip import ops
    r = M.create("resnet_ibn50a", pretrained=False, **C.MODEL["kw"]).to(dev).eval()
    calls = {"multi": 0, "single": 0}
    multi, single = ops.fold_filters_multi, ops.bn_fold
    monkeypatch.setattr(ops, "fold_filters_multi", lambda *a, **k: (calls.__setitem__("multi", calls["multi"] + 1), multi(*a, **k))[1])
    monkeypatch.setattr(ops, "bn_fold", lambda *a, **k: (calls.__setitem__("single", calls["single"] + 1), single(*a, **k))[1])
    x, _ = C.model_input(2)
    with torch.no_grad():
        a = r(x.to(dev))
        b = r(x.to(dev))
    grp = r.base[0]._rg_fold_group
    assert len(grp.pairs) == 40 and grp.usable() and all(isinstance(bn, rnn._BatchNorm) for _, bn in grp.pairs)
    assert calls == {"multi": 1, "single": 0}, calls
    assert torch.equal(a, b)


def _step_pair(dev):
    import clustercontrast.models as M
    from clustercontrast.models.cm import ClusterMemory
    from oracle import ref_torch as O
    o = H.HResNetIBN("50a", pooling_type="gem")
    sd = C.fill(o.state_dict(), "ibn_step")
    o.load_state_dict(sd)
    r = M.create("resnet_ibn50a", pretrained=False, pooling_type="gem")
    r.load_state_dict(sd, strict=True)
    r.to(dev).train()
    o.train()
    D, K = o.num_features, 64
    g = torch.Generator().manual_seed(6)
    bank = F.normalize(torch.randn(K, D, generator=g), dim=1)
    om = O.OClusterMemory(D, K, temp=0.05, momentum=0.1, use_hard=True)
    om.features = bank.clone()
    rm = ClusterMemory(D, K, temp=0.05, momentum=0.1, use_hard=True).to(dev)
    rm.features = bank.clone().to(dev)
    x = O.synth_images(8, 64, 32, seed=10)
    labels = torch.randint(0, K, (2,), generator=g).repeat_interleave(4)
    return O, o, r, om, rm, x, labels


@pytest.fixture(scope="module")
def host_step():
    """the host-model step, computed once for both runs of the device step"""
    def run(dev):
        if "res" not in run.__dict__:
            O, o, r, om, rm, x, labels = _step_pair(dev)
            opt = torch.optim.Adam([{"params": [p]} for p in o.parameters() if p.requires_grad], lr=3.5e-4, weight_decay=5e-4)
            run.res = (O.o_cc_step(o, om, opt, x, labels), om.features.clone())
        return run.res
    return run


@pytest.mark.parametrize("force_reduce", [False, True], ids=["plain", "reducer"])
def test_cc_trainer_step_resnet_ibn50a(dev, monkeypatch, host_step, force_reduce):
    """One ClusterContrastTrainer.step with resnet_ibn50a, GeM and the hard cluster memory on 8 crops of 64 x 32: loss and updated
    bank within 1e-3 of the host-model step (the bounds of test_cc_gpu.test_cc_trainer_step_resnet50); `reducer`: the same step
    through the data-parallel gradient reducer on one rank (stage hooks collect the IN / BN children's parameters)."""
    import torch.distributed as dist
    from clustercontrast.trainers import ClusterContrastTrainer
    from rg_hip import optim as roptim
    monkeypatch.setenv("RG_FORCE_REDUCE", "1" if force_reduce else "0")
    lo, bank_o = host_step(dev)
    started = False
    if force_reduce and not dist.is_initialized():
        dist.init_process_group("nccl", init_method="tcp://127.0.0.1:29641", rank=0, world_size=1)
        started = True
    try:
        O, o, r, om, rm, x, labels = _step_pair(dev)
        ropt = roptim.Adam([{"params": [p]} for p in r.parameters() if p.requires_grad], lr=3.5e-4, weight_decay=5e-4)
        trainer = ClusterContrastTrainer(r, rm)
        seen, launched = set(), []
        if force_reduce:
            red = trainer._reducers.get(ropt, r)              # what step() does first: the reducer and its stage hooks
            hook = r.base[0].__dict__.get("_rg_stage_hook")
            assert red.active() and hook is not None

            def recording(tape, params):
                seen.update(id(p) for p in params)
                launched.append(hook(tape, params))
                return launched[-1]
            r.base[0].__dict__["_rg_stage_hook"] = recording
        lr = trainer.step(x.to(dev), labels.to(dev), ropt).item()
        if force_reduce:
            ibn = r.base[4][0].bn1
            assert all(id(p) in seen for p in ibn.parameters()) and len(list(ibn.parameters())) == 4
            assert len(launched) == 5 and all(n > 0 for n in launched), launched      # layer4..layer1 and the stem
        torch.cuda.synchronize()
    finally:
        if started:
            dist.destroy_process_group()
    print("step loss: device %.6f, host model %.6f (rel %.2e)" % (lr, lo, abs(lr - lo) / abs(lo)))
    assert abs(lr - lo) <= 1e-3 * abs(lo), (lr, lo)
    _check_l2(rm.features, bank_o, 1e-3, "bank after the step")
