"""The multi-part encoder on the MI355X: resnet_mp50 in train and eval mode on the fixture's two crop sizes and both poolings against
the values recorded from the reference's own modules (tests/golden/reference_mp.npz, bound max(2e-5, 4 x the reference's recorded
distance from fp64)), the parameters a fusion leaves without gradient, launch accounting on the rg_hip.lib entry points, and one
ClusterContrastPartTrainer.step against the host-model step (tests/mp_hostmodel.py)."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import mp_hostmodel as H
from tests.golden import cases_mp as C
from tests.test_modules_gpu import _check_anchored, _check_l2
from tests.test_mp_cpu import vs_fixture

pytestmark = pytest.mark.gpu

GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "reference_mp.npz"))


def _cmp(got, key, tol):
    ref = GOLD[key]
    got = np.asarray(got.detach().cpu().numpy() if torch.is_tensor(got) else got, dtype=np.float64).reshape(ref.shape)
    err = np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-12)
    print("%s: rel err vs the recorded reference %.3e (bound %.1e)" % (key, err, tol))
    assert err <= tol, "%s: %.3e > %.1e" % (key, err, tol)


def _encoder(dev, name):
    import clustercontrast.models as M
    kw = C.CASES[name][0]
    r = M.create("resnet_mp50", pretrained=False, **kw)
    r.load_state_dict(C.fill(r.state_dict(), "mp_" + name), strict=True)
    return r.to(dev)


def _record(dev, r, name, mode):
    """cases_mp.record's quantities from the device encoder"""
    x, dys = C.model_input(name)
    if mode != "train":
        r.eval()
        with torch.no_grad():
            out = r(x.to(dev), **C.EVAL_CALLS[mode])
        return dict(zip(("f_gc", "f_g"), out)) if isinstance(out, tuple) else {"f_gc": out}
    r.train()
    r.zero_grad()
    xi = x.to(dev).requires_grad_(True)
    outs = r(xi)
    assert isinstance(outs, tuple) and len(outs) == 4 and all(o.shape == (x.shape[0], 2048) for o in outs)
    sum((o * dy.to(dev)).sum() for o, dy in zip(outs, dys)).backward()
    rec = dict(zip(C.OUTPUTS, outs))
    rec["dx"] = xi.grad
    params, sd = dict(r.named_parameters()), r.state_dict()
    for k in C.grad_keys(name):
        rec["grad:" + k] = params[k].grad
    for layer in C.STATS_LAYERS:
        for k in ("running_mean", "running_var", "num_batches_tracked"):
            rec["stat:" + layer + k] = sd[layer + k]
    return rec, sorted(k for k, p in params.items() if p.grad is None)


@pytest.mark.parametrize("name", list(C.CASES))
def test_resnet_mp50_train(dev, name):
    """the four outputs, dx, the listed gradients and the running statistics (feat_bn_gan's included) of a train-mode pass with
    fusion='sum' and a gradient for all four outputs; the parameters without gradient are the reference's"""
    r = _encoder(dev, name)
    rec, gradless = _record(dev, r, name, "train")
    assert gradless == [str(k) for k in GOLD[name + "_gradless"]]
    vs_fixture({k: v.detach().cpu() for k, v in rec.items()}, name, "train", cmp=_cmp)
    for bn in (r.feat_bn_g, r.feat_bn_p1, r.feat_bn_p2, r.feat_bn_gan):
        assert int(bn.num_batches_tracked) == 1


@pytest.mark.parametrize("name", list(C.CASES))
def test_resnet_mp50_eval(dev, name):
    """f_gc, clustering=True, fusion='cat' and fusion='g' in eval mode; nothing is updated"""
    r = _encoder(dev, name)
    before = {k: v.clone() for k, v in r.state_dict().items() if "running" in k or "num_batches" in k}
    for mode in C.EVAL_CALLS:
        rec = _record(dev, r, name, mode)
        assert set(rec) == ({"f_gc", "f_g"} if mode == "eval_clustering" else {"f_gc"})
        vs_fixture({k: v.cpu() for k, v in rec.items()}, name, mode, cmp=_cmp)
    after = r.state_dict()
    assert all(torch.equal(after[k], v) for k, v in before.items())


def _wrap(monkeypatch, lib, names):
    """{entry point: [argument tuple of every call]}"""
    calls = {n: [] for n in names}
    for n in names:
        fn = getattr(lib, n)

        def counted(*a, _n=n, _fn=fn):
            calls[_n].append(a)
            return _fn(*a)
        monkeypatch.setattr(lib, n, counted, raising=False)
    return calls


def test_launch_accounting(dev, monkeypatch):
    """an eval forward makes ONE rg_part_pool_fwd and ONE rg_mp_head_fwd call (one kernel in eval mode, two in train mode: see
    csrc/part_head.hip) and no slice / concatenation / separate BatchNorm1d / row normalisation launch; a train forward the same
    calls plus the statistics-only pass of feat_bn_gan"""
    from rg_hip.lib import lib
    r = _encoder(dev, "gem64")
    x, _ = C.model_input("gem64")
    xd = x.to(dev)
    r.eval()
    with torch.no_grad():
        r(xd)                                            # folds the frozen BatchNorms, fills the caches
    names = ["rg_part_pool_fwd", "rg_mp_head_fwd", "rg_copy_channels", "rg_gem_pool_fwd", "rg_global_avgpool_fwd", "rg_l2norm_rows_fwd",
             "rg_bn_apply_fwd", "rg_bn_stats", "rg_axpby"]
    calls = _wrap(monkeypatch, lib, names)
    with torch.no_grad():
        r(xd)
    n = {k: len(v) for k, v in calls.items()}
    assert n["rg_part_pool_fwd"] == 1 and n["rg_mp_head_fwd"] == 1 and n["rg_gem_pool_fwd"] == 1, n     # the latter: x_g's pool
    assert n["rg_copy_channels"] == 0 and n["rg_l2norm_rows_fwd"] == 0 and n["rg_bn_apply_fwd"] == 0, n
    assert n["rg_bn_stats"] == 0 and n["rg_axpby"] == 0, n
    for k in calls:
        del calls[k][:]
    r.train()
    outs = r(xd)
    n = {k: len(v) for k, v in calls.items()}
    assert n["rg_part_pool_fwd"] == 1 and n["rg_mp_head_fwd"] <= 2 and n["rg_copy_channels"] == 0 and n["rg_l2norm_rows_fwd"] == 0, n
    # feat_bn_gan: one statistics pass that updates its running statistics, and no normalised map (its gamma meets no apply launch)
    gan = r.feat_bn_gan
    assert sum(a[3] == gan.running_mean.data_ptr() and a[4] == gan.running_var.data_ptr() for a in calls["rg_bn_stats"]) == 1
    head = [bn.weight.data_ptr() for bn in (gan, r.feat_bn_g, r.feat_bn_p1, r.feat_bn_p2)]
    assert not any(a[3] in head for a in calls["rg_bn_apply_fwd"]), "a head BatchNorm ran through the separate apply kernel"
    del outs


@pytest.mark.parametrize("fusion,outputs", [("sum", (3,)), ("g", (3,)), ("sum", (0,)), ("cat", (3,))],
                         ids=["sum_f_gc", "g_f_gc", "sum_f_g", "cat_f_gc"])
def test_parameters_outside_the_fusion_get_no_gradient_and_do_not_move(dev, fusion, outputs):
    """a parameter that takes no part in the chosen fusion / the used outputs has grad None, and one Adam step with weight decay
    leaves it unchanged bit for bit (torch's Adam skips a parameter without gradient)"""
    from rg_hip import optim as roptim
    o = H.HResNetMP(50, norm=True, pooling_type="gem")
    sd = C.fill(o.state_dict(), "mp_gem64")
    o.load_state_dict(sd)
    import clustercontrast.models as M
    r = M.create("resnet_mp50", pretrained=False, norm=True, pooling_type="gem")
    r.load_state_dict(sd, strict=True)
    r.to(dev).train()
    o.train()
    x, dys = C.model_input("gem64")
    outs_o = o(x, fusion=fusion)
    sum((outs_o[k] * dys[k]).sum() for k in outputs).backward()
    want = sorted(k for k, p in o.named_parameters() if p.grad is None)
    opt = roptim.Adam([{"params": [p]} for p in r.parameters() if p.requires_grad], lr=3.5e-4, weight_decay=5e-4)
    before = {k: p.detach().clone() for k, p in r.named_parameters()}
    opt.zero_grad()
    outs = r(x.to(dev), fusion=fusion)
    sum((outs[k] * dys[k].to(dev)).sum() for k in outputs).backward()
    got = sorted(k for k, p in r.named_parameters() if p.grad is None)
    assert got == want, (set(got) ^ set(want))
    if fusion == "g" or outputs == (0,):
        assert "res_p.0.conv1.weight" in got and "feat_bn_p1.weight" in got and "res_g.0.conv1.weight" not in got
    opt.step()
    torch.cuda.synchronize()
    after = dict(r.named_parameters())
    for k in got:
        assert torch.equal(after[k].detach(), before[k]), k
    moved = [k for k in before if k not in got and not torch.equal(after[k].detach(), before[k])]
    assert "base.0.weight" in moved and "res_g.2.conv3.weight" in moved
    if fusion == "cat":
        # the unfused path's gradients (fc_id layers, and through the head's dz inputs), anchored on an fp64 run of the host model
        import copy
        o64 = copy.deepcopy(o).double()
        o64.zero_grad()
        outs64 = o64(x.double(), fusion=fusion)
        sum((outs64[k] * dys[k].double()).sum() for k in outputs).backward()
        po, p64 = dict(o.named_parameters()), dict(o64.named_parameters())
        for k in ("fc_id_g.weight", "fc_id_p1.weight", "fc_id_p2.weight", "feat_bn_g.weight", "feat_bn_p2.weight", "gpool2d.p"):
            _check_anchored(after[k].grad, po[k].grad, p64[k].grad, k)


def _step_pair(dev):
    import clustercontrast.models as M
    from clustercontrast.models.cm import ClusterMemory
    from oracle import ref_torch as O
    o = H.HResNetMP(50, norm=True, pooling_type="gem")
    sd = C.fill(o.state_dict(), "mp_step")
    o.load_state_dict(sd)
    r = M.create("resnet_mp50", pretrained=False, norm=True, pooling_type="gem")
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
    x = O.synth_images(16, 64, 32, seed=10)
    labels = torch.randint(0, K, (4,), generator=g).repeat_interleave(4)
    return O, o, r, om, rm, x, labels


@pytest.fixture(scope="module")
def host_step():
    """the host-model step, computed once for both runs of the device step"""
    def run(dev):
        if "res" not in run.__dict__:
            O, o, r, om, rm, x, labels = _step_pair(dev)
            opt = torch.optim.Adam([{"params": [p]} for p in o.parameters() if p.requires_grad], lr=3.5e-4, weight_decay=5e-4)
            run.res = (H.part_step(o, om, opt, x, labels, 0.05, 4), om.features.clone())
        return run.res
    return run


_STEP_RESULTS = {}


@pytest.mark.parametrize("force_reduce", [False, True], ids=["plain", "reducer"])
def test_part_trainer_step(dev, monkeypatch, host_step, force_reduce):
    """One ClusterContrastPartTrainer.step (group size 4, GeM, the hard cluster memory) on 16 crops of 64 x 32 — the group contrast
    takes group_size^2 rows: loss and updated bank within 1e-3 of the host-model step (the bound of
    test_cc_trainer_step_resnet_ibn50a); `reducer`: the same step through the data-parallel gradient reducer on one rank; the two
    runs agree bit for bit."""
    import torch.distributed as dist
    from clustercontrast.trainers import ClusterContrastPartTrainer
    from rg_hip import optim as roptim
    monkeypatch.setenv("RG_FORCE_REDUCE", "1" if force_reduce else "0")
    lo, bank_o = host_step(dev)
    started = False
    if force_reduce and not dist.is_initialized():
        dist.init_process_group("nccl", init_method="tcp://127.0.0.1:29643", rank=0, world_size=1)
        started = True
    try:
        O, o, r, om, rm, x, labels = _step_pair(dev)
        ropt = roptim.Adam([{"params": [p]} for p in r.parameters() if p.requires_grad], lr=3.5e-4, weight_decay=5e-4)
        trainer = ClusterContrastPartTrainer(r, rm, group_size=4, temperature=0.05)
        if force_reduce:
            red = trainer._reducers.get(ropt, r)
            assert red.active() and r.base[0].__dict__.get("_rg_stage_hook") is None      # no stage hook: reduce() takes everything
        lr = trainer.step(x.to(dev), labels.to(dev), ropt).item()
        torch.cuda.synchronize()
    finally:
        if started:
            dist.destroy_process_group()
    print("step loss: device %.6f, host model %.6f (rel %.2e)" % (lr, lo, abs(lr - lo) / abs(lo)))
    assert abs(lr - lo) <= 1e-3 * abs(lo), (lr, lo)
    _check_l2(rm.features, bank_o, 1e-3, "bank after the step")
    _STEP_RESULTS[force_reduce] = (lr, rm.features.clone(), r.base[0].weight.detach().clone(), r.feat_bn_p2.weight.detach().clone())
    if len(_STEP_RESULTS) == 2:
        a, b = _STEP_RESULTS[False], _STEP_RESULTS[True]
        assert a[0] == b[0] and all(torch.equal(u, v) for u, v in zip(a[1:], b[1:])), "plain and reducer steps differ"
