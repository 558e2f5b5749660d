"""GPU: rg_hip.nn.DSBN2d / DSBN1d and clustercontrast.models.dsbn (convert_dsbn / convert_bn) against the values recorded from the
reference's own dsbn.py (tests/golden/reference_dsbn.npz; tests/test_dsbn_cpu.py ties the host model to the same records).

Tolerances: the layer records are fp32 torch outputs within 2e-7 of fp64 (printed by make_golden_dsbn.py); a second fp32
implementation is held to 2e-5 of the record's largest magnitude, the floor make_golden_ibn.py uses.  The tree records carry the
reference's own distance to the fp64 run of the same tree, and the bound is max(2e-5, 4 x that distance) as there."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import dsbn_hostmodel as D
from tests.golden import cases_dsbn as C
from tests.golden.cases import sub

pytestmark = pytest.mark.gpu

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_dsbn.npz"))
TOL = 2e-5


def _close(got, want, what, tol=TOL):
    got = torch.as_tensor(np.asarray(got, dtype=np.float64)) if not torch.is_tensor(got) else got.detach().double().cpu()
    want = torch.as_tensor(np.asarray(want, dtype=np.float64))
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert bool(torch.isfinite(got).all()), what
    err, scale = (got - want).abs().max().item(), max(want.abs().max().item(), 1e-12)
    print("%-60s max err %.3e scale %.3e" % (what, err, scale))
    assert err <= tol * scale + 1e-12, "%s: max err %.3e, scale %.3e, tol %.1e" % (what, err, scale, tol)


@pytest.mark.parametrize("i", range(len(C.LAYERS)))
def test_layer_vs_reference(dev, i):
    from rg_hip import nn as rnn
    shape, dims = C.LAYERS[i]
    layer = (rnn.DSBN2d if dims == 2 else rnn.DSBN1d)(shape[1])
    assert layer.num_features == shape[1] and isinstance(layer.BN_T, rnn.BatchNorm2d if dims == 2 else rnn.BatchNorm1d)
    layer.load_state_dict(C.layer_state(i, layer.state_dict()), strict=True)
    layer.to(dev).train()
    x, dy = C.layer_input(i)
    xi = x.to(dev).requires_grad_(True)
    y = layer(xi)
    y.backward(dy.to(dev))
    got = [y, xi.grad, layer.BN_S.weight.grad, layer.BN_S.bias.grad, layer.BN_T.weight.grad, layer.BN_T.bias.grad,
           layer.BN_S.running_mean, layer.BN_S.running_var, layer.BN_S.num_batches_tracked,
           layer.BN_T.running_mean, layer.BN_T.running_var, layer.BN_T.num_batches_tracked]
    layer.eval()
    with torch.no_grad():
        got.append(layer(x.to(dev)))
    for name, g in zip(C.LAYER_NAMES, got):
        _close(g, GOLD["layer%d_%s" % (i, name)], "DSBN%dd %s" % (dims, name))
    sd = layer.state_dict()
    assert sd["BN_S.num_batches_tracked"].item() == 1 and sd["BN_T.num_batches_tracked"].item() == 1
    with pytest.raises(AssertionError):
        layer.train()(x[:3].to(dev))


def _tree(dev, mode):
    from clustercontrast.models.dsbn import convert_dsbn
    tree = D.rtree()
    convert_dsbn(tree)
    assert list(tree.state_dict().keys()) == list(GOLD["tree_keys"])
    tree.load_state_dict(C.fill(tree.state_dict(), "dsbn_tree"), strict=True)
    tree.to(dev)
    return tree.train() if mode == "train" else tree.eval()


def test_converted_tree_train_step_vs_reference(dev):
    """one train forward / backward of the converted stem + Bottleneck + BatchNorm1d tree: every DSBN layer runs behind its
    convolution through conv_bn_tf / conv_bn_tb's unfused branch, with the residual add and ReLU epilogues in the forward and the
    dy_masked / mask_input epilogues in the backward"""
    tree = _tree(dev, "train")
    x, dy = C.tree_input()
    xi = x.to(dev).requires_grad_(True)
    emb = tree(xi)
    (emb * dy.to(dev)).sum().backward()
    params, sd = dict(tree.named_parameters()), tree.state_dict()
    rec = {"emb": emb, "dx": xi.grad}
    rec.update(("grad:" + k, params[k].grad) for k in C.TREE_GRAD_KEYS)
    rec.update(("stat:" + k, sd[k]) for k in C.TREE_STATS)
    for k, v in rec.items():
        assert v is not None, k
        tol = max(2e-5, 4.0 * float(GOLD["tree_train_%s_ref_vs_fp64" % k]))
        _close(sub(v.cpu(), 2048)[0] if v.numel() > 2048 else v, GOLD["tree_train_" + k], "tree train " + k, tol)


def test_converted_tree_eval_and_convert_bn_vs_reference(dev):
    from clustercontrast.models.dsbn import convert_bn
    x = C.tree_input()[0].to(dev)
    tree = _tree(dev, "eval")
    with torch.no_grad():
        y_dsbn = tree(x)
    _close(y_dsbn, GOLD["tree_eval_T"], "converted tree, eval mode")
    for use_target, tag in ((True, "tree_eval_T"), (False, "tree_eval_S")):
        t2 = _tree(dev, "eval")
        convert_bn(t2, use_target=use_target)
        assert not any(".BN_" in k for k in t2.state_dict())
        with torch.no_grad():
            y = t2(x)
        _close(y, GOLD[tag], tag)
        if use_target:
            assert torch.equal(y, y_dsbn), "the folded path of a DSBN tree is not its BN_T"


def test_caches_of_replaced_modules_are_dropped(dev):
    """a model evaluated BEFORE convert_dsbn (its FoldGroup and per-convolution folds now exist) gives the converted result after.
    The drop itself is what the attribute asserts check; the values alone would also come out right over a stale FoldGroup, because
    _fold_of re-folds a pair whose BatchNorm tensors changed."""
    from clustercontrast.models.dsbn import convert_dsbn
    x = C.tree_input()[0].to(dev)
    tree = D.rtree()
    tree.load_state_dict(C.fill(tree.state_dict(), "plain"))
    tree.to(dev).eval()
    with torch.no_grad():
        y0 = tree(x)
    assert getattr(tree.base[0], "_rg_fold_group", None) is not None and getattr(tree.base[0], "_rg_fold", None) is not None
    tree.__dict__["_rg_graphs"] = {"stale": None}
    convert_dsbn(tree)
    assert "_rg_graphs" not in tree.__dict__ and "_rg_fold_group" not in tree.base[0].__dict__
    with torch.no_grad():
        assert torch.equal(tree(x), y0)                  # both children start from the replaced BatchNorm's state
    tree.load_state_dict({k: v.to(dev) for k, v in C.fill(tree.state_dict(), "dsbn_tree").items()}, strict=True)
    with torch.no_grad():
        y1 = tree(x)
    _close(y1, GOLD["tree_eval_T"], "evaluated before and after convert_dsbn")


def test_resnet50_convert_load_step_eval(dev):
    import clustercontrast.models as M
    from clustercontrast.models.cm import ClusterMemory
    from clustercontrast.models.dsbn import convert_bn, convert_dsbn
    from clustercontrast.trainers import ClusterContrastTrainer
    from oracle import ref_torch as O
    from rg_hip import nn as rnn
    from rg_hip import optim as roptim
    torch.manual_seed(5)
    model = M.create("resnet50", pretrained=False, num_classes=0)
    convert_dsbn(model)
    filled = C.fill(model.state_dict(), "dsbn_r50")
    assert sum(".BN_S." in k for k in filled) == sum(".BN_T." in k for k in filled) == 5 * 54
    model.load_state_dict(filled, strict=True)
    model.to(dev).train()
    Dm, K = model.num_features, 16
    g = torch.Generator().manual_seed(6)
    mem = ClusterMemory(Dm, K, temp=0.05, momentum=0.1).to(dev)
    mem.features = F.normalize(torch.randn(K, Dm, generator=g), dim=1).to(dev)
    opt = roptim.Adam([{"params": [p]} for p in model.parameters() if p.requires_grad], lr=3.5e-4, weight_decay=5e-4)
    x = O.synth_images(8, 64, 32, seed=12)
    x[4:] = 0.5 * x[4:] + 0.7
    x = x.to(dev)
    labels = torch.tensor([0, 0, 3, 3, 5, 5, 9, 9], device=dev)
    loss = ClusterContrastTrainer(model, mem).step(x, labels, opt).item()
    assert np.isfinite(loss)
    n = 0
    for name, m in model.named_modules():
        if isinstance(m, rnn._DSBN):
            assert m.BN_S.num_batches_tracked.item() == 1 and m.BN_T.num_batches_tracked.item() == 1, name
            for bn in (m.BN_S, m.BN_T):
                for p in (bn.weight, bn.bias):
                    if p.requires_grad:
                        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), name
                        n += 1
    assert n == 4 * 54

    # eval: the converted model IS its BN_T, through the folded convolutions
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    model.eval()
    with torch.no_grad():
        y_dsbn = model(x)
    assert getattr(model.base[0], "_rg_fold_group", None) is not None and model.base[0]._rg_fold_group.usable()
    convert_bn(model, use_target=True)
    model.eval()
    with torch.no_grad():
        y_t = model(x)
    assert torch.equal(y_dsbn, y_t)
    convert_dsbn(model)
    model.load_state_dict(sd, strict=True)
    convert_bn(model, use_target=False)
    model.eval()
    with torch.no_grad():
        y_s = model(x)
    assert (y_s - y_t).abs().max().item() > 1e-3
