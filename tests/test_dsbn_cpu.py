"""CPU: the DSBN host model (tests/dsbn_hostmodel.py) against the values recorded from the reference's own dsbn.py
(tests/golden/reference_dsbn.npz, written by tests/golden/make_golden_dsbn.py), its dispatch mirrors against the library's own
answers, and convert_dsbn / convert_bn on this build's modules: the recorded key list, the refusals with the model left untouched,
and the odd-batch errors.  No GPU: nothing here launches a kernel."""
import os

import numpy as np
import pytest
import torch

from tests import dsbn_hostmodel as D
from tests.golden import cases_dsbn as C
from tests.golden.cases import RECORDING_THREADS, sub

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_dsbn.npz"))
TOL = 1e-5                                   # make_golden_ibn.check: max error relative to the record's largest magnitude


def _close(got, want, what, tol=TOL):
    got, want = torch.as_tensor(np.asarray(got, dtype=np.float64)), torch.as_tensor(np.asarray(want, dtype=np.float64))
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err, scale = (got - want).abs().max().item(), max(want.abs().max().item(), 1e-12)
    assert err <= tol * scale + 1e-12, "%s: max err %.3e, scale %.3e" % (what, err, scale)


@pytest.mark.parametrize("i", range(len(C.LAYERS)))
def test_host_model_layer_vs_reference(i):
    from tests.golden.make_golden_dsbn import host_layer_record
    import torch.nn as nn
    shape, dims = C.LAYERS[i]
    proto = D.HDSBN(shape[1], dims)
    sd = C.layer_state(i, proto.state_dict())
    x, dy = C.layer_input(i)
    for name, hv in zip(C.LAYER_NAMES, host_layer_record(sd, x, dy)):
        _close(hv.detach().double().numpy(), GOLD["layer%d_%s" % (i, name)], "DSBN%dd %s" % (dims, name))
    assert isinstance(proto.BN_S, nn.BatchNorm2d if dims == 2 else nn.BatchNorm1d)


def test_host_tree_vs_reference():
    from tests.golden.make_golden_dsbn import eval_out, tree_record
    torch.set_num_threads(RECORDING_THREADS)
    host = D.convert_h(C.Tree())
    assert list(host.state_dict().keys()) == list(GOLD["tree_keys"])
    sd = C.fill(host.state_dict(), "dsbn_tree")
    host.load_state_dict(sd)
    x, dy = C.tree_input()
    _close(eval_out(host, x).numpy(), GOLD["tree_eval_T"], "converted tree, eval mode = BN_T")
    for pick, tag in ((".BN_T.", "tree_eval_T"), (".BN_S.", "tree_eval_S")):
        plain = C.Tree()
        plain.load_state_dict({k.replace(pick, "."): v for k, v in sd.items() if pick in k or ".BN_" not in k})
        _close(eval_out(plain, x).numpy(), GOLD[tag], tag)
    for k, v in tree_record(host, x, dy).items():
        tol = max(2e-5, 4.0 * float(GOLD["tree_train_%s_ref_vs_fp64" % k]))
        want = GOLD["tree_train_" + k]
        _close(sub(v, 2048)[0] if v.numel() > 2048 else v.double().numpy(), want, "tree train " + k, tol)


def test_dispatch_mirrors_and_case_lists():
    """the case lists reach every route (asserted while they are built), and the mirrors are the library's own arithmetic"""
    from rg_hip.lib import lib
    one, sl = D.one_launch_cases(), D.slice_cases()
    assert sorted(set(D.dsbn_regime(N, C, HW) for N, C, HW, _ in one if HW % 4 == 0 and HW > 1)) == [("reg", u) for u in (1, 2, 4, 8, 16)]
    shapes = [c[:3] for c in one + sl] + [(256, 64, 8192), (256, 256, 2048), (256, 512, 512), (256, 1024, 128), (256, 2048, 128),
                                          (256, 2048, 1), (2, 1, 1), (8, 63, 4096), (8, 64, 4096), (8, 64, 4097), (2, 1024, 16388)]
    for N, Cc, HW in shapes:
        assert lib.rg_dsbn_one_launch(N, Cc, HW) == int(D.dsbn_one_launch(N, Cc, HW)), (N, Cc, HW)
        assert lib.rg_dsbn_slices(N, Cc, HW) == D.dsbn_slices(N, Cc, HW)[0], (N, Cc, HW)
        assert lib.rg_dsbn_workspace(N, Cc, HW) == D.workspace_bytes(N, Cc, HW), (N, Cc, HW)
    assert lib.rg_dsbn_workspace(5, 64, 16) == 0 and lib.rg_dsbn_one_launch(5, 64, 16) == 0      # odd batch: no geometry
    if os.environ.get("RG_BN_REG", "1") != "0":
        from tests import norm_hostmodel as H
        for N, Cc, HW in shapes:
            assert lib.rg_bn_reg_units(N // 2, Cc, HW) == H.bn_reg_units(N // 2, Cc, HW), (N, Cc, HW)


def _ids(model):
    return [(k, id(m)) for k, m in model.named_modules()]


def test_convert_on_this_builds_modules():
    from clustercontrast.models.dsbn import DSBN1d, DSBN2d, convert_bn, convert_dsbn
    from rg_hip import nn as rnn
    tree = D.rtree()
    plain_sd = C.fill(tree.state_dict(), "plain")
    tree.load_state_dict(plain_sd)
    tree.base[0]._rg_fold_group, tree.base[0]._rg_fold = object(), object()         # caches of the replaced modules
    tree.eval()
    convert_dsbn(tree)
    assert list(tree.state_dict().keys()) == list(GOLD["tree_keys"])
    assert [";".join(map(str, v.shape)) for v in tree.state_dict().values()] == list(GOLD["tree_shapes"])
    assert isinstance(tree.base[1], DSBN2d) and isinstance(tree.base[4][0].downsample[1], DSBN2d) and isinstance(tree.feat_bn, DSBN1d)
    assert tree.base[1].num_features == C.TREE["stem"] and not tree.base[1].training and not tree.base[1].BN_T.training
    assert not hasattr(tree.base[0], "_rg_fold_group") and not hasattr(tree.base[0], "_rg_fold")
    sd = tree.state_dict()
    for k, v in plain_sd.items():                         # both children start from the BatchNorm's state
        for d in ("BN_S.", "BN_T."):
            kk = k if k in sd else k.rsplit(".", 1)[0] + "." + d + k.rsplit(".", 1)[1]
            assert torch.equal(sd[kk], v), kk
    filled = C.fill(sd, "dsbn_tree")
    tree.load_state_dict(filled, strict=True)
    for use_target, d in ((True, ".BN_T."), (False, ".BN_S.")):
        import copy
        t2 = copy.deepcopy(tree)
        convert_bn(t2, use_target=use_target)
        assert list(t2.state_dict().keys()) == list(plain_sd.keys())
        assert isinstance(t2.base[1], rnn.BatchNorm2d) and isinstance(t2.feat_bn, rnn.BatchNorm1d)
        for k, v in t2.state_dict().items():
            src = k if k in filled else k.rsplit(".", 1)[0] + d + k.rsplit(".", 1)[1]
            assert torch.equal(v, filled[src]), (k, src)


@pytest.mark.parametrize("name", ["resnet_ibn50a", "resnet_mp50"])
def test_convert_refuses_fused_consumers_and_changes_nothing(name, capsys):
    import clustercontrast.models as M
    from clustercontrast.models.dsbn import convert_dsbn
    model = M.create(name, pretrained=False, norm=True)
    before, keys = _ids(model), list(model.state_dict().keys())
    with pytest.raises(TypeError) as e:
        convert_dsbn(model)
    assert ("bn1.BN" if name == "resnet_ibn50a" else "feat_bn_g") in str(e.value)
    assert _ids(model) == before and list(model.state_dict().keys()) == keys


@pytest.mark.parametrize("name,kw", [("resnet50", {}), ("resnet50", {"num_features": 64}), ("resnet18", {"cut_at_pooling": True})])
def test_convert_supported_encoders(name, kw):
    import clustercontrast.models as M
    from clustercontrast.models.dsbn import convert_bn, convert_dsbn
    from rg_hip import nn as rnn
    model = M.create(name, pretrained=False, **kw)
    keys = list(model.state_dict().keys())
    n_bn = sum(isinstance(m, rnn._BatchNorm) for m in model.modules())
    convert_dsbn(model)
    assert sum(isinstance(m, rnn._DSBN) for m in model.modules()) == n_bn
    assert len(model.state_dict()) == len(keys) + 5 * n_bn
    convert_bn(model)
    assert list(model.state_dict().keys()) == keys


def test_odd_batch_is_an_error():
    from rg_hip import nn as rnn
    from rg_hip import ops
    from rg_hip.tape import Tape
    for layer, shape in ((rnn.DSBN2d(4), (3, 4, 2, 2)), (rnn.DSBN1d(4), (5, 4))):
        layer.train()
        with pytest.raises(AssertionError):
            layer.tf(Tape(), torch.zeros(shape))
        assert layer.BN_S.num_batches_tracked.item() == 0 and layer.BN_T.num_batches_tracked.item() == 0
    w = torch.ones(4)
    with pytest.raises(RuntimeError, match="halves"):
        ops.dsbn_fwd(torch.zeros(3, 4, 2, 2), w, w, w, w)
    with pytest.raises(RuntimeError, match="halves"):
        ops.dsbn_bwd(torch.zeros(3, 4, 2, 2), torch.zeros(3, 4, 2, 2), None, torch.zeros(2, 2, 4), w, w)
