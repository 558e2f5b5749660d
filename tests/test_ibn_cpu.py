"""CPU: the IBN-a encoders' public interface (registry, state_dict layout, local checkpoints) and the host model of
tests/ibn_hostmodel.py against the values tests/golden/make_golden_ibn.py recorded from the reference's own modules.
No reference and no GPU needed."""
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

from tests import ibn_hostmodel as H
from tests.golden import cases_ibn as C
from tests.golden.cases import recording_threads, sub

GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "reference_ibn.npz"))


@pytest.fixture(autouse=True, scope="module")
def _threads_of_the_recording():
    with recording_threads():
        yield


def _cmp(got, key, tol=1e-5):
    ref = GOLD[key]
    got = np.asarray(got.detach().numpy() if torch.is_tensor(got) else got, dtype=np.float64).reshape(ref.shape)
    scale = max(np.abs(ref).max(), 1e-12)
    err = np.abs(got - ref).max()
    assert err <= tol * scale + 1e-12, "%s: %.3e vs scale %.3e (rel %.2e > %.1e)" % (key, err, scale, err / scale, tol)


# ---- the host model reproduces the reference ----------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(C.LAYER_SHAPES)))
def test_hostmodel_ibn_layer(i):
    m = H.HIBN(C.LAYER_SHAPES[i][1])
    m.load_state_dict(C.fill(m.state_dict(), "ibn_layer%d" % i))
    m.train()
    x, dy = C.layer_input(i)
    x.requires_grad_(True)
    y = m(x)
    y.backward(dy)
    sd = m.state_dict()
    for name, v in zip(("y", "dx", "d_in_w", "d_in_b", "d_bn_w", "d_bn_b", "running_mean", "running_var"),
                       (y, x.grad, m.IN.weight.grad, m.IN.bias.grad, m.BN.weight.grad, m.BN.bias.grad, sd["BN.running_mean"],
                        sd["BN.running_var"])):
        _cmp(v, "layer%d_%s" % (i, name))
    assert int(sd["BN.num_batches_tracked"]) == 1


def test_hostmodel_bottleneck():
    cin, w = C.BLOCK["cin"], C.BLOCK["width"]
    m = H.bottleneck(cin, w, 1, nn.Sequential(nn.Conv2d(cin, 4 * w, 1, 1, bias=False), nn.BatchNorm2d(4 * w)))
    m.load_state_dict(C.fill(m.state_dict(), "ibn_block"))
    m.train()
    x, dy = C.block_input()
    x.requires_grad_(True)
    y = m(x)
    y.backward(dy)
    _cmp(y, "block_y")
    _cmp(x.grad, "block_dx")


@pytest.fixture(scope="module")
def host_encoder():
    m = H.HResNetIBN(C.MODEL["depth"], **C.MODEL["kw"])
    return m, C.fill(m.state_dict(), "ibn_model")


@pytest.mark.parametrize("mode", ["train", "eval"])
def test_hostmodel_encoder(host_encoder, mode):
    """Tolerance: 2e-5 (the full-trunk figure of make_golden.py), or 4 x the reference's own distance from the fp64 run of the
    same network where that is larger (`*_ref_vs_fp64`, measured when the fixture was recorded: with 4 crops of 64 x 32 the
    layer-3 instances hold 8 values, and the train-mode embedding is 4.7e-4, its gradients about 1e-2 from fp64; eval-mode
    gradients about 1e-3).  The factor is the one tests/test_modules_gpu._check_anchored gives a second fp32 implementation."""
    m, sd = host_encoder
    m.load_state_dict(sd)
    getattr(m, mode)()
    m.zero_grad()
    x, dy = C.model_input()
    x.requires_grad_(True)
    emb = m(x)
    (emb * dy).sum().backward()
    params, st = dict(m.named_parameters()), m.state_dict()
    rec = {"emb": emb, "dx": x.grad}
    rec.update({"grad:" + k: params[k].grad for k in C.GRAD_KEYS})
    for k, v in rec.items():
        key = "model_%s_%s" % (mode, k)
        tol = max(2e-5, 4.0 * float(GOLD[key + "_ref_vs_fp64"]))
        s, stats = sub(v, 2048)
        _cmp(s, key, tol)
        _cmp(stats, key + "_stats", tol)
    for k in ("running_mean", "running_var", "num_batches_tracked"):
        _cmp(st[C.STATS_LAYER + k].double(), "model_%s_stat:%s" % (mode, k), 2e-5)


# ---- public interface ---------------------------------------------------------------------------------------------------------
def test_registry_lists_the_ibn_encoders():
    import clustercontrast.models as M
    assert "resnet_ibn50a" in M.names() and "resnet_ibn101a" in M.names()
    with pytest.raises(KeyError):
        M.create("resnet_bip50")


@pytest.mark.parametrize("name", ["resnet_ibn50a", "resnet_ibn101a"])
def test_state_dict_layout_is_the_reference_s(name):
    import clustercontrast.models as M
    sd = M.create(name, pretrained=False).state_dict()
    assert list(sd.keys()) == [str(k) for k in GOLD[name + "_keys"]]
    assert [";".join(map(str, v.shape)) for v in sd.values()] == [str(s) for s in GOLD[name + "_shapes"]]


def test_train_mode_returns_the_embedding_alone_and_ibn_sits_in_layers_1_to_3():
    import clustercontrast.models as M
    from rg_hip import nn as rnn
    m = M.create("resnet_ibn50a", pretrained=False)
    assert m._returns_map is False and M.create("resnet50", pretrained=False)._returns_map is True
    kinds = [[type(blk.bn1) for blk in m.base[i]] for i in (4, 5, 6, 7)]
    assert all(k is rnn.IBN for layer in kinds[:3] for k in layer) and all(k is rnn.BatchNorm2d for k in kinds[3])
    assert sum(len(layer) for layer in kinds[:3]) == 13 and m.base[7][0].conv2.stride == (1, 1)
    ibn = m.base[5][0].bn1
    assert ibn.half == 64 and ibn.IN.weight.shape == (64,) and ibn.BN.weight.shape == (64,)
    assert (ibn.IN.weight == 1).all() and (ibn.IN.bias == 0).all()


def _reference_format_checkpoint(path, depth):
    """what the reference reads from ./examples/pretrained/resnet50_ibn_a.pth.tar: {'state_dict': {'module.<key>': tensor}}"""
    from rg_hip.resnet_trunk import IBNResNet
    sd = C.fill(IBNResNet(depth).state_dict(), "ckpt")
    torch.save({"state_dict": {"module." + k: v for k, v in sd.items()}, "epoch": 90}, path)
    return sd


def test_pretrained_loads_a_local_reference_checkpoint(tmp_path, monkeypatch):
    import clustercontrast.models as M
    path = str(tmp_path / "resnet50_ibn_a.pth.tar")
    sd = _reference_format_checkpoint(path, "50a")
    monkeypatch.setenv("RG_RESNET_IBN50A_WEIGHTS", path)
    m = M.create("resnet_ibn50a", pretrained=True, pooling_type="gem")
    got = m.state_dict()
    for src, dst in (("conv1.weight", "base.0.weight"), ("layer1.0.bn1.IN.weight", "base.4.0.bn1.IN.weight"),
                     ("layer2.3.bn1.BN.running_var", "base.5.3.bn1.BN.running_var"), ("layer4.2.bn3.bias", "base.7.2.bn3.bias")):
        assert torch.equal(got[dst], sd[src]), dst
    # strict: a checkpoint without one of the IBN tensors is refused
    ck = torch.load(path)
    del ck["state_dict"]["module.layer3.5.bn1.IN.bias"]
    torch.save(ck, path)
    with pytest.raises(RuntimeError, match="layer3.5.bn1.IN.bias"):
        M.create("resnet_ibn50a", pretrained=True)


def test_pretrained_without_a_checkpoint_says_what_to_do(tmp_path, monkeypatch):
    import clustercontrast.models as M
    monkeypatch.delenv("RG_RESNET_IBN101A_WEIGHTS", raising=False)
    monkeypatch.chdir(tmp_path)                         # the reference's relative path does not exist here
    with pytest.raises(RuntimeError, match="RG_RESNET_IBN101A_WEIGHTS"):
        M.create("resnet_ibn101a", pretrained=True)


# ---- eval-mode folding ---------------------------------------------------------------------------------------------------------
def test_fold_group_pairs():
    """a plain trunk hands its FoldGroup every (conv, BatchNorm) pair, in the order it always did; an IBN trunk hands it the
    same list without the 13 conv1 -> IBN pairs"""
    import clustercontrast.models as M
    from rg_hip import nn as rnn
    from rg_hip.resnet_trunk import _conv_bn_pairs
    mods = list(M.create("resnet50", pretrained=False).base)
    want = [(mods[0], mods[1])]
    for layer in mods[4:]:
        for blk in layer:
            want += [(blk.conv1, blk.bn1), (blk.conv2, blk.bn2), (blk.conv3, blk.bn3)]
            if blk.downsample is not None:
                want.append((blk.downsample[0], blk.downsample[1]))
    got = _conv_bn_pairs(mods)
    assert len(got) == 53 and all(a is c and b is d for (a, b), (c, d) in zip(got, want))
    mods = list(M.create("resnet_ibn50a", pretrained=False).base)
    got = _conv_bn_pairs(mods)
    assert len(got) == 53 - 13 and all(isinstance(bn, rnn._BatchNorm) for _, bn in got)
    ibn_convs = {id(blk.conv1) for layer in mods[4:7] for blk in layer}
    assert not any(id(conv) in ibn_convs for conv, _ in got)


# ---- C ABI: argument checks answer before any launch, so they run without a GPU ------------------------------------------------
def test_entry_points_reject_bad_arguments_before_launching():
    from rg_hip.lib import lib
    p = 4096                                            # stands for a device address; never dereferenced: every call below is refused
    geom = [2, 8, 16, 4, 1]                             # N, C, HW, half, train

    def fwd(residual=None, half=4, act=0, x=p):
        return lib.rg_ibn_fwd(x, p, p, p, p, residual, p, p, p, p, p, p, p, geom[0], geom[1], geom[2], half, 1, 1e-5, 1e-5, 0.1, act,
                              None, 0, None)
    for kw, msg in ((dict(x=None), "bad arguments"), (dict(residual=p), "no residual input"), (dict(half=0), "split point"),
                    (dict(half=8), "split point"), (dict(act=2), "none or ReLU")):
        with pytest.raises(RuntimeError, match=msg):
            fwd(**kw)
    with pytest.raises(RuntimeError, match="forward output"):          # fused ReLU without y
        lib.rg_ibn_bwd(p, p, None, p, p, p, p, p, p, p, p, p, p, p, *geom, 1e-5, 1, p, 1 << 20, None)
    with pytest.raises(RuntimeError, match="workspace too small"):
        lib.rg_ibn_bwd(p, p, None, p, p, p, p, p, p, p, p, p, p, p, *geom, 1e-5, 0, p, 16, None)
    assert lib.rg_ibn_workspace(2, 8, 16, 4) >= 2 * 2 * 8 * 4 and lib.rg_ibn_workspace(2, 8, 16, 8) == 0
