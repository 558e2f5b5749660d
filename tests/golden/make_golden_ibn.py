"""Generates tests/golden/reference_ibn.npz by running the REFERENCE's own IBN-a modules (build container only; /root/reference
does not exist on the GPU box):

  * CC/clustercontrast/models/resnet_ibn_a.py   IBN (:54-68), Bottleneck (:70-109), ResNet (:112-176)
  * CC/clustercontrast/models/pooling.py        GeneralizedMeanPoolingP
  * CC/clustercontrast/models/resnet_ibn.py     ResNetIBN (:16-121), resnet_ibn50a / resnet_ibn101a

loaded by file path under placeholder parent packages (the package `__init__` files import torchvision, which is not installed in
this image; resnet_ibn.py's own unused `import torchvision` gets an empty module object) — the recipe of make_golden_eval.py /
make_golden.py.  Nothing from the reference is copied: the file stores the reference's OUTPUTS on the seeded weights and inputs of
cases_ibn.py (sub-sampled), and the state_dict key names and shapes of both depths.  Every case is also run through the host model
(tests/ibn_hostmodel.py) and asserted to agree before it is stored.

Usage:  python tests/golden/make_golden_ibn.py
"""
from __future__ import absolute_import, print_function

import importlib.util
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
from tests import ibn_hostmodel as H  # noqa: E402
from tests.golden import cases_ibn as C  # noqa: E402
from tests.golden.cases import sub  # noqa: E402

CC = "/root/reference/cluster-contrast-reid-main"


def load_reference_models():
    root = types.ModuleType("cc_ref_ibn")
    root.__path__ = [CC + "/clustercontrast"]
    models = types.ModuleType("cc_ref_ibn.models")
    models.__path__ = [CC + "/clustercontrast/models"]
    sys.modules.update({"cc_ref_ibn": root, "cc_ref_ibn.models": models})
    sys.modules.setdefault("torchvision", types.ModuleType("torchvision"))
    mods = {}
    for name in ("resnet_ibn_a", "pooling", "resnet_ibn"):
        full = "cc_ref_ibn.models." + name
        spec = importlib.util.spec_from_file_location(full, "%s/clustercontrast/models/%s.py" % (CC, name))
        mod = importlib.util.module_from_spec(spec)
        sys.modules[full] = mod
        spec.loader.exec_module(mod)
        mods[name] = mod
    return mods


def check(a, b, what, tol=1e-5):
    a, b = a.detach().double(), b.detach().double()
    err = (a - b).abs().max().item()
    scale = max(b.abs().max().item(), 1e-12)
    print("  %-44s max|host-ref| = %.3e (scale %.3e, rel %.2e)" % (what, err, scale, err / scale))
    assert err <= tol * scale + 1e-12, what


def rel_err(a, b):
    a, b = a.detach().double(), b.detach().double()
    return (a - b).abs().max().item() / max(b.abs().max().item(), 1e-12)


def model_record(net, mode, x, dy):
    """one forward / backward of an encoder -> {name: tensor}"""
    getattr(net, mode)()
    net.zero_grad()
    xi = x.clone().requires_grad_(True)
    emb = net(xi)
    (emb * dy).sum().backward()
    sd = net.state_dict()
    rec = {"emb": emb.detach(), "dx": xi.grad}
    params = dict(net.named_parameters())
    for k in C.GRAD_KEYS:
        rec["grad:" + k] = params[k].grad
    for k in ("running_mean", "running_var", "num_batches_tracked"):
        rec["stat:" + k] = sd[C.STATS_LAYER + k].clone()
    return rec


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    R = load_reference_models()
    out = {}

    # ---- (a) the IBN layer alone, one train step ----------------------------------------------------------------------
    for i, shape in enumerate(C.LAYER_SHAPES):
        ref, host = R["resnet_ibn_a"].IBN(shape[1]), H.HIBN(shape[1])
        sd = C.fill(ref.state_dict(), "ibn_layer%d" % i)
        x, dy = C.layer_input(i)
        res = []
        for m in (ref, host):
            m.load_state_dict(sd)
            m.train()
            xi = x.clone().requires_grad_(True)
            y = m(xi)
            y.backward(dy)
            st = m.state_dict()
            res.append([y, xi.grad, m.IN.weight.grad, m.IN.bias.grad, m.BN.weight.grad, m.BN.bias.grad, st["BN.running_mean"],
                        st["BN.running_var"]])
        for name, r, h in zip(("y", "dx", "d_in_w", "d_in_b", "d_bn_w", "d_bn_b", "running_mean", "running_var"), *res):
            check(h, r, "IBN %s %s" % (shape, name))
            out["layer%d_%s" % (i, name)] = r.detach().numpy().astype(np.float64)

    # ---- (b) Bottleneck(ibn=True), train mode ----------------------------------------------------------------------------
    cin, w = C.BLOCK["cin"], C.BLOCK["width"]

    def ds():
        return nn.Sequential(nn.Conv2d(cin, 4 * w, 1, 1, bias=False), nn.BatchNorm2d(4 * w))
    ref, host = R["resnet_ibn_a"].Bottleneck(cin, w, True, 1, ds()), H.bottleneck(cin, w, 1, ds())
    sd = C.fill(ref.state_dict(), "ibn_block")
    x, dy = C.block_input()
    res = []
    for m in (ref, host):
        m.load_state_dict(sd)
        m.train()
        xi = x.clone().requires_grad_(True)
        y = m(xi)
        y.backward(dy)
        res.append([y, xi.grad])
    for name, r, h in zip(("y", "dx"), *res):
        check(h, r, "Bottleneck(ibn) " + name)
        out["block_" + name] = r.detach().numpy().astype(np.float64)

    # ---- (c) resnet_ibn50a, train and eval --------------------------------------------------------------------------------
    ref = R["resnet_ibn"].resnet_ibn50a(pretrained=False, **C.MODEL["kw"])
    host = H.HResNetIBN(C.MODEL["depth"], **C.MODEL["kw"])
    sd = C.fill(ref.state_dict(), "ibn_model")
    x, dy = C.model_input()
    host64 = H.HResNetIBN(C.MODEL["depth"], **C.MODEL["kw"]).double()
    sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
    for mode in ("train", "eval"):
        recs = []
        for m in (ref, host):
            m.load_state_dict(sd)
            recs.append(model_record(m, mode, x, dy))
        host64.load_state_dict(sd64)
        rec64 = model_record(host64, mode, x.double(), dy.double())
        for k in recs[0]:
            # the reference's own fp32 rounding, measured against the fp64 run of the same network: with 4 crops of 64 x 32 the
            # layer-3 instances hold 8 values and the batch statistics 32, which amplifies fp32 rounding (and ReLU branch flips in the
            # backward) far past 1e-5.  The host model is held to max(2e-5, 4 x this distance) — the factor
            # tests/test_modules_gpu._check_anchored allows a second fp32 implementation of such quantities; the distance is
            # stored and tests/test_ibn_cpu.py applies the same bound.
            e64 = rel_err(recs[0][k], rec64[k])
            check(recs[1][k].double(), recs[0][k].double(), "resnet_ibn50a %s %s (ref vs fp64 %.2e)" % (mode, k, e64),
                  tol=max(2e-5, 4.0 * e64))
            out["model_%s_%s_ref_vs_fp64" % (mode, k)] = np.float64(e64)
            if k.startswith("stat:"):
                out["model_%s_%s" % (mode, k)] = recs[0][k].double().numpy()
            else:
                out["model_%s_%s" % (mode, k)], out["model_%s_%s_stats" % (mode, k)] = sub(recs[0][k], 2048)

    # ---- (d) state_dict key names and shapes of both depths -----------------------------------------------------------------
    for name in ("resnet_ibn50a", "resnet_ibn101a"):
        sd = getattr(R["resnet_ibn"], name)(pretrained=False).state_dict()
        out[name + "_keys"] = np.array(list(sd.keys()))
        out[name + "_shapes"] = np.array([";".join(map(str, v.shape)) for v in sd.values()])

    path = os.path.join(HERE, "reference_ibn.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main()
