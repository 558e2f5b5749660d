"""Generates tests/golden/reference_siamese.npz by running the REFERENCE's own stage-I pieces (build container only; the reference
tree does not exist on the GPU box):

  * FD/reid/models/embedding.py      EltwiseSubEmbed (:7-39)
  * FD/reid/models/multi_branch.py   SiameseNet (:6-16)
  * FD/reid/trainers.py              SiameseTrainer._forward (:69-73), with FD/reid/evaluation_metrics/classification.py `accuracy`

loaded by file path under placeholder parent packages — the recipe of make_golden_mp.py.  Nothing from the reference is copied: the
file stores the reference's OUTPUTS on the seeded inputs of cases_siamese.py with an identity base model, in train mode: logits,
loss, prec, the gradients of the loss with respect to f1, f2 and the four parameters, and the running statistics after the forward.
Before anything is stored every case is checked to have no two logits of a row closer than 1e-4 (no tie for the argmax to settle).

Usage:  python tests/golden/make_golden_siamese.py
"""
from __future__ import absolute_import, print_function

import importlib.util
import os
import sys
import types

import numpy as np
import torch
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
from tests.golden import cases_siamese as C  # noqa: E402

FD = "/root/reference/FD-GAN-master"


def _load(full, path):
    spec = importlib.util.spec_from_file_location(full, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[full] = mod
    spec.loader.exec_module(mod)
    return mod


def load_reference():
    for pkg, sub in (("fd_ref_s", ""), ("fd_ref_s.models", "/models"), ("fd_ref_s.evaluation_metrics", "/evaluation_metrics")):
        m = types.ModuleType(pkg)
        m.__path__ = [FD + "/reid" + sub]
        sys.modules[pkg] = m
    utils = _load("fd_ref_s.utils", FD + "/reid/utils/__init__.py")
    utils.__path__ = [FD + "/reid/utils"]
    _load("fd_ref_s.utils.meters", FD + "/reid/utils/meters.py")
    cls = _load("fd_ref_s.evaluation_metrics.classification", FD + "/reid/evaluation_metrics/classification.py")
    sys.modules["fd_ref_s.evaluation_metrics"].accuracy = cls.accuracy
    return {"embedding": _load("fd_ref_s.models.embedding", FD + "/reid/models/embedding.py"),
            "multi_branch": _load("fd_ref_s.models.multi_branch", FD + "/reid/models/multi_branch.py"),
            "trainers": _load("fd_ref_s.trainers", FD + "/reid/trainers.py")}


def main():
    torch.set_num_threads(1)
    R = load_reference()
    out = {}
    for name, (B, D, Cn) in C.CASES.items():
        inp = C.inputs(name)
        embed = R["embedding"].EltwiseSubEmbed(use_batch_norm=True, use_classifier=True, num_features=D, num_classes=Cn)
        with torch.no_grad():
            embed.bn.weight.copy_(inp["gamma"]), embed.bn.bias.copy_(inp["beta"])
            embed.bn.running_mean.copy_(inp["rm"]), embed.bn.running_var.copy_(inp["rv"])
            embed.classifier.weight.copy_(inp["W"]), embed.classifier.bias.copy_(inp["bias"])
        net = R["multi_branch"].SiameseNet(nn.Identity(), embed)
        net.train()
        trainer = R["trainers"].SiameseTrainer(net, nn.CrossEntropyLoss())
        f1, f2 = inp["f1"].clone().requires_grad_(True), inp["f2"].clone().requires_grad_(True)
        _, _, logits = net(f1, f2)                      # the values only: the running statistics move in the trainer's call below
        with torch.no_grad():
            embed.bn.running_mean.copy_(inp["rm"]), embed.bn.running_var.copy_(inp["rv"])
        top2 = logits.detach().topk(min(2, Cn), 1).values
        assert Cn < 2 or float((top2[:, 0] - top2[:, 1]).min()) > 1e-4, "%s: a row's two largest logits nearly tie" % name
        loss, prec = trainer._forward([f1, f2], inp["targets"])
        loss.backward()
        rec = {"logits": logits, "loss": loss, "prec": prec, "df1": f1.grad, "df2": f2.grad, "dW": embed.classifier.weight.grad,
               "dbias": embed.classifier.bias.grad, "dgamma": embed.bn.weight.grad, "dbeta": embed.bn.bias.grad,
               "running_mean": embed.bn.running_mean, "running_var": embed.bn.running_var}
        assert sorted(rec) == sorted(C.QUANTITIES)
        for k, v in rec.items():
            out["%s_%s" % (name, k)] = torch.as_tensor(v).detach().float().numpy()
        print("  %s: loss %.6f prec %.4f" % (name, float(loss), float(prec)))
    path = os.path.join(HERE, "reference_siamese.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main()
