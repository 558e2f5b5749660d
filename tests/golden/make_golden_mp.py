"""Generates tests/golden/reference_mp.npz by running the REFERENCE's own multi-part encoder (build container only; the reference
tree does not exist on the GPU box):

  * CC/clustercontrast/models/resnet_mp.py   ResNet_MP (:16-205), resnet_mp50
  * CC/clustercontrast/models/pooling.py     build_pooling_layer ('gem', 'avg')

loaded by file path under placeholder parent packages — the recipe of make_golden_ibn.py.  resnet_mp.py takes its trunk from
`torchvision.models.resnet50` and `torchvision.models.resnet.Bottleneck`; torchvision is not installed here, so a placeholder module
serves them with oracle.ref_torch's OTVResNet / OBottleneck (the torchvision layout the project's oracle already pins).  Nothing from
the reference is copied: the file stores the reference's OUTPUTS on the seeded weights and inputs of cases_mp.py (sub-sampled), the
names of the parameters a backward leaves without gradient, and the state_dict key names and shapes with and without predictor.
Every case is also run through the host model (tests/mp_hostmodel.py) and asserted to agree before it is stored, and the reference's
own fp32-vs-fp64 distance is recorded per quantity (the model-level bound is max(2e-5, 4 x that distance), as for the IBN fixture).

Usage:  python tests/golden/make_golden_mp.py
"""
from __future__ import absolute_import, print_function

import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
from oracle import ref_torch as O  # noqa: E402
from tests import mp_hostmodel as H  # noqa: E402
from tests.golden import cases_mp as C  # noqa: E402
from tests.golden.cases import sub  # noqa: E402
from tests.golden.make_golden_ibn import check, rel_err  # noqa: E402

CC = "/root/reference/cluster-contrast-reid-main"


def load_reference_models():
    root = types.ModuleType("cc_ref_mp")
    root.__path__ = [CC + "/clustercontrast"]
    models = types.ModuleType("cc_ref_mp.models")
    models.__path__ = [CC + "/clustercontrast/models"]
    tv, tvm, tvr = types.ModuleType("torchvision"), types.ModuleType("torchvision.models"), types.ModuleType("torchvision.models.resnet")
    for depth in (18, 34, 50, 101, 152):
        setattr(tvm, "resnet%d" % depth, (lambda d: lambda pretrained=False: O.OTVResNet(d))(depth))

    def bottleneck(inplanes, planes, stride=1, downsample=None):
        return O.OBottleneck(inplanes, planes, stride, downsample)
    tvr.Bottleneck = bottleneck
    tv.models, tvm.resnet = tvm, tvr
    sys.modules.update({"cc_ref_mp": root, "cc_ref_mp.models": models, "torchvision": tv, "torchvision.models": tvm,
                        "torchvision.models.resnet": tvr})
    mods = {}
    for name in ("pooling", "resnet_mp"):
        full = "cc_ref_mp.models." + name
        spec = importlib.util.spec_from_file_location(full, "%s/clustercontrast/models/%s.py" % (CC, name))
        mod = importlib.util.module_from_spec(spec)
        sys.modules[full] = mod
        spec.loader.exec_module(mod)
        mods[name] = mod
    return mods


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    R = load_reference_models()
    out = {}
    for name, (kw, _shape) in C.CASES.items():
        ref = R["resnet_mp"].resnet_mp50(pretrained=False, **kw)
        host, host64 = H.HResNetMP(50, **kw), H.HResNetMP(50, **kw).double()
        assert list(ref.state_dict().keys()) == list(host.state_dict().keys())
        sd = C.fill(ref.state_dict(), "mp_" + name)
        sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
        for mode in ("train",) + tuple(C.EVAL_CALLS):
            recs = []
            for m, s in ((ref, sd), (host, sd), (host64, sd64)):
                m.load_state_dict(s)
                recs.append(C.record(m, name, mode))
            r, h, r64 = recs
            if mode == "train":
                assert r.pop("_gradless") == h.pop("_gradless") == r64.pop("_gradless")
                out["%s_gradless" % name] = np.array(sorted(k for k, p in ref.named_parameters() if p.grad is None))
            for k in r:
                e64 = rel_err(r[k], r64[k])
                if k.startswith("stat:"):           # a [2048] vector or a counter: stored whole
                    check(h[k].double(), r[k].double(), "%s %s %s (ref vs fp64 %.2e)" % (name, mode, k, e64), tol=max(2e-5, 4.0 * e64))
                    out["%s_%s_%s_ref_vs_fp64" % (name, mode, k)] = np.float64(e64)
                    out["%s_%s_%s" % (name, mode, k)] = r[k].double().numpy()
                    continue
                check(h[k].double(), r[k].double(), "%s %s %s (ref vs fp64 %.2e)" % (name, mode, k, e64), tol=max(2e-5, 4.0 * e64))
                out["%s_%s_%s_ref_vs_fp64" % (name, mode, k)] = np.float64(e64)
                out["%s_%s_%s" % (name, mode, k)], out["%s_%s_%s_stats" % (name, mode, k)] = sub(r[k], C.SUB)
    for tag, kw in (("plain", {}), ("predictor", dict(need_predictor=True))):
        sd = R["resnet_mp"].resnet_mp50(pretrained=False, norm=True, pooling_type="gem", **kw).state_dict()
        out["keys_" + tag] = np.array(list(sd.keys()))
        out["shapes_" + tag] = np.array([";".join(map(str, v.shape)) for v in sd.values()])
    for depth in (18, 34):                  # the reference cannot build them either: the depths the product refuses
        try:
            getattr(R["resnet_mp"], "resnet_mp%d" % depth)(pretrained=False, norm=True)
            raise AssertionError("resnet_mp%d was built" % depth)
        except RuntimeError as e:
            print("  resnet_mp%d: %s" % (depth, str(e).splitlines()[0]))
    path = os.path.join(HERE, "reference_mp.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main()
