"""Generates tests/golden/reference_dsbn.npz by running the REFERENCE's own CC/clustercontrast/models/dsbn.py (DSBN2d, DSBN1d,
convert_dsbn, convert_bn; build container only: the reference tree does not exist on the GPU box).  The file imports only torch, so
it is loaded by file path.  Nothing from the reference is copied: the npz stores its OUTPUTS on the seeded weights and inputs of
cases_dsbn.py and the state_dict key list its convert_dsbn produces.  Every record is also computed by the host model
(tests/dsbn_hostmodel.py) and asserted to agree before it is stored.

  layer cases   DSBN2d on [4, 6, 5, 3], DSBN1d on [6, 10], distinct S / T parameters and running statistics: train forward, the
                gradients of x and of the four affine tensors, both sets of running statistics and counters afterwards, eval forward
  tree case     stem conv + BN, one Bottleneck with downsample, a BatchNorm1d after pooling (cases_dsbn.Tree): the key list after
                convert_dsbn, one train forward / backward, eval outputs after convert_bn with use_target True and False

Usage:  python tests/golden/make_golden_dsbn.py
"""
from __future__ import absolute_import, print_function

import copy
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
from tests import dsbn_hostmodel as D  # noqa: E402
from tests.golden import cases_dsbn as C  # noqa: E402
from tests.golden.cases import sub  # noqa: E402
from tests.golden.make_golden_ibn import check, rel_err  # noqa: E402

REF_FILE = "/root/reference/cluster-contrast-reid-main/clustercontrast/models/dsbn.py"


def load_reference():
    spec = importlib.util.spec_from_file_location("cc_ref_dsbn", REF_FILE)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def layer_record(m, x, dy):
    """train forward / backward, the state afterwards, then the eval forward -> list in cases_dsbn.LAYER_NAMES order"""
    m.train()
    xi = x.clone().requires_grad_(True)
    y = m(xi)
    y.backward(dy)
    st = {k: v.clone() for k, v in m.state_dict().items()}
    m.eval()
    with torch.no_grad():
        ye = m(x)
    return [y.detach(), xi.grad, m.BN_S.weight.grad, m.BN_S.bias.grad, m.BN_T.weight.grad, m.BN_T.bias.grad,
            st["BN_S.running_mean"], st["BN_S.running_var"], st["BN_S.num_batches_tracked"],
            st["BN_T.running_mean"], st["BN_T.running_var"], st["BN_T.num_batches_tracked"], ye]


def host_layer_record(sd, x, dy, eps=1e-5, momentum=0.1):
    """the same list from the fp64 closed forms of tests/dsbn_hostmodel.py"""
    N, Cc = x.shape[0], x.shape[1]
    x3, dy3 = x.reshape(N, Cc, -1), dy.reshape(N, Cc, -1)
    s = D.Set(sd["BN_S.weight"], sd["BN_S.bias"], sd["BN_S.running_mean"], sd["BN_S.running_var"])
    t = D.Set(sd["BN_T.weight"], sd["BN_T.bias"], sd["BN_T.running_mean"], sd["BN_T.running_var"])
    f = D.forward(x3, s, t, eps=(eps, eps), momentum=(momentum, momentum))
    b = D.backward(x3, dy3, None, f["mean"].value, f["invstd"].value, s.gamma, t.gamma)
    after = (f["running_mean_t"].value, f["running_var_t"].value)          # the eval forward follows the train step
    ye = D.H.forward("bn", x3, t.gamma, t.beta, eps=eps, frozen=after)["y"].value
    one = torch.ones((), dtype=torch.long)
    return [f["y"].value.reshape(x.shape), b["dx"].value.reshape(x.shape), b["d_gamma_s"].value, b["d_beta_s"].value,
            b["d_gamma_t"].value, b["d_beta_t"].value, f["running_mean_s"].value, f["running_var_s"].value, one,
            f["running_mean_t"].value, f["running_var_t"].value, one, ye.reshape(x.shape)]


def tree_record(net, x, dy):
    net.train()
    net.zero_grad()
    xi = x.clone().requires_grad_(True)
    emb = net(xi)
    (emb * dy).sum().backward()
    sd = net.state_dict()
    params = dict(net.named_parameters())
    rec = {"emb": emb.detach(), "dx": xi.grad}
    for k in C.TREE_GRAD_KEYS:
        rec["grad:" + k] = params[k].grad
    for k in C.TREE_STATS:
        rec["stat:" + k] = sd[k].clone()
    return rec


def eval_out(net, x):
    net.eval()
    with torch.no_grad():
        return net(x)


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    R = load_reference()
    out = {}

    # ---- (a) the layers alone ---------------------------------------------------------------------------------------------------
    for i, (shape, dims) in enumerate(C.LAYERS):
        ref = (R.DSBN2d if dims == 2 else R.DSBN1d)(shape[1])
        sd = C.layer_state(i, ref.state_dict())
        ref.load_state_dict(sd)
        x, dy = C.layer_input(i)
        r, h = layer_record(ref, x, dy), host_layer_record(sd, x, dy)
        for name, rv, hv in zip(C.LAYER_NAMES, r, h):
            check(hv, rv, "DSBN%dd %s %s" % (dims, shape, name))
            out["layer%d_%s" % (i, name)] = rv.detach().double().numpy()

    # ---- (b) convert_dsbn / convert_bn on a tree --------------------------------------------------------------------------------
    ref = C.Tree()
    R.convert_dsbn(ref)
    sd = C.fill(ref.state_dict(), "dsbn_tree")
    out["tree_keys"] = np.array(list(sd.keys()))
    out["tree_shapes"] = np.array([";".join(map(str, v.shape)) for v in sd.values()])
    ref.load_state_dict(sd)
    host = D.convert_h(C.Tree())
    assert list(host.state_dict().keys()) == list(sd.keys())
    host.load_state_dict(sd)
    host64 = D.convert_h(C.Tree()).double()
    host64.load_state_dict({k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()})
    x, dy = C.tree_input()
    for use_target in (True, False):
        tag = "tree_eval_T" if use_target else "tree_eval_S"
        plain = copy.deepcopy(ref)
        R.convert_bn(plain, use_target=use_target)
        assert not any("BN_S" in k or "BN_T" in k for k in plain.state_dict())
        hplain = C.Tree()                             # the host side of convert_bn: a plain tree loaded with the chosen set
        pick = ".BN_T." if use_target else ".BN_S."
        hplain.load_state_dict({k.replace(pick, "."): v for k, v in sd.items() if pick in k or ".BN_" not in k})
        ye, he = eval_out(plain, x), eval_out(hplain, x)
        check(he, ye, tag)
        out[tag] = ye.double().numpy()
        if use_target:                                # eval mode of the converted tree IS its BN_T
            check(eval_out(copy.deepcopy(ref), x), ye, "converted tree in eval mode vs convert_bn(use_target=True)", tol=0.0)
    assert rel_err(torch.from_numpy(out["tree_eval_S"]), torch.from_numpy(out["tree_eval_T"])) > 0.1
    recs = [tree_record(ref, x, dy), tree_record(host, x, dy)]
    rec64 = tree_record(host64, x.double(), dy.double())
    for k in recs[0]:
        # the reference's own fp32 rounding against the fp64 run of the same tree; the host model is held to max(2e-5, 4 x that),
        # the factor make_golden_ibn.py uses, and tests/test_dsbn_cpu.py applies the same bound
        e64 = rel_err(recs[0][k], rec64[k])
        check(recs[1][k].double(), recs[0][k].double(), "tree train %s (ref vs fp64 %.2e)" % (k, e64), tol=max(2e-5, 4.0 * e64))
        out["tree_train_%s_ref_vs_fp64" % k] = np.float64(e64)
        if recs[0][k].numel() > 2048:
            out["tree_train_" + k], out["tree_train_%s_stats" % k] = sub(recs[0][k], 2048)
        else:
            out["tree_train_" + k] = recs[0][k].double().numpy()

    path = os.path.join(HERE, "reference_dsbn.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main()
