"""Seeded inputs and weights of the multi-part encoder fixtures (shared by make_golden_mp.py, which runs the reference on them, and
by the tests, which only have the recorded values).  Weights are filled BY PARAMETER NAME with cases_ibn.fill, so the 40 M weights
of an encoder are regenerated instead of stored."""
from __future__ import absolute_import

from oracle import ref_torch as O
from tests.golden.cases_ibn import fill, tensor  # noqa: F401

# name -> (constructor arguments, input shape).  64 x 32 crops: the part map is 4 x 2 (each part 4 elements), x_g is 2 x 1;
# 80 x 32: the part map has 5 rows, split 2 + 3.  The first case carries the predictor, so its grad-less set is the full one.
CASES = {
    "gem64": (dict(norm=True, pooling_type="gem", need_predictor=True), (4, 3, 64, 32)),
    "gem80": (dict(norm=True, pooling_type="gem"), (2, 3, 80, 32)),
    "avg64": (dict(norm=True, pooling_type="avg"), (4, 3, 64, 32)),
    "avg80": (dict(norm=True, pooling_type="avg"), (2, 3, 80, 32)),
}
OUTPUTS = ("f_g", "f_p1", "f_p2", "f_gc")
SUB = 1024                              # elements of every recorded tensor that are stored (tests.golden.cases.sub)
GRAD_KEYS = ["base.0.weight", "base.4.0.conv1.weight", "base.6.5.conv3.weight", "base.6.5.bn3.weight", "res_g.0.conv2.weight",
             "res_g.0.downsample.0.weight", "res_g.2.bn3.weight", "res_p.0.conv2.weight", "res_p.0.downsample.1.weight",
             "res_p.2.conv3.weight", "feat_bn_g.weight", "feat_bn_p1.weight", "feat_bn_p2.weight"]
GEM_GRAD_KEYS = ["gpool2d.p"]
STATS_LAYERS = ("feat_bn_gan.", "feat_bn_g.")
EVAL_CALLS = {"eval": {}, "eval_clustering": dict(clustering=True), "eval_cat": dict(fusion="cat"), "eval_g": dict(fusion="g")}


def grad_keys(name):
    return GRAD_KEYS + (GEM_GRAD_KEYS if CASES[name][0]["pooling_type"] == "gem" else [])


def model_input(name):
    n, _, h, w = CASES[name][1]
    return O.synth_images(n, h, w, seed=83), [tensor("mp_dy_%s_%s" % (name, o), (n, 2048)) for o in OUTPUTS]


def record(net, name, mode):
    """one forward (and, in train mode, a backward through all four outputs with fusion='sum') -> {key: tensor}"""
    x, dys = model_input(name)
    rec = {}
    if mode != "train":
        net.eval()
        import torch
        with torch.no_grad():
            out = net(x.to(next(net.parameters()).dtype), **EVAL_CALLS[mode])
        if isinstance(out, tuple):
            rec["f_gc"], rec["f_g"] = out
        else:
            rec["f_gc"] = out
        return rec
    net.train()
    net.zero_grad()
    dt = next(net.parameters()).dtype
    xi = x.to(dt).requires_grad_(True)
    outs = net(xi)
    sum((o * dy.to(dt)).sum() for o, dy in zip(outs, dys)).backward()
    rec.update(dict(zip(OUTPUTS, [o.detach() for o in outs])))
    rec["dx"] = xi.grad
    params, sd = dict(net.named_parameters()), net.state_dict()
    for k in grad_keys(name):
        rec["grad:" + k] = params[k].grad
    for layer in STATS_LAYERS:
        for k in ("running_mean", "running_var", "num_batches_tracked"):
            rec["stat:" + layer + k] = sd[layer + k].clone()
    rec["_gradless"] = sorted(k for k, p in params.items() if p.grad is None)
    return rec
