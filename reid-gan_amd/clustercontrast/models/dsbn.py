"""Domain-specific BatchNorm — restates CC/clustercontrast/models/dsbn.py:6-78 on the HIP tape runtime.

`DSBN2d` / `DSBN1d` hold two BatchNorms, `BN_S` (source) and `BN_T` (target).  A train-mode batch is [source half | target half]
and each half is normalised with its own batch statistics and parameter set; eval mode is `BN_T` on the whole batch.  The
reference writes the train mode as split + two `.contiguous()` copies + two BatchNorms + cat; here it is one fused layer over
the one tensor (`rg_dsbn_fwd` / `rg_dsbn_bwd`, rg_hip.nn.DSBN2d / DSBN1d).

`convert_dsbn(model)` replaces every BatchNorm child by a DSBN layer that starts from its state, `convert_bn(model, use_target)`
does the reverse with the chosen domain — the reference's names, arguments and recursion over `named_children`
(examples/test.py:69-89: convert_dsbn, copy_state_dict, convert_bn, evaluate).  One difference: the new module takes the train /
eval mode and the device of the child it replaces, where the reference leaves a fresh module in train mode on the CPU.  Under data-parallel ranks every rank's batch must
itself be [source | target].

Not convertible by swapping a child: layers whose fused kernels read a BatchNorm's parameters directly — the `BN` inside an IBN
layer (rg_ibn_*) and the three BatchNorm1d of the multi-part head (rg_mp_head_*).  `convert_dsbn` refuses such a model with a
TypeError BEFORE it changes anything.
"""
from __future__ import absolute_import

from rg_hip import netgraph
from rg_hip import nn as rnn
from rg_hip.tape import invalidate_param_cache

__all__ = ['DSBN2d', 'DSBN1d', 'convert_dsbn', 'convert_bn']

DSBN2d = rnn.DSBN2d
DSBN1d = rnn.DSBN1d


def _refused(model):
    """names of the BatchNorms under `model` that a fused kernel reads directly"""
    out = []
    for name, m in model.named_modules():
        prefix = name + "." if name else ""
        if isinstance(m, rnn.IBN):
            out.append(prefix + "BN (inside an IBN layer)")
        if hasattr(m, "_head_bns"):
            heads = set(id(b) for b in m._head_bns())
            out += [prefix + n + " (multi-part head)" for n, c in m.named_children() if id(c) in heads]
    return out


def _drop_caches(model):
    """forget everything that remembers the replaced modules: the parameter lists of rg_hip.tape.run, captured network programs,
    the trunk's FoldGroup (on its first convolution) and the per-convolution folds"""
    invalidate_param_cache(model)
    for m in model.modules():
        m.__dict__.pop("_rg_fold_group", None)
        m.__dict__.pop("_rg_fold", None)
        netgraph.release(m)


def _swap(model, match, make):
    for child_name, child in list(model.named_children()):
        new = make(child) if match(child) else None
        if new is not None:
            new.train(child.training)
            setattr(model, child_name, new)
        else:
            _swap(child, match, make)


def _to_dsbn(child):
    m = (DSBN2d if isinstance(child, rnn.BatchNorm2d) else DSBN1d)(child.num_features)
    sd = child.state_dict()
    m.BN_S.load_state_dict(sd)
    m.BN_T.load_state_dict(sd)
    return m.to(sd["running_mean"].device)


def convert_dsbn(model):
    bad = _refused(model)
    if bad:
        raise TypeError("convert_dsbn: %s cannot become domain-specific: %s — fused kernels read these BatchNorms' parameters "
                        "directly; the model is left unchanged"
                        % (type(model).__name__, ", ".join(bad[:3]) + (" and %d more" % (len(bad) - 3) if len(bad) > 3 else "")))
    _swap(model, lambda c: isinstance(c, (rnn.BatchNorm2d, rnn.BatchNorm1d)), _to_dsbn)
    _drop_caches(model)


def convert_bn(model, use_target=True):
    def to_bn(child):
        src = child.BN_T if use_target else child.BN_S
        m = (rnn.BatchNorm2d if isinstance(child, DSBN2d) else rnn.BatchNorm1d)(child.num_features)
        sd = src.state_dict()
        m.load_state_dict(sd)
        return m.to(sd["running_mean"].device)
    _swap(model, lambda c: isinstance(c, (DSBN2d, DSBN1d)), to_bn)
    _drop_caches(model)
