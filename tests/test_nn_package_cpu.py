"""The rg_hip.nn package without a GPU and without a built library: the namespace is exactly what its submodules define (a layer
added to a submodule and forgotten in __init__.py fails here), the convolution classes initialise as torch's do under a seed, and
the two host protocols the layers share are stated once: the deferred BatchNorm step counter (_BatchNorm.count_batch, nbt_pending,
nbt_add) and the delivery of parameter gradients (Tape.grad_dst, Tape.add_grads)."""
import ast
import glob
import importlib
import math
import os

import torch

from rg_hip import nn as rnn, ops
from rg_hip.tape import Tape

NN_DIR = os.path.dirname(os.path.abspath(rnn.__file__))
SUBMODULES = sorted(os.path.basename(p)[:-3] for p in glob.glob(os.path.join(NN_DIR, "*.py")) if not p.endswith("__init__.py"))
ACTS = ("ACT_NONE", "ACT_RELU", "ACT_LEAKY", "ACT_TANH")
READ_OUTSIDE = ("_BatchNorm", "_DSBN", "_Act", "_fold_bn", "_KrscCache", "_fold_of")


def _tree(name):
    with open(os.path.join(NN_DIR, name + ".py")) as f:
        return ast.parse(f.read())


def _defined(tree):
    """names bound by def / class / assignment at module level (imports are not definitions)"""
    names = []
    for node in tree.body:
        if isinstance(node, (ast.FunctionDef, ast.ClassDef)):
            names.append(node.name)
        elif isinstance(node, (ast.Assign, ast.AnnAssign, ast.AugAssign)):
            for tgt in (node.targets if isinstance(node, ast.Assign) else [node.target]):
                names += [n.id for n in ast.walk(tgt) if isinstance(n, ast.Name)]
    return names


def test_the_namespace_is_what_the_submodules_define():
    assert SUBMODULES, "no submodules found under %s" % NN_DIR
    owner = {}
    for mod in SUBMODULES:
        for name in _defined(_tree(mod)):
            assert name not in owner, "%s is defined in %s.py and in %s.py" % (name, owner[name], mod)
            owner[name] = mod
    assert not _defined(_tree("__init__")), "rg_hip/nn/__init__.py defines %s: it only re-exports" % _defined(_tree("__init__"))
    loaded = {mod: importlib.import_module("rg_hip.nn." + mod) for mod in SUBMODULES}
    for name, mod in sorted(owner.items()):
        if not name.startswith("_"):
            assert hasattr(rnn, name), "%s.%s is not re-exported by rg_hip/nn/__init__.py" % (mod, name)
        if hasattr(rnn, name):
            assert getattr(rnn, name) is getattr(loaded[mod], name), "nn.%s is not the object %s.py defines" % (name, mod)
    for name in READ_OUTSIDE:
        assert name in owner and getattr(rnn, name) is getattr(loaded[owner[name]], name), name
    for name in ACTS:
        assert getattr(rnn, name) is getattr(ops, name), name
    # everything else the package exposes is a submodule: nothing is defined or imported into it from elsewhere
    extra = sorted(n for n in vars(rnn) if not n.startswith("__") and n not in owner and n not in loaded and n not in ACTS)
    assert not extra, "rg_hip.nn exposes names no submodule defines: %s" % extra


def test_seeded_initialisation_of_the_convolution_classes_is_torchs():
    for ours, theirs in ((rnn.Conv2d, torch.nn.Conv2d), (rnn.ConvTranspose2d, torch.nn.ConvTranspose2d)):
        torch.manual_seed(0)
        m = ours(3, 4, 3)
        torch.manual_seed(0)
        t = theirs(3, 4, 3)
        assert m.weight.shape == t.weight.shape and torch.equal(m.weight, t.weight), ours.__name__
        assert torch.equal(m.bias, t.bias), ours.__name__
        torch.manual_seed(0)
        m = ours(3, 4, 3, bias=False)                       # the filters are drawn first, so they do not depend on the bias
        assert m.bias is None and torch.equal(m.weight, t.weight), ours.__name__
    # SNConv2d: the filter and bias draws of torch.nn.Conv2d, then u and v as torch.nn.utils.spectral_norm draws them
    torch.manual_seed(0)
    m = rnn.SNConv2d(3, 4, 3)
    torch.manual_seed(0)
    w, b = torch.empty(4, 3, 3, 3), torch.empty(4)
    torch.nn.init.kaiming_uniform_(w, a=math.sqrt(5))
    fan_in, _ = torch.nn.init._calculate_fan_in_and_fan_out(w)
    torch.nn.init.uniform_(b, -1 / math.sqrt(fan_in), 1 / math.sqrt(fan_in))
    u = torch.nn.functional.normalize(torch.randn(4), dim=0, eps=1e-12)
    v = torch.nn.functional.normalize(torch.randn(27), dim=0, eps=1e-12)
    assert torch.equal(m.weight_orig, w) and torch.equal(m.bias, b)
    assert torch.equal(m.weight_u, u) and torch.equal(m.weight_v, v)
    assert sorted(m.state_dict()) == ["bias", "weight_orig", "weight_u", "weight_v"]


def test_the_batchnorm_step_counter_is_counted_on_the_host_and_flushed_when_read():
    bn = rnn.BatchNorm2d(4)
    bn.count_batch()
    bn.count_batch()
    assert rnn.nbt_pending(bn) == 2 and int(bn._buffers["num_batches_tracked"]) == 0      # nothing written yet
    assert int(bn.state_dict()["num_batches_tracked"]) == 2
    assert rnn.nbt_pending(bn) == 0
    assert int(bn.num_batches_tracked) == 2 and int(bn.num_batches_tracked) == 2          # reading does not count again
    bn.count_batch()
    assert int(bn.num_batches_tracked) == 3                                               # the attribute read flushes too
    # a loaded counter replaces whatever was pending
    bn.count_batch()
    sd = rnn.BatchNorm2d(4).state_dict()
    sd["num_batches_tracked"] = torch.tensor(5, dtype=torch.long)
    bn.load_state_dict(sd)
    assert rnn.nbt_pending(bn) == 0 and int(bn.num_batches_tracked) == 5
    # what the network programs do: re-apply a recorded delta, take back what an aborted capture counted
    rnn.nbt_add(bn, 3)
    assert rnn.nbt_pending(bn) == 3
    rnn.nbt_add(bn, -3)
    assert rnn.nbt_pending(bn) == 0 and int(bn.num_batches_tracked) == 5
    # a layer without running statistics counts nothing anywhere
    free = rnn.BatchNorm1d(4, track_running_stats=False)
    free.count_batch()
    assert "num_batches_tracked" not in free.state_dict() and free.num_batches_tracked is None


def _params():
    """wanted with an arena view; frozen; wanted without an arena view; wanted with a view, already delivered once"""
    ps = [torch.nn.Parameter(torch.zeros(3)) for _ in range(4)]
    for p in (ps[0], ps[1], ps[3]):
        p._rg_grad = torch.zeros(3)
    ps[1].requires_grad_(False)
    return ps


def test_tape_grad_dst_and_add_grads(monkeypatch):
    """add_grad's accumulation path runs ops.side_sync and ops.axpby, which need the library: they are replaced on rg_hip.ops by
    CPU stand-ins of the same contract (out = alpha a + beta b, written in place), so the path itself is the real one."""
    synced = []
    monkeypatch.setattr(ops, "side_sync", lambda: synced.append(1))
    monkeypatch.setattr(ops, "axpby", lambda a, b, alpha, beta, out: out.copy_(alpha * a + (beta * b if b is not None else 0)))
    want, frozen, no_view, seen = _params()
    tape = Tape()
    first = torch.ones(3)
    tape.add_grad(seen, first)
    assert tape.grads[id(seen)].data_ptr() == seen._rg_grad.data_ptr()          # the first contribution is moved into the arena
    assert tape.grad_dst(want) is want._rg_grad
    assert tape.grad_dst(frozen) is None and tape.grad_dst(no_view) is None and tape.grad_dst(seen) is None
    assert tape.grad_dst(None) is None
    assert Tape(param_grad=False).grad_dst(want) is None

    g = [torch.full((3,), float(i + 2)) for i in range(4)]
    tape.add_grads(zip((want, frozen, no_view, seen), g))
    assert id(frozen) not in tape.grads
    assert torch.equal(tape.grads[id(want)], g[0]) and tape.grads[id(want)].data_ptr() == want._rg_grad.data_ptr()
    assert tape.grads[id(no_view)] is g[2]                                      # no arena: kept as delivered
    assert torch.equal(tape.grads[id(seen)], torch.full((3,), 6.0)) and synced == [1]    # 1 + 5, the one accumulation
    # a second delivery accumulates everywhere an entry exists now, and still skips the frozen parameter
    tape.add_grads([(want, g[0]), (frozen, g[1]), (None, g[1])])
    assert torch.equal(tape.grads[id(want)], torch.full((3,), 4.0)) and id(frozen) not in tape.grads and len(synced) == 2
    # a tape that records no parameter gradients delivers nothing
    off = Tape(param_grad=False)
    off.add_grads([(want, g[0])])
    assert off.grads == {}
