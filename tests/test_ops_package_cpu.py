"""The rg_hip.ops package without a GPU and without a built library: every entry point a wrapper names is a prototype of
include/reidgan_hip.h (a mistyped one would otherwise surface only when that op runs), and the package namespace is exactly what
its submodules define (an op added to a submodule and forgotten in __init__.py fails here)."""
import ast
import glob
import importlib
import os

from rg_hip import ops
from rg_hip.lib import parse_header

OPS_DIR = os.path.dirname(os.path.abspath(ops.__file__))
SUBMODULES = sorted(os.path.basename(p)[:-3] for p in glob.glob(os.path.join(OPS_DIR, "*.py")) if not p.endswith("__init__.py"))


def _tree(name):
    with open(os.path.join(OPS_DIR, name + ".py")) as f:
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


def test_every_entry_point_named_by_a_wrapper_is_declared_in_the_header():
    protos = parse_header()
    used = {}
    for mod in SUBMODULES + ["__init__"]:
        for node in ast.walk(_tree(mod)):
            if isinstance(node, ast.Attribute) and isinstance(node.value, ast.Name) and node.value.id == "lib" \
                    and node.attr.startswith("rg_"):
                used.setdefault(node.attr, mod)
            elif isinstance(node, ast.Call) and isinstance(node.func, ast.Name) and node.func.id == "_ws_query" and node.args:
                fn = node.args[0]
                assert isinstance(fn, ast.Constant) and isinstance(fn.value, str), \
                    "%s.py line %d: _ws_query takes the entry point as a string literal" % (mod, node.lineno)
                used.setdefault(fn.value, mod)
    assert len(used) > 100, "only %d entry points found: the walk no longer sees the wrappers" % len(used)   # 139 when written
    missing = sorted("%s (%s.py)" % (n, m) for n, m in used.items() if n not in protos)
    assert not missing, "not declared in include/reidgan_hip.h: %s" % ", ".join(missing)


def test_the_namespace_is_what_the_submodules_define():
    assert SUBMODULES, "no submodules found under %s" % OPS_DIR
    owner = {}
    for mod in SUBMODULES:
        for name in _defined(_tree(mod)):
            assert name not in owner or owner[name] == mod, "%s is defined in %s.py and in %s.py" % (name, owner[name], mod)
            owner[name] = mod
    assert not _defined(_tree("__init__")), "rg_hip/ops/__init__.py defines %s: it only re-exports" % _defined(_tree("__init__"))
    loaded = {mod: importlib.import_module("rg_hip.ops." + mod) for mod in SUBMODULES}
    for name, mod in sorted(owner.items()):
        if not name.startswith("_"):
            assert hasattr(ops, name), "%s.%s is not re-exported by rg_hip/ops/__init__.py" % (mod, name)
        if hasattr(ops, name):
            assert getattr(ops, name) is getattr(loaded[mod], name), "ops.%s is not the object %s.py defines" % (name, mod)
    assert ops.lib is loaded["_base"].lib
    # everything else the package exposes is a submodule: nothing is defined or imported into it from elsewhere
    extra = sorted(n for n in vars(ops) if not n.startswith("__") and n not in owner and n not in loaded
                   and n not in ("lib", "absolute_import"))
    assert not extra, "rg_hip.ops exposes names no submodule defines: %s" % extra
