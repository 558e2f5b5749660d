"""The README's "Environment switches" table is the list of RG_* variables the code reads, no more and no less, and the A/B
switches retired with profiles/retired_switches.txt stay retired: their names appear nowhere in the sources, the public header,
the tools (tools/debug/ apart) or the README.  No library, no GPU."""
import ast
import glob
import itertools
import os
import re

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "reid-gan_amd")

# names built with a format string: the literal the code holds -> the variables it stands for
FORMATTED = {
    "RG_RESNET%d_WEIGHTS": ["RG_RESNET%d_WEIGHTS" % d for d in (18, 34, 50, 101, 152)],
    "RG_RESNET_IBN%s_WEIGHTS": ["RG_RESNET_IBN50A_WEIGHTS", "RG_RESNET_IBN101A_WEIGHTS"],
}

RETIRED = [
    # conv library, host side
    "RG_CONV_TUNE_PLAN", "RG_CONV_TUNE_PATH", "RG_CONV_TUNE8", "RG_CONV_HALO", "RG_HALO_WG", "RG_THIN_CONV", "RG_THIN_PX4",
    "RG_SMALLC_PX", "RG_CONV_DMA", "RG_SPLITK_VEC", "RG_DGRAD_STRIDED_SPLIT", "RG_WGRAD_WG", "RG_WGRAD_XCD", "RG_WGRAD_SHIFT",
    "RG_WGRAD_FOLD_FUSED", "RG_CONV_PL", "RG_F8_BM",
    # compile-time variants (RG_WGRAD_RSC, the run-time kernel branch, is still there: profiles/retired_switches.txt)
    "RG_F8_NB", "RG_MATH",
    # Python side
    "RG_GRAPH_SIDE", "RG_GRAPH_SIDE_MIN_US", "RG_AUX_SIDE", "RG_NCCL_HIGH_PRIO", "RG_STAGE_BUCKETS", "RG_KRSC_GROUP", "RG_BN_FUSED",
    "RG_AUTOGRAD_MT", "RG_SIDE_MIN_US", "RG_STREAM_PROBE_DEBUG",
]


def _read(path):
    with open(path, encoding="utf-8") as f:
        return f.read()


def _python_sources():
    return sorted(glob.glob(os.path.join(PKG, "**", "*.py"), recursive=True)) + [os.path.join(REPO, "bench.py")]


def _c_sources():
    return sorted(p for ext in ("*.hip", "*.h", "*.c", "*.cpp") for p in glob.glob(os.path.join(PKG, "**", ext), recursive=True))


def _is_environ(node):
    return isinstance(node, ast.Attribute) and node.attr == "environ"


def _literal(node):
    """the RG_* string a name expression holds: a constant, or the constant on the left of a `%` format"""
    if isinstance(node, ast.BinOp) and isinstance(node.op, ast.Mod):
        node = node.left
    if isinstance(node, ast.Constant) and isinstance(node.value, str) and node.value.startswith("RG_"):
        return node.value
    return None


def _python_names(path):
    names = set()
    tree = ast.parse(_read(path), path)
    for node in ast.walk(tree):
        arg = None
        if isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and node.args:
            environ_method = _is_environ(node.func.value) and node.func.attr in ("get", "pop", "setdefault")
            if environ_method or node.func.attr == "getenv":
                arg = node.args[0]
        elif isinstance(node, ast.Subscript) and _is_environ(node.value) and isinstance(node.ctx, ast.Load):
            arg = node.slice.value if type(node.slice).__name__ == "Index" else node.slice      # (ast.Index: Python < 3.9)
        elif isinstance(node, ast.Compare) and len(node.ops) == 1 and isinstance(node.ops[0], (ast.In, ast.NotIn)) \
                and _is_environ(node.comparators[0]):
            arg = node.left
        elif isinstance(node, ast.Constant) and isinstance(node.value, str) and re.match(r"RG_[A-Z0-9_]*%", node.value):
            arg = node                      # a formatted name bound to a variable before it is looked up
        lit = _literal(arg) if arg is not None else None
        if lit is not None:
            names.add(lit)
    return names


def _names_read():
    names = set()
    for path in _python_sources():
        names |= _python_names(path)
    for path in _c_sources():
        names |= set(re.findall(r"\b(?:getenv|env_int)\s*\(\s*\"(RG_[A-Za-z0-9_%]+)\"", _read(path)))
    out = set()
    for n in names:
        if "%" in n:
            assert n in FORMATTED, "formatted variable name %r: add what it stands for to FORMATTED" % n
            out |= set(FORMATTED[n])
        else:
            out.add(n)
    return out


def _readme_table_names():
    lines = _read(os.path.join(REPO, "README.md")).splitlines()
    start = next(i for i, ln in enumerate(lines) if ln.startswith("## Environment switches"))
    names = set()
    for ln in itertools.takewhile(lambda l: not l.startswith("## "), lines[start + 1:]):
        if not ln.startswith("|"):
            continue
        first_cell = ln.split("|")[1]
        for tok in re.findall(r"RG_[A-Z0-9_]*(?:\{[0-9A-Z,]+\}[A-Z0-9_]*)?", first_cell):
            m = re.match(r"(.*)\{(.*)\}(.*)", tok)
            names |= set(m.group(1) + alt + m.group(3) for alt in m.group(2).split(",")) if m else {tok}
    return names


def test_the_readme_table_lists_exactly_the_variables_the_code_reads():
    read, listed = _names_read(), _readme_table_names()
    assert len(read) >= 10, "only %d names found: the walk no longer sees the reads" % len(read)
    assert "RG_CONV_TUNE" in read and "RG_BN_REG" in read and "RG_BENCH_DEBUG" in read and "RG_RESNET50_WEIGHTS" in read
    assert sorted(read - listed) == [], "read by the code, missing in README's table"
    assert sorted(listed - read) == [], "in README's table, read by nothing"


def test_retired_switches_stay_retired():
    files = [os.path.join(REPO, "README.md")]
    for root in (PKG, os.path.join(REPO, "include"), os.path.join(REPO, "tools")):
        for d, dirs, fs in os.walk(root):
            if os.path.abspath(d) == os.path.join(REPO, "tools"):
                dirs[:] = [x for x in dirs if x != "debug"]
            dirs[:] = [x for x in dirs if x not in ("__pycache__", "lib")]
            files += [os.path.join(d, f) for f in fs if not f.endswith((".o", ".so", ".pyc"))]
    assert len(files) > 100, "only %d files walked" % len(files)
    pat = re.compile(r"(?<![A-Za-z0-9_])(%s)(?![A-Za-z0-9_])" % "|".join(sorted(RETIRED, key=len, reverse=True)))
    found = []
    for path in files:
        with open(path, "rb") as f:
            text = f.read().decode("utf-8", "replace")
        found += ["%s: %s" % (os.path.relpath(path, REPO), n) for n in sorted(set(pat.findall(text)))]
    assert found == [], "retired switches named again"
