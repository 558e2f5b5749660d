"""The host steps the retrieval recipes share, without a GPU: the coercion of rg_hip.search, the sort segments and label compaction
of rg_hip.ops, the two-pass list total, and that each of the shared names is defined in one place only."""
import ast
import glob
import os

import numpy as np
import pytest
import torch

from rg_hip import ops, search

PKG = os.path.dirname(os.path.dirname(os.path.abspath(search.__file__)))


def test_as_matrix_accepts_the_documented_forms_and_touches_no_device():
    initialised = torch.cuda.is_initialized()          # true only when an earlier GPU test of the same process did it
    want = np.arange(24, dtype=np.float64).reshape(6, 4) / 8 - 1
    rows = [torch.from_numpy(r.astype(np.float32)) for r in want]
    for x, rows_ok in ((want, False), (torch.from_numpy(want).half(), False), (rows, True), (tuple(rows), True), (want, True)):
        m = search.as_matrix(x, "here: x", rows_ok=rows_ok)
        assert torch.is_tensor(m) and m.dtype == torch.float32 and tuple(m.shape) == (6, 4) and m.device.type == "cpu"
        assert not m.requires_grad and np.array_equal(m.numpy(), want.astype(np.float32))          # n / 8 is exact in fp16
    grad = torch.ones(2, 3, requires_grad=True)
    assert not search.as_matrix(grad, "here: x").requires_grad
    for bad, rows_ok in ((torch.zeros(5), False), (np.zeros((2, 3, 4)), False), ([], True), ([], False), (torch.zeros(5), True)):
        with pytest.raises(ValueError, match=r"\[N, D\]") as e:
            search.as_matrix(bad, "here: x", rows_ok=rows_ok)
        assert "here: x" in str(e.value)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            search.to_device(want, "here: x", refuse_without_gpu=True)
    with pytest.raises(ValueError, match=r"\[N, D\]"):                 # the shape is refused before the device is asked for
        search.to_device(torch.zeros(5), "here: x", refuse_without_gpu=True)
    assert torch.cuda.is_initialized() == initialised


def test_stack_rows():
    feats = {"a": torch.tensor([1.0, 2.0]), "b": torch.tensor([3.0, 4.0]), "c": torch.tensor([5.0, 6.0])}
    got = search.stack_rows(feats, [("c", 0, 1), ("a", 7, 2), ("c", 0, 3)])
    assert torch.equal(got, torch.tensor([[5.0, 6.0], [1.0, 2.0], [5.0, 6.0]]))
    maps = {"a": torch.arange(6.0).view(3, 2, 1), "b": -torch.arange(6.0).view(3, 2, 1)}          # rows that are not flat yet
    assert torch.equal(search.stack_rows(maps, [("b", 0, 0), ("a", 0, 0)]), torch.stack([-torch.arange(6.0), torch.arange(6.0)]))


@pytest.mark.parametrize("ptr_dtype", [torch.int32, torch.int64])
def test_sorted_segments(ptr_dtype):
    uniq, perm, ptr = ops.sorted_segments(torch.tensor([3, 1, 3, 0, 1, 3]), ptr_dtype=ptr_dtype)
    assert uniq.tolist() == [0, 1, 3] and perm.tolist() == [3, 1, 4, 0, 2, 5] and ptr.tolist() == [0, 1, 3, 6]
    assert ptr.dtype == ptr_dtype and perm.dtype == torch.int64
    keys = np.random.RandomState(0).randint(0, 17, size=200)
    uniq, perm, ptr = ops.sorted_segments(torch.from_numpy(keys), ptr_dtype=ptr_dtype)
    want_uniq, want_counts = np.unique(keys, return_counts=True)
    assert np.array_equal(perm.numpy(), np.argsort(keys, kind="stable")) and np.array_equal(uniq.numpy(), want_uniq)
    assert np.array_equal(ptr.numpy(), np.concatenate([[0], np.cumsum(want_counts)])) and ptr.dtype == ptr_dtype


def test_compact_labels():
    inv, count = ops.compact_labels(torch.tensor([7, -1, 7, 40, -1]))
    assert inv.tolist() == [1, 0, 1, 2, 0] and inv.dtype == torch.int32 and inv.is_contiguous() and count == 3
    inv, count = ops.compact_labels(torch.tensor([5, 5, 5], dtype=torch.int32))
    assert inv.tolist() == [0, 0, 0] and count == 1


def test_list_total():
    cnt = torch.tensor([2, 0, 3], dtype=torch.int32)
    rowptr = torch.tensor([0, 2, 2, 5], dtype=torch.int32)
    assert ops._list_total(rowptr, cnt, 3, 9, "here") == 5
    # where the int32 prefix sum could have wrapped, the int64 sum of the counts is the total: a row pointer that disagrees is ignored
    wrapped = torch.tensor([0, 2, 2, -7], dtype=torch.int32)
    assert ops._list_total(wrapped, cnt, 3, 2 ** 31, "here") == 5
    with pytest.raises(RuntimeError, match="int32 row pointers"):
        ops._list_total(wrapped, cnt, 3, 2 ** 31 - 1, "here")          # below the threshold the row pointer is believed: -7
    big = torch.tensor([2 ** 30, 2 ** 30], dtype=torch.int32)
    with pytest.raises(RuntimeError, match="int32 row pointers") as e:
        ops._list_total(torch.zeros(3, dtype=torch.int32), big, 2, 2 ** 40, "here")          # a total of exactly 2^31
    assert "here" in str(e.value) and str(2 ** 31) in str(e.value)
    assert ops._list_total(torch.zeros(3, dtype=torch.int32), big - 1, 2, 2 ** 40, "here") == 2 ** 31 - 2
    assert ops._list_total(torch.zeros(4, dtype=torch.int32), torch.zeros(3, dtype=torch.int32), 3, 9, "here") == 0


def _defined(path):
    """names bound by def / class / assignment at module level (imports are not definitions)"""
    with open(path) as f:
        tree = ast.parse(f.read())
    names = []
    for node in tree.body:
        if isinstance(node, (ast.FunctionDef, ast.ClassDef)):
            names.append(node.name)
        elif isinstance(node, (ast.Assign, ast.AnnAssign, ast.AugAssign)):
            for tgt in (node.targets if isinstance(node, ast.Assign) else [node.target]):
                names += [n.id for n in ast.walk(tgt) if isinstance(n, ast.Name)]
    return names


def test_the_shared_steps_are_defined_once():
    files = [p for pkg in ("clustercontrast", "reid") for p in glob.glob(os.path.join(PKG, pkg, "**", "*.py"), recursive=True)]
    assert len(files) > 20, "the model packages were not found under %s" % PKG
    for path in files:
        again = sorted(set(_defined(path)) & {"_" + name for name in ("device", "BLOCK_ROWS", "dist_block")})      # the private copies
        assert not again, "%s defines %s: rg_hip/search.py states them" % (os.path.relpath(path, PKG), again)
    names = _defined(search.__file__)
    for name in ("BLOCK_ROWS", "device", "dist_block"):
        assert names.count(name) == 1, (name, names.count(name))
    assert search.BLOCK_ROWS == 2048
