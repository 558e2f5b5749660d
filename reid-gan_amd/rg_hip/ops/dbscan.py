"""DBSCAN on the device (csrc/dbscan.hip)."""
from __future__ import absolute_import

import torch

from ._base import _chk_rr, _eps32, _list_total, _p, _stream, lib


# ------------------------------------------------------------------------------------------------
# DBSCAN on a precomputed distance matrix (csrc/dbscan.hip): CSR neighbour lists, union-find, labels
# ------------------------------------------------------------------------------------------------
def _chk_dbscan_matrix(d):
    d = _chk_rr(d, "d", torch.float16 if torch.is_tensor(d) and d.dtype == torch.float16 else torch.float32, 2)
    if d.shape[0] != d.shape[1] or d.shape[0] < 1:
        raise ValueError("rg_hip: d must be a square [N, N] matrix, got shape %s" % (tuple(d.shape),))
    return d


def _chk_dbscan_lists(rowptr, nbr, core):
    rowptr, nbr, core = _chk_rr(rowptr, "rowptr", torch.int32, 1), _chk_rr(nbr, "nbr", torch.int32, 1), _chk_rr(core, "core", torch.int32, 1)
    N = core.numel()
    if N < 1 or rowptr.numel() != N + 1:
        raise ValueError("rg_hip: dbscan: rowptr %s and core %s disagree" % (tuple(rowptr.shape), tuple(core.shape)))
    return rowptr, nbr, core, N


def _nbr_ptr(nbr):
    """an empty list (every row empty) still needs an address: the entry points refuse NULL"""
    return _p(nbr) if nbr.numel() else _p(torch.empty((1,), dtype=torch.int32, device=nbr.device))


def dbscan_count(d, eps):
    """(cnt int32 [N], rowptr int32 [N + 1]): entries of every row of d [N, N] that are <= eps, and their exclusive prefix sum"""
    d = _chk_dbscan_matrix(d)
    N = d.shape[0]
    cnt = torch.empty((N,), dtype=torch.int32, device=d.device)
    rowptr = torch.empty((N + 1,), dtype=torch.int32, device=d.device)
    lib.rg_dbscan_count(_p(d), int(d.dtype == torch.float16), N, N, _eps32(eps), _p(cnt), _p(rowptr), _stream())
    return cnt, rowptr


def dbscan_fill(d, eps, min_samples, rowptr, nnz):
    """(nbr int32 [nnz], core int32 [N]) for the row pointers of dbscan_count on the same matrix (nnz = rowptr[N])"""
    d, rowptr = _chk_dbscan_matrix(d), _chk_rr(rowptr, "rowptr", torch.int32, 1)
    N, min_samples, nnz = d.shape[0], int(min_samples), int(nnz)
    if min_samples < 1:
        raise ValueError("rg_hip: dbscan needs min_samples >= 1, got %d" % min_samples)
    if rowptr.numel() != N + 1 or nnz < 0 or nnz >= 2 ** 31:
        raise ValueError("rg_hip: dbscan_fill: rowptr %s, nnz %d do not fit d %s" % (tuple(rowptr.shape), nnz, tuple(d.shape)))
    nbr = torch.empty((nnz,), dtype=torch.int32, device=d.device)
    core = torch.empty((N,), dtype=torch.int32, device=d.device)
    lib.rg_dbscan_fill(_p(d), int(d.dtype == torch.float16), N, N, _eps32(eps), min_samples, _p(rowptr), _nbr_ptr(nbr), _p(core), _stream())
    return nbr, core


def dbscan_neighbors(d, eps, min_samples):
    """(rowptr int32 [N + 1], nbr int32 [nnz], core int32 [N]) of the symmetric distance matrix d [N, N] (fp32 or fp16):
    nbr[rowptr[i]:rowptr[i + 1]] = the columns j with d[i, j] <= eps, ascending (compared in fp32 against float32(eps); the
    diagonal is an entry like any other), core[i] = 1 where that list has at least min_samples entries.  Two passes over
    the matrix; reads one integer back (nnz) to size the list."""
    d = _chk_dbscan_matrix(d)
    if int(min_samples) < 1:
        raise ValueError("rg_hip: dbscan needs min_samples >= 1, got %d" % int(min_samples))
    N = d.shape[0]
    cnt, rowptr = dbscan_count(d, eps)
    nnz = _list_total(rowptr, cnt, N, N * N, "dbscan_neighbors")      # the int32 prefix sum can wrap only beyond 46 340 rows
    nbr, core = dbscan_fill(d, eps, min_samples, rowptr, nnz)
    return rowptr, nbr, core


def dbscan_components(rowptr, nbr, core):
    """parent int32 [N]: for a core point the lowest core index of its connected component in the core-core graph, -1 for
    the others.  One launch sequence, no host loop; the result does not depend on the order of the integer atomics."""
    rowptr, nbr, core, N = _chk_dbscan_lists(rowptr, nbr, core)
    parent = torch.empty((N,), dtype=torch.int32, device=core.device)
    lib.rg_dbscan_components(_p(rowptr), _nbr_ptr(nbr), _p(core), N, _p(parent), _stream())
    return parent


def dbscan_labels(rowptr, nbr, core, parent):
    """(labels int64 [N], n_clusters int): clusters numbered in ascending order of their lowest core index; a non-core point
    gets the lowest number among its core neighbours, or -1.  Reads one integer back (n_clusters)."""
    rowptr, nbr, core, N = _chk_dbscan_lists(rowptr, nbr, core)
    parent = _chk_rr(parent, "parent", torch.int32, 1)
    if parent.numel() != N:
        raise ValueError("rg_hip: dbscan_labels: parent %s and core %s disagree" % (tuple(parent.shape), tuple(core.shape)))
    isroot = torch.empty((N,), dtype=torch.int32, device=core.device)
    rootnum = torch.empty((N + 1,), dtype=torch.int32, device=core.device)
    labels = torch.empty((N,), dtype=torch.int64, device=core.device)
    lib.rg_dbscan_labels(_p(rowptr), _nbr_ptr(nbr), _p(parent), N, _p(isroot), _p(rootnum), _p(labels), _stream())
    return labels, int(rootnum[N].item())


def dbscan_asymmetry(d):
    """number of entries above the diagonal of d [N, N] whose bits differ from their mirror's (reads one integer back)"""
    d = _chk_dbscan_matrix(d)
    count = torch.empty((1,), dtype=torch.int32, device=d.device)
    lib.rg_dbscan_asymmetry(_p(d), int(d.dtype == torch.float16), d.shape[0], d.shape[0], _p(count), _stream())
    return int(count.item())


def dbscan(d, eps, min_samples, debug=False):
    """(labels int64 [N], n_clusters int) of scikit-learn's DBSCAN(eps, min_samples, metric='precomputed') on the symmetric
    matrix d, which stays on the device.  debug=True also returns {"rowptr", "nbr", "core", "parent"} (device tensors)."""
    rowptr, nbr, core = dbscan_neighbors(d, eps, min_samples)
    parent = dbscan_components(rowptr, nbr, core)
    labels, n_clusters = dbscan_labels(rowptr, nbr, core, parent)
    if debug:
        return labels, n_clusters, dict(rowptr=rowptr, nbr=nbr, core=core, parent=parent)
    return labels, n_clusters
