"""The host steps every retrieval and pseudo-labelling recipe shares, stated once: the process's device, the coercion of
features to a contiguous fp32 [N, D] device matrix, query / gallery row assembly, the pairwise squared distances and the blocked
top-k search.  Host code over `rg_hip.ops`, no kernel of its own; importing it needs neither a GPU nor the built library."""
from __future__ import absolute_import

import numpy as np
import torch

from . import ops

BLOCK_ROWS = 2048        # rows of the [rows, n] score block one GEMM + top-k pass of blocked_topk handles


def device():
    return torch.device("cuda", torch.cuda.current_device())


def as_matrix(x, who, rows_ok=False):
    """detached fp32 2-D tensor of `x` (tensor, numpy array or array-like; with rows_ok also a sequence of row tensors) on the
    device `x` lives on; ValueError naming `who` for anything that is not a matrix.  Touches no device."""
    if not torch.is_tensor(x):
        if rows_ok and not isinstance(x, np.ndarray):
            x = list(x)
        if rows_ok and len(x) and all(torch.is_tensor(r) for r in x):
            x = torch.stack(x, dim=0)
        else:
            x = torch.as_tensor(np.asarray(x))
    if x.dim() != 2:
        raise ValueError("%s must be [N, D], got shape %s" % (who, tuple(x.shape)))
    return x.detach().float()


def to_device(x, who, rows_ok=False, refuse_without_gpu=False):
    """`as_matrix` moved to this process's device, contiguous.  refuse_without_gpu: the RuntimeError of the entry points
    that say so themselves when there is no GPU, raised after the shape check and before the device is touched."""
    x = as_matrix(x, who, rows_ok)
    if refuse_without_gpu and not torch.cuda.is_available():
        raise RuntimeError("%s must live on the GPU; the HIP path has no CPU fallback" % who)
    return x.to(device()).contiguous()


def stack_rows(features, entries):
    """[len(entries), D] block of the (flattened) features of (fname, pid, cam) triples, in their order"""
    return torch.cat([features[f].unsqueeze(0) for f, _, _ in entries], 0).flatten(1)


def dist_block(x, y, xx_scale, with_y_norm):
    """[m, n] block: xx_scale * |x_i|^2 (+ |y_j|^2) - 2 x_i . y_j — the GEMM with -2 folded into the MFMA epilogue."""
    n = y.shape[0]
    minus2 = ops.fill_(torch.empty(n, dtype=torch.float32, device=x.device), -2.0)
    yy = ops.row_sqsum(y) if with_y_norm else None
    d = ops.conv2d_fwd(x.view(x.shape[0], x.shape[1], 1, 1), y.view(n, y.shape[1], 1, 1), scale=minus2, shift=yy)
    d = d.view(x.shape[0], n)
    return ops.add_outer_terms(d, rowv=ops.row_sqsum(x), colv=None, alpha=1.0, a=xx_scale)


def pairwise(features, query=None, gallery=None):
    """(dist, x, y, xd, yd) of the reference's `pairwise_distance`: the squared distances [m, n] on the device, the query and
    gallery blocks [m, D] / [n, D] as the feature dictionary holds them and their fp32 device copies.  Without query and gallery:
    the self-distance matrix of all features, 2 |x_i|^2 - 2 x_i . x_j (the reference's expression), and four None."""
    if query is None and gallery is None:
        x = to_device(torch.cat(list(features.values())).view(len(features), -1), "pairwise_distance: features")
        return dist_block(x, x, 2.0, False), None, None, None, None
    x, y = stack_rows(features, query), stack_rows(features, gallery)
    xd, yd = to_device(x, "pairwise_distance: query features"), to_device(y, "pairwise_distance: gallery features")
    return dist_block(xd, yd, 1.0, True), x, y, xd, yd


def blocked_topk(n, k, score_block, rows=None, want_values=False):
    """int32 [n, k] columns of the k largest scores of every row (ties by lower column), and with want_values the fp32 scores:
    `score_block(r0, r1)` yields the [r1 - r0, cols] device scores of the rows r0 .. r1 - 1, `rows` (default BLOCK_ROWS) at a
    time, so no more than one block of scores is alive."""
    rows = BLOCK_ROWS if rows is None else int(rows)
    dev = device()
    idx = torch.empty((n, k), dtype=torch.int32, device=dev)
    val = torch.empty((n, k), dtype=torch.float32, device=dev) if want_values else None
    for r0 in range(0, n, rows):
        r1 = min(n, r0 + rows)
        i, v = ops.topk_rows(score_block(r0, r1), k)
        idx[r0:r1] = i
        if want_values:
            val[r0:r1] = v
    return (idx, val) if want_values else idx
