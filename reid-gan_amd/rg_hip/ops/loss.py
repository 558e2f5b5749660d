"""Loss kernels (csrc/loss.hip): forward values and their gradients."""
from __future__ import absolute_import

import torch

from ._base import _chk, _p, _same_size, _stream, lib, workspace


# ------------------------------------------------------------------------------------------------
# losses
# ------------------------------------------------------------------------------------------------
def _loss_ws(device):
    return workspace(lib.rg_loss_workspace(), device)


def sigmoid_bce_fwd(x, target):
    x = _chk(x, "x")
    out = torch.empty((), dtype=torch.float32, device=x.device)
    ws = _loss_ws(x.device)
    lib.rg_sigmoid_bce_fwd(_p(x), _p(out), x.numel(), float(target), _p(ws), ws.numel(), _stream())
    return out


def sigmoid_bce_bwd(x, grad_out, target, grad_scale=1.0):
    x = _chk(x, "x")
    dx = torch.empty_like(x)
    lib.rg_sigmoid_bce_bwd(_p(x), _p(grad_out), _p(dx), x.numel(), float(target), grad_scale, _stream())
    return dx


def mse_const_fwd(x, target):
    x = _chk(x, "x")
    out = torch.empty((), dtype=torch.float32, device=x.device)
    ws = _loss_ws(x.device)
    lib.rg_mse_const_fwd(_p(x), _p(out), x.numel(), float(target), _p(ws), ws.numel(), _stream())
    return out


def mse_const_bwd(x, grad_out, target, grad_scale=1.0):
    x = _chk(x, "x")
    dx = torch.empty_like(x)
    lib.rg_mse_const_bwd(_p(x), _p(grad_out), _p(dx), x.numel(), float(target), grad_scale, _stream())
    return dx


def affine_relu_mean_fwd(x, a, b, clamp):
    x = _chk(x, "x")
    loss = torch.empty((), dtype=torch.float32, device=x.device)
    ws = _loss_ws(x.device)
    lib.rg_affine_relu_mean_fwd(_p(x), _p(loss), x.numel(), a, b, int(clamp), _p(ws), ws.numel(), _stream())
    return loss


def affine_relu_mean_bwd(x, grad_out, a, b, clamp, grad_scale=1.0):
    x = _chk(x, "x")
    dx = torch.empty_like(x)
    lib.rg_affine_relu_mean_bwd(_p(x), _p(grad_out), _p(dx), x.numel(), a, b, int(clamp), grad_scale, _stream())
    return dx


def grad_penalty_rows(g, constant, scale):
    """(pen[rows], v[rows, D]): pen[r] = scale * (|g_r + 1e-16| - constant)^2 and its gradient with respect to g_r."""
    g = _chk(g, "g")
    rows, D = g.shape
    pen = torch.empty(rows, dtype=torch.float32, device=g.device)
    v = torch.empty_like(g)
    lib.rg_grad_penalty_rows(_p(g), _p(pen), _p(v), rows, D, float(constant), float(scale), _stream())
    return pen, v


def l1_fwd(a, b, row_labels=None):
    a, b = _chk(a, "a"), _chk(b, "b")
    row_labels = _chk(row_labels, "row_labels", torch.int64)
    rows = a.shape[0]
    inner = a.numel() // rows
    out2 = torch.empty(2, dtype=torch.float32, device=a.device)
    ws = _loss_ws(a.device)
    lib.rg_l1_fwd(_p(a), _p(b), _p(row_labels), _p(out2), rows, inner, _p(ws), ws.numel(), _stream())
    return out2


def l1_bwd(a, b, row_labels, grad_out, out2, need_a=True, need_b=True, grad_scale=1.0):
    a, b = _chk(a, "a"), _chk(b, "b")
    rows = a.shape[0]
    inner = a.numel() // rows
    da = torch.empty_like(a) if need_a else None
    db = torch.empty_like(a) if need_b else None
    lib.rg_l1_bwd(_p(a), _p(b), _p(row_labels), _p(grad_out), _p(out2), _p(da), _p(db), rows, inner, grad_scale,
                  _stream())
    return da, db


def l1_rows_fwd(a, b):
    a, b = _chk(a, "a"), _chk(b, "b")
    _same_size("l1_rows_fwd", a, b=b)
    rows = a.shape[0]
    out = torch.empty(rows, dtype=torch.float32, device=a.device)
    lib.rg_l1_rows_fwd(_p(a), _p(b), _p(out), rows, a.numel() // rows, _stream())
    return out


def l1_rows_bwd(a, b, grad_rows, need_a=True, need_b=True):
    a, b, grad_rows = _chk(a, "a"), _chk(b, "b"), _chk(grad_rows, "grad_rows")
    rows = a.shape[0]
    da = torch.empty_like(a) if need_a else None
    db = torch.empty_like(a) if need_b else None
    lib.rg_l1_rows_bwd(_p(a), _p(b), _p(grad_rows), _p(da), _p(db), rows, a.numel() // rows, _stream())
    return da, db


def mse_const_rows_fwd(x, c):
    x = _chk(x, "x")
    rows = x.shape[0]
    out = torch.empty(rows, dtype=torch.float32, device=x.device)
    lib.rg_mse_const_rows_fwd(_p(x), float(c), _p(out), rows, x.numel() // rows, _stream())
    return out


def mse_const_rows_bwd(x, c, grad_rows):
    x, grad_rows = _chk(x, "x"), _chk(grad_rows, "grad_rows")
    rows = x.shape[0]
    dx = torch.empty_like(x)
    lib.rg_mse_const_rows_bwd(_p(x), float(c), _p(grad_rows), _p(dx), rows, x.numel() // rows, _stream())
    return dx


def softmax_ce_fwd(logits, labels, scale=1.0):
    logits = _chk(logits, "logits")
    labels = _chk(labels, "labels", torch.int64)
    B, K = logits.shape
    loss = torch.empty(B, dtype=torch.float32, device=logits.device)
    lse = torch.empty(B, dtype=torch.float32, device=logits.device)
    lib.rg_softmax_ce_fwd(_p(logits), _p(labels), _p(loss), _p(lse), B, K, scale, _stream())
    return loss, lse


def softmax_ce_bwd(logits, labels, lse, grad_rows, scale=1.0, grad_scale=1.0):
    logits = _chk(logits, "logits")
    grad_rows = _chk(grad_rows, "grad_rows")
    B, K = logits.shape
    dz = torch.empty_like(logits)
    lib.rg_softmax_ce_bwd(_p(logits), _p(labels), _p(lse), _p(grad_rows), _p(dz), B, K, scale, grad_scale, _stream())
    return dz


def weighted_sum_fwd(x, w=None, scale=1.0):
    x, w = _chk(x, "x"), _chk(w, "w")
    out = torch.empty((), dtype=torch.float32, device=x.device)
    lib.rg_weighted_sum_fwd(_p(x), _p(w), _p(out), x.numel(), scale, _stream())
    return out


def weighted_sum_bwd(grad_out, w, n, scale, device):
    dx = torch.empty(n, dtype=torch.float32, device=device)
    lib.rg_weighted_sum_bwd(_p(grad_out), _p(w), _p(dx), n, scale, _stream())
    return dx
