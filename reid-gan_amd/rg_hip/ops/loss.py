"""Loss kernels (csrc/loss.hip): forward values and their gradients; the fused verification head (csrc/verif_head.hip)."""
from __future__ import absolute_import

import torch

from ._base import _chk, _dense, _p, _same_size, _stream, _ws_query, lib, workspace


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


def _ce_ext_shape(la, lb, group):
    """(n, m, t) of the two logit blocks la [n, m] | lb [n, t]; n == t * group, or the group-diagonal mask has no meaning (the
    reference dies in a shape error there)"""
    if la.dim() != 2 or lb.dim() != 2 or la.shape[0] != lb.shape[0]:
        raise ValueError("softmax_ce_ext: logit blocks must be [n, m] and [n, t], got %s and %s" % (tuple(la.shape), tuple(lb.shape)))
    n, m = la.shape
    t = lb.shape[1]
    if group <= 0 or t * group != n:
        raise ValueError("softmax_ce_ext: %d rows are not %d groups of %d" % (n, t, group))
    return n, m, t


def softmax_ce_ext_fwd(la, lb, labels, group, mask, scale=1.0):
    """per-row cross entropy of cat([la, lb + mask * (column == row // group)], 1) * scale without the concatenation or the mask
    tensor -> (loss_rows [n], lse [n])"""
    la, lb = _chk(la, "la"), _chk(lb, "lb")
    labels = _chk(labels, "labels", torch.int64)
    n, m, t = _ce_ext_shape(la, lb, group)
    loss = torch.empty(n, dtype=torch.float32, device=la.device)
    lse = torch.empty(n, dtype=torch.float32, device=la.device)
    lib.rg_softmax_ce_ext_fwd(_p(la), _p(lb), _p(labels), _p(loss), _p(lse), n, m, t, group, mask, scale, _stream())
    return loss, lse


def softmax_ce_ext_bwd(la, lb, labels, lse, grad_rows, group, mask, scale=1.0, grad_scale=1.0):
    """(dla [n, m], dlb [n, t]) = grad_rows (ones when None) * grad_scale * scale * (softmax - onehot)"""
    la, lb = _chk(la, "la"), _chk(lb, "lb")
    grad_rows = _chk(grad_rows, "grad_rows")
    n, m, t = _ce_ext_shape(la, lb, group)
    dla, dlb = torch.empty_like(la), torch.empty_like(lb)
    lib.rg_softmax_ce_ext_bwd(_p(la), _p(lb), _p(labels), _p(lse), _p(grad_rows), grad_scale, _p(dla), _p(dlb), n, m, t, group,
                              mask, scale, _stream())
    return dla, dlb


def _verif_vec(t, name, n):
    t = _dense(t, name)
    if t is not None and t.numel() != n:
        raise ValueError("rg_hip: verif_head %s must hold %d elements, got shape %s" % (name, n, tuple(t.shape)))
    return t


def verif_head_fwd(x1, x2, gamma, beta, running_mean, running_var, weight, bias, labels, train, eps, momentum):
    """The verification head of FD-GAN stage I (csrc/verif_head.hip): logits = Linear(BatchNorm1d((x1 - x2)^2)) and, with
    `labels` (int64 [B]), its mean cross entropy and top-1 precision.  x1, x2 [B, D]; weight [C, D], C <= 16; bias [C] or None.
    Train mode updates running_mean / running_var in place.
    -> logits [B, C], xhat [B, D], mean [D], invstd [D], loss_rows [B], out2 [2] = (loss, correct / B), dlogits [B, C] =
    (softmax - onehot) / B; the last three are None without labels"""
    x1, x2 = _dense(x1, "x1"), _dense(x2, "x2")
    if x1.dim() != 2 or x1.shape != x2.shape:
        raise ValueError("rg_hip: verif_head_fwd inputs must share one [B, D] shape, got %s and %s" % (tuple(x1.shape), tuple(x2.shape)))
    B, D = x1.shape
    weight = _dense(weight, "weight")
    if weight.dim() != 2 or weight.shape[1] != D:
        raise ValueError("rg_hip: verif_head_fwd weight must be [C, %d], got %s" % (D, tuple(weight.shape)))
    C = weight.shape[0]
    gamma, beta = _verif_vec(gamma, "gamma", D), _verif_vec(beta, "beta", D)
    bias = _verif_vec(bias, "bias", C)
    for name, t in (("running_mean", running_mean), ("running_var", running_var)):     # updated in place: a copy would be lost
        if not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != D:
            raise ValueError("rg_hip: verif_head_fwd %s must be a contiguous float32 GPU tensor of %d elements" % (name, D))
    if train and B < 2:
        raise ValueError("Expected more than 1 value per channel when training, got input size %s" % (tuple(x1.shape),))
    labels = _chk(labels, "labels", torch.int64)
    if labels is not None and labels.numel() != B:
        raise ValueError("rg_hip: verif_head_fwd takes one label per row, got %d for %d rows" % (labels.numel(), B))
    dev = x1.device
    logits = torch.empty((B, C), dtype=torch.float32, device=dev)
    xhat = torch.empty((B, D), dtype=torch.float32, device=dev)
    mean = torch.empty(D, dtype=torch.float32, device=dev)
    invstd = torch.empty(D, dtype=torch.float32, device=dev)
    loss_rows = out2 = dlogits = None
    if labels is not None:
        loss_rows = torch.empty(B, dtype=torch.float32, device=dev)
        out2 = torch.empty(2, dtype=torch.float32, device=dev)
        dlogits = torch.empty((B, C), dtype=torch.float32, device=dev)
    ws = workspace(_ws_query("rg_verif_head_workspace", B, D, C), dev) if train else None
    lib.rg_verif_head_fwd(_p(x1), _p(x2), _p(gamma), _p(beta), _p(running_mean), _p(running_var), _p(weight), _p(bias), _p(labels),
                          _p(logits), _p(xhat), _p(mean), _p(invstd), _p(loss_rows), _p(out2), _p(dlogits), B, D, C,
                          1 if train else 0, float(eps), float(momentum), _p(ws), ws.numel() if ws is not None else 0, _stream())
    return logits, xhat, mean, invstd, loss_rows, out2, dlogits


def verif_head_bwd(grad_loss, dlogits, dlogits_up, x1, x2, xhat, invstd, gamma, beta, weight, train, need_dx=(True, True),
                   need_dweight=True, need_dbias=True, need_dgamma=True, need_dbeta=True, out=(None, None, None, None)):
    """The logit gradient is grad_loss (1-element device tensor, None = 1) * dlogits (the forward's, None = no loss) + dlogits_up
    (an upstream gradient of the logits, or None).  out: destinations for (dweight, dbias, dgamma, dbeta), None = allocate.
    -> dx1, dx2, dweight, dbias, dgamma, dbeta (None where not needed)"""
    x1, x2, xhat = _dense(x1, "x1"), _dense(x2, "x2"), _dense(xhat, "xhat")
    B, D = xhat.shape
    weight = _dense(weight, "weight")
    C = weight.shape[0]
    if tuple(x1.shape) != (B, D) or tuple(x2.shape) != (B, D) or weight.shape[1] != D:
        raise ValueError("rg_hip: verif_head_bwd shapes do not match xhat %s" % (tuple(xhat.shape),))
    if dlogits is None and dlogits_up is None:
        raise ValueError("rg_hip: verif_head_bwd needs dlogits or dlogits_up")
    grad_loss = _dense(grad_loss, "grad_loss") if dlogits is not None else None
    dlogits, dlogits_up = _dense(dlogits, "dlogits"), _dense(dlogits_up, "dlogits_up")
    for name, t in (("dlogits", dlogits), ("dlogits_up", dlogits_up)):
        if t is not None and t.numel() != B * C:
            raise ValueError("rg_hip: verif_head_bwd %s must be [%d, %d], got %s" % (name, B, C, tuple(t.shape)))
    gamma, beta, invstd = _verif_vec(gamma, "gamma", D), _verif_vec(beta, "beta", D), _verif_vec(invstd, "invstd", D)
    dev = xhat.device

    def dst(need, given, shape):
        if not need:
            return None
        if given is not None and given.is_contiguous() and given.numel() == (shape[0] if len(shape) == 1 else shape[0] * shape[1]):
            return given
        return torch.empty(shape, dtype=torch.float32, device=dev)
    dx1 = torch.empty((B, D), dtype=torch.float32, device=dev) if need_dx[0] else None
    dx2 = torch.empty((B, D), dtype=torch.float32, device=dev) if need_dx[1] else None
    dw, db = dst(need_dweight, out[0], (C, D)), dst(need_dbias, out[1], (C,))
    dga, dbe = dst(need_dgamma, out[2], (D,)), dst(need_dbeta, out[3], (D,))
    lib.rg_verif_head_bwd(_p(grad_loss), _p(dlogits), _p(dlogits_up), _p(x1), _p(x2), _p(xhat), _p(invstd), _p(gamma), _p(beta),
                          _p(weight), _p(dx1), _p(dx2), _p(dw), _p(db), _p(dga), _p(dbe), B, D, C, 1 if train else 0, _stream())
    return dx1, dx2, dw, db, dga, dbe


def weighted_sum_fwd(x, w=None, scale=1.0):
    x, w = _chk(x, "x"), _chk(w, "w")
    out = torch.empty((), dtype=torch.float32, device=x.device)
    lib.rg_weighted_sum_fwd(_p(x), _p(w), _p(out), x.numel(), scale, _stream())
    return out


def weighted_sum_bwd(grad_out, w, n, scale, device):
    dx = torch.empty(n, dtype=torch.float32, device=device)
    lib.rg_weighted_sum_bwd(_p(grad_out), _p(w), _p(dx), n, scale, _stream())
    return dx
