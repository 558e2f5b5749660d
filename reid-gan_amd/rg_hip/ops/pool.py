"""Pooling and part pooling (csrc/pool.hip) and the fused multi-part head (csrc/part_head.hip)."""
from __future__ import absolute_import

import torch

from ._base import _chk, _dense, _nchw, _p, _pair, _stream, _ws_query, lib, workspace


# ------------------------------------------------------------------------------------------------
# pooling
# ------------------------------------------------------------------------------------------------
def maxpool2d_fwd(x, kernel=3, stride=2, padding=1):
    x = _chk(x, "x")
    N, C, H, W = x.shape
    kh, kw = _pair(kernel)
    sh, sw = _pair(stride)
    ph, pw = _pair(padding)
    P, Q = (H + 2 * ph - kh) // sh + 1, (W + 2 * pw - kw) // sw + 1
    y = torch.empty((N, C, P, Q), dtype=torch.float32, device=x.device)
    arg = torch.empty((N, C, P, Q), dtype=torch.uint8, device=x.device)
    lib.rg_maxpool2d_fwd(_p(x), _p(y), _p(arg), N, C, H, W, kh, kw, sh, sw, ph, pw, P, Q, _stream())
    return y, arg


def maxpool2d_bwd(dy, arg, x_shape, kernel=3, stride=2, padding=1):
    dy = _chk(dy, "dy")
    N, C, H, W = x_shape
    kh, kw = _pair(kernel)
    sh, sw = _pair(stride)
    ph, pw = _pair(padding)
    P, Q = dy.shape[2], dy.shape[3]
    dx = torch.empty(tuple(x_shape), dtype=torch.float32, device=dy.device)
    lib.rg_maxpool2d_bwd(_p(dy), _p(arg), _p(dx), N, C, H, W, kh, kw, sh, sw, ph, pw, P, Q, _stream())
    return dx


def global_avgpool_fwd(x):
    x = _chk(x, "x")
    N, C, HW = _nchw(x)
    y = torch.empty((N, C), dtype=torch.float32, device=x.device)
    lib.rg_global_avgpool_fwd(_p(x), _p(y), N, C, HW, _stream())
    return y


def global_avgpool_bwd(dy, x_shape):
    dy = _chk(dy, "dy")
    N, C = x_shape[0], x_shape[1]
    dx = torch.empty(tuple(x_shape), dtype=torch.float32, device=dy.device)
    lib.rg_global_avgpool_bwd(_p(dy), _p(dx), N, C, dx.numel() // (N * C), _stream())
    return dx


def gem_pool_fwd(x, p, eps=1e-6):
    x, p = _chk(x, "x"), _chk(p, "p")
    N, C, HW = _nchw(x)
    y = torch.empty((N, C), dtype=torch.float32, device=x.device)
    lib.rg_gem_pool_fwd(_p(x), _p(p), _p(y), N, C, HW, eps, _stream())
    return y


def gem_pool_bwd(x, p, y, dy, eps=1e-6, need_dp=True):
    x, p, y, dy = _chk(x, "x"), _chk(p, "p"), _chk(y, "y"), _chk(dy, "dy")
    N, C, HW = _nchw(x)
    dx = torch.empty_like(x)
    dp = torch.empty(1, dtype=torch.float32, device=x.device) if need_dp else None
    ws = workspace(N * C * 4, x.device)
    lib.rg_gem_pool_bwd(_p(x), _p(p), _p(y), _p(dy), _p(dx), _p(dp), N, C, HW, eps, _p(ws), ws.numel(), _stream())
    return dx, dp


def part_pool_fwd(x, split_row, p=None, eps=1e-6):
    """both row ranges [0, split_row) and [split_row, H) of every plane of x [N, C, H, W] pooled in one pass -> y [2, N, C];
    p None: average pooling, else GeM with the one-element device exponent"""
    x = _chk(x, "x")
    N, C, H, W = x.shape
    y = torch.empty((2, N, C), dtype=torch.float32, device=x.device)
    lib.rg_part_pool_fwd(_p(x), _p(None if p is None else _chk(p, "p")), _p(y), N, C, H, W, split_row, eps, _stream())
    return y


def part_pool_bwd(x_or_shape, split_row, dy, p=None, y=None, eps=1e-6, need_dp=True):
    """dy [2, N, C] -> (dx, dp); average pooling (p None) takes the shape of x in place of x and returns dp None"""
    dy = _chk(dy, "dy")
    if p is None:
        N, C, H, W = x_or_shape if not torch.is_tensor(x_or_shape) else x_or_shape.shape
        dx = torch.empty((N, C, H, W), dtype=torch.float32, device=dy.device)
        lib.rg_part_pool_bwd(None, None, None, _p(dy), _p(dx), None, N, C, H, W, split_row, eps, None, 0, _stream())
        return dx, None
    x, p, y = _chk(x_or_shape, "x"), _chk(p, "p"), _chk(y, "y")
    N, C, H, W = x.shape
    dx = torch.empty_like(x)
    dp = torch.empty(1, dtype=torch.float32, device=x.device) if need_dp else None
    ws = workspace(N * C * 4, x.device)
    lib.rg_part_pool_bwd(_p(x), _p(p), _p(y), _p(dy), _p(dx), _p(dp), N, C, H, W, split_row, eps, _p(ws), ws.numel(), _stream())
    return dx, dp


# ------------------------------------------------------------------------------------------------
# fused tail of the multi-part encoder (csrc/part_head.hip)
# ------------------------------------------------------------------------------------------------
def mp_head_fwd(xs, gammas, betas, running_means, running_vars, epss, momenta, train, fusion):
    """xs = (x_g, x_p1, x_p2), each [B, D]; per branch BatchNorm1d parameters / buffers.  fusion: 1 'sum', 0 the global branch.
    -> out [4, B, D] (f_g, f_p1, f_p2, f_gc), xhat [3, B, D], mean [3, D], invstd [3, D], norms [4, B]"""
    xs = [_dense(x, "x") for x in xs]
    B, D = xs[0].shape
    for x in xs:
        if tuple(x.shape) != (B, D):
            raise ValueError("rg_hip: mp_head_fwd inputs must share one [B, D] shape, got %s" % ([tuple(v.shape) for v in xs],))
    vecs = [v for grp in (gammas, betas, running_means, running_vars) for v in grp]
    if any(v.numel() != D or not v.is_contiguous() or not v.is_cuda or v.dtype != torch.float32 for v in vecs):
        raise ValueError("rg_hip: mp_head_fwd per-channel vectors must be contiguous float32 GPU tensors of %d elements" % D)
    dev = xs[0].device
    out = torch.empty((4, B, D), dtype=torch.float32, device=dev)
    xhat = torch.empty((3, B, D), dtype=torch.float32, device=dev)
    mean = torch.empty((3, D), dtype=torch.float32, device=dev)
    invstd = torch.empty((3, D), dtype=torch.float32, device=dev)
    norms = torch.empty((4, B), dtype=torch.float32, device=dev)
    ws = workspace(_ws_query("rg_mp_head_workspace", B, D), dev) if train else None
    lib.rg_mp_head_fwd(*[_p(x) for x in xs], *[_p(v) for v in vecs], _p(out), _p(xhat), _p(mean), _p(invstd), _p(norms), B, D,
                       1 if train else 0, int(fusion), *[float(e) for e in epss], *[float(m) for m in momenta], _p(ws),
                       ws.numel() if ws is not None else 0, _stream())
    return out, xhat, mean, invstd, norms


def mp_head_bwd(dys, xhat, invstd, norms, gammas, betas, train, fusion, need_dgamma=True, need_dbeta=False, dzs=(None, None, None)):
    """dys = (dy_g, dy_p1, dy_p2, dy_gc), None for an unused output; dzs: gradients arriving at the BatchNorm outputs z_j
    themselves.  -> dx [3, B, D], dgamma [3, D] or None, dbeta [3, D] or None,
    reached: per branch whether any given gradient reaches it (the dx / dgamma / dbeta rows of the others are not written)"""
    dys = [_dense(d, "dy") for d in dys]
    _, B, D = xhat.shape
    dzs = [_dense(d, "dz") for d in dzs]
    reached = [dys[0] is not None or dys[3] is not None or dzs[0] is not None]
    reached += [dys[j] is not None or dzs[j] is not None or (bool(fusion) and dys[3] is not None) for j in (1, 2)]
    dev = xhat.device
    dx = torch.empty((3, B, D), dtype=torch.float32, device=dev)
    dgamma = torch.empty((3, D), dtype=torch.float32, device=dev) if need_dgamma else None
    dbeta = torch.empty((3, D), dtype=torch.float32, device=dev) if need_dbeta else None

    def rows(t):
        return [_p(t[j]) if (t is not None and reached[j]) else None for j in range(3)]
    lib.rg_mp_head_bwd(*[_p(d) for d in dys], *[_p(d) for d in dzs], _p(xhat), _p(invstd), _p(norms), *[_p(v) for v in gammas],
                       *[_p(v) for v in betas], *rows(dx), *rows(dgamma), *rows(dbeta), B, D, 1 if train else 0,
                       int(fusion), _stream())
    return dx, dgamma, dbeta, reached
