"""Convolution and linear layers: csrc/conv_*.hip behind rg_conv2d_fwd / rg_conv2d_dgrad / rg_conv2d_wgrad."""
from __future__ import absolute_import

import torch

from ._base import ACT_NONE, _chk, _p, _pair, _stream, _ws_query, lib, workspace
from .streams import _SIDE, _side_session, side_worth


# ------------------------------------------------------------------------------------------------
# convolution
# ------------------------------------------------------------------------------------------------
def conv_out_size(H, W, KH, KW, stride, padding):
    sh, sw = _pair(stride)
    ph, pw = _pair(padding)
    return (H + 2 * ph - KH) // sh + 1, (W + 2 * pw - KW) // sw + 1


def weights_to_krsc(w):
    """[K][C][KH][KW] -> [K][KH*KW][C] copy for the (r,s)-major kernels (1x1 filters need none)."""
    w = _chk(w, "w")
    K, C, KH, KW = w.shape
    wt = torch.empty((K, KH * KW, C), dtype=torch.float32, device=w.device)
    lib.rg_weights_to_krsc(_p(w), _p(wt), K, C, KH, KW, _stream())
    return wt


def conv2d_fwd(x, w, stride=1, padding=0, scale=None, shift=None, residual=None, act=ACT_NONE, slope=0.0,
               w_krsc=None):
    x, w = _chk(x, "x"), _chk(w, "w")
    N, C, H, W = x.shape
    K, Cw, KH, KW = w.shape
    if C != Cw:
        raise ValueError("conv2d_fwd: input has %d channels, weight expects %d" % (C, Cw))
    sh, sw = _pair(stride)
    ph, pw = _pair(padding)
    P, Q = conv_out_size(H, W, KH, KW, (sh, sw), (ph, pw))
    y = torch.empty((N, K, P, Q), dtype=torch.float32, device=x.device)
    scale, shift, residual = _chk(scale, "scale"), _chk(shift, "shift"), _chk(residual, "residual")
    if residual is not None and residual.shape != y.shape:
        raise ValueError("conv2d_fwd: residual shape %s != output shape %s" % (tuple(residual.shape), tuple(y.shape)))
    if w_krsc is None and KH * KW > 1 and C % 16 == 0:
        w_krsc = weights_to_krsc(w)
    nbytes = _ws_query("rg_conv2d_fwd_workspace", N, C, K, KH, KW, P, Q)
    ws = workspace(nbytes, x.device) if nbytes else None
    lib.rg_conv2d_fwd(_p(x), _p(w), _p(w_krsc), _p(y), N, C, H, W, K, KH, KW, sh, sw, ph, pw, P, Q, _p(scale), _p(shift),
                      _p(residual), act, slope, _p(ws), ws.numel() if ws is not None else 0, _stream())
    return y


def conv2d_dgrad(dy, w, x_hw, stride=1, padding=0, scale=None, shift=None, residual=None, act=ACT_NONE, slope=0.0,
                 w_krsc=None, relu_mask=None, want_rowsum=False):
    """dx[N][C][H][W] from dy[N][K][P][Q] and w[K][C][KH][KW]; x_hw = (H, W) of the conv input.
    Also the forward of ConvTranspose2d (weight [in=K][out=C][KH][KW], output size x_hw)."""
    dy, w = _chk(dy, "dy"), _chk(w, "w")
    N, K, P, Q = dy.shape
    Kw, C, KH, KW = w.shape
    if K != Kw:
        raise ValueError("conv2d_dgrad: dy has %d channels, weight expects %d" % (K, Kw))
    H, W = x_hw
    sh, sw = _pair(stride)
    ph, pw = _pair(padding)
    dx = torch.empty((N, C, H, W), dtype=torch.float32, device=dy.device)
    scale, shift, residual = _chk(scale, "scale"), _chk(shift, "shift"), _chk(residual, "residual")
    if residual is not None and residual.shape != dx.shape:
        raise ValueError("conv2d_dgrad: residual shape mismatch")
    if w_krsc is None and KH * KW > 1 and C % 4 == 0:
        w_krsc = weights_to_krsc(w)
    nbytes = _ws_query("rg_conv2d_dgrad_workspace", N, C, H, W, K, KH, KW, sh, sw)
    ws = workspace(nbytes, dy.device) if nbytes else None
    relu_mask = _chk(relu_mask, "relu_mask")
    if relu_mask is not None and relu_mask.shape != dx.shape:
        raise ValueError("conv2d_dgrad: relu_mask shape mismatch")
    rowsum, cols = None, 0
    if want_rowsum:
        # per-channel sums of the final dx in column blocks, written by the epilogue (0 columns: split-K / small-C launch)
        cols = _ws_query("rg_conv2d_dgrad_rowsum_cols", N, C, H, W, K, KH, KW, sh, sw, ph, pw, P, Q)
        if cols > 0:
            rowsum = torch.empty((C, cols), dtype=torch.float32, device=dy.device)
    lib.rg_conv2d_dgrad(_p(dy), _p(w), _p(w_krsc), _p(dx), N, C, H, W, K, KH, KW, sh, sw, ph, pw, P, Q, _p(scale),
                        _p(shift), _p(residual), act, slope, _p(relu_mask), _p(rowsum), cols, _p(ws),
                        ws.numel() if ws is not None else 0, _stream())
    if rowsum is not None:
        dx._rg_rowsum = rowsum          # rides with the gradient to the BatchNorm fold of the layer below (nn.fold.conv_bn_tb)
    return dx


def conv2d_wgrad(x, dy, w_shape, stride=1, padding=0, out=None, side=False, after=None, fold=None):
    """dw[K][C][KH][KW]; side=True launches on the backward session's side stream; `after(dw)` is enqueued right
    behind the wgrad kernels on the same stream; `fold` = (w, scale, invstd, running_mean, sum_g, partials, dbeta, dgamma): the
    folded-BatchNorm finish of rg_conv2d_wgrad_fold (dw = scale G, dgamma, dbeta) runs inside the same call."""
    if side and _SIDE["on"] and side_worth(2e-9 * dy.numel() * w_shape[1] * w_shape[2] * w_shape[3]):
        main, sess = _side_session(create=False)
        if sess is not None and sess.depth > 0:
            x, dy = _chk(x, "x"), _chk(dy, "dy")
            dw = out if out is not None else torch.empty(tuple(w_shape), dtype=torch.float32, device=x.device)
            ev = torch.cuda.Event()
            ev.record(main)
            sess.stream.wait_event(ev)
            with torch.cuda.stream(sess.stream):
                conv2d_wgrad(x, dy, w_shape, stride, padding, out=dw, after=after, fold=fold)
            sess.refs.append((x, dy, dw, after, fold))   # the hook's closure / the fold's operands stay alive too
            sess.used = True
            return dw
    x, dy = _chk(x, "x"), _chk(dy, "dy")
    N, C, H, W = x.shape
    K, Cw, KH, KW = w_shape
    Nd, Kd, P, Q = dy.shape
    if (N, K, C) != (Nd, Kd, Cw):
        raise ValueError("conv2d_wgrad: inconsistent shapes x=%s dy=%s w=%s" % (tuple(x.shape), tuple(dy.shape), w_shape))
    sh, sw = _pair(stride)
    ph, pw = _pair(padding)
    dw = out if out is not None else torch.empty(tuple(w_shape), dtype=torch.float32, device=x.device)
    nbytes = _ws_query("rg_conv2d_wgrad_workspace", N, C, K, KH, KW, P, Q)
    ws = workspace(nbytes, x.device)
    if fold is not None:
        fw, fscale, finvstd, fmean, fsum, fpart, fdbeta, fdgamma = fold
        lib.rg_conv2d_wgrad_fold(_p(x), _p(dy), _p(dw), N, C, H, W, K, KH, KW, sh, sw, ph, pw, P, Q, _p(fw), _p(fscale),
                                 _p(finvstd), _p(fmean), _p(fsum), _p(fpart), fpart.shape[1] if fpart is not None else 0,
                                 _p(fdbeta), _p(fdgamma), _p(ws), ws.numel(), _stream())
    else:
        lib.rg_conv2d_wgrad(_p(x), _p(dy), _p(dw), N, C, H, W, K, KH, KW, sh, sw, ph, pw, P, Q, _p(ws), ws.numel(),
                            _stream())
    if after is not None:
        after(dw)
    return dw


def linear_fwd(x, w, bias=None):
    """y[B][out] = x[B][in] @ w[out][in]^T + bias, as a 1x1 conv on a 1x1 map."""
    B, Cin = x.shape
    y = conv2d_fwd(x.view(B, Cin, 1, 1), w.view(w.shape[0], Cin, 1, 1), shift=bias)
    return y.view(B, w.shape[0])


def linear_dgrad(dy, w):
    B, K = dy.shape
    dx = conv2d_dgrad(dy.view(B, K, 1, 1), w.view(K, w.shape[1], 1, 1), (1, 1))
    return dx.view(B, w.shape[1])


def linear_wgrad(x, dy, out=None):
    B, Cin = x.shape
    K = dy.shape[1]
    return conv2d_wgrad(x.view(B, Cin, 1, 1), dy.view(B, K, 1, 1), (K, Cin, 1, 1), out=out).view(K, Cin)
