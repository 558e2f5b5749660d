"""Blocks of the GAN networks (csrc/gan_extra.hip): average pooling, reflection padding with a fused activation, spectral
normalisation."""
from __future__ import absolute_import

import ctypes

import torch

from ._base import ACT_LEAKY, ACT_NONE, ACT_RELU, _chk, _p, _stream, _ws_query, lib, workspace


def avgpool2d_fwd(x, k=2):
    x = _chk(x, "x")
    N, C, H, W = x.shape
    y = torch.empty((N, C, H // k, W // k), dtype=torch.float32, device=x.device)
    lib.rg_avgpool2d_fwd(_p(x), _p(y), N, C, H, W, k, _stream())
    return y


def avgpool2d_bwd(dy, x_shape, k=2):
    dy = _chk(dy, "dy")
    N, C, H, W = x_shape
    dx = torch.empty((N, C, H, W), dtype=torch.float32, device=dy.device)
    lib.rg_avgpool2d_bwd(_p(dy), _p(dx), N, C, H, W, k, _stream())
    return dx


def reflection_pad_fusable(x, pad, act, slope):
    """can rg_reflection_pad2d_* fold this activation in? (ReLU / LeakyReLU with a positive slope, float4 rows, pad <= 3)"""
    return (act == ACT_RELU or (act == ACT_LEAKY and slope > 0.0)) and x.shape[3] % 4 == 0 and x.shape[3] >= 8 and pad <= 3


def reflection_pad2d_fwd(x, pad, act=ACT_NONE, slope=0.0):
    """pad(act(x)) in one pass"""
    x = _chk(x, "x")
    N, C, H, W = x.shape
    y = torch.empty((N, C, H + 2 * pad, W + 2 * pad), dtype=torch.float32, device=x.device)
    lib.rg_reflection_pad2d_fwd(_p(x), _p(y), N, C, H, W, pad, act, slope, _stream())
    return y


def reflection_pad2d_bwd(dy, pad, x_act=None, act=ACT_NONE, slope=0.0):
    """act'(x_act) * pad^T(dy) in one pass (x_act: what the forward padded; only with act)"""
    dy, x_act = _chk(dy, "dy"), _chk(x_act, "x_act")
    N, C, OH, OW = dy.shape
    H, W = OH - 2 * pad, OW - 2 * pad
    if act != ACT_NONE and (x_act is None or tuple(x_act.shape) != (N, C, H, W)):
        raise ValueError("reflection_pad2d_bwd: the fused activation backward needs the forward input [N, C, H, W]")
    dx = torch.empty((N, C, H, W), dtype=torch.float32, device=dy.device)
    lib.rg_reflection_pad2d_bwd(_p(dy), _p(x_act) if act != ACT_NONE else None, _p(dx), N, C, H, W, pad, act, slope, _stream())
    return dx


def spectral_norm_fwd(w, u, v, training=True, eps=1e-12, save_uv=False):
    """One power iteration in place on u, v (training) and W / sigma; returns (w_sn, sigma[2] = (sigma, 1/sigma)) and, with
    `save_uv`, private copies of the u, v this forward used (written by the same launch)."""
    w = _chk(w, "w")
    K = w.shape[0]
    M = w.numel() // K
    if u.numel() != K or v.numel() != M or not (u.is_contiguous() and v.is_contiguous()):
        raise ValueError("spectral_norm: u / v do not match the weight matrix %d x %d" % (K, M))
    w_sn = torch.empty_like(w)
    sigma = torch.empty(2, dtype=torch.float32, device=w.device)
    saved = torch.empty(K + M, dtype=torch.float32, device=w.device) if save_uv else None
    lib.rg_spectral_norm_fwd(_p(w), _p(u), _p(v), _p(w_sn), _p(sigma), _p(saved), K, M, int(bool(training)), eps, _stream())
    if save_uv:
        return w_sn, sigma, saved[:K], saved[K:]
    return w_sn, sigma


class _SNDesc(ctypes.Structure):
    _fields_ = [("w", ctypes.c_void_p), ("u", ctypes.c_void_p), ("v", ctypes.c_void_p), ("w_sn", ctypes.c_void_p),
                ("sigma", ctypes.c_void_p), ("uv_saved", ctypes.c_void_p), ("K", ctypes.c_int), ("M", ctypes.c_int)]


def spectral_norm_fwd_multi(items, training=True, eps=1e-12, save_uv=False):
    """`items`: [(w, u, v)] of one network forward -> [(w_sn, sigma, u_saved, v_saved)] in two launches (rg_spectral_norm_fwd_multi);
    outputs are views of one allocation."""
    n = len(items)
    dev = items[0][0].device
    sizes = []
    total = 0
    for w, u, v in items:
        w = _chk(w, "w")
        K = w.shape[0]
        M = w.numel() // K
        if u.numel() != K or v.numel() != M or not (u.is_contiguous() and v.is_contiguous()):
            raise ValueError("spectral_norm: u / v do not match the weight matrix %d x %d" % (K, M))
        sizes.append((K, M, total))
        total += (K * M + 3) // 4 * 4 + 4 + ((K + M + 3) // 4 * 4 if save_uv else 0)
    buf = torch.empty(total, dtype=torch.float32, device=dev)
    base = buf.data_ptr()
    descs = (_SNDesc * n)()
    out = []
    for i, ((w, u, v), (K, M, off)) in enumerate(zip(items, sizes)):
        o_sig = off + (K * M + 3) // 4 * 4
        o_uv = o_sig + 4
        d = descs[i]
        d.w, d.u, d.v = w.data_ptr(), u.data_ptr(), v.data_ptr()
        d.w_sn, d.sigma = base + 4 * off, base + 4 * o_sig
        d.uv_saved = base + 4 * o_uv if save_uv else None
        d.K, d.M = K, M
        out.append((buf[off:off + K * M].view(w.shape), buf[o_sig:o_sig + 2],
                    buf[o_uv:o_uv + K] if save_uv else None, buf[o_uv + K:o_uv + K + M] if save_uv else None))
    lib.rg_spectral_norm_fwd_multi(ctypes.addressof(descs), n, int(bool(training)), eps, _stream())
    return out


def spectral_norm_bwd(dw_sn, w_sn, u, v, sigma, out=None, accumulate=False):
    dw_sn = _chk(dw_sn, "dw_sn")
    K = w_sn.shape[0]
    M = w_sn.numel() // K
    dw = out if out is not None else torch.empty_like(w_sn)
    need = _ws_query("rg_spectral_norm_bwd_workspace", K, M)
    ws = workspace(need, w_sn.device) if need else None
    lib.rg_spectral_norm_bwd(_p(dw_sn), _p(w_sn), _p(u), _p(v), _p(sigma), _p(dw), K, M, int(accumulate), _p(ws),
                             ws.numel() if ws is not None else 0, _stream())
    return dw
