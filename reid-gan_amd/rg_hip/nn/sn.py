"""The convolution under spectral normalisation, and the batched power iteration of all such layers of a network."""
from __future__ import absolute_import

import torch
from torch import nn

from .. import lowp, ops
from ..ops import ACT_NONE
from ..tape import RGModule
from ..wcache import krsc_wanted
from ._base import _bias_grad, _conv_geom, _conv_init, _geom_gflop, _pair
from .conv import _f8_backward_operands


def sn_prepare(convs, training):
    """power iteration + W / sigma of every spectral-normed convolution a network forward is about to run, in two launches instead
    of two per layer; each SNConv2d.tf picks its result up (same u / v updates, same values as the per-layer launches)"""
    convs = [m for m in convs if isinstance(m, SNConv2d)]
    if not convs:
        return
    eps = convs[0].eps
    res = ops.spectral_norm_fwd_multi([(m.weight_orig.detach(), m.weight_u, m.weight_v) for m in convs], training, eps,
                                      save_uv=True)
    for m, r in zip(convs, res):
        m.__dict__["_sn_pre"] = r


class SNConv2d(RGModule):
    """nn.Conv2d under torch.nn.utils.spectral_norm (CC/dual_gan/models/base_function.py:121-126): parameters
    `weight_orig`, `bias`; buffers `weight_u`, `weight_v` (same names / shapes as the hook-based original, so its
    checkpoints load).  Every training-mode forward runs one power iteration in place on u, v and convolves with
    W / sigma (`rg_spectral_norm_fwd`); the backward maps the filter gradient through the division."""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, bias=True, eps=1e-12):
        super(SNConv2d, self).__init__()
        self.in_channels, self.out_channels = in_channels, out_channels
        self.kernel_size, self.stride, self.padding = _pair(kernel_size), _pair(stride), _pair(padding)
        self.eps = eps
        self.weight_orig = nn.Parameter(torch.empty(out_channels, in_channels, *self.kernel_size))
        self.bias = nn.Parameter(torch.empty(out_channels)) if bias else None
        _conv_init(self.weight_orig, self.bias)
        h, w = out_channels, self.weight_orig.numel() // out_channels
        self.register_buffer("weight_u", torch.nn.functional.normalize(torch.randn(h), dim=0, eps=eps))
        self.register_buffer("weight_v", torch.nn.functional.normalize(torch.randn(w), dim=0, eps=eps))
        self.weight = None          # W / sigma of the latest forward (plain tensor, as the hook leaves it)

    @classmethod
    def from_conv(cls, conv):
        m = cls(conv.in_channels, conv.out_channels, conv.kernel_size, conv.stride, conv.padding, conv.bias is not None)
        with torch.no_grad():
            m.weight_orig.copy_(conv.weight)
            if conv.bias is not None:
                m.bias.copy_(conv.bias)
        return m

    def tf(self, tape, x, act=ACT_NONE, slope=0.0, residual=None):
        keep_uv = tape.record and tape.wants(self.weight_orig)
        u = v = None
        pre = self.__dict__.pop("_sn_pre", None)      # (w_sn, sigma, u, v) from the network's batched launch (sn_prepare)
        if pre is not None:
            w_sn, sigma, u, v = pre
        elif keep_uv:
            w_sn, sigma, u, v = ops.spectral_norm_fwd(self.weight_orig.detach(), self.weight_u, self.weight_v, self.training,
                                                      self.eps, save_uv=True)
        else:
            w_sn, sigma = ops.spectral_norm_fwd(self.weight_orig.detach(), self.weight_u, self.weight_v, self.training, self.eps)
        self.weight = w_sn
        f8 = self.__dict__.get("_rg_f8")
        if f8 is not None:
            xq, xq_t = f8.quant_act_both(x, keep_uv)
            wq, wq_t = f8.weights(w_sn, None)                      # W / sigma changes with every power iteration
            geom = _conv_geom(self, x)
            y = lowp.conv_fwd(xq, wq, geom, shift=self.bias, residual=residual, act=act, slope=slope)
            tape.push((xq_t, y if act != ACT_NONE else None, act, slope, w_sn, (wq_t, geom), sigma, u, v))
            return y
        wk = ops.weights_to_krsc(w_sn) if krsc_wanted(w_sn.shape) else None
        y = ops.conv2d_fwd(x, w_sn, self.stride, self.padding, shift=self.bias, residual=residual, act=act, slope=slope,
                           w_krsc=wk)
        tape.push((x, y if act != ACT_NONE else None, act, slope, w_sn, wk, sigma, u, v))
        return y

    def tb(self, tape, dy, need_dx=True, residual=None):
        x, y, act, slope, w_sn, wk, sigma, u, v = tape.pop()
        f8 = self.__dict__.get("_rg_f8")
        if f8 is not None:
            wq_t, geom = wk
            want_w = tape.wants(self.weight_orig)
            dyq, dyq_t = _f8_backward_operands(tape, f8, self.bias, dy, y, act, slope, need_dx, want_w)
            if want_w:
                gout = tape.grad_dst(self.weight_orig)
                tape.add_grad(self.weight_orig, ops.side_call(
                    lambda: ops.spectral_norm_bwd(lowp.conv_wgrad(x, dyq_t, geom), w_sn, u, v, sigma, out=gout),
                    x, dyq_t, w_sn, u, v, sigma, gout, worth=ops.side_worth(_geom_gflop(geom, dy), fp8=True)))
            if not need_dx:
                return None
            return lowp.conv_dgrad(dyq, wq_t, geom, (geom[2], geom[3]), residual=residual)
        if act != ACT_NONE:
            dy = ops.act_bwd(dy, y, act, slope)
        if tape.wants(self.weight_orig):
            dw_sn = ops.conv2d_wgrad(x, dy, w_sn.shape, self.stride, self.padding)
            tape.add_grad(self.weight_orig, ops.spectral_norm_bwd(dw_sn, w_sn, u, v, sigma,
                                                                  out=tape.grad_dst(self.weight_orig)))
        if tape.wants(self.bias):
            _bias_grad(tape, self.bias, dy)
        if not need_dx:
            return None
        return ops.conv2d_dgrad(dy, w_sn, x.shape[2:], self.stride, self.padding, residual=residual, w_krsc=wk)
