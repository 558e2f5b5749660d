"""What the layer modules share: size helpers, the torch-identical convolution initialisation, the bias gradient."""
from __future__ import absolute_import

import math

from torch.nn import init

from .. import ops


def _pair(v):
    return (v, v) if isinstance(v, int) else (int(v[0]), int(v[1]))


def _conv_init(weight, bias):
    """torch.nn.Conv2d.reset_parameters / ConvTranspose2d's (fan_in from dim 1 of either layout), same draws in the same order"""
    init.kaiming_uniform_(weight, a=math.sqrt(5))
    if bias is not None:
        fan_in, _ = init._calculate_fan_in_and_fan_out(weight)
        bound = 1 / math.sqrt(fan_in) if fan_in > 0 else 0
        init.uniform_(bias, -bound, bound)


def _conv_geom(m, x):
    """(N, C, H, W, K, KH, KW, stride h, w, padding h, w) of the convolution `m` applied to x; K from the filters m.weight"""
    return (x.shape[0], x.shape[1], x.shape[2], x.shape[3], m.weight.shape[0], m.kernel_size[0], m.kernel_size[1],
            m.stride[0], m.stride[1], m.padding[0], m.padding[1])


def _geom_gflop(geom, dy):
    """algorithmic GFLOP of one conv pass with geometry (N, C, H, W, K, KH, KW, ...) and output gradient dy"""
    return 2e-9 * dy.numel() * geom[1] * geom[5] * geom[6]


def _bias_grad(tape, bias, dy):
    """sum of dy over N and the pixels.  When dy is the tensor an InstanceNorm backward just produced, that kernel already
    summed it per (n, c): one tiny launch over [N][C] instead of another pass over the activation."""
    part = getattr(dy, "_rg_inst_sums", None)
    N, C = dy.shape[0], dy.shape[1]
    if part is not None and part.numel() == N * C:
        db, _ = ops.rows_sum_pair(part, None, N, C, tape.grad_dst(bias), None)
    else:
        db = ops.channel_sum(dy, out=tape.grad_dst(bias))
    tape.add_grad(bias, db)
