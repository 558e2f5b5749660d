"""The small layers: activations, Dropout, pooling, reflection padding, Sequential."""
from __future__ import absolute_import

import torch

from .. import ops
from ..ops import ACT_NONE, ACT_RELU, ACT_LEAKY, ACT_TANH
from ..tape import RGModule
from ._base import _pair


class _Act(RGModule):
    ACT, SLOPE = ACT_NONE, 0.0

    def __init__(self, *args, **kw):
        super(_Act, self).__init__()

    def tf(self, tape, x):
        y = ops.act_fwd(x, self.ACT, self.SLOPE)
        tape.push(y)
        return y

    def tb(self, tape, dy, need_dx=True):
        y = tape.pop()
        return ops.act_bwd(dy, y, self.ACT, self.SLOPE) if need_dx else None


class ReLU(_Act):
    ACT = ACT_RELU

    def __init__(self, inplace=False):
        super(ReLU, self).__init__()
        self.inplace = inplace


class LeakyReLU(_Act):
    ACT = ACT_LEAKY

    def __init__(self, negative_slope=0.01, inplace=False):
        super(LeakyReLU, self).__init__()
        self.negative_slope = negative_slope
        self.SLOPE = negative_slope
        self.inplace = inplace


class Tanh(_Act):
    ACT = ACT_TANH


class Dropout(RGModule):
    """Inverted dropout with a counter-based mask (seed drawn from torch's CPU generator per call, so
    torch.manual_seed makes runs reproducible); identity in eval mode or for p == 0."""

    def __init__(self, p=0.5, inplace=False):
        super(Dropout, self).__init__()
        self.p = float(p)

    def tf(self, tape, x):
        if not self.training or self.p == 0.0:
            tape.push(None)
            return x
        seed = int(torch.randint(0, 2 ** 62, (1,)).item())
        tape.push(seed)
        return ops.dropout(x, self.p, seed)

    def tb(self, tape, dy, need_dx=True):
        seed = tape.pop()
        if seed is None or not need_dx:
            return dy if need_dx else None
        return ops.dropout(dy, self.p, seed)


class MaxPool2d(RGModule):
    def __init__(self, kernel_size, stride=None, padding=0):
        super(MaxPool2d, self).__init__()
        self.kernel_size, self.padding = kernel_size, padding
        self.stride = stride if stride is not None else kernel_size

    def tf(self, tape, x):
        y, arg = ops.maxpool2d_fwd(x, self.kernel_size, self.stride, self.padding)
        tape.push((arg, x.shape))
        return y

    def tb(self, tape, dy, need_dx=True):
        arg, shape = tape.pop()
        return ops.maxpool2d_bwd(dy, arg, shape, self.kernel_size, self.stride, self.padding) if need_dx else None


class AvgPool2d(RGModule):
    """nn.AvgPool2d(kernel_size=k, stride=k) (the only form the dual_gan blocks use)."""

    def __init__(self, kernel_size, stride=None, padding=0):
        super(AvgPool2d, self).__init__()
        stride = kernel_size if stride is None else stride
        if _pair(kernel_size) != _pair(stride) or _pair(kernel_size)[0] != _pair(kernel_size)[1] or _pair(padding) != (0, 0):
            raise NotImplementedError("AvgPool2d: only square kernel == stride, padding 0")
        self.kernel_size = _pair(kernel_size)[0]

    def tf(self, tape, x):
        tape.push(x.shape)
        return ops.avgpool2d_fwd(x, self.kernel_size)

    def tb(self, tape, dy, need_dx=True):
        shape = tape.pop()
        return ops.avgpool2d_bwd(dy, shape, self.kernel_size) if need_dx else None


class ReflectionPad2d(RGModule):
    def __init__(self, padding):
        super(ReflectionPad2d, self).__init__()
        self.padding = int(padding)

    def tf(self, tape, x):
        return ops.reflection_pad2d_fwd(x, self.padding)

    def tb(self, tape, dy, need_dx=True):
        return ops.reflection_pad2d_bwd(dy, self.padding) if need_dx else None


class Sequential(RGModule):
    def __init__(self, *mods):
        super(Sequential, self).__init__()
        for i, m in enumerate(mods):
            self.add_module(str(i), m)

    def __getitem__(self, i):
        return list(self._modules.values())[i]

    def __len__(self):
        return len(self._modules)

    def __iter__(self):
        return iter(self._modules.values())

    def tf(self, tape, x):
        for m in self._modules.values():
            x = m.tf(tape, x)
        return x

    def tb(self, tape, dy, need_dx=True):
        mods = list(self._modules.values())
        for i in range(len(mods) - 1, -1, -1):
            dy = mods[i].tb(tape, dy, need_dx=(need_dx or i > 0))
        return dy
