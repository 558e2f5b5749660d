"""Seeded inputs and weights of the IBN fixtures (shared by make_golden_ibn.py, which runs the reference on them, and by the
tests, which only have the recorded values).  A state_dict is filled BY PARAMETER NAME: every tensor comes from its own
torch.Generator seeded from the key string, so the order in which a model lists its tensors cannot matter and the 23.5 M weights
of an encoder are regenerated instead of stored.  Recipe of cases.trunk_case: conv filters normal with the fan-out standard
deviation, norm weights uniform 0.4-0.6, biases and running means normal 0.1, running variances uniform 0.8-1.2."""
from __future__ import absolute_import

import zlib

import torch

from oracle import ref_torch as O

# (N, planes, H, W).  Even planes only: the reference's IBN.forward splits with torch.split(x, half, 1) and hands chunk 1 (half
# channels) to BatchNorm2d(planes - half), which raises for odd planes ("running_mean should contain 4 elements not 3") — there is
# no reference value to record; the device tests cover odd planes against the layer's definition in fp64.
LAYER_SHAPES = [(3, 6, 6, 5), (2, 8, 8, 4)]
BLOCK = dict(cin=24, width=8, x=(2, 24, 8, 4))         # Bottleneck(ibn=True) with a 1x1 downsample (24 != 4 * 8)
MODEL = dict(depth="50a", kw=dict(norm=True, pooling_type="gem"), x=(4, 3, 64, 32))
GRAD_KEYS = ["base.0.weight", "base.4.0.bn1.IN.weight", "base.4.0.bn1.IN.bias", "base.4.0.bn1.BN.weight", "base.4.2.conv2.weight",
             "base.5.1.bn1.BN.bias", "base.5.3.conv1.weight", "base.6.0.downsample.0.weight", "base.6.5.bn1.IN.weight",
             "base.7.2.conv3.weight", "base.7.2.bn3.weight", "gap.p", "feat_bn.weight"]
STATS_LAYER = "base.5.2.bn1.BN."                        # the IBN layer whose running statistics are recorded


def _gen(key):
    return torch.Generator().manual_seed(zlib.crc32(key.encode()))


def tensor(key, shape, kind="normal", a=0.0, b=1.0):
    g = _gen(key)
    if kind == "uniform":
        return torch.rand(shape, generator=g) * (b - a) + a
    return torch.randn(shape, generator=g) * b + a


def fill(state_dict, tag):
    """a new state_dict with the keys and shapes of `state_dict`, every value drawn from Generator(crc32(tag + key))"""
    out = {}
    for k, v in state_dict.items():
        key, shape = tag + ":" + k, tuple(v.shape)
        if k.endswith("num_batches_tracked"):
            out[k] = torch.zeros_like(v)
        elif k.endswith("running_mean"):
            out[k] = tensor(key, shape, "normal", 0.0, 0.1)
        elif k.endswith("running_var"):
            out[k] = tensor(key, shape, "uniform", 0.8, 1.2)
        elif v.dim() == 4:
            out[k] = tensor(key, shape, "normal", 0.0, (2.0 / (shape[0] * shape[2] * shape[3])) ** 0.5)
        elif v.dim() == 2:
            out[k] = tensor(key, shape, "normal", 0.0, 0.01)
        elif k.endswith(".weight"):
            out[k] = tensor(key, shape, "uniform", 0.4, 0.6)
        elif k.endswith(".bias"):
            out[k] = tensor(key, shape, "normal", 0.0, 0.1)
        else:
            out[k] = v.detach().clone()                # the GeM exponent keeps its initial value
    return out


def layer_input(i):
    shape = LAYER_SHAPES[i]
    return tensor("ibn_layer_x%d" % i, shape, "normal", 0.3, 1.7), tensor("ibn_layer_dy%d" % i, shape)


def block_input():
    return tensor("ibn_block_x", BLOCK["x"], "normal", 0.0, 1.0), tensor("ibn_block_dy", (2, 4 * BLOCK["width"], 8, 4))


def model_input(n=4):
    return O.synth_images(n, MODEL["x"][2], MODEL["x"][3], seed=71), tensor("ibn_model_dy", (n, 2048))
