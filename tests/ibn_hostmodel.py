"""Plain-torch model of the IBN-a encoders — the comparison partner of the device tests (tests/test_ibn_cpu.py ties it to the
values recorded from the reference's own modules, tests/golden/reference_ibn.npz):

  IBN(planes): InstanceNorm2d(int(planes / 2), affine) on the first channels, BatchNorm2d on the rest, written as
  F.instance_norm / F.batch_norm on channel views and one concatenation;
  Bottleneck(ibn=True) / the trunks: oracle.ref_torch's OBottleneck / OTVResNet with `bn1` replaced in every block of
  layer1..layer3 (planes != 512); depths '50a' = [3, 4, 6, 3], '101a' = [3, 4, 23, 3];
  encoder: oracle.ref_torch's OCCResNet head on that trunk, whose train-mode forward returns bn_x alone.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle import ref_torch as O

DEPTHS = {"50a": 50, "101a": 101}


class HIBN(nn.Module):
    def __init__(self, planes):
        super(HIBN, self).__init__()
        self.half = int(planes / 2)
        self.IN = nn.InstanceNorm2d(self.half, affine=True)
        self.BN = nn.BatchNorm2d(planes - self.half)

    def forward(self, x):
        a = F.instance_norm(x[:, :self.half], weight=self.IN.weight, bias=self.IN.bias, eps=self.IN.eps)
        bn = self.BN
        if bn.training:
            bn.num_batches_tracked += 1
        b = F.batch_norm(x[:, self.half:], bn.running_mean, bn.running_var, bn.weight, bn.bias, bn.training, bn.momentum, bn.eps)
        return torch.cat((a, b), 1)


def bottleneck(cin, width, stride=1, downsample=None):
    blk = O.OBottleneck(cin, width, stride, downsample)
    blk.bn1 = HIBN(width)
    return blk


def _ibn_layers(layers):
    for layer in layers:
        for blk in layer:
            blk.bn1 = HIBN(blk.conv1.out_channels)


def trunk(depth):
    t = O.OTVResNet(DEPTHS[depth])
    _ibn_layers((t.layer1, t.layer2, t.layer3))
    return t


class HResNetIBN(O.OCCResNet):
    def __init__(self, depth, **kw):
        super(HResNetIBN, self).__init__(DEPTHS[depth], **kw)
        _ibn_layers((self.base[4], self.base[5], self.base[6]))

    def forward(self, x):
        out = super(HResNetIBN, self).forward(x)
        return out[0] if isinstance(out, tuple) else out
