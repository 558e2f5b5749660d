"""Cluster-contrast IBN-a ResNet — restates CC/clustercontrast/models/resnet_ibn.py:16-129 on the HIP tape runtime.

The trunk is rg_hip.resnet_trunk.IBNResNet (bn1 of every Bottleneck of layer1..3 is the fused IBN layer, rg_hip.nn.IBN);
the head — layer4 stride 1, `base = Sequential(conv1, bn1, relu, maxpool, layer1..4)`, pooling from the factory, `feat_bn` with
frozen bias, L2-normalised embedding in eval mode — is the one of `ResNet` in resnet.py.  Unlike that class the train-mode
forward returns `bn_x` alone (:91-102), not a tuple with the feature map.
"""
from __future__ import absolute_import

from torch.nn import init

from rg_hip import nn as rnn
from rg_hip.resnet_trunk import IBNResNet, load_pretrained_ibn

from .resnet import ResNet

__all__ = ['ResNetIBN', 'resnet_ibn50a', 'resnet_ibn101a']


class ResNetIBN(ResNet):
    _depths = ('50a', '101a')
    _returns_map = False

    def _build_trunk(self, depth, pretrained):
        if depth not in self._depths:
            raise KeyError("Unsupported depth:", depth)
        resnet = IBNResNet(depth)
        if pretrained:
            load_pretrained_ibn(resnet, depth)
        return resnet

    def forward(self, x):
        return super(ResNetIBN, self).forward(x)

    def reset_params(self):
        super(ResNetIBN, self).reset_params()
        for m in self.modules():                    # the trunk's constructor leaves them there (resnet_ibn_a.py:137-139)
            if isinstance(m, rnn.InstanceNorm2d) and m.affine:
                init.constant_(m.weight, 1)
                init.constant_(m.bias, 0)


def resnet_ibn50a(**kwargs):
    return ResNetIBN('50a', **kwargs)


def resnet_ibn101a(**kwargs):
    return ResNetIBN('101a', **kwargs)
