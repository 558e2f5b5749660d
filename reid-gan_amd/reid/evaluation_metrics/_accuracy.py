"""`accuracy` of FD/reid/evaluation_metrics/classification.py:6-19, restated for a tree with no reference behind it: the fraction
of rows whose top-k predictions hold the target, one 1-element tensor per k."""
from __future__ import absolute_import

import torch


def accuracy(output, target, topk=(1,)):
    output, target = torch.as_tensor(output), torch.as_tensor(target)
    pred = output.topk(max(topk), 1, True, True)[1]
    hit = pred.eq(target.reshape(-1, 1))
    return [hit[:, :k].float().sum().reshape(1) * (1.0 / target.size(0)) for k in topk]
