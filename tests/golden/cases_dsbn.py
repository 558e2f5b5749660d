"""Seeded inputs and weights of the DSBN fixtures (shared by make_golden_dsbn.py, which runs the reference's dsbn.py on them, and
by the tests, which only have the recorded values).  State dicts are filled BY PARAMETER NAME (cases_ibn.fill), so `...BN_S.*` and
`...BN_T.*` receive different values; on top of that the T set of the layer cases is moved far from the S set."""
from __future__ import absolute_import

import torch
import torch.nn as nn

from oracle import ref_torch as O
from tests.golden.cases_ibn import fill, tensor  # noqa: F401

# (shape, dims): DSBN2d on [N, C, H, W], DSBN1d on [N, C]
LAYERS = [((4, 6, 5, 3), 2), ((6, 10), 1)]
LAYER_NAMES = ("y", "dx", "d_w_s", "d_b_s", "d_w_t", "d_b_t", "rm_s", "rv_s", "nbt_s", "rm_t", "rv_t", "nbt_t", "y_eval")

# stem conv + BN (+ ReLU, max-pool), one Bottleneck with a 1x1 downsample, average pooling, BatchNorm1d
TREE = dict(x=(8, 3, 16, 8), stem=8, width=4, feat=16)
TREE_GRAD_KEYS = ["base.0.weight", "base.1.BN_S.weight", "base.1.BN_T.bias", "base.4.0.conv2.weight", "base.4.0.bn2.BN_S.bias",
                  "base.4.0.bn3.BN_T.weight", "base.4.0.downsample.0.weight", "base.4.0.downsample.1.BN_S.weight", "feat_bn.BN_S.weight",
                  "feat_bn.BN_T.weight", "feat_bn.BN_T.bias"]
TREE_STATS = ["base.1.BN_S.running_mean", "base.1.BN_T.running_mean", "base.4.0.bn3.BN_S.running_var", "base.4.0.bn3.BN_T.running_var",
              "feat_bn.BN_S.running_mean", "feat_bn.BN_T.running_var", "base.4.0.bn1.BN_S.num_batches_tracked",
              "feat_bn.BN_T.num_batches_tracked"]


def layer_state(i, state_dict):
    """S set by cases_ibn.fill; T set moved apart: weight in -1.6..-1.4, bias around 2, running mean around 4, running variance in 8.5..9.5"""
    sd = fill(state_dict, "dsbn_layer%d" % i)
    sd["BN_T.weight"] = -(sd["BN_T.weight"] + 1.0)
    sd["BN_T.bias"] = sd["BN_T.bias"] + 2.0
    sd["BN_T.running_mean"] = sd["BN_T.running_mean"] + 4.0
    sd["BN_T.running_var"] = sd["BN_T.running_var"] + 7.7
    return sd


def layer_input(i):
    """source half around 0 with unit scale, target half around 4 with scale 3"""
    shape = LAYERS[i][0]
    x, dy = tensor("dsbn_layer_x%d" % i, shape), tensor("dsbn_layer_dy%d" % i, shape)
    h = shape[0] // 2
    x[h:] = 3.0 * x[h:] + 4.0
    return x, dy


class Tree(nn.Module):
    """the torch.nn tree the reference's convert_dsbn / convert_bn are applied to"""

    def __init__(self):
        super(Tree, self).__init__()
        s, w, f = TREE["stem"], TREE["width"], TREE["feat"]
        ds = nn.Sequential(nn.Conv2d(s, 4 * w, 1, 1, bias=False), nn.BatchNorm2d(4 * w))
        self.base = nn.Sequential(nn.Conv2d(3, s, 3, 1, 1, bias=False), nn.BatchNorm2d(s), nn.ReLU(inplace=True), nn.MaxPool2d(3, 2, 1),
                                  nn.Sequential(O.OBottleneck(s, w, 1, ds)))
        self.feat_bn = nn.BatchNorm1d(f)

    def forward(self, x):
        return self.feat_bn(self.base(x).mean((2, 3)))


def tree_input():
    x = O.synth_images(TREE["x"][0], TREE["x"][2], TREE["x"][3], seed=91)
    h = TREE["x"][0] // 2
    x[h:] = 0.5 * x[h:] + 0.7                    # the target domain: another contrast and brightness
    return x, tensor("dsbn_tree_dy", (TREE["x"][0], TREE["feat"]))
