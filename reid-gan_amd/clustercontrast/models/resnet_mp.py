"""Cluster-contrast multi-part ResNet — restates CC/clustercontrast/models/resnet_mp.py:16-205 on the HIP tape runtime.

`base = Sequential(conv1, bn1, relu, maxpool, layer1, layer2, layer3)` (:39-41); two branches on its output: `res_g`, the trunk's
layer4 with its stride 2 kept (:43), and `res_p`, three Bottlenecks at stride 1 loaded from layer4's state (:45-50).  The part map
`res_p(x)` is pooled over its upper and lower half of the rows (:111-114) by ONE launch of the part pooling kernel (csrc/pool.hip:
both halves of an NCHW plane are contiguous, so neither is sliced out); the global map goes through the pooling module; the three
BatchNorm1d layers, the fusion and the four row normalisations (:118-143) are the fused head of csrc/part_head.hip.  `feat_bn_gan`
(:121) only updates its running statistics in train mode: the reference discards its output.  `predictor`, `proj_gan` (and, outside
fusion='cat', `fc_id_*`) are constructed and never called, as in the reference: they exist so that checkpoints load strictly.

Train mode returns (f_g, f_p1, f_p2, f_gc); eval mode f_gc, or (f_gc, f_g) with clustering=True.
"""
from __future__ import absolute_import

from torch import nn
from torch.nn import init

from rg_hip import nn as rnn
from rg_hip import ops
from rg_hip.resnet_trunk import Bottleneck, TVResNet, _conv_bn_pairs, load_pretrained, trunk_tb, trunk_tf
from rg_hip.tape import RGModule

from .pooling import GeneralizedMeanPooling, build_pooling_layer

__all__ = ['ResNet_MP', 'resnet_mp50', 'resnet_mp101', 'resnet_mp152']


def _layer_tb(tape, layer, dy):
    """backward of a branch whose input is the ReLU output of `base`: every block applies the ReLU backward of the layer below in its
    conv1 data-gradient epilogue, the first one included, so both branches hand `base` an already masked gradient"""
    blocks = list(layer)
    for i in range(len(blocks) - 1, -1, -1):
        dy = blocks[i].tb(tape, dy, dy_masked=(i != len(blocks) - 1), mask_input=True)
    return dy


class ResNet_MP(RGModule):
    _depths = (50, 101, 152)            # 18 / 34: the reference's `res_p.load_state_dict(layer4.state_dict())` fails on BasicBlock keys

    def __init__(self, depth, pretrained=True, cut_at_pooling=False,
                 num_features=2048, norm=False, dropout=0, num_proj=256, pooling_type='avg',
                 need_predictor=False):
        super(ResNet_MP, self).__init__()
        self.pretrained = pretrained
        self.depth = depth
        self.cut_at_pooling = cut_at_pooling
        self.need_predictor = need_predictor
        if depth not in self._depths:
            raise KeyError("Unsupported depth:", depth)
        if not norm:
            raise ValueError("resnet_mp: norm=False is not usable: the reference's forward leaves f_g, f_p1, f_p2 and f_gc unassigned "
                             "without it (UnboundLocalError at resnet_mp.py:147-158); pass norm=True")
        resnet = TVResNet(depth)
        if pretrained:
            load_pretrained(resnet, depth)

        self.base = rnn.Sequential(resnet.conv1, resnet.bn1, resnet.relu, resnet.maxpool,
                                   resnet.layer1, resnet.layer2, resnet.layer3)
        self.res_g = resnet.layer4
        self.res_p = rnn.Sequential(
            Bottleneck(1024, 512, downsample=rnn.Sequential(rnn.Conv2d(1024, 2048, 1, bias=False), rnn.BatchNorm2d(2048))),
            Bottleneck(2048, 512),
            Bottleneck(2048, 512))
        self.res_p.load_state_dict(resnet.layer4.state_dict())

        self.gpool2d = build_pooling_layer(pooling_type)

        self.norm = norm
        self.dropout = dropout
        self.has_embedding = num_features > 0
        self.num_proj = num_proj
        self.num_features = resnet.fc.in_features       # 2048 whatever the argument says (:60-62)

        for name in ("feat_bn_g", "feat_bn_p1", "feat_bn_p2"):
            bn = rnn.BatchNorm1d(self.num_features)
            bn.bias.requires_grad_(False)
            setattr(self, name, bn)
        self.feat_bn_gan = rnn.BatchNorm2d(self.num_features)
        self.feat_bn_gan.bias.requires_grad_(False)

        if self.dropout > 0:
            self.drop = rnn.Dropout(self.dropout)

        if self.need_predictor:
            print("build predictor for cl loss")
            dim, mlp_dim = self.num_features, 2 * self.num_features
            self.predictor = rnn.Sequential(rnn.Linear(dim, mlp_dim, bias=False), rnn.BatchNorm1d(mlp_dim), rnn.ReLU(inplace=True),
                                            rnn.Linear(mlp_dim, dim, bias=False))

        self.fc_id_g = rnn.Linear(self.num_features, self.num_features // 2, bias=False)
        self.fc_id_p1 = rnn.Linear(self.num_features, self.num_features // 4, bias=False)
        self.fc_id_p2 = rnn.Linear(self.num_features, self.num_features // 4, bias=False)

        self.proj_gan = rnn.Conv2d(self.num_features, self.num_proj, 1, bias=False)
        init.kaiming_normal_(self.proj_gan.weight, mode='fan_out')

        if not pretrained:
            self.reset_params()

        for fc in (self.fc_id_g, self.fc_id_p1, self.fc_id_p2):
            init.kaiming_normal_(fc.weight, mode='fan_out')

    def forward(self, x, clustering=False, fusion='sum'):
        self._clustering = bool(clustering)
        self._fusion = fusion
        return super(ResNet_MP, self).forward(x)

    def _head_bns(self):
        return (self.feat_bn_g, self.feat_bn_p1, self.feat_bn_p2)

    # ---- tape program ---------------------------------------------------------------------------
    def tf(self, tape, x):
        clustering, fusion = getattr(self, "_clustering", False), getattr(self, "_fusion", 'sum')
        base = list(self.base)
        if not base[1].training and getattr(base[0], "_rg_fold_group", None) is None:
            # frozen statistics: ONE fold launch per weight version for the trunk and both branches (trunk_tf finds the group)
            base[0]._rg_fold_group = rnn.FoldGroup(_conv_bn_pairs(base + [self.res_g, self.res_p]))
        h = trunk_tf(tape, base, x)
        mark = len(tape.stack)
        x_g = self.res_g.tf(tape, h)
        n_g = len(tape.stack) - mark
        x_p = self.res_p.tf(tape, h)
        n_p = len(tape.stack) - mark - n_g
        N, C, Hp, Wp = x_p.shape
        split_row = Hp // 2
        if split_row < 1:
            raise ValueError("resnet_mp: the part map has %d row(s): its upper half is empty (input too small)" % Hp)
        pool = self.gpool2d
        gem = isinstance(pool, GeneralizedMeanPooling)
        p = pool._p_tensor(x_p.device) if gem else None
        eps = pool.eps if gem else 0.0
        y_p = ops.part_pool_fwd(x_p, split_row, p, eps)                    # [2, N, C]: both halves in one pass
        g = pool.tf(tape, x_g).reshape(N, C)
        train = self.training
        if train:
            gan = self.feat_bn_gan                                         # running statistics only: its output is discarded
            ops.bn_stats(x_p, gan.running_mean, gan.running_var, gan.eps, gan.momentum)
            for bn in (gan,) + self._head_bns():
                bn.count_batch()
        bns = self._head_bns()
        fus = 1 if fusion == 'sum' else 0
        out, xhat, _mean, invstd, norms = ops.mp_head_fwd(
            (g, y_p[0], y_p[1]), [bn.weight for bn in bns], [bn.bias for bn in bns], [bn.running_mean for bn in bns],
            [bn.running_var for bn in bns], [bn.eps for bn in bns], [bn.momentum for bn in bns], train, fus)
        f_g, f_p1, f_p2, f_gc = out[0], out[1], out[2], out[3]
        cat = None
        if fusion == 'cat':
            # not fused: the three fc_id layers read the BatchNorm outputs z_j = f_j |z_j| (the head keeps xhat, not z)
            zs = [ops.scale_rows(out[j], norms[j]) for j in range(3)]
            us = [fc.tf(tape, z) for fc, z in zip((self.fc_id_g, self.fc_id_p1, self.fc_id_p2), zs)]
            f_gc, cat_norm = ops.l2norm_rows_fwd(ops.cat_channels(us))
            cat = (f_gc, cat_norm, [u.shape[1] for u in us])
        dropped = train and self.dropout > 0
        if dropped:
            f_g = self.drop.tf(tape, f_g)
            f_gc = self.drop.tf(tape, f_gc)
        tape.push((x_p if gem else x_p.shape, p, y_p, split_row, eps, xhat, invstd, norms, train, fus, cat, dropped, n_g, n_p))
        if not train:
            return (f_gc, f_g) if clustering else f_gc
        return f_g, f_p1, f_p2, f_gc

    def tb(self, tape, *dys, **kw):
        need_dx = kw.get("need_dx", True)
        x_p, p, y_p, split_row, eps, xhat, invstd, norms, train, fus, cat, dropped, n_g, n_p = tape.pop()
        if train:
            d_g, d_p1, d_p2, d_gc = (tuple(dys) + (None,) * 4)[:4]
        else:
            d_gc = dys[0]
            d_g = dys[1] if len(dys) > 1 else None
            d_p1 = d_p2 = None
        if dropped:                                                         # pushed f_g then f_gc
            d_gc = self._drop_tb(tape, d_gc)
            d_g = self._drop_tb(tape, d_g)
        dzs = [None, None, None]
        fcs = (self.fc_id_g, self.fc_id_p1, self.fc_id_p2)
        if cat is not None:
            f_cat, cat_norm, widths = cat
            if d_gc is not None:
                d_u = ops.l2norm_rows_bwd(f_cat, d_gc, cat_norm)
                c1 = widths[0] + widths[1]
                parts = [ops.slice_channels(d_u, 0, widths[0]), ops.slice_channels(d_u, widths[0], c1),
                         ops.slice_channels(d_u, c1, c1 + widths[2])]
                for j in (2, 1, 0):
                    dzs[j] = fcs[j].tb(tape, parts[j])
            else:
                for _ in fcs:
                    tape.pop()
            d_gc = None
        bns = self._head_bns()
        if all(d is None for d in (d_g, d_p1, d_p2, d_gc)) and all(d is None for d in dzs):
            raise RuntimeError("resnet_mp: backward without a gradient for any output")
        want_gamma = any(tape.wants(bn.weight) for bn in bns)
        want_beta = any(tape.wants(bn.bias) for bn in bns)
        dx, dgamma, dbeta, reached = ops.mp_head_bwd((d_g, d_p1, d_p2, d_gc), xhat, invstd, norms, [bn.weight for bn in bns],
                                                     [bn.bias for bn in bns], train, fus, need_dgamma=want_gamma,
                                                     need_dbeta=want_beta, dzs=dzs)
        for j, bn in enumerate(bns):                   # a branch no gradient reaches leaves its parameters without one
            if reached[j] and tape.wants(bn.weight):
                tape.add_grad(bn.weight, dgamma[j])
            if reached[j] and tape.wants(bn.bias):
                tape.add_grad(bn.bias, dbeta[j])
        # the global branch: pooling module, then res_g
        pool = self.gpool2d
        d_h = None
        if reached[0]:
            N, C = dx.shape[1], dx.shape[2]
            d_xg = pool.tb(tape, dx[0].reshape(N, C, 1, 1))
        else:
            tape.pop()
            d_xg = None
        # the part branch: one launch writes the whole dx plane
        d_xp = None
        if reached[1] or reached[2]:
            if not (reached[1] and reached[2]):
                ops.fill_(dx[2 if reached[1] else 1], 0.0)
            gem = p is not None
            want_p = gem and isinstance(pool.p, nn.Parameter) and tape.wants(pool.p)
            d_xp, dp = ops.part_pool_bwd(x_p, split_row, dx[1:3], p, y_p if gem else None, eps, need_dp=want_p)
            if want_p:
                tape.add_grad(pool.p, dp)
        d_h = self._branch_tb(tape, self.res_p, d_xp, n_p)
        d_hg = self._branch_tb(tape, self.res_g, d_xg, n_g)
        if d_h is None:
            d_h = d_hg
        elif d_hg is not None:
            d_h = ops.add(d_hg, d_h)                   # the two gradients arriving at the output of `base`, added once
        if d_h is None:
            raise RuntimeError("resnet_mp: no gradient reaches the trunk")
        return trunk_tb(tape, list(self.base), d_h, need_dx, dy_masked=True)

    @staticmethod
    def _branch_tb(tape, layer, dy, n_records):
        if dy is not None:
            return _layer_tb(tape, layer, dy)
        # no gradient reaches this branch (e.g. f_g alone, or fusion 'g' without the part outputs): drop the records its forward
        # pushed; its parameters get no gradient
        for _ in range(n_records):
            tape.pop()
        return None

    def _drop_tb(self, tape, dy):
        if dy is not None:
            return self.drop.tb(tape, dy)
        tape.pop()
        return None

    def reset_params(self):
        for m in self.modules():
            if isinstance(m, rnn.Conv2d):
                init.kaiming_normal_(m.weight, mode='fan_out')
                if m.bias is not None:
                    init.constant_(m.bias, 0)
            elif isinstance(m, (rnn.BatchNorm2d, rnn.BatchNorm1d)):
                init.constant_(m.weight, 1)
                init.constant_(m.bias, 0)
            elif isinstance(m, rnn.Linear):
                init.normal_(m.weight, std=0.001)
                if m.bias is not None:
                    init.constant_(m.bias, 0)


def resnet_mp50(**kwargs):
    return ResNet_MP(50, **kwargs)


def resnet_mp101(**kwargs):
    return ResNet_MP(101, **kwargs)


def resnet_mp152(**kwargs):
    return ResNet_MP(152, **kwargs)
