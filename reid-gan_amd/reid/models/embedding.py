"""EltwiseSubEmbed — restates FD-GAN-master/reid/models/embedding.py:7-39: (x1-x2)^2|abs -> BN1d -> Linear."""
from __future__ import absolute_import

import torch

from rg_hip import nn as rnn
from rg_hip import ops
from rg_hip.tape import RGModule


class EltwiseSubEmbed(RGModule):
    def __init__(self, nonlinearity='square', use_batch_norm=False,
                 use_classifier=False, num_features=0, num_classes=0):
        super(EltwiseSubEmbed, self).__init__()
        self.nonlinearity = nonlinearity
        if nonlinearity is not None and nonlinearity not in ['square', 'abs']:
            raise KeyError("Unknown nonlinearity:", nonlinearity)
        if nonlinearity != 'square':
            raise NotImplementedError("rg_hip EltwiseSubEmbed: only nonlinearity='square' (the FD-GAN setting, "
                                      "FD/fdgan/model.py:43,47) has a HIP kernel")
        self.use_batch_norm = use_batch_norm
        self.use_classifier = use_classifier
        if self.use_batch_norm:
            self.bn = rnn.BatchNorm1d(num_features)
            self.bn.weight.data.fill_(1)
            self.bn.bias.data.zero_()
        if self.use_classifier:
            assert num_features > 0 and num_classes > 0
            self.classifier = rnn.Linear(num_features, num_classes)
            self.classifier.weight.data.normal_(0, 0.001)
            self.classifier.bias.data.zero_()

    def tf(self, tape, x1, x2):
        x1 = x1.reshape(x1.size(0), -1)
        x2 = x2.reshape(x2.size(0), -1)
        tape.push((x1, x2))
        x = ops.sub_square_fwd(x1, x2)
        if self.use_batch_norm:
            x = self.bn.tf(tape, x)
        if self.use_classifier:
            x = self.classifier.tf(tape, x)
        else:
            tape.push(x.shape)
            ones = ops.fill_(torch.empty(x.shape[1], 1, dtype=torch.float32, device=x.device), 1.0)
            x = ops.linear_fwd(x, ones.view(1, -1)).view(-1)      # x.sum(1)
        return x

    # ---- the stage-I program: embedding, nn.CrossEntropyLoss() and top-1 precision on csrc/verif_head.hip -------------------------
    @property
    def has_fused_loss(self):
        """BatchNorm and classifier with at most 16 classes: what `tf_loss` / `tb_loss` fuse"""
        return bool(self.use_batch_norm and self.use_classifier and self.classifier.out_features <= 16)

    def tf_loss(self, tape, x1, x2, targets):
        """-> (logits [B, C], loss, prec): `self(x1, x2)`, the mean cross entropy against `targets` and the fraction of rows
        whose argmax (lowest index on a tie) is the target, the last two as 0-d device tensors.  `bn`'s buffers end as `self.bn.tf`
        leaves them (train mode: running statistics updated, one batch counted)."""
        if not self.has_fused_loss:
            raise RuntimeError("EltwiseSubEmbed.tf_loss needs use_batch_norm, use_classifier and at most 16 classes")
        x1 = x1.reshape(x1.size(0), -1)
        x2 = x2.reshape(x2.size(0), -1)
        bn, fc = self.bn, self.classifier
        train = bn.training
        if train:
            bn.count_batch()
        logits, xhat, _, invstd, _, out2, dlogits = ops.verif_head_fwd(
            x1, x2, bn.weight.detach(), bn.bias.detach(), bn.running_mean, bn.running_var, fc.weight.detach(),
            None if fc.bias is None else fc.bias.detach(), targets, train, bn.eps, bn.momentum)
        tape.push((x1, x2, xhat, invstd, dlogits, train))
        return logits, out2[0], out2[1]

    def tb_loss(self, tape, dlogits_up, dloss, need_dx=True):
        """dlogits_up: gradient arriving at the logits themselves, dloss: at the loss (0-d device tensor); either may be None.
        -> (dx1, dx2), (None, None) when neither is given or need_dx is False"""
        x1, x2, xhat, invstd, dlogits, train = tape.pop()
        if dloss is None and dlogits_up is None:
            return None, None
        bn, fc = self.bn, self.classifier
        params = (fc.weight, fc.bias, bn.weight, bn.bias)
        need = [tape.wants(p) for p in params]
        dx1, dx2, dw, db, dga, dbe = ops.verif_head_bwd(
            None if dloss is None else dloss.reshape(1), None if dloss is None else dlogits, dlogits_up, x1, x2, xhat, invstd,
            bn.weight.detach(), bn.bias.detach(), fc.weight.detach(), train, need_dx=(need_dx, need_dx), need_dweight=need[0],
            need_dbias=need[1], need_dgamma=need[2], need_dbeta=need[3], out=tuple(tape.grad_dst(p) for p in params))
        tape.add_grads(zip(params, (dw, db, dga, dbe)))
        return dx1, dx2

    def tb(self, tape, dy, need_dx=True):
        if self.use_classifier:
            d = self.classifier.tb(tape, dy)
        else:
            shape = tape.pop()
            ones = ops.fill_(torch.empty(1, shape[1], dtype=torch.float32, device=dy.device), 1.0)
            d = ops.linear_dgrad(dy.reshape(-1, 1), ones)
        if self.use_batch_norm:
            d = self.bn.tb(tape, d)
        x1, x2 = tape.pop()
        return ops.sub_square_bwd(x1, x2, d)
