"""BatchNorm, domain-specific BatchNorm, InstanceNorm and IBN, and the deferred `num_batches_tracked` counter they share
(_BatchNorm.count_batch; nbt_pending / nbt_add for the network programs that replay a layer without running its Python)."""
from __future__ import absolute_import

import torch
from torch import nn

from .. import ops
from ..ops import ACT_NONE
from ..tape import RGModule


class _BatchNorm(RGModule):
    def __init__(self, num_features, eps=1e-5, momentum=0.1, affine=True, track_running_stats=True):
        super(_BatchNorm, self).__init__()
        self.num_features, self.eps, self.momentum = num_features, eps, momentum
        self.affine, self.track_running_stats = affine, track_running_stats
        if affine:
            self.weight = nn.Parameter(torch.ones(num_features))
            self.bias = nn.Parameter(torch.zeros(num_features))
        else:
            self.register_parameter("weight", None)
            self.register_parameter("bias", None)
        if track_running_stats:
            self.register_buffer("running_mean", torch.zeros(num_features))
            self.register_buffer("running_var", torch.ones(num_features))
            self.register_buffer("num_batches_tracked", torch.tensor(0, dtype=torch.long))
        else:
            self.register_buffer("running_mean", None)
            self.register_buffer("running_var", None)
            self.register_buffer("num_batches_tracked", None)

    def extra_repr(self):
        return "%d, eps=%g, momentum=%g, affine=%s" % (self.num_features, self.eps, self.momentum, self.affine)

    def count_batch(self):
        """one train-mode batch went through this layer's statistics.  `num_batches_tracked` is a bookkeeping counter (int64
        buffer): counted on the host, written to the buffer when someone looks (attribute access, state_dict: _flush_nbt)
        instead of one tiny device launch per layer and step.  Every program that updates the running statistics of a
        _BatchNorm calls this, whichever kernel it uses."""
        d = self.__dict__
        d["_nbt_pending"] = d.get("_nbt_pending", 0) + 1

    def _flush_nbt(self):
        n = self.__dict__.get("_nbt_pending", 0)
        if n:
            self.__dict__["_nbt_pending"] = 0
            buf = self._buffers.get("num_batches_tracked")
            if buf is not None:
                buf += n

    def __getattr__(self, name):
        if name == "num_batches_tracked":
            self._flush_nbt()
        return super(_BatchNorm, self).__getattr__(name)

    def _save_to_state_dict(self, destination, prefix, keep_vars):
        self._flush_nbt()
        super(_BatchNorm, self)._save_to_state_dict(destination, prefix, keep_vars)

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        self.__dict__["_nbt_pending"] = 0          # the loaded counter replaces whatever was pending
        super(_BatchNorm, self)._load_from_state_dict(state_dict, prefix, *args, **kwargs)

    def tf(self, tape, x, residual=None, act=ACT_NONE, slope=0.0):
        batch_stats = self.training or not self.track_running_stats
        if batch_stats:
            rm = self.running_mean if self.track_running_stats else None
            rv = self.running_var if self.track_running_stats else None
            if self.track_running_stats:
                self.count_batch()
            if ops.bn_train_fused_ok(x):
                # small per-channel extent: statistics, running-statistics update and the normalisation in ONE launch
                y, mean, stat = ops.bn_train_fwd_fused(x, self.weight, self.bias, residual, rm, rv, self.eps, self.momentum, act,
                                                       slope)
                tape.push((x, y if act != ACT_NONE else None, mean, stat, False, True, act, slope, residual is not None))
                return y
            mean, stat = ops.bn_stats(x, rm, rv, self.eps, self.momentum)
            is_var = False
        else:
            mean, stat, is_var = self.running_mean, self.running_var, True
        y = ops.bn_apply_fwd(x, mean, stat, self.weight, self.bias, residual, is_var, self.eps, act, slope)
        tape.push((x, y if act != ACT_NONE else None, mean, stat, is_var, batch_stats, act, slope, residual is not None))
        return y

    def tb(self, tape, dy, need_dx=True, dy_masked=False):
        """dy_masked: dy already went through this layer's activation backward (the consumer's dgrad epilogue applied the
        ReLU mask, see Conv2d.tb(mask_input=True)), so the forward output is not read again."""
        x, y, mean, stat, is_var, train, act, slope, has_res = tape.pop()
        if dy_masked:
            act, y = ACT_NONE, None
        w, b = self.weight, self.bias
        need_affine = tape.wants(w) or tape.wants(b)
        if not train and is_var:
            # running statistics: dx does not depend on the channel sums -> one fused pass
            dx, dres, s1, s2 = ops.bn_eval_bwd(x, dy, y, mean, stat, w, self.eps, act, slope,
                                               need_dx=need_dx or not has_res, need_dres=has_res,
                                               need_sums=need_affine, out_sum_dy=tape.grad_dst(b), out_sum_dy_xhat=tape.grad_dst(w))
            tape.add_grads(((w, s2), (b, s1)))
            return (dx, dres) if has_res else dx
        s1 = s2 = None
        if train and not is_var and ops.bn_train_fused_ok(x):
            dx, dres, s1, s2 = ops.bn_train_bwd_fused(x, dy, y, mean, stat, w, act, slope,
                                                      need_dx=need_dx or not has_res, need_dres=has_res,
                                                      out_sum_dy=tape.grad_dst(b), out_sum_dy_xhat=tape.grad_dst(w))
            tape.add_grads(((w, s2), (b, s1)))
            return (dx, dres) if has_res else dx
        if need_affine or (train and need_dx):
            s1, s2 = ops.bn_bwd_reduce(x, dy, y, mean, stat, is_var, self.eps, act, slope, tape.grad_dst(b), tape.grad_dst(w))
            tape.add_grads(((w, s2), (b, s1)))
        dx, dres = ops.bn_bwd_apply(x, dy, y, mean, stat, w, s1, s2, train, is_var, self.eps, act, slope,
                                    need_dx=need_dx or not has_res, need_dres=has_res)
        return (dx, dres) if has_res else dx


class BatchNorm2d(_BatchNorm):
    pass


class BatchNorm1d(_BatchNorm):
    pass


def nbt_pending(bn):
    """batches `bn` has counted (count_batch) and not yet written to its `num_batches_tracked` buffer"""
    return bn.__dict__.get("_nbt_pending", 0)


def nbt_add(bn, delta):
    """count `delta` batches for `bn` at once: a replayed network program re-applies what its capture counted, an aborted
    capture takes back what it counted (negative delta)"""
    bn.__dict__["_nbt_pending"] = bn.__dict__.get("_nbt_pending", 0) + delta


class _DSBN(RGModule):
    """Domain-specific BatchNorm (CC/clustercontrast/models/dsbn.py:6-42): a train-mode batch is [source half | target half] and
    each half is normalised with its own batch statistics, affine parameters and running statistics; eval mode is `BN_T` on the
    whole batch.  The children `BN_S` / `BN_T` only hold the parameters and buffers (so the reference's keys `...BN_S.weight`,
    `...BN_T.running_mean` load unchanged); the train-mode arithmetic is `rg_dsbn_fwd` / `rg_dsbn_bwd` on the ONE tensor — no
    split copies, no concatenation.  `tf` / `tb` have `_BatchNorm`'s signatures."""
    _bn_cls = None

    def __init__(self, planes):
        super(_DSBN, self).__init__()
        self.num_features = planes
        self.BN_S = self._bn_cls(planes)
        self.BN_T = self._bn_cls(planes)

    def tf(self, tape, x, residual=None, act=ACT_NONE, slope=0.0):
        s, t = self.BN_S, self.BN_T
        if not self.training:
            y = t.tf(tape, x, residual=residual, act=act, slope=slope)
            tape.push(None)
            return y
        if x.shape[0] % 2:
            raise AssertionError("DSBN: a train-mode batch is [source half | target half]; got %d samples" % x.shape[0])
        s.count_batch()
        t.count_batch()
        y, stats = ops.dsbn_fwd(x, s.weight.detach(), s.bias.detach(), t.weight.detach(), t.bias.detach(),
                                (s.running_mean, s.running_var), (t.running_mean, t.running_var), (s.eps, t.eps),
                                (s.momentum, t.momentum), residual=residual, act=act, slope=slope)
        tape.push((x, y if act != ACT_NONE else None, stats, act, slope, residual is not None))
        return y

    def tb(self, tape, dy, need_dx=True, dy_masked=False):
        """dy_masked: the consumer's dgrad already applied this layer's ReLU mask (see _BatchNorm.tb): y is not read."""
        rec = tape.pop()
        if rec is None:
            return self.BN_T.tb(tape, dy, need_dx=need_dx, dy_masked=dy_masked)
        x, y, stats, act, slope, has_res = rec
        if dy_masked:
            act, y = ACT_NONE, None
        s, t = self.BN_S, self.BN_T
        params = (s.weight, s.bias, t.weight, t.bias)
        res = ops.dsbn_bwd(x, dy, y, stats, s.weight.detach(), t.weight.detach(), act, slope, need_dx=need_dx or not has_res,
                           need_dres=has_res, out=tuple(tape.grad_dst(p) for p in params))
        tape.add_grads(zip(params, res[2:]))
        return (res[0], res[1]) if has_res else res[0]


class DSBN2d(_DSBN):
    _bn_cls = BatchNorm2d


class DSBN1d(_DSBN):
    _bn_cls = BatchNorm1d


class InstanceNorm2d(RGModule):
    """One launch per direction (`rg_instnorm_fwd` / `rg_instnorm_bwd`): statistics, affine map, residual add and activation in the
    forward; activation gradient, both per-instance sums, dx and the residual gradient in the backward.  affine=False is the
    FD-GAN setting (FD/fdgan/networks.py:30); affine=True dual_gan's (CC/dual_gan/models/base_function.py:38-48)."""

    def __init__(self, num_features, eps=1e-5, affine=False):
        super(InstanceNorm2d, self).__init__()
        self.num_features, self.eps, self.affine = num_features, eps, affine
        if affine:
            self.weight = nn.Parameter(torch.ones(num_features))
            self.bias = nn.Parameter(torch.zeros(num_features))
        else:
            self.register_parameter("weight", None)
            self.register_parameter("bias", None)

    def tf(self, tape, x, residual=None, act=ACT_NONE, slope=0.0):
        g = self.weight.detach() if self.affine else None
        b = self.bias.detach() if self.affine else None
        y, mean, invstd = ops.instnorm_fwd(x, g, b, residual, self.eps, act, slope)
        tape.push((x, y if act != ACT_NONE else None, mean, invstd, g, act, slope, residual is not None))
        return y

    def tb(self, tape, dy, need_dx=True):
        x, y, mean, invstd, g, act, slope, has_res = tape.pop()
        N, C = x.shape[0], x.shape[1]
        dx, dres, s1, s2, s3 = ops.instnorm_bwd(x, dy, y, mean, invstd, g, act, slope, need_dx=True, need_dres=has_res)
        if self.affine and (tape.wants(self.weight) or tape.wants(self.bias)):
            dg, db = ops.rows_sum_pair(s2, s1, N, C, tape.grad_dst(self.weight), tape.grad_dst(self.bias))
            tape.add_grads(((self.weight, dg), (self.bias, db)))
        dx._rg_inst_sums = s3           # per-(n, c) sums of dx: the bias gradient of a convolution in front (see _bias_grad)
        return (dx, dres) if has_res else dx


class InstanceNorm1d(InstanceNorm2d):
    """[B, C, L] token maps (the PTM blocks, CC/dual_gan/models/PTM.py:176-181): the same kernels on a [B, C, L, 1] view."""

    def tf(self, tape, x, residual=None, act=ACT_NONE, slope=0.0):
        y = super(InstanceNorm1d, self).tf(tape, x.unsqueeze(-1), None if residual is None else residual.unsqueeze(-1),
                                           act, slope)
        return y.squeeze(-1)

    def tb(self, tape, dy, need_dx=True):
        out = super(InstanceNorm1d, self).tb(tape, dy.unsqueeze(-1), need_dx)
        if isinstance(out, tuple):
            return tuple(o.squeeze(-1) for o in out)
        return out.squeeze(-1)


class IBN(RGModule):
    """The IBN layer of the IBN-a ResNets (CC/clustercontrast/models/resnet_ibn_a.py:54-68): InstanceNorm2d(half, affine) on the
    first `half` channels, BatchNorm2d on the rest.  The children `IN` / `BN` only hold the parameters and running statistics
    (so the reference's state_dict keys load unchanged); the arithmetic is `rg_ibn_fwd` / `rg_ibn_bwd` on the whole tensor —
    no slice copies, no concatenation."""

    def __init__(self, planes):
        super(IBN, self).__init__()
        half1 = int(planes / 2)
        self.half = half1
        self.IN = InstanceNorm2d(half1, affine=True)
        self.BN = BatchNorm2d(planes - half1)

    def tf(self, tape, x, residual=None, act=ACT_NONE, slope=0.0):
        bn = self.BN
        train = bn.training
        if train:
            bn.count_batch()
        y, in_mean, in_invstd, bn_mean, bn_invstd = ops.ibn_fwd(
            x, self.half, self.IN.weight.detach(), self.IN.bias.detach(), bn.weight.detach(), bn.bias.detach(), bn.running_mean,
            bn.running_var, train, self.IN.eps, bn.eps, bn.momentum, residual=residual, act=act)
        if not train:
            bn_mean, bn_invstd = bn.running_mean, bn.running_var
        tape.push((x, y if act != ACT_NONE else None, in_mean, in_invstd, bn_mean, bn_invstd, train, act))
        return y

    def tb(self, tape, dy, need_dx=True, dy_masked=False):
        """dy_masked: the consumer's dgrad already applied this layer's ReLU mask (see _BatchNorm.tb): y is not read."""
        x, y, in_mean, in_invstd, bn_mean, bn_stat, train, act = tape.pop()
        if dy_masked:
            act, y = ACT_NONE, None
        params = (self.IN.weight, self.IN.bias, self.BN.weight, self.BN.bias)
        res = ops.ibn_bwd(x, dy, y, self.half, in_mean, in_invstd, bn_mean, bn_stat, self.IN.weight.detach(),
                          self.BN.weight.detach(), train, self.BN.eps, act, out=tuple(tape.grad_dst(p) for p in params))
        tape.add_grads(zip(params, res[1:]))
        return res[0]
