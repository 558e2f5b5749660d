"""Convolution + BatchNorm as one layer.

With running statistics (FD-GAN's E and D_id: `set_bn_fix`, every eval-mode network) the normalisation is a per-channel
affine map of the conv output: it runs in the conv epilogue together with the residual add and the ReLU, and the
pre-normalisation tensor is never written or read again (see csrc/norm_fold.hip, "conv + frozen-statistics BatchNorm").
Train-mode BatchNorm keeps the separate statistics / apply passes.

Network programs call conv_bn_tf / conv_bn_tb as attributes of the rg_hip.nn package, looked up at call time (tests replace
them there); nothing in the package calls either."""
from __future__ import absolute_import

import torch

from .. import ops
from ..ops import ACT_NONE
from ..wcache import krsc_wanted, weight_key
from .conv import Conv2d
from .norm import _BatchNorm, _DSBN


class _Fold(object):
    __slots__ = ("key", "scale", "shift", "invstd", "w_scaled", "w_scaled_krsc")


def _fold_bn(bn):
    """the BatchNorm whose running statistics and affine parameters make the eval-mode map of `bn`: a DSBN layer in eval mode IS
    its BN_T (CC/clustercontrast/models/dsbn.py:14-15); every other module stands for itself"""
    return bn.BN_T if isinstance(bn, _DSBN) else bn


def _foldable(conv, bn):
    own = bn                                             # a DSBN layer's own mode decides; its BN_T supplies the map
    bn = _fold_bn(bn)
    return (isinstance(bn, _BatchNorm) and not own.training and not bn.training and bn.track_running_stats and bn.affine
            and conv.bias is None and isinstance(conv, Conv2d))


_FOLD_IN_CAPTURE = ("a network that folds BatchNorm into its convolutions cannot be captured: a replay would keep the filters "
                    "scaled at capture time after every later optimizer step")


def _fold_key(conv, bn):
    """weight_key of the five tensors a fold is made from (read from the modules' own dicts: nn.Module.__getattr__ per tensor would
    cost several times the key, and conv_bn_tf asks on every call)"""
    bn = _fold_bn(bn)
    p, b = bn._parameters, bn._buffers
    return weight_key(conv._parameters["weight"], p["weight"], p["bias"], b["running_mean"], b["running_var"])


def _fold_of(conv, bn):
    """Per-pair fold (one small launch group); networks fold all their pairs at once through FoldGroup."""
    if ops.CAPTURING[0]:
        raise RuntimeError(_FOLD_IN_CAPTURE)
    bn = _fold_bn(bn)
    key = _fold_key(conv, bn)
    f = getattr(conv, "_rg_fold", None)
    if f is None or f.key != key:
        f = _Fold()
        f.key = key
        f.scale, f.shift, f.invstd = ops.bn_fold(bn.weight.detach(), bn.bias.detach(), bn.running_mean, bn.running_var, bn.eps)
        ws = f.w_scaled = ops.scale_rows(conv.weight.detach(), f.scale)
        f.w_scaled_krsc = ops.weights_to_krsc(ws) if krsc_wanted(ws.shape) else None
        conv._rg_fold = f
    return f


class FoldGroup(object):
    """All (conv, BatchNorm) pairs of one network, folded by ONE kernel launch per weight version
    (`rg_fold_filters_multi`): scale / shift / invstd and the scaled filters of every pair live in two flat buffers."""

    def __init__(self, pairs):
        self.pairs = [(conv, _fold_bn(bn)) for conv, bn in pairs]
        self.keys = None                  # per pair: _fold_key its fold in `folds` was made for
        self.ptrs = None                  # per pair: the five input addresses `table` holds

    def _build(self, device):
        chunk = lib_fold_chunk()
        n_w = n_k = n_c = 0
        for conv, bn in self.pairs:
            w = conv.weight
            n_w += (w.numel() + 63) // 64 * 64
            if krsc_wanted(w.shape):
                n_k += (w.numel() + 63) // 64 * 64
            n_c += (w.shape[0] + 63) // 64 * 64
        self.buf_w = torch.empty(n_w + n_k, dtype=torch.float32, device=device)
        self.buf_c = torch.empty(3 * n_c, dtype=torch.float32, device=device)
        rows, ow, oc, blocks = [], 0, 0, 0
        self.folds = []
        for conv, bn in self.pairs:
            w = conv.weight
            K, C, RS = w.shape[0], w.shape[1], w.shape[2] * w.shape[3]
            f = _Fold()
            f.w_scaled = self.buf_w[ow:ow + w.numel()].view(w.shape)
            ow += (w.numel() + 63) // 64 * 64
            if krsc_wanted(w.shape):
                f.w_scaled_krsc = self.buf_w[ow:ow + w.numel()].view(K, RS, C)
                ow += (w.numel() + 63) // 64 * 64
            else:
                f.w_scaled_krsc = None
            kc = (K + 63) // 64 * 64
            f.scale, f.shift, f.invstd = (self.buf_c[oc:oc + K], self.buf_c[oc + kc:oc + kc + K],
                                          self.buf_c[oc + 2 * kc:oc + 2 * kc + K])
            oc += 3 * kc
            eps_bits = int(torch.tensor(bn.eps, dtype=torch.float32).view(torch.int32).item())
            rows.append([w.data_ptr(), bn.weight.data_ptr(), bn.bias.data_ptr(), bn.running_mean.data_ptr(),
                         bn.running_var.data_ptr(), f.w_scaled.data_ptr(),
                         f.w_scaled_krsc.data_ptr() if f.w_scaled_krsc is not None else 0, f.scale.data_ptr(),
                         f.shift.data_ptr(), f.invstd.data_ptr(), K, C, RS, eps_bits, blocks, 0])
            blocks += (w.numel() + chunk - 1) // chunk
            self.folds.append(f)
        self.table = torch.tensor(rows, dtype=torch.int64).to(device)
        self.blocks = blocks

    def usable(self):
        return all(_foldable(conv, bn) for conv, bn in self.pairs)

    def prepare(self):
        """Fold every pair if any weight changed or moved since the last call; afterwards conv._rg_fold is current."""
        if ops.CAPTURING[0]:
            raise RuntimeError(_FOLD_IN_CAPTURE)
        keys = [_fold_key(conv, bn) for conv, bn in self.pairs]
        if keys == self.keys:
            return
        ptrs = [[p for _, _, p in key] for key in keys]
        if ptrs != self.ptrs:
            self._build(self.pairs[0][0].weight.device)
            self.ptrs = ptrs
        ops.fold_filters_multi(self.table, len(self.pairs), self.blocks)
        self.keys = keys
        for (conv, _), f, key in zip(self.pairs, self.folds, keys):
            f.key = key
            conv._rg_fold = f


def invalidate_folds(net):
    """Forget every fold made for `net`.  A fold is keyed on the weights' arena epoch / version / address; the train-mode
    BatchNorm kernels write the running statistics behind torch's version counters, so an eval-mode pass that follows a
    train-mode pass of the SAME weight version (no optimizer step in between: the second encoder pass of the hard-mix step after
    an evaluation, say) would be served the fold of the older statistics.  Callers that alternate the two modes call this
    between them; the next eval-mode forward folds again (one launch per network)."""
    for m in net.modules():
        d = m.__dict__
        if "_rg_fold_group" in d:
            d["_rg_fold_group"].keys = None
        if "_rg_fold" in d:
            del d["_rg_fold"]


def lib_fold_chunk():
    return ops.lib.rg_fold_chunk()


def conv_bn_tf(tape, conv, bn, x, residual=None, act=ACT_NONE):
    """act(bn(conv(x)) [+ residual])"""
    if not _foldable(conv, bn):
        y = bn.tf(tape, conv.tf(tape, x), residual=residual, act=act)
        tape.push(None)
        return y
    f = _fold_of(conv, bn)               # a hit when the network's FoldGroup ran for this weight version
    y = ops.conv2d_fwd(x, f.w_scaled, conv.stride, conv.padding, shift=f.shift, residual=residual, act=act,
                       w_krsc=f.w_scaled_krsc)
    tape.push((x, y if act != ACT_NONE else None, f, act, residual is not None))
    return y


def conv_bn_tb(tape, conv, bn, dy, need_dx=True, residual=None, dy_masked=False, mask_input=False, want_rowsum=None):
    """-> dx, or (dx, d_residual) when the forward had a residual input; `residual` here is added to dx.
    dy_masked: dy already carries this layer's ReLU backward (the consumer's dgrad applied it, see mask_input);
    mask_input: apply the ReLU backward of the layer BELOW (whose output is this conv's input) to dx + residual."""
    rec = tape.pop()
    if rec is None:
        r = bn.tb(tape, dy, dy_masked=dy_masked)
        d, dres = r if isinstance(r, tuple) else (r, None)
        dx = conv.tb(tape, d, need_dx=need_dx, residual=residual, mask_input=mask_input)
        return (dx, dres) if isinstance(r, tuple) else dx
    if want_rowsum is None:
        want_rowsum = mask_input and tape.param_grad      # the layer below is a fold that will want the channel sums
    x, y, f, act, has_res = rec
    bn = _fold_bn(bn)
    want_w, want_g, want_b = tape.wants(conv.weight), tape.wants(bn.weight), tape.wants(bn.bias)
    need_sum = want_g or want_b
    ob = tape.grad_out(bn.bias) if want_b else None
    fused_sums = need_sum and (want_w or want_g)          # the wgrad finishing pass adds the slice partials up
    sg = part = None
    if act != ACT_NONE and not dy_masked:
        if fused_sums:
            g, part = ops.act_bwd_partial(dy, y, act, 0.0, need_g=True)
        else:
            g, sg = ops.act_bwd_sum(dy, y, act, 0.0, need_g=True, need_sum=need_sum, out_sum=ob)
    else:
        g = dy
        if fused_sums:
            part = getattr(dy, "_rg_rowsum", None) if dy_masked else None      # written by the dgrad epilogue that made dy
            if part is None:
                part = ops.act_bwd_partial(dy, None, ACT_NONE, need_g=False)[1]
        elif need_sum:
            sg = ops.act_bwd_sum(dy, None, ACT_NONE, need_g=False, need_sum=True, out_sum=ob)[1]
    dbeta = None
    dbeta_late = False
    if want_b:
        dbeta = sg if sg is not None else (ob if ob is not None else torch.empty(dy.shape[1], dtype=torch.float32, device=dy.device))
        # with fused sums dbeta is WRITTEN by finish() on the side stream: register it only after that launch is
        # enqueued, so an accumulating add_grad (second backward of the pair in one tape) reads finished values
        dbeta_late = part is not None and (want_w or want_g)
        if not dbeta_late:
            tape.add_grad(bn.bias, dbeta)
    if want_w or want_g:
        w = conv.weight.detach()
        og = tape.grad_out(bn.weight) if want_g else None
        dgamma = (og if og is not None else torch.empty_like(f.scale)) if want_g else None

        # G = wgrad(x, g) and the fold's finish (dgamma, dbeta, dW = scale G) in ONE call: with split-K the finish runs inside the
        # reduction launch (rg_conv2d_wgrad_fold)
        dw = ops.conv2d_wgrad(x, g, conv.weight.shape, conv.stride, conv.padding,
                              out=tape.grad_out(conv.weight) if want_w else None, side=True,
                              fold=(w, f.scale, f.invstd, bn.running_mean, sg, part, dbeta if part is not None else None, dgamma))
        if want_w:
            tape.add_grad(conv.weight, dw)
        if want_g:
            tape.add_grad(bn.weight, dgamma)
        if dbeta_late:
            tape.add_grad(bn.bias, dbeta)
    dx = None
    if need_dx:
        dx = ops.conv2d_dgrad(g, f.w_scaled, x.shape[2:], conv.stride, conv.padding, residual=residual,
                              w_krsc=f.w_scaled_krsc, relu_mask=x if mask_input else None, want_rowsum=want_rowsum)
    return (dx, g) if has_res else dx
