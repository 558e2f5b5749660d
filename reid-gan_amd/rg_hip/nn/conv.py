"""Conv2d / ConvTranspose2d / Linear with their fp8 branch (rg_hip.lowp), and the (r,s)-major filter cache of the plain
convolutions: per layer (_KrscCache) or one launch per network and optimizer step (KrscGroup, group_krsc)."""
from __future__ import absolute_import

import math

import torch
from torch import nn
from torch.nn import init

from .. import lowp, ops
from ..ops import ACT_NONE
from ..tape import RGModule
from ..wcache import GroupStamp, Stamp, krsc_wanted, weight_key
from ._base import _bias_grad, _conv_geom, _conv_init, _geom_gflop, _pair


def _f8_backward_operands(tape, f8, bias, dy, y, act, slope, need_dx, want_w):
    """fp8 backward head shared by the convolution classes: activation backward, e5m2 quantisation in both layouts and the bias
    gradient from ONE pass over dy (lowp.F8Layer.quant_grad_fused).  An InstanceNorm backward that produced dy has already summed
    it per (n, c): that shortcut (see _bias_grad) is kept when there is no activation in between."""
    want_b = tape.wants(bias)
    inst = getattr(dy, "_rg_inst_sums", None) if act == ACT_NONE else None
    use_inst = want_b and inst is not None and inst.numel() == dy.shape[0] * dy.shape[1]
    dyq, dyq_t, part = f8.quant_grad_fused(dy, y, act, slope, need_dx, want_w, want_b and not use_inst)
    if want_b:
        if use_inst:
            db, _ = ops.rows_sum_pair(inst, None, dy.shape[0], dy.shape[1], tape.grad_dst(bias), None)
        else:
            db, _ = ops.rows_sum_pair(part, None, part.shape[0], part.shape[1], tape.grad_dst(bias), None)
        tape.add_grad(bias, db)
    return dyq, dyq_t


class _KrscCache(object):
    """[K][KH*KW][C] copy of a filter tensor for the (r,s)-major kernels, rebuilt only when the weights changed (wcache.Stamp).
    Convolutions of one network share a KrscGroup (group_krsc): the first stale member re-lays ALL of them out in one launch."""

    def _krsc(self):
        w = self.weight
        if not krsc_wanted(w.shape):
            return None
        d = self.__dict__
        grp = d.get("_krsc_group")
        if grp is not None:
            return grp.get(self)
        stamp = d.get("_wk_stamp")
        if stamp is None:
            stamp = d["_wk_stamp"] = Stamp()
        key = weight_key(w)
        if stamp.stale(key):
            self._wk = ops.weights_to_krsc(w.detach())
            stamp.set(key)
        return self._wk


class KrscGroup(object):
    """The (r,s)-major filter copies of every plain convolution of one network, refreshed together by ONE launch
    (`rg_weights_to_krsc_multi`) when the first member finds its copy stale — after an optimizer step every member is
    (wcache.GroupStamp).  The copies are persistent buffers; the device table is rebuilt when a parameter moved (load_state_dict,
    .to())."""

    def __init__(self, candidates):
        self.members = []                 # the candidates that actually asked for their copy (folded convolutions never do)
        self.stamps = []                  # their `_wk_stamp`
        self.stamp = GroupStamp()
        self.ptrs = None
        self.table = None
        self.blocks = 0
        for m in candidates:
            m.__dict__["_krsc_group"] = self

    def _build(self):
        chunk = ops.lib.rg_krsc_chunk()
        rows, first = [], 0
        for m in self.members:
            w = m.weight
            K, C, RS = w.shape[0], w.shape[1], w.shape[2] * w.shape[3]
            wk = m.__dict__.get("_wk")
            if wk is None or tuple(wk.shape) != (K, RS, C) or wk.device != w.device:
                wk = m._wk = torch.empty((K, RS, C), dtype=torch.float32, device=w.device)
            rows.append([w.data_ptr(), wk.data_ptr(), K, C, RS, first])
            first += (K * C * RS + chunk - 1) // chunk
        dev = self.members[0].weight.device
        self.table = torch.tensor(rows, dtype=torch.int64).to(dev)
        self.blocks = first
        self.ptrs = tuple(m.weight.data_ptr() for m in self.members)

    def refresh(self):
        if self.ptrs != tuple(m.weight.data_ptr() for m in self.members):
            if ops.CAPTURING[0]:
                raise RuntimeError("KrscGroup: a parameter moved while a network program is being captured")
            self._build()
        ops.lib.rg_weights_to_krsc_multi(ops._p(self.table), len(self.members), self.blocks, ops._stream())
        self.stamp.set(self.stamps, [weight_key(m.weight) for m in self.members])

    def get(self, m):
        d = m.__dict__
        if not d.get("_krsc_member"):
            if ops.CAPTURING[0]:
                raise RuntimeError("KrscGroup: a convolution asked for its (r,s)-major filters for the first time inside a capture")
            d["_krsc_member"] = True
            d["_wk_stamp"] = Stamp()      # stale: the refresh below rebuilds the table with the new member in it
            self.members.append(m)
            self.stamps.append(d["_wk_stamp"])
            self.ptrs = None
        if self.stamp.stale(d["_wk_stamp"], weight_key(m.weight)):
            self.refresh()
        return m._wk


def group_krsc(net):
    """give the plain convolutions of `net` one shared KrscGroup (idempotent; called on a network's first run)"""
    if net.__dict__.get("_krsc_grouped"):
        return
    net.__dict__["_krsc_grouped"] = True
    root = net if isinstance(net, nn.Module) else getattr(net, "net", None)     # tape programs over another module's layers
    if not isinstance(root, nn.Module):
        return
    members = [m for m in root.modules() if isinstance(m, _KrscCache) and isinstance(getattr(m, "weight", None), torch.Tensor)
               and m.weight.is_cuda and krsc_wanted(m.weight.shape) and "_krsc_group" not in m.__dict__]
    if len(members) >= 2:
        KrscGroup(members)


class Conv2d(RGModule, _KrscCache):
    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, bias=True):
        super(Conv2d, self).__init__()
        self.in_channels, self.out_channels = in_channels, out_channels
        self.kernel_size, self.stride, self.padding = _pair(kernel_size), _pair(stride), _pair(padding)
        self.weight = nn.Parameter(torch.empty(out_channels, in_channels, *self.kernel_size))
        self.bias = nn.Parameter(torch.empty(out_channels)) if bias else None
        self.reset_parameters()

    def reset_parameters(self):          # identical to torch.nn.Conv2d.reset_parameters
        _conv_init(self.weight, self.bias)

    def extra_repr(self):
        return "%d, %d, kernel_size=%s, stride=%s, padding=%s, bias=%s" % (
            self.in_channels, self.out_channels, self.kernel_size, self.stride, self.padding, self.bias is not None)

    def tf(self, tape, x, act=ACT_NONE, slope=0.0, residual=None):
        """y = act(conv(x) + bias + residual): bias, residual add and activation run in the MFMA epilogue."""
        f8 = self.__dict__.get("_rg_f8")
        if f8 is not None:
            # fp8 MFMA family (rg_hip.lowp): e4m3 operands, fp32 accumulate, same fused epilogue
            want_w = tape.record and tape.wants(self.weight)
            xq, xq_t = f8.quant_act_both(x, want_w)
            wq, _ = f8.weights(self.weight.detach(), weight_key(self.weight))
            geom = _conv_geom(self, x)
            y = lowp.conv_fwd(xq, wq, geom, shift=self.bias, residual=residual, act=act, slope=slope)
            tape.push((xq_t, y if act != ACT_NONE else None, act, slope, geom))
            return y
        if self._full_extent(x):
            # the filter covers the whole (unpadded) map — the generator's 512 -> 128 (8,4) bottleneck,
            # FD/fdgan/networks.py:96-100: a plain GEMM x[N][C*H*W] . w[K][C*KH*KW]^T, run with 1x1 geometry
            K = self.weight.shape[0]
            y = ops.conv2d_fwd(x.view(x.shape[0], -1, 1, 1), self.weight.view(K, -1, 1, 1), 1, 0, shift=self.bias,
                               residual=residual, act=act, slope=slope)
        else:
            y = ops.conv2d_fwd(x, self.weight, self.stride, self.padding, shift=self.bias, residual=residual, act=act,
                               slope=slope, w_krsc=self._krsc())
        tape.push((x, y if act != ACT_NONE else None, act, slope))
        return y

    def _full_extent(self, x):
        return (tuple(x.shape[2:]) == self.kernel_size and self.padding == (0, 0) and self.kernel_size != (1, 1)
                and x.is_contiguous())

    def tb(self, tape, dy, need_dx=True, residual=None, mask_input=False, dx_channels=None, want_rowsum=False):
        """mask_input: the conv's input x is the ReLU output of the layer below — its backward (zero where x <= 0) is
        applied to dx (+ residual) in the dgrad epilogue.  dx_channels=(c0, c1): only that channel range of the input
        receives a gradient (the rest of a concatenated input is constant) -> dx has c1 - c0 channels."""
        f8 = self.__dict__.get("_rg_f8")
        if f8 is not None:
            if mask_input or dx_channels is not None or want_rowsum:
                raise NotImplementedError("Conv2d(fp8): mask_input / dx_channels / want_rowsum belong to the fp32 ResNet programs")
            xq_t, y, act, slope, geom = tape.pop()
            want_w = tape.wants(self.weight)
            dyq, dyq_t = _f8_backward_operands(tape, f8, self.bias, dy, y, act, slope, need_dx, want_w)
            if want_w:
                gout = tape.grad_dst(self.weight)
                tape.add_grad(self.weight, ops.side_call(lambda: lowp.conv_wgrad(xq_t, dyq_t, geom, out=gout), xq_t, dyq_t, gout,
                                                           worth=ops.side_worth(_geom_gflop(geom, dy), fp8=True)))
            if not need_dx:
                return None
            _, wq_t = f8.weights(self.weight.detach(), weight_key(self.weight))
            return lowp.conv_dgrad(dyq, wq_t, geom, (geom[2], geom[3]), residual=residual)
        x, y, act, slope = tape.pop()
        if act != ACT_NONE:
            dy = ops.act_bwd(dy, y, act, slope)
        if tape.wants(self.weight):
            tape.add_grad(self.weight, ops.conv2d_wgrad(x, dy, self.weight.shape, self.stride, self.padding,
                                                        out=tape.grad_dst(self.weight), side=True))
        if tape.wants(self.bias):
            _bias_grad(tape, self.bias, dy)
        if not need_dx:
            return None
        if self._full_extent(x) and dx_channels is None and residual is None and not mask_input and not want_rowsum:
            K = self.weight.shape[0]
            return ops.conv2d_dgrad(dy, self.weight.view(K, -1, 1, 1), (1, 1), 1, 0).view(x.shape)
        if dx_channels is not None:
            c0, c1 = dx_channels
            return ops.conv2d_dgrad(dy, self.weight.detach()[:, c0:c1].contiguous(), x.shape[2:], self.stride, self.padding)
        return ops.conv2d_dgrad(dy, self.weight, x.shape[2:], self.stride, self.padding, residual=residual,
                                w_krsc=self._krsc(), relu_mask=x if mask_input else None, want_rowsum=want_rowsum)


class ConvTranspose2d(RGModule, _KrscCache):
    """weight [in][out][kh][kw] as torch; forward is the dgrad kernel, backward-data the forward kernel."""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, output_padding=0, bias=True):
        super(ConvTranspose2d, self).__init__()
        self.in_channels, self.out_channels = in_channels, out_channels
        self.kernel_size, self.stride, self.padding = _pair(kernel_size), _pair(stride), _pair(padding)
        self.output_padding = _pair(output_padding)
        self.weight = nn.Parameter(torch.empty(in_channels, out_channels, *self.kernel_size))
        self.bias = nn.Parameter(torch.empty(out_channels)) if bias else None
        self.reset_parameters()

    def reset_parameters(self):          # identical to torch.nn.ConvTranspose2d (fan_in from dim 1)
        _conv_init(self.weight, self.bias)

    def out_hw(self, H, W):
        return ((H - 1) * self.stride[0] - 2 * self.padding[0] + self.kernel_size[0] + self.output_padding[0],
                (W - 1) * self.stride[1] - 2 * self.padding[1] + self.kernel_size[1] + self.output_padding[1])

    def _geom(self, hw):
        """geometry of the convolution whose data gradient is this layer's forward: (N filled by the caller, C = out_channels,
        H, W = output size, K = in_channels, ...)"""
        return (self.out_channels, hw[0], hw[1], self.in_channels, self.kernel_size[0], self.kernel_size[1], self.stride[0],
                self.stride[1], self.padding[0], self.padding[1])

    def tf(self, tape, x, act=ACT_NONE, slope=0.0, residual=None):
        hw = self.out_hw(x.shape[2], x.shape[3])
        f8 = self.__dict__.get("_rg_f8")
        if f8 is not None:
            # forward == data gradient of the convolution with this weight tensor: x plays dy (e4m3 here), filters [C][RS][Kp]
            want_w = tape.record and tape.wants(self.weight)
            xq, xq_t = f8.quant_act_both(x, want_w)
            _, wq_t = f8.weights(self.weight.detach(), weight_key(self.weight))
            geom = (x.shape[0],) + self._geom(hw)
            y = lowp.conv_dgrad(xq, wq_t, geom, hw, shift=self.bias, residual=residual, act=act, slope=slope)
            tape.push((xq_t, y if act != ACT_NONE else None, act, slope, geom))
            return y
        if (x.shape[2] == 1 and x.shape[3] == 1 and self.padding == (0, 0) and self.output_padding == (0, 0)
                and self.bias is None and act == ACT_NONE and residual is None):
            # a 1x1 input makes the transposed conv a plain GEMM x[N][K] . w[K][C*KH*KW] (the generator's
            # 2432 -> 512 (8,4) layer, FD/fdgan/networks.py:105-109): run it with 1x1 geometry so no
            # MFMA work is spent on taps that fall outside the single input pixel
            K, C, KH, KW = self.weight.shape
            y = ops.conv2d_dgrad(x, self.weight.view(K, C * KH * KW, 1, 1), (1, 1), 1, 0).view(x.shape[0], C, KH, KW)
            tape.push((x, None, act, slope))
            return y
        y = ops.conv2d_dgrad(x, self.weight, hw, self.stride, self.padding, shift=self.bias, residual=residual, act=act,
                             slope=slope, w_krsc=self._krsc())
        tape.push((x, y if act != ACT_NONE else None, act, slope))
        return y

    def tb(self, tape, dy, need_dx=True, residual=None):
        f8 = self.__dict__.get("_rg_f8")
        if f8 is not None:
            xq_t, y, act, slope, geom = tape.pop()
            want_w = tape.wants(self.weight)
            dyq, dyq_t = _f8_backward_operands(tape, f8, self.bias, dy, y, act, slope, need_dx, want_w)
            if want_w:
                # filter gradient with the roles swapped: the "input" is dy (e5m2), the "output gradient" is x (e4m3)
                gout = tape.grad_dst(self.weight)
                tape.add_grad(self.weight, ops.side_call(lambda: lowp.conv_wgrad(dyq_t, xq_t, geom, out=gout), xq_t, dyq_t, gout,
                                                           worth=ops.side_worth(_geom_gflop(geom, dy), fp8=True)))
            if not need_dx:
                return None
            wq, _ = f8.weights(self.weight.detach(), weight_key(self.weight))
            return lowp.conv_fwd(dyq, wq, geom, residual=residual)
        x, y, act, slope = tape.pop()
        if act != ACT_NONE:
            dy = ops.act_bwd(dy, y, act, slope)
        if tape.wants(self.weight):
            tape.add_grad(self.weight, ops.conv2d_wgrad(dy, x, self.weight.shape, self.stride, self.padding,
                                                        out=tape.grad_dst(self.weight), side=True))
        if tape.wants(self.bias):
            _bias_grad(tape, self.bias, dy)
        if not need_dx:
            return None
        if (x.shape[2] == 1 and x.shape[3] == 1 and self.padding == (0, 0) and self.output_padding == (0, 0)
                and tuple(dy.shape[2:]) == self.kernel_size and dy.is_contiguous()):
            # 1x1 input (see tf): dx[N][K] = dy[N][C*KH*KW] . w[K][C*KH*KW]^T, no (r,s)-major filter copy needed
            K = self.weight.shape[0]
            return ops.conv2d_fwd(dy.view(dy.shape[0], -1, 1, 1), self.weight.view(K, -1, 1, 1), 1, 0, residual=residual)
        return ops.conv2d_fwd(dy, self.weight, self.stride, self.padding, residual=residual, w_krsc=self._krsc())


class Linear(RGModule):
    def __init__(self, in_features, out_features, bias=True):
        super(Linear, self).__init__()
        self.in_features, self.out_features = in_features, out_features
        self.weight = nn.Parameter(torch.empty(out_features, in_features))
        self.bias = nn.Parameter(torch.empty(out_features)) if bias else None
        self.reset_parameters()

    def reset_parameters(self):
        init.kaiming_uniform_(self.weight, a=math.sqrt(5))
        if self.bias is not None:
            bound = 1 / math.sqrt(self.in_features)
            init.uniform_(self.bias, -bound, bound)

    def tf(self, tape, x):
        tape.push(x)
        return ops.linear_fwd(x, self.weight, self.bias)

    def tb(self, tape, dy, need_dx=True):
        x = tape.pop()
        if tape.wants(self.weight):
            tape.add_grad(self.weight, ops.linear_wgrad(x, dy, out=tape.grad_dst(self.weight)))
        if tape.wants(self.bias):
            _bias_grad(tape, self.bias, dy)
        return ops.linear_dgrad(dy, self.weight) if need_dx else None
