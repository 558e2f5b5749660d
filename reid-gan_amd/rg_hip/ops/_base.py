"""What every wrapper module of rg_hip.ops stands on: the library handle, the activation codes, the process's device binding,
the three tensor validators, the small shape helpers, and the per-stream workspace with the split-K arrival counters.
Imports nothing from its siblings."""
from __future__ import absolute_import

import os

import torch

from ..lib import lib


ACT_NONE, ACT_RELU, ACT_LEAKY, ACT_TANH = 0, 1, 2, 3


_DEV = [None]
CAPTURE_GEN = [0]    # one number per capture (rg_hip.netgraph): "already refreshed inside THIS capture" for grouped caches
CAPTURING = [0]      # > 0 while rg_hip.netgraph captures a network program: caches refresh unconditionally (their launches are recorded)


def _stream():
    """raw hipStream_t of torch's current stream on this process's device (fast path: no Stream object is built; one process
    drives one GPU, so the device index is looked up once)"""
    d = _DEV[0]
    if d is None:
        d = _DEV[0] = torch._C._cuda_getDevice()
    return torch._C._cuda_getCurrentRawStream(d)


def _bind_device(t):
    """the process's GPU is the device of the FIRST tensor an op sees (not whatever torch's current device happened to be when the
    first op ran: a rank that touches an op before torch.cuda.set_device(local_rank) must not launch on device 0's stream handle
    forever after); tensors of another GPU are refused — one process drives one GPU"""
    i = t.device.index
    if _DEV[0] is None:
        _DEV[0] = i
    elif i != _DEV[0]:
        raise RuntimeError("rg_hip: tensor on cuda:%d, but this process has been launching on cuda:%d (one process drives one GPU; "
                           "call torch.cuda.set_device(local_rank) before building the networks)" % (i, _DEV[0]))


# ---- the three tensor validators -------------------------------------------------------------------------------------------
# _chk is the rule: fp32 (or the given dtype) on this process's GPU, and a tensor that is not contiguous or not 16-byte aligned is
# COPIED into one that is (None passes through).  _dense and _chk_rr say in their docstrings where they depart from it.
def _chk(t, name="tensor", dtype=torch.float32):
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError("rg_hip: %s must live on the GPU (got %s); the HIP path has no CPU fallback"
                           % (name, t.device))
    if t.dtype != dtype:
        raise TypeError("rg_hip: %s must be %s, got %s" % (name, dtype, t.dtype))
    if t.device.index != _DEV[0]:
        _bind_device(t)
    if not t.is_contiguous() or (t.data_ptr() & 15):
        t = t.contiguous()
        if t.data_ptr() & 15:
            t = t.clone()
    return t


def _dense(t, name):
    """as _chk without the 16-byte rule: csrc/part_head.hip reads and writes single floats, and a copy of a buffer it UPDATES (the
    running statistics) or of a row of a stacked tensor would be wrong or wasted"""
    if t is None:
        return None
    if not t.is_cuda or t.dtype != torch.float32:
        raise TypeError("rg_hip: %s must be a float32 tensor on the GPU, got %s on %s" % (name, t.dtype, t.device))
    if t.device.index != _DEV[0]:
        _bind_device(t)
    return t if t.is_contiguous() else t.contiguous()


def _chk_rr(t, name, dtype=torch.float32, dim=None):
    """as _chk, but a non-contiguous tensor is refused instead of copied: these arrays index each other by position"""
    if not torch.is_tensor(t):
        raise TypeError("rg_hip: %s must be a tensor, got %s" % (name, type(t).__name__))
    if not t.is_cuda:
        raise RuntimeError("rg_hip: %s must live on the GPU (got %s); the HIP path has no CPU fallback" % (name, t.device))
    if t.dtype != dtype:
        raise TypeError("rg_hip: %s must be %s, got %s" % (name, dtype, t.dtype))
    if dim is not None and t.dim() != dim:
        raise ValueError("rg_hip: %s must have %d dimensions, got shape %s" % (name, dim, tuple(t.shape)))
    if not t.is_contiguous():
        raise ValueError("rg_hip: %s must be contiguous (shape %s, strides %s)" % (name, tuple(t.shape), t.stride()))
    if t.device.index != _DEV[0]:
        _bind_device(t)
    return t


def _p(t):
    return None if t is None else t.data_ptr()


def _pair(v):
    return (v, v) if isinstance(v, int) else (int(v[0]), int(v[1]))


def _nchw(x):
    if x.dim() == 2:
        return x.shape[0], x.shape[1], 1
    N, C = x.shape[0], x.shape[1]
    return N, C, x.numel() // (N * C)


def _same_size(what, ref, **others):
    """element-wise operands must cover the same elements: the C ABI takes one length, so a mismatch (e.g. a residual branch with
    another stride, as in the reference's ResNet-18 wrapper) would read out of bounds instead of failing like torch does"""
    for name, t in others.items():
        if t is not None and t.numel() != ref.numel():
            raise RuntimeError("%s: the size of tensor %s %s must match %s" % (what, name, tuple(t.shape), tuple(ref.shape)))


def _eps32(eps):
    return float(torch.tensor(float(eps), dtype=torch.float32))


def _list_total(rowptr, cnt, n, worst_case, who):
    """the one readback between the two passes of a list builder (count + scan, then fill): the length of the list, rowptr[n]
    of the int32 exclusive prefix sum of cnt int32 [n].  Where the worst case could wrap that sum it is the int64 sum of cnt
    instead.  Refused outside [0, 2^31): the fill pass indexes with the int32 row pointers."""
    total = int(cnt.sum(dtype=torch.int64).item()) if worst_case >= 2 ** 31 else int(rowptr[n].item())
    if not 0 <= total < 2 ** 31:
        raise RuntimeError("rg_hip: %s: %d entries do not fit the int32 row pointers" % (who, total))
    return total


_SPLITK_INKERNEL = os.environ.get("RG_SPLITK_INKERNEL", "0") not in ("", "0")


class _Workspace(object):
    """One growing scratch buffer per (device, stream); kernels on a stream are ordered, so reuse is safe."""

    ARRIVALS = 4096      # arrival counters per stream (split-K launches have at most 1 536 workgroups: <= 768 tiles)

    def __init__(self):
        self.bufs = {}
        self.pinned = {}
        self.arrivals = {}

    def register_arrivals(self, key, device):
        """the split-K arrival counters of the stream key = (device index, raw stream): zeroed once, the launches leave them at
        zero; never freed, never written from here"""
        cnt = self.arrivals[key] = torch.zeros(self.ARRIVALS, dtype=torch.int32, device=device)
        lib.rg_conv_splitk_arrivals(cnt.data_ptr(), self.ARRIVALS, key[1])

    def get(self, nbytes, device):
        key = (device.index, _stream())
        if _SPLITK_INKERNEL and key not in self.arrivals and not CAPTURING[0]:
            # RG_SPLITK_INKERNEL=1: split-K convolutions on this stream finish inside the kernel (rg_conv_splitk_arrivals) — measured
            # equal to the finishing kernel, so off by default
            self.register_arrivals(key, device)
        buf = self.bufs.get(key)
        if buf is None or buf.numel() < nbytes:
            buf = torch.empty(max(int(nbytes), 1 << 20), dtype=torch.uint8, device=device)
            self.bufs[key] = buf
        if CAPTURING[0]:
            # a captured launch keeps this ADDRESS: the buffer must outlive the graph even if a later, larger request replaces it
            # in `bufs` (the allocator would otherwise hand the freed block to a live tensor that the replays then overwrite)
            self.pinned[buf.data_ptr()] = buf
        return buf


_ws = _Workspace()


def splitk_inkernel(enable):
    """(tests, A/B runs) register or remove the current stream's split-K arrival counters: with them the split forward /
    unit-stride data-gradient launches finish inside the convolution kernel, without them a finishing kernel follows — the same
    bits either way.  Returns whether they were registered before."""
    d = _DEV[0]
    if d is None:
        d = _DEV[0] = torch._C._cuda_getDevice()
    key = (d, _stream())
    cnt = _ws.arrivals.get(key)
    was = cnt is not None and cnt is not False
    if enable:
        if not was:
            _ws.register_arrivals(key, torch.device("cuda", d))
    else:
        _ws.arrivals[key] = False              # keeps _Workspace.get from registering again
        lib.rg_conv_splitk_arrivals(None, 0, key[1])
    return was


_ws_sizes = {}


def _ws_query(fn, *dims):
    """workspace size queries are pure functions of the geometry: ask the library once per shape (the small-kernel
    steps are host-bound; this removes a third of their ctypes calls).  The planner force knob changes the answer, so
    rg_conv_set_force users call _ws_sizes.clear()."""
    key = (fn,) + dims
    v = _ws_sizes.get(key)
    if v is None:
        v = _ws_sizes[key] = getattr(lib, fn)(*dims)
    return v


def workspace(nbytes, device):
    return _ws.get(nbytes, device)
