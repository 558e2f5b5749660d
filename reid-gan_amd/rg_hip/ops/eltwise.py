"""Element-wise kernels, row / channel normalisation, channel copies, row mixing, softmax, the batched GEMM and the bicubic
resize: csrc/eltwise.hip, csrc/bgemm.hip, csrc/resize.hip."""
from __future__ import absolute_import

import torch

from ._base import _chk, _nchw, _p, _same_size, _stream, lib


# ------------------------------------------------------------------------------------------------
# element-wise
# ------------------------------------------------------------------------------------------------
def act_fwd(x, act, slope=0.0, out=None):
    x = _chk(x, "x")
    y = out if out is not None else torch.empty_like(x)
    lib.rg_act_fwd(_p(x), _p(y), x.numel(), act, slope, _stream())
    return y


def act_bwd(dy, y, act, slope=0.0):
    dy, y = _chk(dy, "dy"), _chk(y, "y")
    _same_size("act_bwd", dy, y=y)
    dx = torch.empty_like(dy)
    lib.rg_act_bwd(_p(dy), _p(y), _p(dx), dy.numel(), act, slope, _stream())
    return dx


def axpby(a, b, alpha=1.0, beta=1.0, out=None):
    a, b = _chk(a, "a"), _chk(b, "b")
    _same_size("axpby", a, b=b, out=out)
    y = out if out is not None else torch.empty_like(a)
    if out is not None and getattr(out, "_rg_inst_sums", None) is not None:
        out._rg_inst_sums = None        # accumulating into an InstanceNorm's dx invalidates the sums that kernel attached to it
    lib.rg_axpby(_p(a), _p(b), _p(y), a.numel(), alpha, beta, _stream())
    return y


def add(a, b):
    return axpby(a, b, 1.0, 1.0)


def scale(a, alpha):
    return axpby(a, None, alpha, 0.0)


def pair_cat(a, b, take_a=None):
    """[2B, ...]: rows 0..B-1 = a, rows B.. = a[i] where take_a[i] != 0 else b[i] (take_a None: b) — one launch."""
    a, b = _chk(a, "a"), _chk(b, "b")
    _same_size("pair_cat", a, b=b)
    take_a = _chk(take_a, "take_a", torch.int64)
    B = a.shape[0]
    out = torch.empty((2 * B,) + tuple(a.shape[1:]), dtype=torch.float32, device=a.device)
    lib.rg_pair_cat(_p(a), _p(b), _p(take_a), _p(out), B, a.numel() // B, _stream())
    return out


def fill_(t, v):
    lib.rg_fill(_p(t), t.numel(), float(v), _stream())
    return t


def zeros(shape, device):
    return fill_(torch.empty(shape, dtype=torch.float32, device=device), 0.0)


_CONST_FILL = {}


def const_fill(n, v, device):
    """a cached read-only device vector of n copies of v (identity mean / invstd, unit cotangents): filled once, never on the
    step path afterwards"""
    key = (n, float(v), device.index)
    t = _CONST_FILL.get(key)
    if t is None:
        t = _CONST_FILL[key] = fill_(torch.empty(n, dtype=torch.float32, device=device), v)
    return t


def sub_square_fwd(a, b):
    a, b = _chk(a, "a"), _chk(b, "b")
    y = torch.empty_like(a)
    lib.rg_sub_square_fwd(_p(a), _p(b), _p(y), a.numel(), _stream())
    return y


def sub_square_bwd(a, b, dy, need_a=True, need_b=True):
    a, b, dy = _chk(a, "a"), _chk(b, "b"), _chk(dy, "dy")
    da = torch.empty_like(a) if need_a else None
    db = torch.empty_like(a) if need_b else None
    lib.rg_sub_square_bwd(_p(a), _p(b), _p(dy), _p(da), _p(db), a.numel(), _stream())
    return da, db


_CLOCK = {}


def step_clock(device):
    """device-side step counter (uint64 as int64 storage) mixed into dropout seeds; advanced by rg_hip.graph per captured step"""
    c = _CLOCK.get(device.index)
    if c is None:
        c = _CLOCK[device.index] = torch.zeros(1, dtype=torch.int64, device=device)
    return c


def advance_step_clock(device):
    lib.rg_u64_add(_p(step_clock(device)), 1, _stream())


def dropout(x, p, seed):
    """keep iff hash(seed + K * clock, element) >= p 2^32; the clock is 0 unless a captured step advances it (rg_hip.graph), so
    eager runs reproduce the (seed, index) -> bit function of the oracle exactly"""
    x = _chk(x, "x")
    y = torch.empty_like(x)
    lib.rg_dropout_clocked(_p(x), _p(y), x.numel(), p, seed, _p(step_clock(x.device)), _stream())
    return y


def l2norm_rows_fwd(x, eps=1e-12):
    x = _chk(x, "x")
    rows, D = x.shape
    y = torch.empty_like(x)
    norm = torch.empty(rows, dtype=torch.float32, device=x.device)
    lib.rg_l2norm_rows_fwd(_p(x), _p(y), _p(norm), rows, D, eps, _stream())
    return y, norm


def l2norm_rows_bwd(y, dy, norm, eps=1e-12):
    y, dy = _chk(y, "y"), _chk(dy, "dy")
    rows, D = y.shape
    dx = torch.empty_like(y)
    lib.rg_l2norm_rows_bwd(_p(y), _p(dy), _p(norm), _p(dx), rows, D, eps, _stream())
    return dx


def l2norm_channels_fwd(x, eps=1e-12):
    """F.normalize(x, dim=1) of [N, C, H, W] -> (y, norm [N, H*W]) without permuted copies"""
    x = _chk(x, "x")
    N, C, HW = _nchw(x)
    y = torch.empty_like(x)
    norm = torch.empty((N, HW), dtype=torch.float32, device=x.device)
    lib.rg_l2norm_channels_fwd(_p(x), _p(y), _p(norm), N, C, HW, eps, _stream())
    return y, norm


def l2norm_channels_bwd(y, dy, norm, eps=1e-12):
    y, dy = _chk(y, "y"), _chk(dy, "dy")
    _same_size("l2norm_channels_bwd", y, dy=dy)
    N, C, HW = _nchw(y)
    dx = torch.empty_like(y)
    lib.rg_l2norm_channels_bwd(_p(y), _p(dy), _p(norm), _p(dx), N, C, HW, eps, _stream())
    return dx


def copy_channels(src, dst, c_count, src_c0, dst_c0, accumulate=False):
    src, dstc = _chk(src, "src"), dst
    if not dst.is_contiguous():
        raise ValueError("copy_channels: destination must be contiguous")
    N, Cs, HW = _nchw(src)
    Nd, Cd, HWd = _nchw(dst)
    if N != Nd or HW != HWd:
        raise ValueError("copy_channels: batch / spatial mismatch")
    lib.rg_copy_channels(_p(src), _p(dstc), N, c_count, HW, Cs, src_c0, Cd, dst_c0, int(accumulate), _stream())
    return dst


def bicubic_normalize_fwd(x, size, mean=None, std=None):
    """[N,C,H,W] -> [N,C,OH,OW] bicubic (align_corners False) then (v - mean[c]) / std[c]; mean/std device [C] or None."""
    x = _chk(x, "x")
    if x.dim() != 4:
        raise ValueError("bicubic_normalize: expected NCHW")
    N, C, H, W = x.shape
    OH, OW = int(size[0]), int(size[1])
    y = torch.empty((N, C, OH, OW), dtype=torch.float32, device=x.device)
    lib.rg_bicubic_normalize_fwd(_p(x), _p(y), N, C, H, W, OH, OW, _p(mean) if mean is not None else None,
                                 _p(std) if std is not None else None, _stream())
    return y


def bicubic_normalize_bwd(dy, in_hw, std=None):
    dy = _chk(dy, "dy")
    N, C, OH, OW = dy.shape
    H, W = int(in_hw[0]), int(in_hw[1])
    dx = torch.empty((N, C, H, W), dtype=torch.float32, device=dy.device)
    lib.rg_bicubic_normalize_bwd(_p(dy), _p(dx), N, C, H, W, OH, OW, _p(std) if std is not None else None, _stream())
    return dx


def bgemm(A, B, C, M, N, K, a_str, b_str, c_str, batch, a_b, b_b, c_b, alpha=1.0, beta=0.0):
    """C[b0][b1] = alpha A[b0][b1] . B[b0][b1] + beta C; a_str = (row, k) strides of A, b_str = (k, col) of B,
    c_str = (row, col) of C, batch = (n0, n1), *_b = (stride b0, stride b1); all in elements.  Tensors are base buffers."""
    lib.rg_bgemm(_p(A), _p(B), _p(C), M, N, K, a_str[0], a_str[1], b_str[0], b_str[1], c_str[0], c_str[1], batch[0], batch[1],
                 a_b[0], a_b[1], b_b[0], b_b[1], c_b[0], c_b[1], alpha, beta, _stream())
    return C


def softmax_rows_fwd(x, scale=1.0, out=None):
    x = _chk(x, "x")
    cols = x.shape[-1]
    y = out if out is not None else torch.empty_like(x)
    lib.rg_softmax_rows_fwd(_p(x), _p(y), x.numel() // cols, cols, scale, _stream())
    return y


def softmax_rows_bwd(p, dp, scale=1.0, out=None):
    p, dp = _chk(p, "p"), _chk(dp, "dp")
    cols = p.shape[-1]
    ds = out if out is not None else torch.empty_like(p)
    lib.rg_softmax_rows_bwd(_p(p), _p(dp), _p(ds), p.numel() // cols, cols, scale, _stream())
    return ds


def mix_rows_fwd(src, ia, ib, lam):
    src = _chk(src, "src")
    ia, ib = _chk(ia, "idx_a", torch.int64), _chk(ib, "idx_b", torch.int64)
    R, n = src.shape[0], ia.numel()
    length = src.numel() // R
    out = torch.empty((n,) + tuple(src.shape[1:]), dtype=torch.float32, device=src.device)
    lib.rg_mix_rows_fwd(_p(src), _p(ia), _p(ib), lam, _p(out), R, n, length, _stream())
    return out


def mix_rows_bwd(g, ia, ib, lam, src_shape):
    g = _chk(g, "g")
    R, n = src_shape[0], ia.numel()
    dsrc = torch.empty(tuple(src_shape), dtype=torch.float32, device=g.device)
    lib.rg_mix_rows_bwd(_p(g), _p(ia), _p(ib), lam, _p(dsrc), R, n, dsrc.numel() // R, _stream())
    return dsrc


def cat_channels(tensors):
    """torch.cat(tensors, dim=1) for NCHW (or NC) tensors."""
    N = tensors[0].shape[0]
    Ct = sum(t.shape[1] for t in tensors)
    out = torch.empty((N, Ct) + tuple(tensors[0].shape[2:]), dtype=torch.float32, device=tensors[0].device)
    c0 = 0
    for t in tensors:
        copy_channels(t, out, t.shape[1], 0, c0)
        c0 += t.shape[1]
    return out


def slice_channels(src, c0, c1):
    out = torch.empty((src.shape[0], c1 - c0) + tuple(src.shape[2:]), dtype=torch.float32, device=src.device)
    return copy_channels(src, out, c1 - c0, c0, 0)
