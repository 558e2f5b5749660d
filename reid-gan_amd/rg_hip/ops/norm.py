"""BatchNorm, InstanceNorm, IBN, DSBN and the folded-BatchNorm helpers: csrc/norm_bn.hip, norm_instnorm.hip, norm_ibn.hip,
norm_dsbn.hip, norm_fold.hip."""
from __future__ import absolute_import


import torch

from ._base import ACT_NONE, _chk, _nchw, _p, _same_size, _stream, _ws_query, lib, workspace
from .eltwise import const_fill


# ------------------------------------------------------------------------------------------------
# batch norm on [N][C][HW]
# ------------------------------------------------------------------------------------------------
def bn_stats(x, running_mean=None, running_var=None, eps=1e-5, momentum=0.1):
    x = _chk(x, "x")
    N, C, HW = _nchw(x)
    mean = torch.empty(C, dtype=torch.float32, device=x.device)
    invstd = torch.empty(C, dtype=torch.float32, device=x.device)
    ws = workspace(_ws_query("rg_bn_workspace", N, C, HW), x.device)
    lib.rg_bn_stats(_p(x), _p(mean), _p(invstd), _p(running_mean), _p(running_var), N, C, HW, eps, momentum, _p(ws),
                    ws.numel(), _stream())
    return mean, invstd


def bn_apply_fwd(x, mean, stat, gamma, beta, residual=None, stat_is_var=False, eps=1e-5, act=ACT_NONE, slope=0.0):
    x = _chk(x, "x")
    residual = _chk(residual, "residual")
    _same_size("bn_apply_fwd", x, residual=residual)
    N, C, HW = _nchw(x)
    y = torch.empty_like(x)
    lib.rg_bn_apply_fwd(_p(x), _p(mean), _p(stat), _p(gamma), _p(beta), _p(residual), _p(y), N, C, HW,
                        int(stat_is_var), eps, act, slope, _stream())
    return y


def bn_bwd_reduce(x, dy, y_act, mean, stat, stat_is_var=False, eps=1e-5, act=ACT_NONE, slope=0.0,
                  out_sum_dy=None, out_sum_dy_xhat=None):
    x, dy, y_act = _chk(x, "x"), _chk(dy, "dy"), _chk(y_act, "y")
    _same_size("bn_bwd_reduce", x, dy=dy, y=y_act)
    N, C, HW = _nchw(x)
    sum_dy = out_sum_dy if out_sum_dy is not None else torch.empty(C, dtype=torch.float32, device=x.device)
    sum_dy_xhat = out_sum_dy_xhat if out_sum_dy_xhat is not None else \
        torch.empty(C, dtype=torch.float32, device=x.device)
    ws = workspace(_ws_query("rg_bn_workspace", N, C, HW), x.device)
    lib.rg_bn_bwd_reduce(_p(x), _p(dy), _p(y_act), _p(mean), _p(stat), _p(sum_dy), _p(sum_dy_xhat), N, C, HW,
                         int(stat_is_var), eps, act, slope, _p(ws), ws.numel(), _stream())
    return sum_dy, sum_dy_xhat


def bn_train_fused_ok(x):
    """does this activation qualify for the one-launch train-mode BatchNorm kernels (small per-channel extent, many channels)?"""
    N, C, HW = _nchw(x)
    return bool(_ws_query("rg_bn_train_fused_ok", N, C, HW))


def bn_train_fwd_fused(x, gamma, beta, residual, running_mean, running_var, eps, momentum, act=ACT_NONE, slope=0.0):
    """batch statistics + running-statistics update + normalise + affine + residual + activation -> (y, mean[C], invstd[C])"""
    x, residual = _chk(x, "x"), _chk(residual, "residual")
    _same_size("bn_train_fwd_fused", x, residual=residual)
    N, C, HW = _nchw(x)
    y = torch.empty_like(x)
    stats = torch.empty(2, C, dtype=torch.float32, device=x.device)
    lib.rg_bn_train_fwd_fused(_p(x), _p(gamma), _p(beta), _p(residual), _p(y), _p(stats[0]), _p(stats[1]), _p(running_mean),
                              _p(running_var), N, C, HW, eps, momentum, act, slope, _stream())
    return y, stats[0], stats[1]


def bn_train_bwd_fused(x, dy, y_act, mean, invstd, gamma, act=ACT_NONE, slope=0.0, need_dx=True, need_dres=False,
                       out_sum_dy=None, out_sum_dy_xhat=None):
    """-> (dx, dres, sum_g[C], sum_g_xhat[C]) in one launch"""
    x, dy, y_act = _chk(x, "x"), _chk(dy, "dy"), _chk(y_act, "y")
    _same_size("bn_train_bwd_fused", dy, x=x, y=y_act)
    N, C, HW = _nchw(x)
    dx = torch.empty_like(dy) if need_dx else None
    dres = torch.empty_like(dy) if need_dres else None
    s1 = out_sum_dy if out_sum_dy is not None else torch.empty(C, dtype=torch.float32, device=x.device)
    s2 = out_sum_dy_xhat if out_sum_dy_xhat is not None else torch.empty(C, dtype=torch.float32, device=x.device)
    lib.rg_bn_train_bwd_fused(_p(x), _p(dy), _p(y_act), _p(mean), _p(invstd), _p(gamma), _p(dx), _p(dres), _p(s1), _p(s2), N, C, HW,
                              act, slope, _stream())
    return dx, dres, s1, s2


def instnorm_fwd(x, gamma=None, beta=None, residual=None, eps=1e-5, act=ACT_NONE, slope=0.0):
    """InstanceNorm over the trailing dims of x[N][C][...] in one launch -> (y, mean[N*C], invstd[N*C])."""
    x, residual = _chk(x, "x"), _chk(residual, "residual")
    _same_size("instnorm_fwd", x, residual=residual)
    N, C, HW = _nchw(x)
    y = torch.empty_like(x)
    stats = torch.empty(2, N * C, dtype=torch.float32, device=x.device)
    lib.rg_instnorm_fwd(_p(x), _p(gamma), _p(beta), _p(residual), _p(y), _p(stats[0]), _p(stats[1]), N, C, HW, eps, act, slope,
                        _stream())
    return y, stats[0], stats[1]


def instnorm_bwd(x, dy, y_act, mean, invstd, gamma=None, act=ACT_NONE, slope=0.0, need_dx=True, need_dres=False):
    """-> (dx, dres, sum_g[N*C], sum_g_xhat[N*C], sum_dx[N*C]) in one launch."""
    x, dy, y_act = _chk(x, "x"), _chk(dy, "dy"), _chk(y_act, "y")
    _same_size("instnorm_bwd", dy, x=x, y=y_act)
    N, C, HW = _nchw(x)
    dx = torch.empty_like(dy) if need_dx else None
    dres = torch.empty_like(dy) if need_dres else None
    sums = torch.empty(3, N * C, dtype=torch.float32, device=x.device)
    lib.rg_instnorm_bwd(_p(x), _p(dy), _p(y_act), _p(mean), _p(invstd), _p(gamma), _p(dx), _p(dres), _p(sums[0]), _p(sums[1]),
                        _p(sums[2]) if need_dx else None, N, C, HW, act, slope, _stream())
    return dx, dres, sums[0], sums[1], (sums[2] if need_dx else None)


def rows_sum_pair(a, b, N, C, out_a=None, out_b=None):
    """column sums of two [N][C] matrices in one launch (InstanceNorm affine gradients)."""
    dev = (a if a is not None else b).device
    if a is not None and out_a is None:
        out_a = torch.empty(C, dtype=torch.float32, device=dev)
    if b is not None and out_b is None:
        out_b = torch.empty(C, dtype=torch.float32, device=dev)
    lib.rg_rows_sum_pair(_p(a), _p(b), _p(out_a), _p(out_b), N, C, _stream())
    return out_a, out_b


def ibn_fwd(x, half, in_gamma, in_beta, bn_gamma, bn_beta, running_mean, running_var, train, in_eps=1e-5, bn_eps=1e-5,
            momentum=0.1, residual=None, act=ACT_NONE):
    """IBN layer (InstanceNorm on channels [0, half), BatchNorm on the rest) on the whole tensor, no slice / cat copies
    -> (y, in_mean[N*half], in_invstd[N*half], bn_mean[C-half], bn_invstd[C-half]); the BN statistics are None in eval mode."""
    x, residual = _chk(x, "x"), _chk(residual, "residual")
    _same_size("ibn_fwd", x, residual=residual)
    N, C, HW = _nchw(x)
    y = torch.empty_like(x)
    in_stats = torch.empty(2, N * half, dtype=torch.float32, device=x.device)
    bn_stats_ = torch.empty(2, C - half, dtype=torch.float32, device=x.device) if train else None
    ws = workspace(_ws_query("rg_ibn_workspace", N, C, HW, half), x.device)
    lib.rg_ibn_fwd(_p(x), _p(in_gamma), _p(in_beta), _p(bn_gamma), _p(bn_beta), _p(residual), _p(y), _p(in_stats[0]),
                   _p(in_stats[1]), _p(bn_stats_[0]) if train else None, _p(bn_stats_[1]) if train else None,
                   _p(running_mean), _p(running_var), N, C, HW, half, int(train), in_eps, bn_eps, momentum, act, _p(ws),
                   ws.numel(), _stream())
    return y, in_stats[0], in_stats[1], (bn_stats_[0] if train else None), (bn_stats_[1] if train else None)


def ibn_bwd(x, dy, y_act, half, in_mean, in_invstd, bn_mean, bn_stat, in_gamma, bn_gamma, train, bn_eps=1e-5, act=ACT_NONE,
            out=(None, None, None, None)):
    """-> (dx, d_in_gamma, d_in_beta, d_bn_gamma, d_bn_beta).  bn_mean / bn_stat: the saved batch mean / invstd (train) or the
    running mean / variance (eval).  `out`: preallocated gradient outputs in that order."""
    x, dy, y_act = _chk(x, "x"), _chk(dy, "dy"), _chk(y_act, "y")
    _same_size("ibn_bwd", dy, x=x, y=y_act)
    N, C, HW = _nchw(x)
    dx = torch.empty_like(dy)
    sizes = (half, half, C - half, C - half)
    grads = [o if o is not None else torch.empty(n, dtype=torch.float32, device=x.device) for o, n in zip(out, sizes)]
    ws = workspace(_ws_query("rg_ibn_workspace", N, C, HW, half), x.device)
    lib.rg_ibn_bwd(_p(x), _p(dy), _p(y_act), _p(in_mean), _p(in_invstd), _p(bn_mean), _p(bn_stat), _p(in_gamma), _p(bn_gamma),
                   _p(dx), _p(grads[0]), _p(grads[1]), _p(grads[2]), _p(grads[3]), N, C, HW, half, int(train), bn_eps, act,
                   _p(ws), ws.numel(), _stream())
    return (dx,) + tuple(grads)


def dsbn_fwd(x, gamma_s, beta_s, gamma_t, beta_t, running_s=(None, None), running_t=(None, None), eps=(1e-5, 1e-5),
             momentum=(0.1, 0.1), residual=None, act=ACT_NONE, slope=0.0):
    """train-mode domain-specific BatchNorm on the whole [source | target] batch, no slice / cat copies: samples [0, N/2) with
    their batch statistics and the S set, samples [N/2, N) with theirs and the T set; running_s / running_t = (mean, var), updated
    in place -> (y, stats[2][2][C]): stats[0] the two means, stats[1] the two invstd (S row, T row)."""
    if x.shape[0] % 2:
        raise RuntimeError("dsbn_fwd: a batch of %d samples has no [source | target] halves" % x.shape[0])
    x, residual = _chk(x, "x"), _chk(residual, "residual")
    _same_size("dsbn_fwd", x, residual=residual)
    N, C, HW = _nchw(x)
    y = torch.empty_like(x)
    stats = torch.empty(2, 2, C, dtype=torch.float32, device=x.device)
    ws = workspace(_ws_query("rg_dsbn_workspace", N, C, HW), x.device)
    lib.rg_dsbn_fwd(_p(x), _p(gamma_s), _p(beta_s), _p(gamma_t), _p(beta_t), _p(residual), _p(y), _p(stats[0]), _p(stats[1]),
                    _p(running_s[0]), _p(running_s[1]), _p(running_t[0]), _p(running_t[1]), N, C, HW, eps[0], eps[1], momentum[0],
                    momentum[1], act, slope, _p(ws), ws.numel(), _stream())
    return y, stats


def dsbn_bwd(x, dy, y_act, stats, gamma_s, gamma_t, act=ACT_NONE, slope=0.0, need_dx=True, need_dres=False,
             out=(None, None, None, None)):
    """-> (dx, dres, d_gamma_s, d_beta_s, d_gamma_t, d_beta_t).  stats: what dsbn_fwd returned.  `out`: preallocated gradient
    outputs in that order."""
    if x.shape[0] % 2:
        raise RuntimeError("dsbn_bwd: a batch of %d samples has no [source | target] halves" % x.shape[0])
    x, dy, y_act = _chk(x, "x"), _chk(dy, "dy"), _chk(y_act, "y")
    _same_size("dsbn_bwd", dy, x=x, y=y_act)
    N, C, HW = _nchw(x)
    dx = torch.empty_like(dy) if need_dx else None
    dres = torch.empty_like(dy) if need_dres else None
    grads = [o if o is not None else torch.empty(C, dtype=torch.float32, device=x.device) for o in out]
    ws = workspace(_ws_query("rg_dsbn_workspace", N, C, HW), x.device)
    lib.rg_dsbn_bwd(_p(x), _p(dy), _p(y_act), _p(stats[0]), _p(stats[1]), _p(gamma_s), _p(gamma_t), _p(dx), _p(dres), _p(grads[0]),
                    _p(grads[1]), _p(grads[2]), _p(grads[3]), N, C, HW, act, slope, _p(ws), ws.numel(), _stream())
    return (dx, dres) + tuple(grads)


def bn_bwd_apply(x, dy, y_act, mean, stat, gamma, sum_dy, sum_dy_xhat, train, stat_is_var=False, eps=1e-5,
                 act=ACT_NONE, slope=0.0, need_dx=True, need_dres=False):
    x, dy, y_act = _chk(x, "x"), _chk(dy, "dy"), _chk(y_act, "y")
    _same_size("bn_bwd_apply", dy, x=x, y=y_act)
    N, C, HW = _nchw(dy)
    dx = torch.empty_like(dy) if need_dx else None
    dres = torch.empty_like(dy) if need_dres else None
    lib.rg_bn_bwd_apply(_p(x), _p(dy), _p(y_act), _p(mean), _p(stat), _p(gamma), _p(sum_dy), _p(sum_dy_xhat), _p(dx),
                        _p(dres), N, C, HW, int(train), int(stat_is_var), eps, act, slope, _stream())
    return dx, dres


def bn_eval_bwd(x, dy, y_act, running_mean, running_var, gamma, eps=1e-5, act=ACT_NONE, slope=0.0, need_dx=True,
                need_dres=False, need_sums=True, out_sum_dy=None, out_sum_dy_xhat=None):
    """Eval-mode BatchNorm backward in one pass -> (dx, dres, sum_dy, sum_dy_xhat)."""
    x, dy, y_act = _chk(x, "x"), _chk(dy, "dy"), _chk(y_act, "y")
    _same_size("bn_eval_bwd", dy, x=x, y=y_act)
    N, C, HW = _nchw(dy)
    dx = torch.empty_like(dy) if need_dx else None
    dres = torch.empty_like(dy) if need_dres else None
    s1 = s2 = None
    if need_sums:
        s1 = out_sum_dy if out_sum_dy is not None else torch.empty(C, dtype=torch.float32, device=dy.device)
        s2 = out_sum_dy_xhat if out_sum_dy_xhat is not None else torch.empty(C, dtype=torch.float32, device=dy.device)
    ws = workspace(_ws_query("rg_bn_workspace", N, C, HW), dy.device)
    lib.rg_bn_eval_bwd(_p(x), _p(dy), _p(y_act), _p(running_mean), _p(running_var), _p(gamma), _p(dx), _p(dres), _p(s1),
                       _p(s2), N, C, HW, eps, act, slope, _p(ws), ws.numel(), _stream())
    return dx, dres, s1, s2


def bn_fold(gamma, beta, running_mean, running_var, eps=1e-5):
    """(scale, shift, invstd) of a frozen-statistics BatchNorm: y = z * scale + shift."""
    C = running_mean.numel()
    buf = torch.empty(3, C, dtype=torch.float32, device=running_mean.device)
    lib.rg_bn_fold(_p(gamma), _p(beta), _p(running_mean), _p(running_var), eps, _p(buf[0]), _p(buf[1]), _p(buf[2]), C,
                   _stream())
    return buf[0], buf[1], buf[2]


def act_bwd_sum(dy, y_act, act, slope=0.0, need_g=True, need_sum=True, out_sum=None):
    """g = dy * act'(y) and its per-channel sums over N, HW -> (g, sum_g)."""
    dy, y_act = _chk(dy, "dy"), _chk(y_act, "y")
    _same_size("act_bwd_sum", dy, y=y_act)
    N, C, HW = _nchw(dy)
    g = torch.empty_like(dy) if need_g else None
    sg = None
    if need_sum:
        sg = out_sum if out_sum is not None else torch.empty(C, dtype=torch.float32, device=dy.device)
    ws = workspace(_ws_query("rg_bn_workspace", N, C, HW), dy.device)
    lib.rg_act_bwd_sum(_p(dy), _p(y_act), _p(g), _p(sg), N, C, HW, act, slope, _p(ws), ws.numel(), _stream())
    return g, sg


def bn_fold_wgrad(w, g, scale, invstd, running_mean, sum_g, dgamma=None, partials=None, dbeta=None):
    """in place: g (= wgrad of the un-normalised output gradient) *= scale per filter; dgamma from sum(w * g); the channel
    sums come as sum_g[K] or as slice partials [K, S] (then dbeta is written here too)."""
    K = w.shape[0]
    M = w.numel() // K
    S = partials.shape[1] if partials is not None else 0
    lib.rg_bn_fold_wgrad(_p(w), _p(g), _p(scale), _p(invstd), _p(running_mean), _p(sum_g), _p(partials), S, _p(dbeta),
                         _p(dgamma), K, M, _stream())
    return g


def act_bwd_partial(dy, y_act, act, slope=0.0, need_g=True):
    """g = dy * act'(y) (or None) and the slice partials [C, S] of its channel sums (no finalize launch)."""
    dy, y_act = _chk(dy, "dy"), _chk(y_act, "y")
    _same_size("act_bwd_partial", dy, y=y_act)
    N, C, HW = _nchw(dy)
    g = torch.empty_like(dy) if need_g else None
    S = _ws_query("rg_bn_slices", N, C, HW)
    part = torch.empty((C, S), dtype=torch.float32, device=dy.device)
    lib.rg_act_bwd_partial(_p(dy), _p(y_act), _p(g), _p(part), N, C, HW, act, slope, _stream())
    return g, part


def fold_filters_multi(table, n_pairs, blocks):
    lib.rg_fold_filters_multi(_p(table), n_pairs, blocks, _stream())


def scale_rows(w, scale):
    w = _chk(w, "w")
    out = torch.empty_like(w)
    K = w.shape[0]
    lib.rg_scale_rows(_p(w), _p(scale), _p(out), K, w.numel() // K, _stream())
    return out


def channel_sum(dy, out=None):
    """sum over N and HW of dy[N][C][HW] (bias gradient)."""
    dy = _chk(dy, "dy")
    N, C, HW = _nchw(dy)
    if _ws_query("rg_channel_sum_ok", N, C, HW):
        s = out if out is not None else torch.empty(C, dtype=torch.float32, device=dy.device)
        lib.rg_channel_sum(_p(dy), _p(s), N, C, HW, _stream())
        return s
    s, _ = bn_bwd_reduce(dy, dy, None, const_fill(C, 0.0, dy.device), const_fill(C, 1.0, dy.device), out_sum_dy=out)
    return s
