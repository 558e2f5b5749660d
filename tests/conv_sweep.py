"""Shared machinery of the per-element conv sweeps (tests/test_conv_candidates_gpu.py: the bench's geometries;
tests/test_conv_ragged_gpu.py: ragged geometries under forced plans; tests/test_conv_ragged_cpu.py: the references and the bound).

  * fp64 references of the three convolution GEMMs (torch unfold / fold / matmul only, on whichever device the operands live),
    each with the same contraction on absolute values;
  * the epilogues the library fuses behind them (scale, shift, residual, activation, ReLU mask, row sums, BatchNorm fold) with
    the per-element bound each composes;
  * _Sweep: runs every combination of a call's nested measured choices, pinned one at a time with rg_conv_set_pick and read back
    through rg_conv_pick_log;
  * NaN-filled output storage with a NaN guard behind it.

Bound, per element: |out - ref| <= 2^-20 * (|a| (*) |b|) + 1e-30 with (|a| (*) |b|) the contraction on absolute values plus the
absolute epilogue operands.  ReLU and leaky ReLU are 1-Lipschitz: the bound of their argument carries through.  tanh is
1-Lipschitz too and adds its own evaluation error, the tanh term of tests/body_hostmodel.py: C_KIND["tanh"] * 2^-24 *
(|y| + |z| (1 - y^2)) for y = tanh(z).  A masked element must be 0 (the 1e-30 floor only)."""
import math

import numpy as np
import torch
import torch.nn.functional as F

from tests.body_hostmodel import C_KIND

ALL_KINDS = (1, 2, 4, 16, 32, 64, 128, 256)
FAMILY_OF = {1: "fwd", 16: "fwd", 64: "fwd", 2: "dgrad", 32: "dgrad", 128: "dgrad", 4: "wgrad", 256: "wgrad"}
LEVELS = {"fwd": (16, 64, 1), "dgrad": (32, 128, 2), "wgrad": (256, 4)}     # outer -> inner: path, plan, implementation
TOL = 2.0 ** -20
TINY = 1e-30
SLOPE = float(np.float32(0.2))
CHUNK_BYTES = 1 << 30           # fp64 unfolded columns per reference chunk
ACT_NONE, ACT_RELU, ACT_LEAKY, ACT_TANH = 0, 1, 2, 3
TANH_TOL = C_KIND["tanh"] * 2.0 ** -24


def _out_hw(H, W, KH, KW, SH, SW, PH, PW):
    return (H + 2 * PH - KH) // SH + 1, (W + 2 * PW - KW) // SW + 1


def _chunks(N, per_sample_bytes):
    step = max(1, CHUNK_BYTES // max(1, per_sample_bytes))
    for n0 in range(0, N, step):
        yield n0, min(N, n0 + step)


# ---- fp64 references (torch unfold / fold / matmul only), each with its contraction on absolute values ----
def ref_fwd(x, w, stride, pad):
    N, C, H, W = x.shape
    K, _, KH, KW = w.shape
    P, Q = _out_hw(H, W, KH, KW, stride[0], stride[1], pad[0], pad[1])
    wm = w.reshape(K, -1)
    wa = wm.abs()
    y = torch.empty((N, K, P * Q), dtype=torch.float64, device=x.device)
    a = torch.empty_like(y)
    for n0, n1 in _chunks(N, 2 * C * KH * KW * P * Q * 8):
        cols = F.unfold(x[n0:n1], (KH, KW), padding=pad, stride=stride)
        y[n0:n1] = torch.matmul(wm, cols)
        a[n0:n1] = torch.matmul(wa, cols.abs_())
    return y.view(N, K, P, Q), a.view(N, K, P, Q)


def ref_dgrad(dy, w, hw, stride, pad):
    N, K, P, Q = dy.shape
    _, C, KH, KW = w.shape
    wt = w.reshape(K, -1).t()
    wa = wt.abs()
    dx = torch.empty((N, C) + tuple(hw), dtype=torch.float64, device=dy.device)
    a = torch.empty_like(dx)
    for n0, n1 in _chunks(N, C * KH * KW * P * Q * 8):
        d = dy[n0:n1].reshape(n1 - n0, K, P * Q)
        dx[n0:n1] = F.fold(torch.matmul(wt, d), hw, (KH, KW), padding=pad, stride=stride)
        a[n0:n1] = F.fold(torch.matmul(wa, d.abs()), hw, (KH, KW), padding=pad, stride=stride)
    return dx, a


def ref_wgrad(x, dy, ksize, stride, pad):
    N, C, H, W = x.shape
    K, P, Q = dy.shape[1], dy.shape[2], dy.shape[3]
    KH, KW = ksize
    g = torch.zeros((K, C * KH * KW), dtype=torch.float64, device=x.device)
    a = torch.zeros_like(g)
    for n0, n1 in _chunks(N, 2 * C * KH * KW * P * Q * 8):
        cols = F.unfold(x[n0:n1], (KH, KW), padding=pad, stride=stride)
        d = dy[n0:n1].reshape(n1 - n0, K, P * Q)
        g += torch.matmul(d, cols.transpose(1, 2)).sum(0)
        a += torch.matmul(d.abs(), cols.abs_().transpose(1, 2)).sum(0)
    return g.view(K, C, KH, KW), a.view(K, C, KH, KW)


# ---- the fused epilogues: out = mask(act(acc * scale[m] + shift[m] + residual)), m the output channel (dim 1) ----
def ref_epilogue(acc, acc_abs, scale=None, shift=None, res=None, act=ACT_NONE, slope=SLOPE, mask=None):
    """(ref, tol) of the epilogue behind a forward (m = k) or a data gradient (m = c: ConvTranspose2d's bias and activation, or the
    residual add and ReLU backward of a trunk); every operand fp64 or None.  acc / acc_abs are left unchanged."""
    ch = (1, -1, 1, 1)
    z, mag = acc, acc_abs
    if scale is not None:
        z, mag = z * scale.view(ch), mag * scale.abs().view(ch)
    if shift is not None:
        z, mag = z + shift.view(ch), mag + shift.abs().view(ch)
    if res is not None:
        z, mag = z + res, mag + res.abs()
    tol = mag * TOL
    if act == ACT_RELU:
        ref = z.clamp(min=0.0)
    elif act == ACT_LEAKY:
        ref = torch.where(z > 0, z, z * slope)
    elif act == ACT_TANH:
        ref = torch.tanh(z)
        tol = tol + TANH_TOL * (ref.abs() + z.abs() * (1.0 - ref * ref))
    else:
        assert act == ACT_NONE, act
        ref = z if z is not acc else acc.clone()
    if mask is not None:
        keep = mask > 0
        ref = ref * keep
        tol = tol * keep
    return ref, tol + TINY


def ref_rowsum(ref, tol):
    """channel sums of the FINAL values (what the fused row sums add up to over their columns), with the summed bound"""
    return ref.sum((0, 2, 3)), tol.sum((0, 2, 3))


def ref_fold(G, G_abs, wf, scale, invstd, mean, partials=None, sum_g=None):
    """frozen-statistics BatchNorm folded behind the weight gradient: dw = scale G, dgamma = invstd (sum_m w G - mean sum_g), dbeta =
    sum_g (from slice partials [K][slices], else sum_g is given and dbeta is not written).  {name: (ref, tol)}, operands fp64."""
    K = G.shape[0]
    out = {"wgrad": (G * scale.view(K, 1, 1, 1), G_abs * (scale.abs().view(K, 1, 1, 1) * TOL) + TINY)}
    if partials is not None:
        sg, sg_abs = partials.sum(1), partials.abs().sum(1)
        out["wgrad fold dbeta"] = (sg, sg_abs * TOL + TINY)
    else:
        sg, sg_abs = sum_g, sum_g.abs()
    wm, g2, ga2 = wf.reshape(K, -1), G.reshape(K, -1), G_abs.reshape(K, -1)
    out["wgrad fold dgamma"] = (invstd * ((wm * g2).sum(1) - mean * sg),
                                invstd.abs() * ((wm.abs() * ga2).sum(1) + mean.abs() * sg_abs) * TOL + TINY)
    return out


class _Sweep(object):
    def __init__(self, lib):
        self.lib = lib
        self.buf = np.zeros(18 * 64, dtype=np.int32)
        self.keys = {}                          # every key the library reported -> its candidate count
        self.worst = {}                         # check name -> worst ratio
        self.count = {"fwd": 0, "dgrad": 0, "wgrad": 0}
        self.calls = {"fwd": 0, "dgrad": 0, "wgrad": 0}
        self.bad = []
        self.ran = {}                           # (key, index run) -> worst ratio of the launches it was part of
        self.recs = {}                          # the records of the last launch, by kind

    def log(self):
        n = self.lib.rg_conv_pick_log(self.buf.ctypes.data, 64)
        assert 0 <= n <= 64, n
        recs = self.buf[:18 * n].reshape(n, 18)
        out = {}
        for r in recs:
            key, ncand, idx = tuple(int(v) for v in r[:16]), int(r[16]), int(r[17])
            assert key[0] not in out, "two choices of kind %d in one call" % key[0]
            out[key[0]] = (key, ncand, idx)
            assert self.keys.setdefault(key, ncand) == ncand, ("candidate count of a key changed", key)
        self.recs = out
        return out

    def sweep(self, fam, label, launch, check):
        """runs every combination of the family's nested choices exactly once: a run with the inner levels at 0 reports how many
        candidates each inner level has under the pinned outer ones"""
        levels = LEVELS[fam]
        results = []

        def run(pins):
            for kind, i in zip(levels, pins):
                self.lib.rg_conv_set_pick(kind, i)
            launch()
            recs = self.log()
            for kind, i in zip(levels, pins):
                if kind in recs:
                    assert recs[kind][2] == i, (label, pins, recs[kind])
                else:
                    assert i == 0, (label, pins, kind)
            results.append((pins, check(), [(v[0], v[2]) for v in recs.values()]))
            return {k: v[1] for k, v in recs.items()}

        def visit(prefix):
            pins = prefix + [0] * (len(levels) - len(prefix))
            nc = run(pins)
            for j in range(len(prefix), len(levels)):
                for i in range(1, nc.get(levels[j], 1)):
                    visit(prefix + [0] * (j - len(prefix)) + [i])

        visit([])
        for kind in levels:
            self.lib.rg_conv_set_pick(kind, 0)
        names = list(results[0][1].keys())
        ratios = torch.stack([torch.stack([r[n] for n in names]) for _, r, _ in results]).cpu().numpy()
        for ci, (pins, _, ran) in enumerate(results):
            for ni, n in enumerate(names):
                v = float(ratios[ci, ni])
                self.worst[n] = max(self.worst.get(n, 0.0), v)
                if not v <= 1.0:
                    self.bad.append("%s %s pins %s: %s ratio %.3g" % (label, fam, dict(zip(levels, pins)), n, v))
            top = float(np.nan_to_num(ratios[ci], nan=math.inf).max())
            for rec in ran:
                self.ran[rec] = max(self.ran.get(rec, 0.0), top)
        self.count[fam] += len(results)
        self.calls[fam] += 1
        return [ran for _, _, ran in results]


def _ratio(out, ref, tol):
    q = (out.double() - ref).abs_().div_(tol)
    return torch.nan_to_num(q, nan=math.inf, posinf=math.inf).amax()


def _nan_buffer(numel, dev, guard=256):
    """output storage with a NaN guard behind it (a store past the end shows up as a written guard)"""
    buf = torch.empty(numel + guard, dtype=torch.float32, device=dev)
    return buf, buf[:numel], buf[numel:]


def _guard_ok(ratio, guard):
    return torch.where(guard.isnan().all(), ratio, torch.full_like(ratio, math.inf))


def _workspace(nbytes, dev):
    if not nbytes:
        return None
    return torch.empty((int(nbytes) + 3) // 4, dtype=torch.float32, device=dev)
