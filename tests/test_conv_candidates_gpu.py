"""GPU: every candidate kernel of every measured conv choice, at the geometries the bench runs, against an fp64 reference.

The bench pins its conv choices from profiles/conv_choices_mi355x.txt (one line per choice key: path, tile / split-K plan, kernel
implementation).  This sweep rebuilds each (family, geometry, epilogue) call those keys describe and runs EVERY candidate of the
nested choices — pinned one at a time with rg_conv_set_pick, counted through rg_conv_pick_log — on buffers the test owns, filled
with NaN before each candidate (outputs, row sums, dgamma / dbeta and the split-K workspace), so an element a candidate leaves
unwritten cannot inherit the previous candidate's value.

Bound, per element: |out - ref| <= 2^-20 * (|a| (*) |b|) + 1e-30, where (|a| (*) |b|) is the same contraction on absolute values
(plus the absolute epilogue operands), all in fp64 on the device with no project kernel involved.  One dropped or doubled term of
a reduction exceeds it; the split-bf16 products with fp32 accumulation land near 2^-24 of it.  The references, _Sweep and the
NaN-buffer helpers live in tests/conv_sweep.py, shared with the ragged-geometry sweep (tests/test_conv_ragged_gpu.py)."""
import math
import os
import time

import pytest
import torch
import torch.nn.functional as F

from tests.conv_sweep import (ALL_KINDS, FAMILY_OF, SLOPE, TINY, TOL, _Sweep, _guard_ok, _nan_buffer, _out_hw, _ratio, _workspace,
                              ref_dgrad, ref_fwd, ref_wgrad)

pytestmark = pytest.mark.gpu

CHOICES = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "conv_choices_mi355x.txt")


def _lib():
    from rg_hip.lib import lib
    return lib


def _choice_rows():
    with open(CHOICES) as f:
        return [[int(v) for v in ln.split()] for ln in f if ln.strip()]


def _calls(rows):
    """the (family, geometry, epilogue) calls behind the file's keys, in file order of first appearance.  Epilogue: forward
    res*4 + act (field 15), data gradient res*16 + mask*8 + rowsum*4 + act (field 15), weight gradient the BatchNorm fold (field
    12 of the plan key; a geometry without a plan key is called unfolded — the implementation key does not carry the fold)."""
    calls, seen, wg_geoms, wg_folds = [], set(), [], {}
    for r in rows:
        fam, geom = FAMILY_OF[r[0]], tuple(r[1:12])
        if fam == "wgrad":
            if geom not in wg_folds:
                wg_folds[geom] = set()
                wg_geoms.append(geom)
            if r[0] == 256:
                wg_folds[geom].add(r[12])
            continue
        c = (fam, geom, r[15])
        if c not in seen:
            seen.add(c)
            calls.append(c)
    for geom in wg_geoms:
        for fold in sorted(wg_folds[geom] or {0}):
            calls.append(("wgrad", geom, fold))
    return calls


@pytest.mark.parametrize("geom", [(2, 5, 7, 6, 4, 3, 3, 1, 1, 1, 1),        # 3x3 / stride 1 / pad 1
                                  (3, 4, 10, 9, 6, 4, 4, 2, 2, 1, 1),       # strided 4x4, odd width (an uncovered column)
                                  (2, 8, 5, 3, 7, 1, 1, 1, 1, 0, 0)])       # 1x1
def test_fp64_reference_matches_cpu_autograd(dev, geom):
    """the device references of the sweep equal torch's CPU conv2d and its autograd gradients in fp64 (1e-12 relative), and their
    absolute-value contractions equal the same convolutions of |x|, |w|, |dy|"""
    N, C, H, W, K, KH, KW, SH, SW, PH, PW = geom
    g = torch.Generator().manual_seed(7 + C)
    x = torch.randn(N, C, H, W, generator=g, dtype=torch.float64)
    w = torch.randn(K, C, KH, KW, generator=g, dtype=torch.float64)
    P, Q = _out_hw(H, W, KH, KW, SH, SW, PH, PW)
    dy = torch.randn(N, K, P, Q, generator=g, dtype=torch.float64)
    xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    y = F.conv2d(xr, wr, stride=(SH, SW), padding=(PH, PW))
    y.backward(dy)
    ya = F.conv2d(x.abs(), w.abs(), stride=(SH, SW), padding=(PH, PW))
    dxa = torch.nn.grad.conv2d_input(x.shape, w.abs(), dy.abs(), stride=(SH, SW), padding=(PH, PW))
    dwa = torch.nn.grad.conv2d_weight(x.abs(), w.shape, dy.abs(), stride=(SH, SW), padding=(PH, PW))
    got = {"fwd": ref_fwd(x.to(dev), w.to(dev), (SH, SW), (PH, PW)),
           "dgrad": ref_dgrad(dy.to(dev), w.to(dev), (H, W), (SH, SW), (PH, PW)),
           "wgrad": ref_wgrad(x.to(dev), dy.to(dev), (KH, KW), (SH, SW), (PH, PW))}
    want = {"fwd": (y.detach(), ya), "dgrad": (xr.grad, dxa), "wgrad": (wr.grad, dwa)}
    for name in got:
        for part, v, r in zip(("value", "abs"), got[name], want[name]):
            v = v.cpu()
            assert v.shape == r.shape, (name, part)
            err = (v - r).abs().max().item()
            assert err <= 1e-12 * r.abs().max().item(), "%s %s: %.3e" % (name, part, err)


def _sweep_fwd(sw, lib, dev, stream, geom, epis, gen):
    N, C, H, W, K, KH, KW, SH, SW, PH, PW = geom
    P, Q = _out_hw(H, W, KH, KW, SH, SW, PH, PW)
    x = torch.randn(N, C, H, W, device=dev, generator=gen)
    w = torch.randn(K, C, KH, KW, device=dev, generator=gen) / math.sqrt(C * KH * KW)
    wk = w.permute(0, 2, 3, 1).reshape(K, KH * KW, C).contiguous() if (KH * KW > 1 and C % 16 == 0) else None
    scale = torch.rand(K, device=dev, generator=gen) + 0.5
    shift = torch.randn(K, device=dev, generator=gen) * 0.1
    acc, acc_abs = ref_fwd(x.double(), w.double(), (SH, SW), (PH, PW))
    ws = _workspace(lib.rg_conv2d_fwd_workspace(N, C, K, KH, KW, P, Q), dev)
    buf, y, guard = _nan_buffer(N * K * P * Q, dev)
    y = y.view(N, K, P, Q)
    sc, sh = scale.double().view(1, K, 1, 1), shift.double().view(1, K, 1, 1)
    for epi in epis:
        act, has_res = epi & 3, epi >> 2
        res = torch.randn(N, K, P, Q, device=dev, generator=gen) if has_res else None
        ref = acc * sc + sh
        mag = acc_abs * sc.abs() + sh.abs()
        if res is not None:
            ref += res.double()
            mag += res.double().abs()
        if act == 1:
            ref.clamp_(min=0.0)
        elif act == 2:
            ref = torch.where(ref > 0, ref, ref * SLOPE)
        else:
            assert act == 0, epi
        tol = mag.mul_(TOL).add_(TINY)

        def launch():
            buf.fill_(math.nan)
            if ws is not None:
                ws.fill_(math.nan)
            lib.rg_conv2d_fwd(x.data_ptr(), w.data_ptr(), None if wk is None else wk.data_ptr(), y.data_ptr(), N, C, H, W, K, KH,
                              KW, SH, SW, PH, PW, P, Q, scale.data_ptr(), shift.data_ptr(), None if res is None else res.data_ptr(),
                              act, SLOPE, None if ws is None else ws.data_ptr(), 0 if ws is None else ws.numel() * 4, stream)

        sw.sweep("fwd", "%s epi %d" % (geom, epi), launch, lambda: {"fwd": _guard_ok(_ratio(y, ref, tol), guard)})
        del ref, tol, mag


def _sweep_dgrad(sw, lib, dev, stream, geom, epis, gen):
    N, C, H, W, K, KH, KW, SH, SW, PH, PW = geom
    P, Q = _out_hw(H, W, KH, KW, SH, SW, PH, PW)
    dy = torch.randn(N, K, P, Q, device=dev, generator=gen)
    w = torch.randn(K, C, KH, KW, device=dev, generator=gen) / math.sqrt(K * KH * KW)
    wk = w.permute(0, 2, 3, 1).reshape(K, KH * KW, C).contiguous() if (KH * KW > 1 and C % 4 == 0) else None
    acc, acc_abs = ref_dgrad(dy.double(), w.double(), (H, W), (SH, SW), (PH, PW))
    ws = _workspace(lib.rg_conv2d_dgrad_workspace(N, C, H, W, K, KH, KW, SH, SW), dev)
    buf, dx, guard = _nan_buffer(N * C * H * W, dev)
    dx = dx.view(N, C, H, W)
    for epi in epis:
        act, want_rs, has_mask, has_res = epi & 3, (epi >> 2) & 1, (epi >> 3) & 1, epi >> 4
        assert act == 0, "the sweep reproduces data-gradient epilogues without activation (key %d)" % epi
        res = torch.randn(N, C, H, W, device=dev, generator=gen) if has_res else None
        mask = torch.randn(N, C, H, W, device=dev, generator=gen) if has_mask else None
        ref, mag = acc.clone(), acc_abs.clone()
        if res is not None:
            ref += res.double()
            mag += res.double().abs()
        if mask is not None:
            keep = mask > 0
            ref.mul_(keep)
            mag.mul_(keep)
        cols = 0
        rs = None
        if want_rs:
            cols = lib.rg_conv2d_dgrad_rowsum_cols(N, C, H, W, K, KH, KW, SH, SW, PH, PW, P, Q)
            assert cols > 0, ("a row-sum key for a launch without row sums", geom, epi)
            rs = torch.empty(C, cols, dtype=torch.float32, device=dev)
            rs_ref = ref.sum((0, 2, 3))
            rs_tol = mag.sum((0, 2, 3)).mul_(TOL).add_(TINY)
        tol = mag.mul_(TOL).add_(TINY)

        def launch():
            buf.fill_(math.nan)
            if ws is not None:
                ws.fill_(math.nan)
            if rs is not None:
                rs.fill_(math.nan)
            lib.rg_conv2d_dgrad(dy.data_ptr(), w.data_ptr(), None if wk is None else wk.data_ptr(), dx.data_ptr(), N, C, H, W, K, KH,
                                KW, SH, SW, PH, PW, P, Q, None, None, None if res is None else res.data_ptr(), act, SLOPE,
                                None if mask is None else mask.data_ptr(), None if rs is None else rs.data_ptr(), cols,
                                None if ws is None else ws.data_ptr(), 0 if ws is None else ws.numel() * 4, stream)

        def check():
            out = {"dgrad": _guard_ok(_ratio(dx, ref, tol), guard)}
            if rs is not None:
                out["dgrad row sums"] = _ratio(rs.double().sum(1), rs_ref, rs_tol)
            return out

        sw.sweep("dgrad", "%s epi %d" % (geom, epi), launch, check)
        del ref, tol, mag


def _sweep_wgrad(sw, lib, dev, stream, geom, folds, gen):
    N, C, H, W, K, KH, KW, SH, SW, PH, PW = geom
    P, Q = _out_hw(H, W, KH, KW, SH, SW, PH, PW)
    x = torch.randn(N, C, H, W, device=dev, generator=gen)
    dy = torch.randn(N, K, P, Q, device=dev, generator=gen) / math.sqrt(N * P * Q)
    G, G_abs = ref_wgrad(x.double(), dy.double(), (KH, KW), (SH, SW), (PH, PW))
    ws = _workspace(max(lib.rg_conv2d_wgrad_workspace(N, C, K, KH, KW, P, Q), 1 << 20), dev)
    buf, dw, guard = _nan_buffer(K * C * KH * KW, dev)
    dw = dw.view(K, C, KH, KW)
    for fold in folds:
        if not fold:
            ref, tol = G, G_abs * TOL + TINY

            def launch():
                buf.fill_(math.nan)
                ws.fill_(math.nan)
                lib.rg_conv2d_wgrad(x.data_ptr(), dy.data_ptr(), dw.data_ptr(), N, C, H, W, K, KH, KW, SH, SW, PH, PW, P, Q,
                                    ws.data_ptr(), ws.numel() * 4, stream)

            sw.sweep("wgrad", "%s" % (geom,), launch, lambda: {"wgrad": _guard_ok(_ratio(dw, ref, tol), guard)})
            continue
        # folded frozen-statistics BatchNorm: dw = scale G, dgamma = invstd (sum_m w G - mean sum_g), dbeta = sum_g (slice partials)
        nsl = 8
        wf = torch.randn(K, C, KH, KW, device=dev, generator=gen) / math.sqrt(C * KH * KW)
        scale = torch.rand(K, device=dev, generator=gen) + 0.5
        invstd = torch.rand(K, device=dev, generator=gen) + 0.5
        mean = torch.randn(K, device=dev, generator=gen) * 0.3
        partials = torch.randn(K, nsl, device=dev, generator=gen)
        dgamma = torch.empty(K, dtype=torch.float32, device=dev)
        dbeta = torch.empty(K, dtype=torch.float32, device=dev)
        sc, inv, mu, pt = scale.double(), invstd.double(), mean.double(), partials.double()
        ref = G * sc.view(K, 1, 1, 1)
        tol = G_abs * (sc.view(K, 1, 1, 1) * TOL) + TINY
        sum_g = pt.sum(1)
        wm, g2, ga2 = wf.double().reshape(K, -1), G.reshape(K, -1), G_abs.reshape(K, -1)
        dg_ref = inv * ((wm * g2).sum(1) - mu * sum_g)
        dg_tol = inv * ((wm.abs() * ga2).sum(1) + mu.abs() * pt.abs().sum(1)) * TOL + TINY
        db_tol = pt.abs().sum(1) * TOL + TINY

        def launch():
            buf.fill_(math.nan)
            ws.fill_(math.nan)
            dgamma.fill_(math.nan)
            dbeta.fill_(math.nan)
            lib.rg_conv2d_wgrad_fold(x.data_ptr(), dy.data_ptr(), dw.data_ptr(), N, C, H, W, K, KH, KW, SH, SW, PH, PW, P, Q,
                                     wf.data_ptr(), scale.data_ptr(), invstd.data_ptr(), mean.data_ptr(), None, partials.data_ptr(),
                                     nsl, dbeta.data_ptr(), dgamma.data_ptr(), ws.data_ptr(), ws.numel() * 4, stream)

        sw.sweep("wgrad", "%s fold" % (geom,), launch,
                 lambda: {"wgrad": _guard_ok(_ratio(dw, ref, tol), guard), "wgrad fold dgamma": _ratio(dgamma, dg_ref, dg_tol),
                          "wgrad fold dbeta": _ratio(dbeta, sum_g, db_tol)})


def test_every_candidate_at_bench_geometries(dev):
    lib = _lib()
    rows = _choice_rows()
    calls = _calls(rows)
    stats_before = lib.rg_conv_tune_stats(None)
    stream = torch.cuda.current_stream().cuda_stream
    sw = _Sweep(lib)
    lib.rg_conv_pick_log(None, 0)
    groups = {}
    for fam, geom, epi in calls:
        groups.setdefault((fam, geom), []).append(epi)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    try:
        for kind in ALL_KINDS:
            assert lib.rg_conv_set_pick(kind, 0) == -1, "a kind was pinned before the sweep"
        for i, ((fam, geom), epis) in enumerate(groups.items()):
            gen = torch.Generator(device=dev).manual_seed(1000 + i)
            {"fwd": _sweep_fwd, "dgrad": _sweep_dgrad, "wgrad": _sweep_wgrad}[fam](sw, lib, dev, stream, geom, epis, gen)
    finally:
        for kind in ALL_KINDS:
            lib.rg_conv_set_pick(kind, -1)
        lib.rg_conv_pick_log(None, 0)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    print("\nconv candidate sweep: %.1f s, %d geometries" % (wall, len({g for _, g, _ in calls})))
    for fam in ("fwd", "dgrad", "wgrad"):
        print("  %-5s %3d calls, %5d candidates" % (fam, sw.calls[fam], sw.count[fam]))
    for name in sorted(sw.worst):
        print("  worst |out - ref| / (2^-20 |a|(*)|b|)  %-18s %.4f  (2^%.1f)"
              % (name, sw.worst[name], math.log2(sw.worst[name]) if sw.worst[name] > 0 else -math.inf))
    assert not sw.bad, "%d candidates exceed the per-element bound:\n%s" % (len(sw.bad), "\n".join(sw.bad[:40]))
    # every recorded choice of the bench's file is a key this library builds, and names one of its candidates
    missing = [r for r in rows if tuple(r[:16]) not in sw.keys]
    assert not missing, "%d choice-file keys were not built by the sweep: %s" % (len(missing), missing[:5])
    beyond = [r for r in rows if r[16] >= sw.keys[tuple(r[:16])]]
    assert not beyond, "choice-file indices beyond the candidate count: %s" % beyond[:5]
    # the pinned runs measured and recorded nothing that later calls (tests, the bench) could see
    assert lib.rg_conv_tune_stats(None) == stats_before
    assert wall < 120.0, "the sweep took %.1f s" % wall
