"""The host model of the cascade's second stage (tests/cascade_hostmodel.py) against what it restates: the oracle's
OEltwiseSubEmbed in float64 (pair logits and scores), the oracle's o_cascade_second_stage (the merge), float32 torch (the
calibration of the budget constant), the planted defects the comparisons must catch, and the host side of the feature that needs
no GPU: the header's prototypes, the dispatch mirror, the wrappers' refusals and `reid.evaluators` without a reference tree."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import ref_torch as O
from tests import cascade_hostmodel as H

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = H.pair_cases()


def _id(c):
    return "Q%d-G%d-k%d-D%d-C%d-%s%s" % (c.Q, c.G, c.k, c.D, c.C, c.planted, "" if c.bias else "-nobias")


def _oracle_embed(inp, dtype=torch.float64):
    D, C = inp["probe"].shape[1], inp["W"].shape[0]
    m = O.OEltwiseSubEmbed(use_batch_norm=True, use_classifier=True, num_features=D, num_classes=C).to(dtype).eval()
    m.bn.eps = H.vh._f32(inp["eps"])
    with torch.no_grad():
        m.bn.weight.copy_(inp["gamma"]), m.bn.bias.copy_(inp["beta"])
        m.bn.running_mean.copy_(inp["rm"]), m.bn.running_var.copy_(inp["rv"])
        m.classifier.weight.copy_(inp["W"])
        m.classifier.bias.copy_(inp["bias"]) if inp["bias"] is not None else m.classifier.bias.zero_()
    return m


def _close(a, b, what, tol):
    a, b = torch.as_tensor(a).double().reshape(-1), torch.as_tensor(b).double().reshape(-1)
    err = float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))
    assert err <= tol, "%s: relative distance %.3e" % (what, err)


def test_the_case_table_holds_what_the_device_test_needs():
    shapes = {(c.Q, c.G, c.k, c.D, c.C) for c in CASES}
    for D in H.SWEEP_D:
        assert (3, 9, 5, D, 2) in shapes
    for k in H.SWEEP_K:
        assert (3, 9, k, 64, 2) in shapes
    for C in H.SWEEP_C:
        assert (3, 9, 5, 64, C) in shapes
    for Q in H.SWEEP_Q:
        assert (Q, 40, 6, 64, 2) in shapes
    assert H.BIG in shapes
    assert {c.planted for c in CASES} >= set(H.PLANTED) and any(not c.bias for c in CASES)
    # every combination of the two regime bits has a shape, and the mirror gives what the table names
    assert sorted(set(H.REGIME_SHAPES.values())) == list(range(4))
    for shape, bits in H.REGIME_SHAPES.items():
        Q, G, k, D, C = shape
        assert H.regime(Q, k, D, C) == bits, shape
    # both grid shapes of the Q sweep
    assert H.regime(1, 6, 64, 2) & H.SPLIT_K and H.regime(2, 6, 64, 2) & H.SPLIT_K and not H.regime(300, 6, 64, 2) & H.SPLIT_K


def test_the_indices_hold_the_planted_entries():
    for case in CASES:
        inp = H.case_input(case)
        idx = inp["idx"].long()
        assert int(idx.min()) >= 0 and int(idx.max()) < case.G
        assert all(len(set(r.tolist())) == case.k for r in idx), "a row repeats an index: %s" % (case,)
        assert (idx == 0).any() and ((idx == case.G - 1).any() or (case.k == 1 and case.Q == 1))
        if case.Q >= 2 and case.k >= 2:
            assert int((idx[:, 0] == 0).sum()) == case.Q                 # one gallery row under several queries
        if case.planted is None and (case.k >= 2 or case.Q == 1):
            assert torch.equal(inp["probe"][case.Q - 1], inp["gallery"][0])    # a query equal to a gallery row it lists: d == 0


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_model_is_the_oracle_embedding_in_float64(case):
    inp = H.case_input(case)
    m = _oracle_embed(inp)
    ref = H.pair_refs(inp)
    with torch.no_grad():
        for q in range(case.Q):                                          # the oracle's call: a [1, D] probe broadcast against [k, D]
            g = inp["gallery"][inp["idx"][q].long()].double()
            l = m(inp["probe"][q].double().view(1, -1), g)
            tol = 1e-6 if case.planted in ("bigmean", "var0") else 1e-9     # float64 itself cancels there
            _close(ref["logits"].value[q], l, "logits of query %d" % q, tol)
            if case.planted not in ("far_low",):                         # a score of e^-200: compared below, absolutely
                _close(ref["score"].value[q], F.softmax(l, dim=1)[:, 0], "score of query %d" % q, tol)
            assert float((ref["score"].value[q] - F.softmax(l, dim=1)[:, 0]).abs().max()) <= 1e-9
    assert bool(torch.isfinite(ref["score"].value).all()) and bool((ref["score"].M >= 0).all())
    if case.planted == "ties":
        assert bool((ref["score"].value == 1.0 / case.C).all()), "the ties case does not tie"
    if case.planted in ("far_low", "far_high"):
        l = ref["logits"].value
        assert float((l.max(2).values - l.min(2).values).min()) > 190.0


def _f32_ratios(case):
    inp = H.case_input(case)
    ref = H.pair_refs(inp)
    l32, s32 = H.pair_values(inp, torch.float32)
    return {k: H.compare(v, ref[k], H.C_KIND).ratio for k, v in (("logits", l32), ("score", s32))}


def test_float32_torch_lies_within_a_quarter_of_every_budget():
    """the calibration of C_KIND (the module docstring): C_KIND = max(8, 4 x the float32 torch ratio)"""
    torch.set_num_threads(1)
    worst = {}
    for case in CASES + [H.PairCase(*s, None, True) for s in H.ORDER_CASES]:
        for k, r in _f32_ratios(case).items():
            worst[k] = max(worst.get(k, 0.0), r)
    print("float32 torch ratios:", {k: round(v, 2) for k, v in sorted(worst.items())})
    for k, r in worst.items():
        assert r <= H.C_KIND[k] / 4.0 + 1e-9, "%s: float32 torch ratio %.2f, C_KIND %.2f" % (k, r, H.C_KIND[k])
    assert H.C_KIND["score"] >= H.C_KIND["logits"]          # the score budget carries the logit errors at the logits' constant


@pytest.mark.parametrize("defect", H.DEFECTS)
def test_planted_pair_defect_is_caught(defect):
    case = H.PairCase(3, 9, 5, 65, 3, "var0" if defect == "no_eps" else None, True)
    inp = H.case_input(case)
    ref = H.pair_refs(inp)
    bl, bs = H.pair_values(inp, defect=defect)
    sl, ss = H.pair_values(inp)
    assert H.compare(sl, ref["logits"], H.C_KIND).ok and H.compare(ss, ref["score"], H.C_KIND).ok
    assert not H.compare(bs, ref["score"], H.C_KIND).ok, "%s passes the comparison of the scores" % defect
    if defect != "class1":
        assert not H.compare(bl, ref["logits"], H.C_KIND).ok, "%s passes the comparison of the logits" % defect


def test_every_case_keeps_its_undecided_rows_under_the_cap():
    """the ordering check of the device test asks something: in every ordering case the model alone decides at least seven rows
    in eight, and the float32 torch scores order the decided rows as the model does"""
    for shape in H.ORDER_CASES:
        inp = H.make_input(*shape)
        ref = H.pair_refs(inp)["score"]
        dec = H.decided_rows(ref)
        und = int((~dec).sum())
        print(shape, "undecided rows:", und, "score range %.3f .. %.3f" % (float(ref.value.min()), float(ref.value.max())))
        assert und * H.UNDECIDED_CAP <= dec.numel(), "%s: %d of %d rows undecided" % (shape, und, dec.numel())
        assert H.check_order(H.pair_values(inp, torch.float32)[1], ref, str(shape)) == und
        # a row whose order is wrong is caught: swap the two best-separated neighbours of a decided row
        q = int(torch.nonzero(dec)[0])
        bad = ref.value.clone()
        o = torch.argsort(bad[q])
        bad[q, o[0]], bad[q, o[1]] = ref.value[q, o[1]], ref.value[q, o[0]]
        with pytest.raises(AssertionError):
            H.check_order(bad, ref, "swapped")


# ---- the merge -------------------------------------------------------------------------------------------------------------------
def _ulp32(v):
    v = np.abs(np.asarray(v, dtype=np.float32))
    return (np.nextafter(v, np.float32(np.inf)) - v).astype(np.float64)


@pytest.mark.parametrize("shape", [(7, 40, 6, 64, 2), (5, 33, 4, 100, 2), (3, 12, 11, 16, 3)], ids=str)
def test_merge_model_is_the_oracle_second_stage(shape):
    """k < G.  The model is handed the oracle's own scores (rounded to float32, as the reference's matrix holds them) and the
    oracle's stable argsort; every entry then equals the oracle's float64 `gap` arithmetic to one float32 ulp of the entry"""
    Q, G, k, D, C = shape
    inp = H.make_input(*shape)
    m = _oracle_embed(inp, torch.float32)
    probe, gal = inp["probe"], inp["gallery"]
    dist = O.o_pairwise_distance(probe, gal)
    fn = lambda x: F.softmax(x, dim=1)[:, 0]         # noqa: E731
    ref = O.o_cascade_second_stage(dist, probe, gal, m, k, fn)
    order = np.argsort(dist.numpy(), axis=1, kind="stable")[:, :k]
    score = ref[np.arange(Q)[:, None], order]                              # what the oracle wrote into the top-k columns
    got = H.merge_model(dist.numpy(), order, score)
    assert got.dtype == np.float32 and ref.dtype == np.float32
    assert (np.abs(got.astype(np.float64) - ref.astype(np.float64)) <= _ulp32(ref)).all()
    assert (got[np.arange(Q)[:, None], order] == score).all()


@pytest.mark.parametrize("shape", H.MERGE_SHAPES[:4], ids=str)
@pytest.mark.parametrize("planted", [None, "gap0", "inf", "descending"])
def test_merge_model_properties(shape, planted):
    Q, G, k = shape
    dist, idx, score = H.merge_input(Q, G, k, planted=planted)
    got = H.merge_model(dist, idx, score)
    rows = np.arange(Q)[:, None]
    assert (got[rows, idx] == score).all()
    inside = np.zeros((Q, G), dtype=bool)
    inside[rows, idx] = True
    if k == G:
        return
    if planted == "gap0":
        assert (got[~inside] == dist[~inside]).all()                        # the gap is exactly 0: nothing outside moves
    else:
        # every entry outside ranks behind every entry inside, by at least 1 up to one rounding
        assert (got.min(axis=1, where=~inside, initial=np.inf) >= score.max(axis=1) + 1.0 - 1e-6).all()
    if planted == "inf":
        assert np.isinf(got[~inside]).any() and not np.isnan(got).any()


@pytest.mark.parametrize("defect", H.MERGE_DEFECTS)
def test_planted_merge_defect_is_caught(defect):
    # scores above some of the outside distances, so that reading nxt after the overwrite reads another entry
    dist, idx, score = H.merge_input(3, 33, 4)
    score = (score * 3.0 + 1.0).astype(np.float32)
    good, bad = H.merge_model(dist, idx, score), H.merge_model(dist, idx, score, defect=defect)
    assert not np.array_equal(good, bad), "%s leaves the merged matrix unchanged" % defect


# ---- host side of the feature ----------------------------------------------------------------------------------------------------
def test_header_declares_the_entry_points():
    from rg_hip.lib import parse_header
    protos = parse_header()
    assert protos["rg_pair_score_regime"][0] == "int64_t" and protos["rg_pair_score"][0] == "int" and protos["rg_cascade_merge"][0] == "int"
    assert [n for _, n in protos["rg_pair_score"][1]] == ["probe", "gallery", "idx", "gamma", "beta", "running_mean", "running_var", "W",
                                                          "bias", "logits", "score", "Q", "G", "k", "D", "C", "eps", "stream"]
    assert [(t, n) for t, n in protos["rg_cascade_merge"][1]] == [("float*", "dist"), ("int64_t", "ld"), ("const int*", "idx"),
                                                                  ("const float*", "score"), ("int", "Q"), ("int", "G"), ("int", "k"),
                                                                  ("rg_stream_t", "stream")]


def test_regime_query_matches_the_mirror():
    from rg_hip import ops
    for c in CASES:
        for aligned in (True, False):
            assert ops.pair_score_regime(c.Q, c.k, c.D, c.C, aligned) == H.regime(c.Q, c.k, c.D, c.C, aligned), c
    assert ops.pair_score_regime(3368, 100, 2048, 2) == H.VEC4
    assert ops.pair_score_regime(3, 5, 8193, 2) == -1 and ops.pair_score_regime(3, 5, 64, 17) == -1


def test_library_refuses_bad_arguments_before_any_launch():
    from rg_hip.lib import lib
    ok = dict(probe=16, gallery=16, idx=16, gamma=16, beta=16, rm=16, rv=16, W=16, bias=0, logits=0, score=16)

    def call(Q=3, G=9, k=5, D=64, C=2, **ptr):
        a = dict(ok, **ptr)
        return lib.rg_pair_score(a["probe"], a["gallery"], a["idx"], a["gamma"], a["beta"], a["rm"], a["rv"], a["W"], a["bias"] or None,
                                 a["logits"] or None, a["score"] or None, Q, G, k, D, C, 1e-5, None)
    for kw in (dict(score=0), dict(C=17), dict(C=0), dict(D=8193), dict(D=0), dict(k=10), dict(k=0), dict(Q=0), dict(probe=0)):
        with pytest.raises(RuntimeError, match="rg_pair_score"):
            call(**kw)
    for Q, G, k, ld in ((0, 9, 5, 9), (3, 9, 10, 9), (3, 9, 0, 9), (3, 9, 5, 8), (3, (1 << 20) + 1, 5, (1 << 20) + 1)):
        with pytest.raises(RuntimeError, match="rg_cascade_merge"):
            lib.rg_cascade_merge(16, ld, 16, 16, Q, G, k, None)


def test_wrappers_refuse_host_tensors_and_bad_shapes():
    from rg_hip import ops
    inp = H.make_input(3, 9, 5, 64, 2)
    with pytest.raises((RuntimeError, TypeError, ValueError)):
        ops.pair_score(inp["probe"], inp["gallery"], inp["idx"], inp["gamma"], inp["beta"], inp["rm"], inp["rv"], inp["W"], inp["bias"], 1e-5)
    with pytest.raises(ValueError):
        ops.cascade_merge(torch.zeros(3, 9), inp["idx"], torch.zeros(3, 5))


def test_evaluators_import_and_names_without_a_reference_tree():
    code = ("import sys, inspect, torch\n"
            "import reid.evaluators as E\n"
            "assert not hasattr(E, 'evaluate_all') and not hasattr(E, 'extract_features'), 'a reference tree is on the path'\n"
            "sig = inspect.signature(E.DeviceCascadeEvaluator.evaluate)\n"
            "assert str(sig) == str(inspect.signature(E.CascadeEvaluator.evaluate)), sig\n"
            "assert list(inspect.signature(E.evaluate_all_device).parameters) == ['distmat', 'query', 'gallery', 'query_ids', "
            "'gallery_ids', 'query_cams', 'gallery_cams', 'cmc_topk', 'dataset', 'top1']\n"
            "x = torch.tensor([[1.0, 2.0, 0.5], [0.0, 0.0, 0.0]])\n"
            "assert torch.equal(E.softmax_class0(x), torch.nn.functional.softmax(x, dim=1)[:, 0])\n"
            "ev = E.DeviceCascadeEvaluator(None, None)\n"
            "assert ev.embed_dist_fn is E.softmax_class0 and not ev.fusable(2048)\n"
            "print('IMPORT-OK')\n")
    env = dict(os.environ)
    env["PYTHONPATH"] = os.path.join(REPO, "reid-gan_amd")
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "IMPORT-OK" in out.stdout, out.stdout + out.stderr
