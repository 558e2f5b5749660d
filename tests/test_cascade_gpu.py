"""GPU: the second stage of the cascade evaluation — csrc/cascade.hip through the C ABI and `ops.pair_score` /
`ops.cascade_merge`, per element against tests/cascade_hostmodel.py (every element compared, outputs between guard rows, the launch
regime of every shape asserted), the order inside the top-k, the merge bit for bit against the float32 model, and
`reid.evaluators.DeviceCascadeEvaluator` (second_stage_device on its three paths, evaluate on a synthetic loader).

Each per-element check prints `RATIO <output> <case> <max err / (2^-24 M)>` (pytest -s shows them)."""
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import ref_torch as O
from tests import cascade_hostmodel as H
from tests import head_hostmodel as HH
from tests import rank_eval_hostmodel as RH
from tests import verif_hostmodel as VH
from tests.test_head_elementwise_gpu import _Out, _lib, _ptr, _st, _to

pytestmark = pytest.mark.gpu

CASES = H.pair_cases()
_REFS = {}


def _id(c):
    return "Q%d-G%d-k%d-D%d-C%d-%s%s" % (c.Q, c.G, c.k, c.D, c.C, c.planted, "" if c.bias else "-nobias")


def _case(case):
    """(inputs, references) of a case, computed once"""
    if case not in _REFS:
        inp = H.case_input(case)
        _REFS[case] = (inp, H.pair_refs(inp))
    return _REFS[case]


def _ops():
    from rg_hip import ops
    return ops


def _dev_inputs(dev, inp):
    names = ("probe", "gallery", "idx", "gamma", "beta", "rm", "rv", "W", "bias")
    return dict(zip(names, _to(dev, *(inp[n] for n in names))))


def _pair_score(d, eps, **kw):
    return _ops().pair_score(d["probe"], d["gallery"], d["idx"], d["gamma"], d["beta"], d["rm"], d["rv"], d["W"], d["bias"], eps, **kw)


def _check(got, ref, what):
    w = HH.compare(got, ref, H.C_KIND)
    assert w.ok, "%s: worst element %s err %.3e > budget %.3e (%s, max err/(2^-24 M) = %.2f)" % (
        what, w.index, w.err, w.budget, ref.kind, w.ratio)
    print("RATIO %s %.3f" % (what, w.ratio))


# ---- rg_pair_score ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_pair_score_per_element(dev, case):
    """logits and score of every pair against the fp64 model, through the C ABI onto guarded outputs; the launch regime is the one
    the table names; the wrapper returns the same bytes; one output alone (the other NULL) returns the same bytes too"""
    inp, ref = _case(case)
    d = _dev_inputs(dev, inp)
    Q, G, k, D, C = case.Q, case.G, case.k, case.D, case.C
    ops = _ops()
    want = H.REGIME_SHAPES.get((Q, G, k, D, C))
    got_regime = ops.pair_score_regime(Q, k, D, C)
    assert got_regime == H.regime(Q, k, D, C) and (want is None or got_regime == want), (got_regime, want)
    assert all(t is None or t.data_ptr() % 16 == 0 for t in d.values())
    logits, score = _Out((Q, k, C), dev), _Out((Q, k), dev)
    _lib().rg_pair_score(d["probe"].data_ptr(), d["gallery"].data_ptr(), d["idx"].data_ptr(), d["gamma"].data_ptr(), d["beta"].data_ptr(),
                         d["rm"].data_ptr(), d["rv"].data_ptr(), d["W"].data_ptr(), _ptr(d["bias"]), logits.ptr, score.ptr, Q, G, k, D, C,
                         inp["eps"], _st())
    tag = _id(case)
    logits.guards("logits | " + tag), score.guards("score | " + tag)
    _check(logits.t, ref["logits"], "logits " + tag)
    _check(score.t, ref["score"], "score " + tag)
    assert bool(torch.isfinite(score.t).all()) and bool(((score.t >= 0) & (score.t <= 1)).all())
    if case.planted == "ties":
        assert bool((score.t == torch.tensor(1.0 / C, dtype=torch.float32)).all()), "tied logits must score exactly 1 / C"
    if C == 1:
        assert bool((score.t == 1.0).all())
    l2, s2 = _pair_score(d, inp["eps"], want_logits=True, want_score=True)
    assert torch.equal(l2, logits.t) and torch.equal(s2, score.t)
    l3, none = _pair_score(d, inp["eps"], want_logits=True, want_score=False)
    none2, s3 = _pair_score(d, inp["eps"])
    assert none is None and none2 is None and torch.equal(l3, logits.t) and torch.equal(s3, score.t)


@pytest.mark.parametrize("shape", [(3, 9, 5, 64, 2), (3, 9, 5, 257, 3), H.BIG, (3, 9, 5, 1000, 16)], ids=str)
def test_pair_logits_agree_with_the_verification_head_on_the_expanded_pairs(dev, shape):
    """the same pairs, expanded and gathered on the host, through ops.verif_head_fwd(train=False): both results lie within their
    budget of the fp64 value, so they agree to the sum of both budgets"""
    case = H.PairCase(*shape, None, True)
    inp, ref = _case(case)
    d = _dev_inputs(dev, inp)
    e = H.expanded(inp)
    x1, x2 = _to(dev, e["x1"], e["x2"])
    rm, rv = d["rm"].clone(), d["rv"].clone()
    head = _ops().verif_head_fwd(x1, x2, d["gamma"], d["beta"], rm, rv, d["W"], d["bias"], None, False, inp["eps"], VH.MOM)[0]
    mine, _ = _pair_score(d, inp["eps"], want_logits=True, want_score=False)
    M = ref["logits"].M.reshape(-1, case.C)
    bud = (H.C_KIND["logits"] + VH.C_KIND["logits"]) * HH.U24 * (M + HH.TINY_M)
    err = (mine.view(-1, case.C).double().cpu() - head.double().cpu()).abs()
    assert bool((err <= bud).all()), "worst err / budget %.3f" % float((err / bud).max())


@pytest.mark.parametrize("shape", H.ORDER_CASES, ids=str)
def test_order_inside_the_topk_on_decided_rows(dev, shape):
    case = H.PairCase(*shape, None, True)
    inp, ref = _case(case)
    _, score = _pair_score(_dev_inputs(dev, inp), inp["eps"])
    _check(score, ref["score"], "score order-case " + str(shape))
    und = H.check_order(score, ref["score"], str(shape))
    print("ORDER %s undecided rows %d of %d" % (shape, und, case.Q))


def test_pair_score_refuses_bad_arguments(dev):
    inp, _ = _case(H.PairCase(3, 9, 5, 64, 2, None, True))
    d = _dev_inputs(dev, inp)
    ops = _ops()
    bad = [dict(d, idx=d["idx"].long()), dict(d, probe=d["probe"][:, :32]), dict(d, gallery=d["gallery"][:4]),
           dict(d, W=torch.zeros(17, 64, device=dev)), dict(d, gamma=d["gamma"][:10]), dict(d, probe=d["probe"].t().contiguous().t())]
    for b in bad:
        with pytest.raises((ValueError, TypeError)):
            _pair_score(b, inp["eps"])
    with pytest.raises(ValueError):
        _pair_score(d, inp["eps"], want_logits=False, want_score=False)
    with pytest.raises(ValueError):
        _pair_score(d, inp["eps"], chunk=0)
    with pytest.raises(ValueError):
        ops.cascade_merge(torch.zeros(3, 9, device=dev), d["idx"][:2], torch.zeros(3, 5, device=dev))
    with pytest.raises(ValueError):
        ops.cascade_merge(torch.zeros(3, 4, device=dev), d["idx"], torch.zeros(3, 5, device=dev))


# ---- rg_cascade_merge ------------------------------------------------------------------------------------------------------------
def _merge_on_device(dev, dist, idx, score, ld=None):
    Q, G = dist.shape
    ld = G if ld is None else ld
    buf = _Out((Q, ld), dev)
    buf.t[:, :G] = torch.from_numpy(dist).to(dev)
    out = _ops().cascade_merge(buf.t[:, :G], torch.from_numpy(idx).to(dev), torch.from_numpy(score).to(dev))
    assert out.data_ptr() == buf.t.data_ptr()
    buf.guards("merge")
    if ld > G:
        assert bool((buf.t[:, G:] == buf.fill).all()), "columns beyond G were written"
    return buf.t[:, :G].cpu().numpy()


@pytest.mark.parametrize("shape", H.MERGE_SHAPES, ids=str)
def test_cascade_merge_is_bit_equal_to_the_float32_model(dev, shape):
    Q, G, k = shape
    dist, idx, score = H.merge_input(Q, G, k)
    got = _merge_on_device(dev, dist, idx, score)
    assert np.array_equal(got, H.merge_model(dist, idx, score))


@pytest.mark.parametrize("planted", ["gap0", "inf", "descending", "ld"])
def test_cascade_merge_planted_rows(dev, planted):
    Q, G, k = 3, 33, 4
    dist, idx, score = H.merge_input(Q, G, k, planted=None if planted == "ld" else planted)
    got = _merge_on_device(dev, dist, idx, score, ld=G + 7 if planted == "ld" else None)
    want = H.merge_model(dist, idx, score)
    assert np.array_equal(got, want)
    if planted == "gap0":
        inside = np.zeros((Q, G), dtype=bool)
        inside[np.arange(Q)[:, None], idx] = True
        assert (got[~inside] == dist[~inside]).all()
    if planted == "inf":
        assert np.isinf(got).any() and not np.isnan(got).any()


# ---- DeviceCascadeEvaluator.second_stage_device ------------------------------------------------------------------------------------
def _embed(dev, inp, classifier=True):
    from reid.models.embedding import EltwiseSubEmbed
    D, C = inp["probe"].shape[1], inp["W"].shape[0]
    m = EltwiseSubEmbed(use_batch_norm=True, use_classifier=classifier, num_features=D, num_classes=C if classifier else 0)
    with torch.no_grad():
        m.bn.weight.copy_(inp["gamma"]), m.bn.bias.copy_(inp["beta"])
        m.bn.running_mean.copy_(inp["rm"]), m.bn.running_var.copy_(inp["rv"])
        if classifier:
            m.classifier.weight.copy_(inp["W"]), m.classifier.bias.copy_(inp["bias"])
    return m.to(dev).eval()


def _oracle_embed(inp, classifier=True):
    D, C = inp["probe"].shape[1], inp["W"].shape[0]
    m = O.OEltwiseSubEmbed(True, classifier, D, C if classifier else 0).double().eval()
    m.bn.eps = VH._f32(inp["eps"])
    with torch.no_grad():
        m.bn.weight.copy_(inp["gamma"]), m.bn.bias.copy_(inp["beta"])
        m.bn.running_mean.copy_(inp["rm"]), m.bn.running_var.copy_(inp["rv"])
        if classifier:
            m.classifier.weight.copy_(inp["W"]), m.classifier.bias.copy_(inp["bias"])
    return m


def _first_stage(dev, inp):
    from rg_hip import search
    probe, gal = _to(dev, inp["probe"], inp["gallery"])
    return search.dist_block(probe, gal, 1.0, True), probe, gal


@pytest.mark.parametrize("shape", H.ORDER_CASES, ids=str)        # k < G: the reference indexes out of range at k == G
def test_second_stage_device_is_topk_pair_score_merge_and_matches_the_oracle(dev, shape):
    from reid.evaluators import DeviceCascadeEvaluator, rank_topk, softmax_class0
    Q, G, k, D, C = shape
    inp = H.make_input(*shape)
    ev = DeviceCascadeEvaluator(None, _embed(dev, inp))
    assert ev.embed_dist_fn is softmax_class0
    d1, probe, gal = _first_stage(dev, inp)
    first = d1.clone()
    merged = ev.second_stage_device(d1, probe, gal, rerank_topk=k)
    assert merged.data_ptr() == d1.data_ptr() and ev.last_path == "score"
    # bit for bit: cascade_merge applied to the existing rank_topk and the kernel's own scores
    top = rank_topk(first, k).to(torch.int32)
    bn, fc = ev.embed_model.bn, ev.embed_model.classifier
    _, score = _ops().pair_score(probe, gal, top, bn.weight.detach(), bn.bias.detach(), bn.running_mean, bn.running_var,
                                 fc.weight.detach(), fc.bias.detach(), bn.eps)
    assert torch.equal(merged, _ops().cascade_merge(first.clone(), top, score))
    # the oracle in float64 on the float32 inputs
    p64, g64 = inp["probe"].double(), inp["gallery"].double()
    ref = O.o_cascade_second_stage(O.o_pairwise_distance(p64, g64), p64, g64, _oracle_embed(inp), k, lambda x: F.softmax(x, dim=1)[:, 0])
    order = np.argsort(O.o_pairwise_distance(p64, g64).numpy(), axis=1, kind="stable")[:, :k]
    assert np.array_equal(order, top.cpu().numpy()), "the first-stage ranking differs: the case is not separated enough"
    budgets = H.pair_refs(dict(inp, idx=top.cpu()))["score"]
    rows = np.arange(Q)[:, None]
    inside = HH.Ref(torch.from_numpy(ref[rows, order]), budgets.M, "score")
    _check(merged.cpu()[torch.from_numpy(rows), torch.from_numpy(order)], inside, "second stage top-k entries " + str(shape))
    mask = np.ones((Q, G), dtype=bool)
    mask[rows, order] = False
    got = merged.cpu().numpy()
    assert np.abs(got[mask] - ref[mask]).max(initial=0.0) <= 1e-4 * np.abs(ref).max()
    H.check_order(torch.from_numpy(got[rows, order]), inside, "second stage order " + str(shape))
    # and everything outside the top-k ranks behind it
    assert (got.min(axis=1, where=mask, initial=np.inf) > got[rows, order].max(axis=1)).all()


def test_second_stage_device_builds_no_pair_operand(dev):
    from reid.evaluators import DeviceCascadeEvaluator
    Q, G, k, D, C = 64, 256, 32, 2048, 2
    inp = H.make_input(Q, G, k, D, C)
    ev = DeviceCascadeEvaluator(None, _embed(dev, inp))
    d1, probe, gal = _first_stage(dev, inp)
    ev.second_stage_device(d1.clone(), probe, gal, rerank_topk=k)            # warm: library load, allocator pools
    torch.cuda.synchronize(dev)
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    ev.second_stage_device(d1, probe, gal, rerank_topk=k)
    torch.cuda.synchronize(dev)
    grown = torch.cuda.max_memory_allocated(dev) - base
    print("PEAK second_stage_device extra bytes %d (pair operand would be %d)" % (grown, Q * k * D * 4))
    assert grown < Q * k * D * 4 // 4


def test_custom_dist_fn_takes_the_logits_path(dev):
    from reid.evaluators import DeviceCascadeEvaluator
    shape = (7, 40, 6, 64, 2)
    inp = H.make_input(*shape)
    d1, probe, gal = _first_stage(dev, inp)
    fused = DeviceCascadeEvaluator(None, _embed(dev, inp))
    a = fused.second_stage_device(d1.clone(), probe, gal, rerank_topk=6)
    custom = DeviceCascadeEvaluator(None, _embed(dev, inp), lambda x: F.softmax(x, dim=1)[:, 0])
    b = custom.second_stage_device(d1.clone(), probe, gal, rerank_topk=6)
    assert fused.last_path == "score" and custom.last_path == "logits"
    from reid.evaluators import rank_topk
    top = rank_topk(d1, 6).cpu()
    ref = H.pair_refs(dict(inp, idx=top.to(torch.int32)))["score"]
    rows = torch.arange(7)[:, None]
    _check(b.cpu()[rows, top], ref, "logits path top-k entries")
    _check(a.cpu()[rows, top], ref, "score path top-k entries")


def test_a_model_the_kernel_does_not_cover_takes_the_composed_path_in_chunks(dev):
    from reid.evaluators import DeviceCascadeEvaluator
    Q, G, k, D = 7, 40, 6, 64
    inp = H.make_input(Q, G, k, D, 2)
    emb = _embed(dev, inp, classifier=False)                                  # x.sum(1): no classifier, nothing to fuse
    ev = DeviceCascadeEvaluator(None, emb, None)
    assert not ev.fusable(D)
    d1, probe, gal = _first_stage(dev, inp)
    one = ev.second_stage_device(d1.clone(), probe, gal, rerank_topk=k)
    assert ev.last_path == "composed" and ev.last_chunks == 1
    many = ev.second_stage_device(d1.clone(), probe, gal, rerank_topk=k, pair_bytes=2 * k * D * 4)      # two queries per chunk
    assert ev.last_path == "composed" and ev.last_chunks == 4
    assert torch.allclose(one, many, rtol=1e-5, atol=1e-6)
    p64, g64 = inp["probe"].double(), inp["gallery"].double()
    ref = O.o_cascade_second_stage(O.o_pairwise_distance(p64, g64), p64, g64, _oracle_embed(inp, classifier=False), k, None)
    assert np.abs(many.cpu().numpy() - ref).max() <= 1e-4 * np.abs(ref).max()


# ---- determinism -----------------------------------------------------------------------------------------------------------------
def test_scores_and_merge_are_byte_equal_across_runs_streams_and_chunkings(dev):
    for shape in [(5, 64, 16, 2048, 2), (300, 40, 6, 64, 2), (3, 9, 5, 1001, 16)]:
        inp = H.make_input(*shape)
        d = _dev_inputs(dev, inp)
        l0, s0 = _pair_score(d, inp["eps"], want_logits=True)
        l1, s1 = _pair_score(d, inp["eps"], want_logits=True)
        assert torch.equal(l0, l1) and torch.equal(s0, s1)
        for chunk in (1, 2, 7):                                              # other grids (Q per launch changes the k split)
            lc, sc = _pair_score(d, inp["eps"], want_logits=True, chunk=chunk)
            assert torch.equal(l0, lc) and torch.equal(s0, sc), (shape, chunk)
        dist = torch.rand(shape[0], shape[1], device=dev) + 0.5
        m0 = _ops().cascade_merge(dist.clone(), d["idx"], s0)
        m1 = _ops().cascade_merge(dist.clone(), d["idx"], s0)
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            ls, ss = _pair_score(d, inp["eps"], want_logits=True)
            ms = _ops().cascade_merge(dist.clone(), d["idx"], ss)
        side.synchronize()
        assert torch.equal(l0, ls) and torch.equal(s0, ss) and torch.equal(m0, m1) and torch.equal(m0, ms)


# ---- DeviceCascadeEvaluator.evaluate ---------------------------------------------------------------------------------------------
class _Flatten(torch.nn.Module):
    """stand-in base model: the 'images' ARE the features"""

    def forward(self, x):
        return x.flatten(1)


def _synthetic_set(D=64, seed=3):
    """3 identities: 5 query and 12 gallery images as (fname, pid, cam) triples, their features, and a loader of 4-tuple batches"""
    g = HH.gen(seed)
    centres = torch.randn(3, D, generator=g)
    query, gallery, feats = [], [], {}
    for i in range(5):
        query.append(("q%d.jpg" % i, i % 3, 0))
    for j in range(12):
        gallery.append(("g%d.jpg" % j, j % 3, 1 + j % 2))
    for name, pid, _ in query + gallery:
        feats[name] = (centres[pid] + 3.0 * torch.randn(D, generator=g)).float()      # first-stage mAP near 0.6: a ranking with errors
    names = [n for n, _, _ in query + gallery]
    pids = {n: p for n, p, _ in query + gallery}
    cams = {n: c for n, _, c in query + gallery}
    loader = []
    for b0 in range(0, len(names), 6):
        nb = names[b0:b0 + 6]
        loader.append((torch.stack([feats[n] for n in nb]).view(len(nb), D, 1, 1), nb, [pids[n] for n in nb], [cams[n] for n in nb]))
    return query, gallery, feats, loader


def test_device_cascade_evaluator_evaluate(dev, capsys):
    import reid.evaluators as E
    assert not hasattr(E, "evaluate_all") and not hasattr(E, "extract_features"), "a reference tree sits on sys.path"
    D, k = 64, 4
    query, gallery, feats, loader = _synthetic_set(D)
    inp = H.make_input(5, 12, k, D, 2, seed=1)
    ev = E.DeviceCascadeEvaluator(_Flatten(), _embed(dev, inp))
    qid, gid = [p for _, p, _ in query], [p for _, p, _ in gallery]
    qcam, gcam = [c for _, _, c in query], [c for _, _, c in gallery]

    def model_values(mat):
        npos, ap, first, hits = RH.per_query(mat, qid, gid, qcam, gcam, topk=100)
        return RH.summarize(npos, ap, first, hits)

    capsys.readouterr()
    top1, mAP = ev.evaluate(loader, query, gallery, rerank_topk=k, dataset="market1501")
    out = capsys.readouterr().out
    assert ev.last_path == "score"
    merged = ev.last_distmat.cpu().numpy()
    want_map, want_first, want_all = model_values(merged)
    assert abs(mAP - want_map) <= 1e-12 and abs(top1 - want_first[0]) <= 1e-12
    lines = out.splitlines()
    extract = [l for l in lines if l.startswith("Extract Features:")]
    assert len(extract) == len(loader)
    assert re.match(r"^Extract Features: \[1/3\]\tTime \d+\.\d{3} \(\d+\.\d{3}\)\tData \d+\.\d{3} \(\d+\.\d{3}\)\t$", extract[0]), repr(extract[0])
    rest = [l for l in lines if not l.startswith("Extract Features:")]
    assert rest[0] == "First stage evaluation:" and rest[1].startswith("Mean AP: ")
    assert rest[2] == "CMC Scores{:>12}".format("market1501")
    assert rest[6] == "Second stage evaluation:"
    assert rest[7] == "Mean AP: {:4.1%}".format(want_map)
    assert rest[8] == "CMC Scores{:>12}".format("market1501")
    assert rest[9:12] == ["  top-{:<4}{:12.1%}".format(t, want_first[t - 1]) for t in (1, 5, 10)] and len(rest) == 12
    # the second stage re-scored exactly the top-k columns of the first stage with the embedding network
    probe = torch.stack([feats[n] for n, _, _ in query]).to(dev)
    gal = torch.stack([feats[n] for n, _, _ in gallery]).to(dev)
    again = ev.second_stage_device(__import__("rg_hip").search.dist_block(probe, gal, 1.0, True), probe, gal, rerank_topk=k)
    assert torch.equal(again, ev.last_distmat)
    merged_dev = ev.last_distmat
    # top1=False returns the mAP alone; the first stage alone scores the first-stage matrix
    assert abs(ev.evaluate(loader, query, gallery, rerank_topk=k, top1=False) - want_map) <= 1e-12
    out = capsys.readouterr().out
    assert "CMC Scores" not in out and out.count("Mean AP: ") == 2
    m1 = ev.evaluate(loader, query, gallery, second_stage=False, top1=False)
    assert abs(m1 - model_values(ev.last_distmat.cpu().numpy())[0]) <= 1e-12
    assert 0.3 < m1 < 0.95 and m1 != want_map, "the synthetic set ranks trivially: the comparison above shows nothing"
    # dataset=None needs the cuhk03 column, which this build does not sample on the device: the refusal propagates
    with pytest.raises(NotImplementedError):
        ev.evaluate(loader, query, gallery, rerank_topk=k)
    # allshots, through evaluate_all_device with ids given directly
    capsys.readouterr()
    got = E.evaluate_all_device(merged_dev, query_ids=qid, gallery_ids=gid, query_cams=qcam, gallery_cams=gcam, dataset="duke")
    assert abs(got[0] - want_first[0]) <= 1e-12 and abs(got[1] - want_map) <= 1e-12
