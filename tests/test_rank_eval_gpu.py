"""CMC / mAP scoring on the device (csrc/rank_eval.hip) through ops.rank_eval, clustercontrast.evaluation_metrics and
clustercontrast.evaluators.DeviceEvaluator, against the reference's recorded results (tests/golden/reference_eval.npz) and
the numpy model (tests/rank_eval_hostmodel.py, tied to the reference and to scikit-learn by tests/test_rank_eval_cpu.py).

Tolerances.  npos, first and hits are integers and the `market1501` CMC is a cumulative sum of integers over an integer:
compared for equality.  AP, mAP and the CMC variants that weight by 1 / npos are fp64 sums of at most G terms per query and
Q per bin, taken in another order than the reference's: about (G + Q) * 2^-53 = 1.2e-13 at the fixture's G <= 1 000,
Q <= 40; the bound used everywhere is 1e-12 absolute, that with one decade of room.  (The device adds the AP terms as 64.64
fixed point, error P * 2^-64; what the bound covers is the fp64 summation on the host side of the comparison, whose terms
are at most 1 / P each.)"""
import os
import re

import numpy as np
import pytest
import torch

from tests import rank_eval_hostmodel as M
from tests.golden import cases_eval as C

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(REPO, "tests", "golden", "reference_eval.npz"))
TOL = 1e-12


def _dev_ids(dev, *vs):
    return [torch.from_numpy(np.ascontiguousarray(v, dtype=np.int32)).to(dev) for v in vs]


def _run(d, qid, gid, qcam, gcam, dev, **kw):
    from rg_hip import ops
    return ops.rank_eval(torch.from_numpy(np.ascontiguousarray(d)).to(dev), *_dev_ids(dev, qid, gid, qcam, gcam), debug=True, **kw)


def _check_against_model(d, qid, gid, qcam, gcam, dev, topk=100, sep=False, chunk=0):
    """per-query outputs and the sums over the queries of one ops.rank_eval call against the model; returns the outputs"""
    want = M.per_query(d, qid, gid, qcam, gcam, topk=topk, separate_camera_set=sep)
    res = _run(d, qid, gid, qcam, gcam, dev, topk=topk, separate_camera_set=sep, chunk=chunk)
    got = [res[k].cpu().numpy() for k in ("npos", "ap", "first", "hits")]
    assert got[0].dtype == np.int32 and got[1].dtype == np.float64 and got[2].dtype == np.int32 and got[3].shape == (len(d), topk)
    assert np.array_equal(got[0], want[0]), "npos differs"
    assert np.array_equal(got[2], want[2]), "first differs"
    assert np.array_equal(got[3], want[3]), "hits differ"
    err = float(np.abs(got[1] - want[1]).max())
    assert err <= TOL, "ap differs by %.2e" % err
    ok = want[0] > 0
    assert res["num_valid"] == int(ok.sum()) and res["status"] == 0
    if ok.any():
        mAP, cmc_first, cmc_all = M.summarize(*want)
        n = res["num_valid"]
        assert abs(res["ap_sum"] / n - mAP) <= TOL
        assert np.array_equal(res["first_hist"].cumsum() / n, cmc_first)
        assert np.abs(res["allshots"].cumsum() / n - cmc_all).max() <= TOL
    return got


def _random_case(Q, G, seed, n_id=5, n_cam=3, levels=0, dtype=np.float32):
    g = np.random.RandomState(seed)
    d = g.rand(Q, G) + 0.3 * g.rand(Q, 1)
    if levels:
        d = np.floor(d * levels / d.max()).clip(0, levels - 1) / 4.0
    return (d.astype(dtype), g.randint(0, n_id, Q), g.randint(0, n_id, G), g.randint(0, n_cam, Q), g.randint(0, n_cam, G))


# ---------------------------------------------------------------------------------------------------------------------------
# the reference's recorded results through the drop-in functions
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", C.TIE_FREE)
def test_fixture_cases_through_cmc_and_mean_ap(dev, name):
    from clustercontrast.evaluation_metrics import cmc, mean_ap
    import reid.evaluation_metrics as RE
    assert RE.cmc is cmc and RE.mean_ap is mean_ap
    d, qid, gid, qcam, gcam = C.load(GOLD, name)
    for dt in (np.float32, np.float64):
        dd = d.astype(dt)
        for form in (dd, torch.from_numpy(dd), torch.from_numpy(dd).to(dev)):
            got = mean_ap(form, qid, gid, qcam, gcam)
            assert isinstance(got, float) and abs(got - float(GOLD[name + "_map"])) <= TOL
            for cfg, kw in C.CMC_CONFIGS.items():
                curve = cmc(form, qid, gid, qcam, gcam, topk=C.TOPK, **kw)
                want = GOLD["%s_cmc_%s" % (name, cfg)]
                assert isinstance(curve, np.ndarray) and curve.dtype == np.float64 and curve.shape == (C.TOPK,)
                if cfg == "market1501":
                    assert np.array_equal(curve, want), cfg
                else:
                    assert np.abs(curve - want).max() <= TOL, cfg
    # ids as Python lists and as int64 tensors, as the evaluators pass them
    got = cmc(d, qid.tolist(), torch.from_numpy(gid.astype(np.int64)), list(qcam), gcam.astype(np.int64), first_match_break=True)
    assert np.array_equal(got, GOLD[name + "_cmc_market1501"])


def test_tied_fixture_case_and_defaults(dev):
    from clustercontrast.evaluation_metrics import cmc, mean_ap
    d, qid, gid, qcam, gcam = C.load(GOLD, "tied")
    for form in (d, torch.from_numpy(d.astype(np.float64)).to(dev)):
        assert abs(mean_ap(form, qid, gid, qcam, gcam) - float(GOLD["tied_map"])) <= TOL
    # the reference's defaults: ids arange, query cameras 0, gallery cameras 1 — the diagonal entry is each query's only match
    g = np.random.RandomState(1)
    sq = g.rand(9, 9).astype(np.float32)
    want = M.summarize(*M.per_query(sq, np.arange(9), np.arange(9), np.zeros(9, int), np.ones(9, int), topk=4))
    assert abs(mean_ap(sq) - want[0]) <= TOL
    assert np.array_equal(cmc(sq, topk=4, first_match_break=True), want[1])
    assert np.abs(cmc(sq, topk=4) - want[2]).max() <= TOL


# ---------------------------------------------------------------------------------------------------------------------------
# per-query outputs against the model
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", [1, 63, 64, 65, 257, 1000])
def test_per_query_outputs_equal_the_model(dev, G):
    for t, topk in enumerate((1, 100, G + 5)):
        for dtype in (np.float32, np.float64):
            case = _random_case(7, G, seed=100 * G + t, dtype=dtype)
            _check_against_model(*case, dev=dev, topk=topk)
            _check_against_model(*case, dev=dev, topk=topk, sep=True)
            tied = _random_case(7, G, seed=100 * G + t + 50, levels=4, dtype=dtype)
            _check_against_model(*tied, dev=dev, topk=topk)
            _check_against_model(*tied, dev=dev, topk=topk, chunk=1 + t)


def test_special_values_and_degenerate_rows(dev):
    g = np.random.RandomState(5)
    Q, G = 6, 130
    _, qid, gid, qcam, gcam = _random_case(Q, G, seed=9)
    for dtype in (np.float32, np.float64):
        d = g.choice(np.array([-0.0, 0.0, 1.0, np.inf, -np.inf, 0.5]), size=(Q, G)).astype(dtype)
        assert np.signbit(d[d == 0]).any() and not np.signbit(d[d == 0]).all()
        _check_against_model(d, qid, gid, qcam, gcam, dev)
        _check_against_model(d, qid, gid, qcam, gcam, dev, sep=True, chunk=3)
        same = np.full((Q, G), 0.25, dtype=dtype)                      # all entries equal: ranks follow the gallery index
        _check_against_model(same, qid, gid, qcam, gcam, dev, topk=G + 5)
    # a query with no positive among queries that have some, and a matrix offset by one element from 16-byte alignment
    qid2 = qid.copy()
    qid2[2] = 999
    d = g.rand(Q, G).astype(np.float32)
    got = _check_against_model(d, qid2, gid, qcam, gcam, dev)
    assert got[0][2] == 0 and got[2][2] == -1 and got[1][2] == 0.0 and not got[3][2].any()
    from rg_hip import ops
    flat = torch.zeros(Q * G + 1, dtype=torch.float32, device=dev)
    flat[1:] = torch.from_numpy(d).to(dev).reshape(-1)
    res = ops.rank_eval(flat[1:].view(Q, G), *_dev_ids(dev, qid2, gid, qcam, gcam), debug=True)
    assert np.array_equal(res["hits"].cpu().numpy(), got[3]) and np.array_equal(res["ap"].cpu().numpy(), got[1])


def test_no_valid_query_and_nan(dev):
    from clustercontrast.evaluation_metrics import cmc, mean_ap
    from rg_hip import ops
    d, qid, gid, qcam, gcam = _random_case(5, 70, seed=2)
    for fn in (cmc, mean_ap):
        with pytest.raises(RuntimeError, match="No valid query"):
            fn(d, qid + 100, gid, qcam, gcam)
    # every match shares the query's camera
    with pytest.raises(RuntimeError, match="No valid query"):
        mean_ap(d, qid, gid, np.zeros(5, int), np.zeros(70, int))
    bad = d.copy()
    bad[3, 41] = np.nan
    for fn in (cmc, mean_ap):
        with pytest.raises(ValueError, match="NaN"):
            fn(bad, qid, gid, qcam, gcam)
    with pytest.raises(ValueError, match="NaN"):                       # in a row without a positive, too
        q2 = qid.copy()
        q2[3] = 999
        mean_ap(bad.astype(np.float64), q2, gid, qcam, gcam)
    # argument checks of the wrapper
    dd, ids = torch.from_numpy(d).to(dev), _dev_ids(dev, qid, gid, qcam, gcam)
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        ops.rank_eval(torch.from_numpy(d), *ids)
    with pytest.raises(TypeError):
        ops.rank_eval(dd.half(), *ids)
    with pytest.raises(TypeError):
        ops.rank_eval(dd, ids[0].long(), *ids[1:])
    with pytest.raises(ValueError):
        ops.rank_eval(dd, ids[0][:-1], *ids[1:])
    with pytest.raises(ValueError):
        ops.rank_eval(dd, *ids, topk=0)
    with pytest.raises(ValueError):
        ops.rank_eval(dd, *ids, chunk=2048)
    with pytest.raises(ValueError):
        ops.rank_eval(dd.t(), ids[1], ids[0], ids[3], ids[2])           # not contiguous


def test_more_positives_than_one_pass_holds(dev):
    g = np.random.RandomState(3)
    Q, G = 3, 5000
    gid = np.where(np.arange(G) < 4500, 7, g.randint(8, 12, G))
    gid = gid[g.permutation(G)]
    gcam = g.randint(0, 4, G)
    qid, qcam = np.array([7, 9, 7]), np.array([0, 1, 5])
    d = np.floor(g.rand(Q, G) * 900).astype(np.float32) / 8.0          # ties inside and across the passes
    auto = _check_against_model(d, qid, gid, qcam, gcam, dev)
    assert auto[0][2] == 4500 and auto[0][0] > 3000
    for chunk in (64, 100):
        got = _check_against_model(d, qid, gid, qcam, gcam, dev, chunk=chunk)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(auto, got)), "chunk=%d changes the bits" % chunk


def test_two_runs_and_a_side_stream_give_the_same_bytes(dev):
    from rg_hip import ops
    d, qid, gid, qcam, gcam = _random_case(64, 3001, seed=8, n_id=4, levels=40)
    dd, ids = torch.from_numpy(d).to(dev), _dev_ids(dev, qid, gid, qcam, gcam)

    def run():
        res = ops.rank_eval(dd, *ids, topk=50, debug=True)
        return [res[k].cpu().numpy().tobytes() for k in ("npos", "ap", "first", "hits")] + [
            res["first_hist"].tobytes(), res["allshots"].tobytes(), np.float64(res["ap_sum"]).tobytes()]
    a, b = run(), run()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        c = run()
    side.synchronize()
    assert a == b and a == c


def test_moderate_size_from_device_distances(dev):
    from clustercontrast.evaluators import pairwise_distance
    from rg_hip import ops
    g = np.random.RandomState(12)
    Q, G, D, n_id = 256, 15913, 64, 751
    centres = g.randn(n_id, D)
    qid, gid = g.randint(0, n_id, Q), g.randint(0, n_id, G)
    qcam, gcam = g.randint(0, 6, Q), g.randint(0, 6, G)
    x = torch.from_numpy((centres[np.concatenate([qid, gid])] + 0.8 * g.randn(Q + G, D)).astype(np.float32))
    x = x / x.norm(dim=1, keepdim=True)
    feats = {i: x[i] for i in range(Q + G)}
    query = [(i, int(qid[i]), int(qcam[i])) for i in range(Q)]
    gallery = [(Q + j, int(gid[j]), int(gcam[j])) for j in range(G)]
    dist, xq, yg = pairwise_distance(feats, query, gallery, return_device=True)
    assert dist.is_cuda and xq.is_cuda and yg.is_cuda and tuple(dist.shape) == (Q, G) and dist.dtype == torch.float32
    host = pairwise_distance(feats, query, gallery)
    assert not host[0].is_cuda and isinstance(host[1], np.ndarray) and np.array_equal(host[0].numpy(), dist.cpu().numpy())
    _check_against_model(host[0].numpy(), qid, gid, qcam, gcam, dev)


# ---------------------------------------------------------------------------------------------------------------------------
# DeviceEvaluator end to end
# ---------------------------------------------------------------------------------------------------------------------------
class _TinyModel(torch.nn.Module):
    def __init__(self):
        super(_TinyModel, self).__init__()
        self.fc = torch.nn.Linear(3 * 8 * 4, 64)

    def forward(self, x):
        return torch.nn.functional.normalize(self.fc(x.flatten(1)), dim=1)


def _tiny_eval_setup(dev):
    g = torch.Generator().manual_seed(21)
    n_q, n_g, n_id = 16, 64, 8
    pids = [i % n_id for i in range(n_q)] + [j % n_id for j in range(n_g)]
    cams = [0] * n_q + [1 + (j // n_id) % 3 for j in range(n_g)]
    base = torch.randn(n_id, 3, 8, 4, generator=g)
    imgs = torch.stack([base[p] for p in pids]) + 0.7 * torch.randn(n_q + n_g, 3, 8, 4, generator=g)
    names = ["img_%03d.jpg" % i for i in range(n_q + n_g)]
    half = (n_q + n_g) // 2
    loader = [(imgs[s], names[s], torch.tensor(pids[s]), torch.tensor(cams[s]), torch.arange(n_q + n_g)[s])
              for s in (slice(0, half), slice(half, None))]
    entries = list(zip(names, pids, cams))
    torch.manual_seed(4)
    return _TinyModel().to(dev), loader, entries[:n_q], entries[n_q:]


@pytest.mark.parametrize("rerank", [False, True])
def test_device_evaluator_end_to_end(dev, rerank, capsys, monkeypatch):
    from clustercontrast.evaluators import DeviceEvaluator, evaluate_all_device, extract_cnn_feature, pairwise_distance
    from clustercontrast.utils.rerank import re_ranking
    model, loader, query, gallery = _tiny_eval_setup(dev)
    # the separately computed matrices: features through the host dictionary, as the reference's Evaluator holds them
    feats = {}
    for imgs, fnames, _, _, _ in loader:
        for f, o in zip(fnames, extract_cnn_feature(model.eval(), imgs)):
            feats[f] = o
    d_qg = pairwise_distance(feats, query, gallery, return_device=True)[0]
    want = [evaluate_all_device(d_qg, query=query, gallery=gallery, cmc_flag=True)]
    if rerank:
        d_qq = pairwise_distance(feats, query, query, return_device=True)[0]
        d_gg = pairwise_distance(feats, gallery, gallery, return_device=True)[0]
        rr = re_ranking(d_qg, d_qq, d_gg, return_device=True)
        assert rr.is_cuda and np.array_equal(rr.cpu().numpy(), re_ranking(d_qg, d_qq, d_gg))
        want.append(evaluate_all_device(rr, query=query, gallery=gallery, cmc_flag=True))
        host = M.summarize(*M.per_query(rr.cpu().numpy(), [p for _, p, _ in query], [p for _, p, _ in gallery],
                                        [c for _, _, c in query], [c for _, _, c in gallery]))
        assert abs(want[1][1] - host[0]) <= TOL and np.array_equal(want[1][0], host[1])
    capsys.readouterr()

    copied = []
    real_cpu = torch.Tensor.cpu

    def counting_cpu(self, *a, **k):
        copied.append(self.numel())
        return real_cpu(self, *a, **k)
    monkeypatch.setattr(torch.Tensor, "cpu", counting_cpu)
    got = DeviceEvaluator(model).evaluate(loader, query, gallery, cmc_flag=True, rerank=rerank)
    map_only = DeviceEvaluator(model).evaluate(loader, query, gallery, rerank=rerank)
    monkeypatch.undo()
    assert copied and max(copied) <= 100 + 2, copied                   # topk + 2 numbers at the most leave the device at once

    scores, mAP = got
    assert isinstance(mAP, float) and isinstance(scores, np.ndarray) and scores.dtype == np.float64 and scores.shape == (100,)
    assert mAP == want[-1][1] and np.array_equal(scores, want[-1][0]) and map_only == mAP
    assert 0.0 < mAP <= 1.0 and scores[-1] == 1.0
    lines = capsys.readouterr().out.splitlines()
    block = ["Mean AP: {:4.1%}", "CMC Scores:"] + ["  top-{:<4}{:12.1%}"] * 3
    expect = []
    for w in want:
        expect += [block[0].format(w[1]), block[1]] + [block[2].format(k, w[0][k - 1]) for k in (1, 5, 10)]
        if rerank and w is want[0]:
            expect.append("Applying person re-ranking ...")
    assert lines[:len(expect)] == expect
    assert re.match(r"^Mean AP: +\d+\.\d%$", lines[0]) and re.match(r"^  top-1 +\d+\.\d%$", lines[2])
    # the second call printed the mAP lines only
    rest = lines[len(expect):]
    assert rest == [ln for ln in expect if ln.startswith("Mean AP") or ln.startswith("Applying")]
