"""Single-gallery-shot CMC on the device (csrc/cmc_shot.hip) through ops.cmc_shot, clustercontrast.evaluation_metrics.
cmc_single_shot, reid.evaluators.evaluate_all_single_shot and DeviceCascadeEvaluator(single_shot=...), against the
numpy model (tests/sgs_hostmodel.py, tied to the reference by tests/test_sgs_hostmodel_cpu.py) and the reference's recorded
curves and generator states (tests/golden/reference_sgs.npz).

Tolerances.  n, slot, high, rank and hist are integers: compared for equality with the model's.  The curve is the model's
expression on the same integers: byte-equal.  Against the fixture the bound is 1e-12, derived in
tests/test_sgs_hostmodel_cpu.py (the reference adds 0.1 up to 400 times where the histogram is multiplied once); curves under
first_match_break are integers over num_valid and must be equal.  The generator state is compared for equality."""
import os

import numpy as np
import pytest
import torch

from tests import sgs_hostmodel as M
from tests.golden import cases_eval as CE
from tests.golden import cases_sgs as C

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(REPO, "tests", "golden", "reference_sgs.npz"))
GOLD_EVAL = np.load(os.path.join(REPO, "tests", "golden", "reference_eval.npz"))
TOL = 1e-12


def _state(rs=None):
    s = (np.random if rs is None else rs).get_state()
    return s[1].copy(), int(s[2])


def _same_state(a, b):
    return np.array_equal(a[0], b[0]) and a[1] == b[1]


def _host(res):
    return {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in res.items()}


def _check(d, qid, gid, qcam, gcam, seed=0, topk=20, sep=False, first=False, repeat=10, chunk=0, form=None):
    """one cmc_single_shot call from numpy's global generator seeded with `seed` against the model run from the same seed: every
    integer equal, the curve byte-equal, the generator left in the same state.  Returns the host copies of the debug outputs."""
    from clustercontrast.evaluation_metrics import cmc_single_shot
    np.random.seed(seed)
    want = M.run(d, qid, gid, qcam, gcam, topk=topk, separate_camera_set=sep, first_match_break=first, repeat=repeat)
    want_state = _state()
    np.random.seed(seed)
    curve, res = cmc_single_shot(d if form is None else form, qid, gid, qcam, gcam, topk=topk, separate_camera_set=sep,
                                 first_match_break=first, repeat=repeat, chunk=chunk, debug=True)
    assert _same_state(_state(), want_state), "the generator is not where the model leaves it"
    got = _host(res)
    assert all(got[k].dtype == np.int32 for k in ("n", "slot", "high", "rank")) and got["hist"].dtype == np.int64
    nid = len(np.unique(gid))
    assert got["slot"].shape == (len(d), nid) and got["rank"].shape == (len(d), repeat) and got["hist"].shape == (topk,)
    for k in ("n", "slot", "high", "rank", "hist"):
        assert np.array_equal(got[k], want[k]), "%s differs" % k
    assert got["num_valid"] == want["num_valid"]
    assert curve.dtype == np.float64 and curve.tobytes() == want["curve"].tobytes()
    got["curve"] = curve
    return got


def _random_case(Q, G, seed, n_id=5, n_cam=3, levels=0, dtype=np.float32):
    g = np.random.RandomState(seed)
    d = g.rand(Q, G) + 0.3 * g.rand(Q, 1)
    if levels:
        d = np.floor(d * levels / d.max()).clip(0, levels - 1) / 4.0
    gid = g.randint(0, n_id, G)
    gid[:min(n_id, G)] = np.arange(min(n_id, G))                        # every identity is present: nid = min(n_id, G)
    return d.astype(dtype), g.randint(0, min(n_id, G), Q), gid, g.randint(0, n_cam, Q), g.randint(0, n_cam, G)


# ---------------------------------------------------------------------------------------------------------------------------
# 1. the reference's recorded results
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", C.CASES)
def test_fixture_configurations(dev, name):
    d, qid, gid, qcam, gcam = C.load(GOLD, GOLD_EVAL, name)
    for dt in (np.float32, np.float64):
        dd = d.astype(dt)
        for cfg, kw in C.CONFIGS.items():
            for seed in C.SEEDS:
                got = _check(dd, qid, gid, qcam, gcam, seed=seed, topk=C.TOPK, sep=kw["separate_camera_set"],
                             first=kw["first_match_break"], repeat=C.REPEAT)
                want = GOLD[C.key(name, cfg, seed, "curve")]
                if kw["first_match_break"]:
                    assert np.array_equal(got["curve"], want), (cfg, seed)
                else:
                    assert np.abs(got["curve"] - want).max() <= TOL, (cfg, seed)
                assert _same_state(_state(), (GOLD[C.key(name, cfg, seed, "key")], int(GOLD[C.key(name, cfg, seed, "pos")])))
    # a CPU tensor, a device tensor, ids as lists and int64 tensors
    kw = C.CONFIGS["sepcam"]
    a = _check(d, qid, gid, qcam, gcam, seed=11, topk=C.TOPK, sep=True, form=torch.from_numpy(d))
    b = _check(d, qid, gid, qcam, gcam, seed=11, topk=C.TOPK, sep=True, form=torch.from_numpy(d.astype(np.float64)).to(dev))
    assert a["curve"].tobytes() == b["curve"].tobytes()
    from clustercontrast.evaluation_metrics import cmc_single_shot
    np.random.seed(11)
    c = cmc_single_shot(d, qid.tolist(), torch.from_numpy(gid.astype(np.int64)), list(qcam), gcam.astype(np.int64), topk=C.TOPK, **kw)
    assert c.tobytes() == a["curve"].tobytes()


# ---------------------------------------------------------------------------------------------------------------------------
# 2. edges, each against the model exactly
# ---------------------------------------------------------------------------------------------------------------------------
def test_tied_case_follows_the_stable_order(dev):
    d, qid, gid, qcam, gcam = CE.load(GOLD_EVAL, "tied")
    assert not CE.rows_tie_free(d)
    for dt in (np.float32, np.float64):
        for kw in C.CONFIGS.values():
            _check(d.astype(dt), qid, gid, qcam, gcam, seed=3, sep=kw["separate_camera_set"], first=kw["first_match_break"])
    # all entries equal, and signed zeros: the order is the gallery index alone
    same = np.full_like(d, 0.25)
    _check(same, qid, gid, qcam, gcam, seed=4, topk=5)
    g = np.random.RandomState(5)
    mixed = g.choice(np.array([-0.0, 0.0, 1.0, np.inf, -np.inf, 0.5]), size=d.shape).astype(np.float32)
    _check(mixed, qid, gid, qcam, gcam, seed=6, sep=True)


def test_id_edges(dev):
    # gallery ids -1 and 0
    d, qid, gid, qcam, gcam = C.load(GOLD, GOLD_EVAL, "edge_ids")
    assert (gid == -1).any() and (gid == 0).any()
    _check(d, qid, gid, qcam, gcam, seed=1, repeat=3)
    # a query with no valid match among queries that have one: n = 0, rank = -1, nothing drawn for it
    d, qid, gid, qcam, gcam = _random_case(6, 130, seed=9)
    qid2 = qid.copy()
    qid2[2] = 999                                                       # an identity the gallery does not hold
    gcam2 = gcam.copy()
    gcam2[gid == qid2[4]] = qcam[4]                                     # every match of query 4 shares its camera
    got = _check(d, qid2, gid, qcam, gcam2, seed=2)
    assert got["n"][2] == 0 and got["n"][4] == 0 and (got["rank"][[2, 4]] == -1).all() and (got["slot"][[2, 4]] == -1).all()
    assert got["num_valid"] == int((got["n"] > 0).sum()) <= 4
    # an own identity with exactly one valid entry: its draw consumes nothing and always selects that entry
    gid3, gcam3 = gid.copy(), gcam.copy()
    own = np.nonzero(gid3 == qid[0])[0]
    gcam3[own] = qcam[0]
    gcam3[own[0]] = qcam[0] + 1
    got = _check(d, qid, gid3, qcam, gcam3, seed=3)
    assert got["high"][0, list(got["slot"][0]).index(np.unique(gid3).tolist().index(qid[0]))] == 1
    # separate_camera_set removes every entry of some identities
    gcam4 = gcam.copy()
    gcam4[np.isin(gid, [x for x in range(5) if x != qid[1]][:2])] = qcam[1]
    plain = _check(d, qid, gid, qcam, gcam4, seed=4)
    sep = _check(d, qid, gid, qcam, gcam4, seed=4, sep=True)
    assert plain["n"][1] == 5 and sep["n"][1] == 3


@pytest.mark.parametrize("nid", [1, 63, 64, 65, 129])
def test_identity_counts(dev, nid):
    for t, dtype in enumerate((np.float32, np.float64)):
        case = _random_case(5, 300, seed=10 * nid + t, n_id=nid, dtype=dtype)
        assert len(np.unique(case[2])) == nid
        _check(*case, seed=nid)
        _check(*case, seed=nid, sep=True, first=True, repeat=3)
        tied = _random_case(5, 300, seed=10 * nid + t + 5, n_id=nid, levels=5, dtype=dtype)
        _check(*tied, seed=nid, repeat=1)


@pytest.mark.parametrize("G", [1, 64, 65, 257])
def test_gallery_sizes(dev, G):
    for t, dtype in enumerate((np.float32, np.float64)):
        case = _random_case(7, G, seed=100 * G + t, n_id=4, dtype=dtype)
        _check(*case, seed=G, topk=1)
        _check(*case, seed=G, topk=G + 5, sep=True)
        tied = _random_case(7, G, seed=100 * G + t + 50, n_id=4, levels=4, dtype=dtype)
        _check(*tied, seed=G, topk=3, repeat=3)


def test_long_segment_beside_single_entries_and_a_low_topk(dev):
    g = np.random.RandomState(7)
    G = 700 + 40
    gid = np.concatenate([np.full(700, 5), 100 + np.arange(40)])[g.permutation(G)]
    gcam = g.randint(1, 4, G)
    qid, qcam = np.array([5, 117, 5, 100]), np.array([0, 0, 2, 0])
    d = g.rand(4, G).astype(np.float32)
    d[0, gid == 5] += 0.5                                               # query 0: its own entries come late, most ranks are high
    got = _check(d, qid, gid, qcam, gcam, seed=8, topk=3)
    assert (got["rank"][0] >= 3).sum() >= 5 and got["high"].max() == 700 and got["hist"].sum() < got["rank"].size
    assert (got["high"][1, :got["n"][1]] == np.where(got["slot"][1, :got["n"][1]] == 0, 700, 1)).all()
    _check(np.floor(d * 50) / 8, qid, gid, qcam, gcam, seed=8, topk=1, sep=True)   # ties inside the long segment


def test_random_state_argument_leaves_the_global_generator_alone(dev):
    from clustercontrast.evaluation_metrics import cmc_single_shot
    d, qid, gid, qcam, gcam = C.load(GOLD, GOLD_EVAL, "narrow")
    np.random.seed(21)
    before = _state()
    rs = np.random.RandomState(11)
    curve = cmc_single_shot(d, qid, gid, qcam, gcam, topk=C.TOPK, separate_camera_set=True, random_state=rs)
    assert _same_state(_state(), before)
    assert np.abs(curve - GOLD[C.key("narrow", "sepcam", 11, "curve")]).max() <= TOL
    assert _same_state(_state(rs), (GOLD[C.key("narrow", "sepcam", 11, "key")], int(GOLD[C.key("narrow", "sepcam", 11, "pos")])))
    with pytest.raises(TypeError, match="random_state"):
        cmc_single_shot(d, qid, gid, qcam, gcam, random_state=11)
    with pytest.raises(RuntimeError, match="No valid query"):
        cmc_single_shot(d, qid + 1000, gid, qcam, gcam)
    assert _same_state(_state(), before)


# ---------------------------------------------------------------------------------------------------------------------------
# 3. both gather regimes, chunks of queries
# ---------------------------------------------------------------------------------------------------------------------------
def test_both_gather_regimes_and_chunks(dev):
    from rg_hip import ops
    last_lds = 32768 // 8                                               # fp64 rows: the largest G whose row is staged in LDS
    assert ops.cmc_shot_regime(last_lds, 7, True) == ops.CMC_SHOT_LDS_ROW == 1
    assert ops.cmc_shot_regime(last_lds + 1, 7, True) == ops.CMC_SHOT_GLOBAL == 0
    assert ops.cmc_shot_regime(2 * last_lds, 7, False) == 1 and ops.cmc_shot_regime(2 * last_lds + 1, 7, False) == 0
    assert ops.cmc_shot_regime(15913, 752, False) == 0 and ops.cmc_shot_regime(15913, 752, True) == 0     # Market-1501 rows are gathered
    assert ops.cmc_shot_regime(100, 4097, False) == -1 and ops.cmc_shot_regime(0, 1, False) == -1 and ops.cmc_shot_regime(5, 6, False) == -1
    for G in (last_lds + 1, last_lds, last_lds - 3):
        case = _random_case(3, G, seed=G, n_id=7, n_cam=2, dtype=np.float64)
        whole = _check(*case, seed=5, sep=True)
        tied = _random_case(3, G, seed=G + 1, n_id=7, n_cam=2, levels=9, dtype=np.float64)
        _check(*tied, seed=5, repeat=3)
    # an fp32 matrix one element off 16-byte alignment: the LDS image is shifted with it
    d, qid, gid, qcam, gcam = _random_case(5, 1001, seed=13, n_id=6)
    flat = torch.zeros(5 * 1001 + 1, dtype=torch.float32, device=dev)
    flat[1:] = torch.from_numpy(d).to(dev).reshape(-1)
    assert flat[1:].data_ptr() % 16 == 4
    whole = _check(d, qid, gid, qcam, gcam, seed=6, form=flat[1:].view(5, 1001))
    # chunks of queries: same bits, same end state
    d, qid, gid, qcam, gcam = _random_case(23, 500, seed=17, n_id=11, levels=30)
    qid[[0, 8, 22]] = 999                                               # skipped queries at both ends of a chunk
    whole = _check(d, qid, gid, qcam, gcam, seed=7)
    for chunk in (1, 7, 23):
        got = _check(d, qid, gid, qcam, gcam, seed=7, chunk=chunk)
        assert all(got[k].tobytes() == whole[k].tobytes() for k in ("n", "slot", "high", "rank", "hist", "curve")), chunk


# ---------------------------------------------------------------------------------------------------------------------------
# 4. reproducibility and allocation
# ---------------------------------------------------------------------------------------------------------------------------
def _dev_ids(dev, *vs):
    return [torch.from_numpy(np.ascontiguousarray(v, dtype=np.int32)).to(dev) for v in vs]


def test_two_runs_and_a_side_stream_give_the_same_bytes(dev):
    from rg_hip import ops
    d, qid, gid, qcam, gcam = _random_case(64, 3001, seed=8, n_id=40, levels=40)
    dd, ids = torch.from_numpy(d).to(dev), _dev_ids(dev, qid, gid, qcam, gcam)

    def run():
        res = ops.cmc_shot(dd, *ids, topk=10, random_state=np.random.RandomState(3), debug=True)
        return [res[k].cpu().numpy().tobytes() for k in ("n", "slot", "high", "rank")] + [res["hist"].tobytes()]
    a, b = run(), run()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        c = run()
    side.synchronize()
    assert a == b and a == c


def test_no_matrix_sized_temporary(dev):
    from clustercontrast.evaluation_metrics import cmc_single_shot
    Q, G, nid, repeat = 64, 8192, 16, 10
    d, qid, gid, qcam, gcam = _random_case(Q, G, seed=4, n_id=nid)
    dd, ids = torch.from_numpy(d).to(dev), _dev_ids(dev, qid, gid, qcam, gcam)
    cmc_single_shot(dd, *ids, random_state=np.random.RandomState(0))   # the library and the allocator are warm
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    curve = cmc_single_shot(dd, *ids, random_state=np.random.RandomState(0))
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated() - base
    bound = 8 * Q * nid + 4 * Q * repeat * nid + 64 * 1024
    print("peak above the matrix and the id vectors: %d bytes, bound %d, the matrix %d" % (extra, bound, 4 * Q * G))
    assert 0 < extra < bound < 4 * Q * G
    assert curve.tobytes() == M.run(d, qid, gid, qcam, gcam, random_state=np.random.RandomState(0))["curve"].tobytes()


# ---------------------------------------------------------------------------------------------------------------------------
# 5. failure paths: refused before the first draw
# ---------------------------------------------------------------------------------------------------------------------------
def test_nan_and_too_many_identities_leave_the_generator_untouched(dev, monkeypatch):
    from clustercontrast.evaluation_metrics import cmc_single_shot
    from rg_hip import ops
    d, qid, gid, qcam, gcam = _random_case(5, 70, seed=2)
    np.random.seed(31)
    before = _state()
    for row, q in ((3, qid), (1, np.where(np.arange(5) == 1, 999, qid))):       # in a scored row and in a skipped one
        bad = d.copy()
        bad[row, 41] = np.nan
        for dt in (np.float32, np.float64):
            with pytest.raises(ValueError, match="NaN"):
                cmc_single_shot(bad.astype(dt), q, gid, qcam, gcam)
    assert _same_state(_state(), before)
    # 4097 identities: refused before anything is enqueued
    G = 4097
    wide = np.random.RandomState(1).rand(2, G).astype(np.float32)
    launched = []
    real = ops.lib.rg_cmc_shot_order
    monkeypatch.setattr(ops.lib, "rg_cmc_shot_order", lambda *a: launched.append(a) or real(*a))
    with pytest.raises(ValueError, match="4096"):
        cmc_single_shot(wide, [0, 1], np.arange(G), [0, 0], np.ones(G, dtype=int))
    assert not launched and _same_state(_state(), before)
    got = cmc_single_shot(wide[:, :4096].astype(np.float64), [0, 1], np.arange(4096), [0, 0], np.ones(4096, dtype=int), topk=5)
    assert launched and got.shape == (5,)                               # 4096 are served (fp64: the 64 KB of sort keys)
    monkeypatch.undo()
    # the wrappers' own checks
    dd, ids = torch.from_numpy(d).to(dev), _dev_ids(dev, qid, gid, qcam, gcam)
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        ops.cmc_shot(torch.from_numpy(d), *ids)
    with pytest.raises(TypeError):
        ops.cmc_shot(dd.half(), *ids)
    with pytest.raises(TypeError):
        ops.cmc_shot(dd, ids[0].long(), *ids[1:])
    with pytest.raises(ValueError):
        ops.cmc_shot(dd, ids[0][:-1], *ids[1:])
    with pytest.raises(ValueError):
        ops.cmc_shot(dd, *ids, repeat=65)
    with pytest.raises(ValueError):
        ops.cmc_shot(dd, *ids, chunk=-1)
    assert _same_state(_state(), before)


# ---------------------------------------------------------------------------------------------------------------------------
# 6. Market-1501 size
# ---------------------------------------------------------------------------------------------------------------------------
class _Recorder(object):
    """a generator that keeps what it was asked for and what it handed out"""

    def __init__(self, rs):
        self.rs, self.highs, self.parts = rs, [], []

    def randint(self, low, high):
        out = self.rs.randint(low, high)
        self.highs.append(np.asarray(high).copy())
        self.parts.append(out)
        return out


def test_market_size(dev):
    from rg_hip import ops
    g = np.random.RandomState(12)
    Q, G, n_id, repeat, topk = 3368, 15913, 752, 10, 100
    gid = np.concatenate([np.arange(n_id), g.randint(0, n_id, G - n_id)])[g.permutation(G)]
    qid, qcam, gcam = g.randint(0, n_id + 3, Q), g.randint(0, 6, Q), g.randint(0, 6, G)      # a few queries ask for absent ids
    gen = torch.Generator(device=dev).manual_seed(5)
    dd = torch.rand(Q, G, device=dev, generator=gen)
    ids = _dev_ids(dev, qid, gid, qcam, gcam)
    dd -= 0.2 * (ids[1][None, :] == ids[0][:, None])
    assert ops.cmc_shot_regime(G, n_id, False) == ops.CMC_SHOT_GLOBAL
    rec = _Recorder(np.random.RandomState(77))
    res = ops.cmc_shot(dd, *ids, topk=topk, separate_camera_set=True, repeat=repeat, random_state=rec, debug=True)
    n, rank, high = res["n"].cpu().numpy(), res["rank"].cpu().numpy(), res["high"].cpu().numpy()
    assert res["num_valid"] == ops.rank_eval(dd, *ids, topk=1, separate_camera_set=True)["num_valid"] == int((n > 0).sum())
    assert 0 < res["num_valid"] < Q and ((rank == -1).all(axis=1) == (n == 0)).all()
    assert res["hist"].sum() == int(((rank >= 0) & (rank < topk)).sum()) and (rank >= topk).any()
    # 8 queries against the per-query model, given their slices of the stream the call consumed (several launches' worth)
    stream = np.concatenate(rec.parts)
    assert len(rec.parts) > 1 and max(4 * len(p) for p in rec.parts) <= ops.CMC_SHOT_DRAW_BYTES
    assert stream.size == int(n.sum()) * repeat and (stream < np.concatenate(rec.highs)).all() and stream.min() == 0
    starts = np.concatenate([[0], np.cumsum(n.astype(np.int64) * repeat)])
    picks = list(g.choice(np.nonzero(n > 0)[0], size=7, replace=False)) + [int(np.nonzero(n > 0)[0][-1])]
    rows = dd[torch.as_tensor(picks, device=dev)].cpu().numpy()
    m, uniq = M.Model(), np.unique(gid)
    for row, q in zip(rows, picks):
        info = m.query_order(row, qid[q], qcam[q], gid, gcam, uniq, separate_camera_set=True)
        assert info["n"] == n[q] and np.array_equal(info["high"], high[q, :n[q]])
        u = stream[starts[q]:starts[q + 1]].reshape(repeat, n[q])
        assert np.array_equal(m.query_ranks(info, u), rank[q]), q


# ---------------------------------------------------------------------------------------------------------------------------
# 7. the evaluators
# ---------------------------------------------------------------------------------------------------------------------------
def test_evaluate_all_single_shot(dev, capsys):
    import reid.evaluators as E
    from tests import rank_eval_hostmodel as RH
    d, qid, gid, qcam, gcam = C.load(GOLD, GOLD_EVAL, "narrow")
    dd = torch.from_numpy(d).to(dev)
    mAP, first, allshots = RH.summarize(*RH.per_query(d, qid, gid, qcam, gcam))
    np.random.seed(0)
    shot = M.run(d, qid, gid, qcam, gcam, topk=100, separate_camera_set=True)["curve"]
    want_state = _state()
    assert np.abs(shot[:C.TOPK] - GOLD[C.key("narrow", "sepcam", 0, "curve")]).max() <= TOL
    ids = dict(query_ids=qid, gallery_ids=gid, query_cams=qcam, gallery_cams=gcam)
    capsys.readouterr()
    np.random.seed(0)
    import inspect
    base, more = (list(inspect.signature(f).parameters.values()) for f in (E.evaluate_all_device, E.evaluate_all_single_shot))
    assert [str(p) for p in more[:-1]] == [str(p) for p in base] and str(more[-1]) == "single_shot=True"
    got = E.evaluate_all_single_shot(dd, **ids)
    lines = capsys.readouterr().out.splitlines()
    assert _same_state(_state(), want_state) and abs(got - allshots[0]) <= TOL
    assert lines[0] == "Mean AP: {:4.1%}".format(mAP)
    assert lines[1] == "CMC Scores{:>12}{:>12}{:>12}".format("allshots", "cuhk03", "market1501")
    assert lines[2:] == ["  top-{:<4}{:12.1%}{:12.1%}{:12.1%}".format(k, allshots[k - 1], shot[k - 1], first[k - 1]) for k in (1, 5, 10)]
    # dataset='cuhk03' returns (top-1, mAP), from a RandomState of the caller's
    np.random.seed(4)
    before = _state()
    top1, got_map = E.evaluate_all_single_shot(dd, dataset="cuhk03", single_shot=np.random.RandomState(0), **ids)
    lines = capsys.readouterr().out.splitlines()
    assert _same_state(_state(), before) and top1 == shot[0] and abs(got_map - mAP) <= TOL
    assert lines == ["Mean AP: {:4.1%}".format(mAP), "CMC Scores{:>12}".format("cuhk03")] + [
        "  top-{:<4}{:12.1%}".format(k, shot[k - 1]) for k in (1, 5, 10)]
    # evaluate_all_device, and single_shot=False here, keep the refusal, after the 'Mean AP' line
    for refuse in (lambda: E.evaluate_all_device(dd, dataset="cuhk03", **ids),
                   lambda: E.evaluate_all_single_shot(dd, dataset="cuhk03", single_shot=False, **ids)):
        with pytest.raises(NotImplementedError, match="single_gallery_shot"):
            refuse()
        assert capsys.readouterr().out.splitlines() == ["Mean AP: {:4.1%}".format(mAP)]
    assert _same_state(_state(), before)


def test_device_cascade_evaluator_single_shot(dev, capsys):
    import reid.evaluators as E
    from tests import cascade_hostmodel as H
    from tests import rank_eval_hostmodel as RH
    from tests.test_cascade_gpu import _Flatten, _embed, _synthetic_set
    D, k = 64, 4
    query, gallery, feats, loader = _synthetic_set(D)
    ev = E.DeviceCascadeEvaluator(_Flatten(), _embed(dev, H.make_input(5, 12, k, D, 2, seed=1)), single_shot=True)
    qid, gid = [p for _, p, _ in query], [p for _, p, _ in gallery]
    qcam, gcam = [c for _, _, c in query], [c for _, _, c in gallery]
    capsys.readouterr()
    np.random.seed(2)
    got = ev.evaluate(loader, query, gallery, rerank_topk=k)            # dataset=None: the three-column table, twice
    rest = [ln for ln in capsys.readouterr().out.splitlines() if not ln.startswith("Extract Features:")]
    merged = ev.last_distmat.cpu().numpy()
    mAP, first, allshots = RH.summarize(*RH.per_query(merged, qid, gid, qcam, gcam))
    assert abs(got - allshots[0]) <= TOL
    head = "CMC Scores{:>12}{:>12}{:>12}".format("allshots", "cuhk03", "market1501")
    assert rest[0] == "First stage evaluation:" and rest[2] == head and rest[6] == "Second stage evaluation:" and rest[8] == head
    assert rest[7] == "Mean AP: {:4.1%}".format(mAP) and len(rest) == 12
    # the second table's cuhk03 column: the stream goes on where the first stage's call left it
    probe = torch.stack([feats[n] for n, _, _ in query]).to(dev)
    gal = torch.stack([feats[n] for n, _, _ in gallery]).to(dev)
    stage1 = __import__("rg_hip").search.dist_block(probe, gal, 1.0, True).cpu().numpy()
    np.random.seed(2)
    M.run(stage1, qid, gid, qcam, gcam, topk=100, separate_camera_set=True)
    shot = M.run(merged, qid, gid, qcam, gcam, topk=100, separate_camera_set=True)["curve"]
    assert rest[9:] == ["  top-{:<4}{:12.1%}{:12.1%}{:12.1%}".format(t, allshots[t - 1], shot[t - 1], first[t - 1]) for t in (1, 5, 10)]
    # the default evaluator keeps the refusal
    with pytest.raises(NotImplementedError):
        E.DeviceCascadeEvaluator(ev.base_model, ev.embed_model).evaluate(loader, query, gallery, rerank_topk=k)
