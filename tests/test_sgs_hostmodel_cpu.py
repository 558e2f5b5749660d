"""CPU: the numpy model of the single-gallery-shot CMC (tests/sgs_hostmodel.py) against the reference's recorded curves and
generator states (tests/golden/reference_sgs.npz), the vectorised draw against a loop of `np.random.choice`, five planted
defects that the fixture must catch, and the argument checks of `cmc_single_shot` that need no device.

Tolerance.  The reference adds 0.1 at most Q * repeat times into bins that hold at most Q, the model multiplies an integer
histogram by 0.1 once: for the largest case that is 400 additions of at most 40 * 2^-53 = 1.8e-12 before the division by
about 39 valid queries, 5e-14 after it; the bound is 1e-12.  Under first_match_break both sides are integers over
num_valid and must be equal.  The generator state must be equal in every case."""
import os

import numpy as np
import pytest

from tests import sgs_hostmodel as M
from tests.golden import cases_eval as CE
from tests.golden import cases_sgs as C

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(REPO, "tests", "golden", "reference_sgs.npz"))
GOLD_EVAL = np.load(os.path.join(REPO, "tests", "golden", "reference_eval.npz"))
TOL = 1e-12


def _state():
    s = np.random.get_state()
    return s[1].copy(), int(s[2])


def _same_state(a, b):
    return np.array_equal(a[0], b[0]) and a[1] == b[1]


def _fixture_mismatches(model, names=C.CASES):
    """the (case, configuration, seed) triples at which `model` misses the recorded curve or generator state"""
    bad = []
    for name in names:
        inputs = C.load(GOLD, GOLD_EVAL, name)
        for cfg, kw in C.CONFIGS.items():
            for seed in C.SEEDS:
                np.random.seed(seed)
                res = model.run(*inputs, topk=C.TOPK, repeat=C.REPEAT, **kw)
                want = GOLD[C.key(name, cfg, seed, "curve")]
                ok = np.array_equal(res["curve"], want) if kw["first_match_break"] else np.abs(res["curve"] - want).max() <= TOL
                ok = ok and _same_state(_state(), (GOLD[C.key(name, cfg, seed, "key")], int(GOLD[C.key(name, cfg, seed, "pos")])))
                if not ok:
                    bad.append((name, cfg, seed))
    return bad


def test_fixture_holds_what_the_cases_describe():
    assert os.path.getsize(os.path.join(REPO, "tests", "golden", "reference_sgs.npz")) < 256 * 1024
    for name in C.CASES:
        got = C.load(GOLD, GOLD_EVAL, name)
        want = C.make_inputs(name)
        assert all(np.array_equal(a, b) and a.dtype == b.dtype for a, b in zip(got, want)), name
        assert CE.rows_tie_free(got[0]) and got[0].shape[0] <= 40, name
        for cfg in C.CONFIGS:
            for seed in C.SEEDS:
                assert GOLD[C.key(name, cfg, seed, "curve")].shape == (C.TOPK,) and GOLD[C.key(name, cfg, seed, "key")].shape == (624,)
    d, qid, gid, qcam, gcam = C.load(GOLD, GOLD_EVAL, "bigseg")
    sizes = np.bincount(gid)
    assert len(np.unique(gid)) == 65 and sizes.max() >= 700 and (qid == np.argmax(sizes)).sum() >= 4
    assert set(GOLD.files) == {"bigseg_%s" % k for k in ("dist", "qid", "gid", "qcam", "gcam")} | {
        C.key(n, c, s, w) for n in C.CASES for c in C.CONFIGS for s in C.SEEDS for w in ("curve", "key", "pos")}


@pytest.mark.parametrize("name", C.CASES)
def test_model_equals_reference(name):
    assert _fixture_mismatches(M.Model(), [name]) == []
    # fp64 inputs and a RandomState of its own give the same curve and leave the global generator alone
    inputs = C.load(GOLD, GOLD_EVAL, name)
    np.random.seed(5)
    before = _state()
    rs = np.random.RandomState(11)
    res = M.run(inputs[0].astype(np.float64), *inputs[1:], topk=C.TOPK, random_state=rs, **C.CONFIGS["sepcam"])
    assert np.abs(res["curve"] - GOLD[C.key(name, "sepcam", 11, "curve")]).max() <= TOL
    assert _same_state(_state(), before)
    assert np.array_equal(rs.get_state()[1], GOLD[C.key(name, "sepcam", 11, "key")])
    if name == "wide":
        assert res["n"][0] == 0 and (res["rank"][0] == -1).all() and (res["n"][1:] > 0).all()       # the skipped query
    if name == "bigseg":
        assert res["high"].max() >= 200 and 60 <= res["n"].max() <= 65


def test_vectorised_draw_equals_a_loop_of_choice():
    g = np.random.RandomState(2)
    lengths = np.concatenate([[1, 2, 65536, 70000, 1, 1, 3, 2 ** 16 - 1, 2 ** 16 + 1], g.randint(1, 40, size=300),
                              g.randint(1, 5000, size=60), [1, 70000, 65536, 2, 1]])
    lists = {n: list(range(n)) for n in set(lengths.tolist())}
    for seed in (0, 11):
        np.random.seed(seed)
        want = np.array([np.random.choice(lists[n]) for n in lengths.tolist()])
        want_state = _state()
        np.random.seed(seed)
        got = M.draw(None, lengths)
        assert np.array_equal(got, want) and _same_state(_state(), want_state)
        rs = np.random.RandomState(seed)
        assert np.array_equal(M.draw(rs, lengths), want) and np.array_equal(rs.get_state()[1], want_state[0])
        # drawn in pieces: the same stream
        np.random.seed(seed)
        parts = np.concatenate([M.draw(None, lengths[:7]), M.draw(None, lengths[7:200]), M.draw(None, lengths[200:])])
        assert np.array_equal(parts, want) and _same_state(_state(), want_state)
    np.random.seed(3)
    before = _state()
    assert np.array_equal(M.draw(None, np.ones(50, dtype=np.int64)), np.zeros(50)) and _same_state(_state(), before)   # length 1 consumes nothing


# ---- planted defects: each copy of the model must miss the fixture ------------------------------------------------------------
class _IdOrderDraws(M.Model):
    """draws assigned in identity order instead of first-appearance order"""

    def id_order(self, kept_ids):
        return np.unique(kept_ids)


class _IdMajorDraws(M.Model):
    """the stream read identity-major instead of repeat-major"""

    def highs_of(self, info, repeat):
        return np.zeros(0, dtype=np.int64) if info["skip"] else np.repeat(info["high"], repeat)

    def draws_of(self, flat, info, repeat):
        return np.asarray(flat).reshape(info["n"], repeat).T


class _ReversedTies(M.Model):
    """equal distances ordered by DEscending gallery index"""

    def sort_row(self, d_row):
        return np.lexsort((-np.arange(len(d_row)), d_row))


class _SkippedDraws(M.Model):
    """a query without a valid match consumes draws for the identities it sees"""

    def highs_of(self, info, repeat):
        return np.tile(info["high"], repeat)


class _OwnCounted(M.Model):
    """the own identity counted among those before it"""

    def rank_of(self, sampled, own):
        return int((sampled <= sampled[own]).sum())


@pytest.mark.parametrize("defect", [_IdOrderDraws, _IdMajorDraws, _SkippedDraws, _OwnCounted])
def test_planted_defect_misses_the_fixture(defect):
    bad = _fixture_mismatches(defect())
    print("%s: %d of %d fixture comparisons fail" % (defect.__name__, len(bad), len(C.CASES) * len(C.CONFIGS) * len(C.SEEDS)))
    assert bad, defect.__doc__
    if defect is _SkippedDraws:
        # exactly the (case, configuration) pairs in which a query is skipped
        skips = {(name, cfg) for name in C.CASES for cfg, kw in C.CONFIGS.items()
                 if (M.run(*C.load(GOLD, GOLD_EVAL, name), topk=C.TOPK, random_state=np.random.RandomState(0), **kw)["n"] == 0).any()}
        assert {b[:2] for b in bad} == skips and ("wide", "plain") in skips and len(bad) == 2 * len(skips)
    else:
        assert {b[0] for b in bad} == set(C.CASES)


def test_reversed_tie_rule_shows_on_a_tied_input():
    # tie-free rows do not see the rule ...
    assert _fixture_mismatches(_ReversedTies(), ["narrow"]) == []
    # ... the quantised case does, against the model itself
    inputs = CE.load(GOLD_EVAL, "tied")
    for kw in C.CONFIGS.values():
        a = M.run(*inputs, topk=C.TOPK, random_state=np.random.RandomState(0), **kw)
        b = _ReversedTies().run(*inputs, topk=C.TOPK, random_state=np.random.RandomState(0), **kw)
        assert np.array_equal(a["n"], b["n"])
        assert not np.array_equal(a["rank"], b["rank"]) and not np.array_equal(a["curve"], b["curve"])


def test_per_query_part_stands_alone():
    d, qid, gid, qcam, gcam = C.load(GOLD, GOLD_EVAL, "edge_ids")
    m = M.Model()
    whole = m.run(d, qid, gid, qcam, gcam, topk=C.TOPK, random_state=np.random.RandomState(4))
    rs = np.random.RandomState(4)
    uniq = np.unique(gid)
    for i in range(len(d)):
        info = m.query_order(d[i], qid[i], qcam[i], gid, gcam, uniq)
        assert info["n"] == whole["n"][i]
        if info["skip"]:
            continue
        u = M.draw(rs, np.tile(info["high"], C.REPEAT)).reshape(C.REPEAT, info["n"])
        assert np.array_equal(m.query_ranks(info, u), whole["rank"][i])
        assert np.array_equal(info["slot"], whole["slot"][i, :info["n"]]) and (u < info["high"][None, :]).all()
    # one hand-made row: id 7 / camera 0; the same-camera entry of id 7 is junk; ids in first-appearance order 3, 7, 5
    row = np.array([0.05, 0.1, 0.2, 0.3, 0.4, 0.5])
    gid2, gcam2 = np.array([7, 3, 7, 5, 3, 7]), np.array([0, 1, 1, 1, 1, 1])
    info = m.query_order(row, 7, 0, gid2, gcam2, np.unique(gid2))
    assert info["ids"].tolist() == [3, 7, 5] and info["high"].tolist() == [2, 2, 1] and info["own"] == 1 and info["slot"].tolist() == [0, 2, 1]
    # draws (id 3 -> its 2nd entry d 0.4, id 7 -> its 1st d 0.2, id 5 -> d 0.3): nobody before 0.2; then id 7 -> d 0.5: both before
    assert m.query_ranks(info, np.array([[1, 0, 0], [1, 1, 0], [0, 0, 0]])).tolist() == [0, 2, 1]


def test_argument_checks_need_no_device():
    from clustercontrast.evaluation_metrics import cmc_single_shot
    import reid.evaluation_metrics as RE
    import clustercontrast.evaluation_metrics.ranking as R
    import inspect
    assert RE.cmc_single_shot is cmc_single_shot is R.cmc_single_shot
    assert str(inspect.signature(cmc_single_shot)) == (
        "(distmat, query_ids=None, gallery_ids=None, query_cams=None, gallery_cams=None, topk=100, separate_camera_set=False, "
        "first_match_break=False, repeat=10, random_state=None, chunk=0, debug=False)")
    d = np.zeros((2, 3), dtype=np.float32)
    np.random.seed(9)
    before = _state()
    with pytest.raises(ValueError, match="repeat"):
        cmc_single_shot(d, repeat=0)
    with pytest.raises(ValueError, match="topk"):
        cmc_single_shot(d, topk=0)
    with pytest.raises(ValueError, match="entries"):
        cmc_single_shot(d, query_ids=[1, 2, 3])
    with pytest.raises(ValueError, match="entries"):
        cmc_single_shot(d, gallery_cams=[1, 2])
    with pytest.raises(ValueError, match="integers"):
        cmc_single_shot(d, gallery_ids=np.array([1.0, 2.0, 3.0]))
    with pytest.raises(ValueError, match="matrix"):
        cmc_single_shot(np.zeros(3, dtype=np.float32))
    assert _same_state(_state(), before)
    # the refusal of cmc(single_gallery_shot=True) still stands and names the opt-in
    with pytest.raises(NotImplementedError, match="single_gallery_shot") as e:
        R.cmc(d, single_gallery_shot=True)
    assert "cmc_single_shot" in str(e.value)
