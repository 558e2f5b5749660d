"""The k-means definition without a GPU: the numpy fp64 model of tests/kmeans_hostmodel.py is pinned (mt19937 known answer, the
permutation rule, scikit-learn's Lloyd iteration where it imports, the split rule on a hand-made case, the early-stop fixed
point), and the driver's validation that needs no device."""
import numpy as np
import pytest
import torch

from tests import kmeans_hostmodel as M

BLOB_SEEDS = (0, 2, 4, 5)


def test_mt19937_known_answer():
    # std::mt19937's default seed 5489 gives 3499211612 first (the C++ standard's check value is its 10000th draw, 4123659995)
    raw = M.mt19937_raw(5489, 10000)
    assert int(raw[0]) == 3499211612 and int(raw[9999]) == 4123659995
    assert raw.max() < 2 ** 32


@pytest.mark.parametrize("n,k,seed", [(600, 6, 1234), (5, 5, 0), (7, 1, 3), (1000, 999, 7), (2, 2, 1)])
def test_init_perm_is_a_prefix_of_a_permutation(n, k, seed):
    p = M.init_perm(n, k, seed)
    assert p.shape == (k,) and len(set(p.tolist())) == k and p.min() >= 0 and p.max() < n
    full = M.rand_perm(n, n, seed + 1)
    assert sorted(full.tolist()) == list(range(n)) and np.array_equal(full[:k], p)
    # the driver's copy of the rule is the model's
    from rg_hip import ops
    assert np.array_equal(ops.kmeans_rand_perm(n, k, seed + 1), p)


def test_rand_perm_first_swap_by_hand():
    # perm[0] <-> perm[0 + draw0 % n], perm[1] <-> perm[1 + draw1 % (n - 1)]
    n = 10
    d = M.mt19937_raw(42, 2)
    want = list(range(n))
    j = int(d[0]) % n
    want[0], want[j] = want[j], want[0]
    j = 1 + int(d[1]) % (n - 1)
    want[1], want[j] = want[j], want[1]
    assert M.rand_perm(n, 2, 42).tolist() == want[:2]


@pytest.mark.parametrize("seed", [s for s in BLOB_SEEDS if s != 4])      # seed 4 goes through a split: no scikit-learn counterpart
def test_lloyd_against_scikit_learn(seed):
    cluster = pytest.importorskip("sklearn.cluster")
    x, _ = M.blobs(seed)
    x = x.astype(np.float64)
    c0 = x[M.init_perm(x.shape[0], 6, 1234)]
    r = M.lloyd(x, c0, 300)
    assert r["n_split"] == 0 and np.bincount(r["labels"], minlength=6).min() > 0
    km = cluster.KMeans(n_clusters=6, init=c0, n_init=1, algorithm="lloyd", tol=0, max_iter=300).fit(x)
    assert r["converged"]
    assert np.array_equal(km.labels_, r["labels"])
    assert np.abs(km.cluster_centers_ - r["centroids"]).max() <= 1e-10


def test_at_least_three_blob_runs_reach_scikit_learn():
    runs = [M.lloyd(x.astype(np.float64), x.astype(np.float64)[M.init_perm(600, 6, 1234)], 300) for x, _ in map(M.blobs, BLOB_SEEDS)]
    assert sum(1 for r in runs if r["n_split"] == 0) >= 3 and [r["n_split"] for r in runs] == [0, 0, 1, 0]
    assert all(r["converged"] and 3 <= r["iterations"] <= 9 for r in runs)


def test_split_rule_by_hand():
    # clusters 1 and 4 are empty; 0 and 3 tie for the largest: 1 takes from 0 (lowest index), then 3 is the largest alone
    c = np.array([[2.0, -1.0, 3.0], [9.0, 9.0, 9.0], [1.0, 1.0, 1.0], [-2.0, 3.0, 0.0], [7.0, 7.0, 7.0]])
    cnt = np.array([10, 0, 3, 10, 0])
    c2, cnt2, ns = M.split(c, cnt)
    e = 1.0 / 1024.0
    assert ns == 2 and cnt2.tolist() == [5, 5, 3, 5, 5]
    assert np.array_equal(c2[1], c[0] * np.array([1 + e, 1 - e, 1 + e])) and np.array_equal(c2[0], c[0] * np.array([1 - e, 1 + e, 1 - e]))
    assert np.array_equal(c2[4], c[3] * np.array([1 + e, 1 - e, 1 + e])) and np.array_equal(c2[3], c[3] * np.array([1 - e, 1 + e, 1 - e]))
    assert np.array_equal(c2[2], c[2])
    # odd donor count: the empty cluster gets the smaller half; a donor of one member gives nothing away
    assert M.split(np.ones((2, 2)), np.array([0, 7]))[1].tolist() == [3, 4]
    assert M.split(np.ones((3, 2)), np.array([1, 0, 1]))[1].tolist() == [1, 0, 1]
    # nothing empty: untouched
    c3, cnt3, ns3 = M.split(c, np.array([1, 2, 3, 4, 5]))
    assert ns3 == 0 and np.array_equal(c3, c) and cnt3.tolist() == [1, 2, 3, 4, 5]


@pytest.mark.parametrize("case", ["blob4", "lattice"])
def test_early_stop_is_a_fixed_point(case):
    """the iteration after one whose labels repeat reproduces the same centroids, so stopping equals running on"""
    if case == "blob4":
        x, _ = M.blobs(4)
        c0 = x.astype(np.float64)[M.init_perm(600, 6, 1234)]
    else:
        x, c0 = M.lattice(20)
    r = M.lloyd(x, c0, 300)
    assert r["converged"] and r["iterations"] < 300
    c = r["centroids"]
    for _ in range(3):
        lab, _ = M.assign(x, c)
        assert np.array_equal(lab, r["labels"])
        cn, _, _ = M.split(M.update(x, lab, c), np.bincount(lab, minlength=c.shape[0]))
        assert np.array_equal(cn, c)
        c = cn
    # a cap equal to the iteration count gives the same run
    r2 = M.lloyd(x, c0, r["iterations"])
    assert r2["converged"] and np.array_equal(r2["labels"], r["labels"]) and np.array_equal(r2["centroids"], c) and r2["obj"] == r["obj"]


def test_lattice_run_of_the_model():
    x, c0 = M.lattice(20)
    r = M.lloyd(x, c0, 300, trace=True)
    assert (r["iterations"], r["n_split"], r["converged"]) == (15, 6, True) and r["cnt"].min() > 0
    # after the first iteration (all exact ties between the duplicated centroids, exact in any arithmetic) no row is near a tie
    assert all(not M.excused(x, c).any() for _, c in r["steps"][1:])


def test_tally_model():
    cnt, rowptr, order = M.tally(np.array([2, 0, 2, 2, 0]), 4)
    assert cnt.tolist() == [2, 0, 3, 0] and rowptr.tolist() == [0, 2, 2, 5, 5] and order.tolist() == [1, 4, 0, 2, 3]


def test_driver_validation_without_a_device():
    from rg_hip import ops
    x = torch.zeros((4, 3))
    with pytest.raises(ValueError):
        ops.kmeans(x, 5)                          # K > N
    with pytest.raises(ValueError):
        ops.kmeans(x, 0)                          # K = 0
    with pytest.raises(ValueError):
        ops.kmeans(torch.zeros((4,)), 2)          # wrong rank
    with pytest.raises(ValueError):
        ops.kmeans(torch.zeros((2, 3, 4)), 2)
    with pytest.raises(ValueError):
        ops.kmeans(torch.zeros((9000, 1)), ops.KMEANS_MAX_K + 1)
    with pytest.raises(ValueError):
        ops.kmeans(torch.zeros((4, ops.KMEANS_MAX_D + 1)), 2)
    with pytest.raises(ValueError):
        ops.kmeans(x, 2, check_every=0)
    with pytest.raises(TypeError):
        ops.kmeans(x, 2, 300, 1234, None, 4)      # max_points_per_centroid is keyword-only
