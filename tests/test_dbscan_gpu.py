"""DBSCAN pseudo-labelling on the device (csrc/dbscan.hip) through ops.dbscan*, clustercontrast.utils.dbscan.DBSCAN and
clustercontrast.utils.pseudo_labels, against the reference's recorded labels (tests/golden/reference_rerank.npz) and the
numpy model of scikit-learn's rules (tests/dbscan_hostmodel.py, tied to scikit-learn by tests/test_dbscan_cpu.py).
Labels are integers: every comparison is for equality."""
import os

import numpy as np
import pytest
import torch

from tests import dbscan_hostmodel as M
from tests.golden import cases_rerank as C

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(REPO, "tests", "golden", "reference_rerank.npz"))
EPS, MS = C.DBSCAN_EPS, C.DBSCAN_MIN_SAMPLES


def _cjd(x, **kw):
    from clustercontrast.utils.faiss_rerank import compute_jaccard_distance
    return compute_jaccard_distance(torch.from_numpy(np.ascontiguousarray(x)), print_flag=False, **kw)


def _lists(dbg):
    rowptr, nbr = dbg["rowptr"].cpu().numpy().astype(np.int64), dbg["nbr"].cpu().numpy().astype(np.int64)
    assert rowptr[0] == 0 and rowptr[-1] == len(nbr) and (np.diff(rowptr) >= 0).all()
    return [nbr[rowptr[i]:rowptr[i + 1]] for i in range(len(rowptr) - 1)]


def _check_against_model(d, eps, ms, dev):
    """every stage of ops.dbscan on the host matrix d (uploaded as it is) against the model; returns the labels"""
    from rg_hip import ops
    want_lists = M.neighbor_lists(d, eps)
    want, want_core, want_parent = M.labels_from_lists(want_lists, ms)
    labels, n_clusters, dbg = ops.dbscan(torch.from_numpy(d).to(dev), eps, ms, debug=True)
    assert labels.dtype == torch.int64 and tuple(labels.shape) == (len(d),)
    got_lists = _lists(dbg)
    assert all(np.array_equal(a, b) for a, b in zip(got_lists, want_lists)), "neighbour lists differ"
    assert np.array_equal(np.nonzero(dbg["core"].cpu().numpy())[0], want_core)
    assert np.array_equal(dbg["parent"].cpu().numpy(), want_parent)
    assert np.array_equal(labels.cpu().numpy(), want)
    assert n_clusters == int(want.max()) + 1
    return want


@pytest.mark.parametrize("name", ["a", "c"])
def test_labels_equal_reference(dev, name):
    from clustercontrast.utils.dbscan import DBSCAN
    cs, x = C.CASES[name], GOLD[name + "_x"]
    n = len(x)
    ref = C.unpack_upper(GOLD[name + "_jaccard_upper"], n)
    off = ref[~np.eye(n, dtype=bool)]
    assert np.abs(off - EPS).min() > 1e-2               # no reference entry near eps: the labels cannot hinge on rounding
    want = GOLD[name + "_dbscan"]
    cluster = DBSCAN(eps=EPS, min_samples=MS, metric="precomputed", n_jobs=-1)
    got = cluster.fit_predict(ref)
    assert got.dtype == np.int64 and np.array_equal(got, want)
    assert cluster.n_clusters_ == cs["n_id"] and np.array_equal(cluster.labels_device_.cpu().numpy(), want)
    assert cluster.core_sample_indices_.dtype == np.int64
    assert np.array_equal(cluster.core_sample_indices_, M.dbscan(ref, EPS, MS)[1])
    # the device's own Jaccard matrix, never copied to the host, and the same matrix as a numpy array
    J = _cjd(x, k1=cs["k1"], k2=cs["k2"], return_device=True)
    assert torch.is_tensor(J) and J.is_cuda and J.dtype == torch.float32 and tuple(J.shape) == (n, n)
    assert np.array_equal(DBSCAN(eps=EPS, min_samples=MS).fit_predict(J), want)
    Jh = _cjd(x, k1=cs["k1"], k2=cs["k2"])
    assert np.array_equal(Jh, J.cpu().numpy())
    assert np.array_equal(DBSCAN(eps=EPS, min_samples=MS).fit_predict(Jh), want)
    assert np.array_equal(DBSCAN(eps=EPS, min_samples=MS).fit_predict(torch.from_numpy(Jh)), want)
    # float16 matrix (use_float16=True upstream): entries are at least 1e-2 from eps, half rounding is 5e-4 at most
    assert np.array_equal(DBSCAN(eps=EPS, min_samples=MS).fit_predict(Jh.astype(np.float16)), want)


def test_random_point_sets_equal_the_model(dev):
    shared = 0
    for seed in range(200):
        d, eps, ms = M.random_case(seed)
        _check_against_model(d, eps, ms, dev)
        shared += M.shared_border_points(d, eps, ms)
    assert shared > 0
    for seed in range(0, 200, 10):                      # float16 entries: 8 per 16-byte load, rows rarely aligned
        d, eps, ms = M.random_case(seed)
        d16 = d.astype(np.float16)
        assert np.abs(d16.astype(np.float32) - np.float32(eps)).min() > 5e-3
        _check_against_model(d16, eps, ms, dev)


def _far(n):
    d = np.full((n, n), 0.9, dtype=np.float32)
    np.fill_diagonal(d, 0)
    return d


def _link(d, a, b):
    d[a, b] = d[b, a] = 0.1


def test_long_chain_in_shuffled_order(dev):
    """4 000 core points in one path whose order along the path is a random permutation of the indices: component
    diameter 3 999, one cluster, rooted at index 0"""
    n = 4000
    perm = np.random.RandomState(0).permutation(n)
    d = _far(n)
    _link(d, perm[:-1], perm[1:])
    want = _check_against_model(d, 0.5, 2, dev)
    assert (want == 0).all()


def test_two_chains_joined_through_a_non_core_point(dev):
    """the bridge (its own diagonal above eps: two neighbours, below min_samples = 3) must not merge the chains and takes
    the lower cluster number; the chain ends are border points too"""
    n = 203
    perm = np.random.RandomState(1).permutation(n)
    a, b, bridge = perm[:101], perm[101:202], perm[202]
    d = _far(n)
    _link(d, a[:-1], a[1:])
    _link(d, b[:-1], b[1:])
    _link(d, bridge, a[50])
    _link(d, bridge, b[50])
    d[bridge, bridge] = 0.9
    want = _check_against_model(d, 0.5, 3, dev)
    assert int(want.max()) == 1 and (want >= 0).all()
    assert want[a[50]] != want[b[50]] and want[bridge] == 0
    assert len(set(want[a])) == 1 and len(set(want[b])) == 1


def test_star_noise_and_one_big_cluster(dev):
    n = 131                                              # not a multiple of 64, odd: rows start at every alignment
    star = _far(n)
    _link(star, 77, np.delete(np.arange(n), 77))
    want = _check_against_model(star, 0.5, 3, dev)       # leaves: themselves + the centre = 2 < 3
    assert (want == 0).all()
    noise = np.full((n, n), 0.9, dtype=np.float32)       # diagonal included: no neighbour at all, an empty list
    want = _check_against_model(noise, 0.5, 1, dev)
    assert (want == -1).all()
    want = _check_against_model(np.zeros((300, 300), dtype=np.float32), 0.5, 4, dev)
    assert (want == 0).all()
    # exactly eps (representable) is a neighbour
    tie = _far(5)
    tie[0, 1] = tie[1, 0] = 0.5
    want = _check_against_model(tie, 0.5, 2, dev)
    assert want.tolist() == [0, 0, -1, -1, -1]
    one = np.zeros((1, 1), dtype=np.float32)
    assert _check_against_model(one, 0.5, 1, dev).tolist() == [0]
    assert _check_against_model(one, 0.5, 2, dev).tolist() == [-1]


def test_deterministic_across_runs_and_streams(dev):
    from rg_hip import ops
    x = C.make_features(150, 20, 256, 0.30, seed=7)
    J = _cjd(x, k1=30, k2=6, return_device=True)
    first = ops.dbscan(J, EPS, MS, debug=True)
    second = ops.dbscan(J, EPS, MS, debug=True)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        third = ops.dbscan(J, EPS, MS, debug=True)
    side.synchronize()
    for other in (second, third):
        assert torch.equal(first[0], other[0]) and first[1] == other[1]
        for key in ("rowptr", "nbr", "core", "parent"):
            assert torch.equal(first[2][key], other[2][key]), key


def test_pseudo_labels_end_to_end(dev):
    """3 000 rows (150 identities x 20): labels against the model on the numpy Jaccard matrix, centroids bit for bit against
    the host-loop generate_cluster_features.  The model on the host-computed Jaccard matrix (tests/rerank_hostmodel.py)
    gives 150 clusters of 20 and no outlier for this input, which is what the construction suggests."""
    from clustercontrast.utils.infomap_cluster import generate_cluster_features
    from clustercontrast.utils.pseudo_labels import dbscan_pseudo_labels
    x = C.make_features(150, 20, 256, 0.30, seed=7)
    feats = torch.from_numpy(x)
    labels, num_cluster, centroids = dbscan_pseudo_labels(feats, k1=30, k2=6, eps=EPS, min_samples=MS)
    assert isinstance(labels, np.ndarray) and labels.dtype == np.int64 and labels.shape == (3000,)
    J = _cjd(x, k1=30, k2=6)
    print("3000 rows: smallest |J - eps| = %.3e" % float(np.abs(J - np.float32(EPS)).min()))
    want, _, n_want = M.dbscan(J, EPS, MS)
    print("3000 rows: model gives %d clusters, %d outliers" % (n_want, int((want < 0).sum())))
    assert np.array_equal(labels, want) and num_cluster == n_want
    assert centroids.is_cuda and centroids.dtype == torch.float32 and tuple(centroids.shape) == (num_cluster, 256)
    assert torch.equal(centroids, generate_cluster_features(labels, feats))
    assert num_cluster == 150 and (labels >= 0).all() and (np.bincount(labels) == 20).all()
    # a device tensor as input, and labels with outliers in them, through the device-side centroid helper
    from clustercontrast.utils.infomap_cluster import generate_cluster_features_device
    labels2, num2, centroids2 = dbscan_pseudo_labels(feats.to(dev), k1=30, k2=6, eps=EPS, min_samples=MS)
    assert np.array_equal(labels2, labels) and num2 == num_cluster and torch.equal(centroids2, centroids)
    holes = labels.copy()
    holes[::7] = -1
    holes[holes == 3] = -1                               # a label that disappears: rows stay in ascending label order
    assert torch.equal(generate_cluster_features_device(torch.from_numpy(holes).to(dev), feats),
                       generate_cluster_features(holes, feats))


@pytest.mark.timeout(120)          # measured: 0.5 s; the bound test_rerank_gpu.test_market_size uses for its 4 s
def test_market_size(dev):
    """N = 12 936 (646 identities x 20 + 16 singles, the input of test_rerank_gpu.test_market_size): the matrix stays on the
    device, only the CSR lists come back; 64 sampled rows of them are checked against the matrix rows, the model runs on
    the lists.  The feature must not copy the matrix: peak memory grows by less than one [N, N] fp32 matrix."""
    from clustercontrast.utils.dbscan import DBSCAN
    from clustercontrast.utils.faiss_rerank import compute_jaccard_distance
    from rg_hip import ops
    D = 2048
    g = np.random.RandomState(3)
    singles = g.randn(16, D)
    singles /= np.linalg.norm(singles, axis=1, keepdims=True)
    x = np.concatenate([C.make_features(646, 20, D, 0.30, seed=3), singles.astype(np.float32)])
    n = len(x)
    assert n == 12936
    J = compute_jaccard_distance(torch.from_numpy(x).to(dev), k1=30, k2=6, print_flag=False, return_device=True)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated(dev)
    torch.cuda.reset_peak_memory_stats(dev)
    labels, n_clusters, dbg = ops.dbscan(J, EPS, MS, debug=True)
    torch.cuda.synchronize()
    grown = torch.cuda.max_memory_allocated(dev) - base
    print("market size: peak memory grows by %.1f MB over the Jaccard output (%.1f MB)" % (grown / 1e6, n * n * 4 / 1e6))
    assert grown < n * n * 4
    lists = _lists(dbg)
    assert all((np.diff(nb) > 0).all() for nb in lists)
    rows = np.sort(g.choice(n, 64, replace=False))
    sampled = J[torch.from_numpy(rows).to(dev)].cpu().numpy()
    for r, row in zip(rows, sampled):
        assert np.array_equal(lists[r], np.nonzero(row <= np.float32(EPS))[0]), r
    want, want_core, want_parent = M.labels_from_lists(lists, MS)
    print("market size: nnz %d, model gives %d clusters, %d outliers, %d core points"
          % (sum(len(nb) for nb in lists), int(want.max()) + 1, int((want < 0).sum()), len(want_core)))
    assert np.array_equal(labels.cpu().numpy(), want) and n_clusters == int(want.max()) + 1
    assert np.array_equal(dbg["parent"].cpu().numpy(), want_parent)
    assert np.array_equal(np.nonzero(dbg["core"].cpu().numpy())[0], want_core)
    # the construction suggests 646 clusters of 20 and 16 outliers.  The model says otherwise about the singles (measured:
    # nnz 259 056 = 12 920 x 20 + 16 x 41, 12 936 core points, 646 clusters, 0 outliers): each single lies within eps of all
    # 20 members of one identity (members of an identity share their nearest strangers, so the single is k-reciprocal with
    # all of them) and is a core point of that cluster.  Asserted: the identities, and agreement with the model above.
    assert n_clusters == 646
    sizes = np.bincount(want[want >= 0])
    assert sizes.min() >= 20 and sizes.sum() + int((want < 0).sum()) == n
    ident = want[:12920]
    assert (ident >= 0).all() and (np.bincount(ident, minlength=646) == 20).all()
    cluster = DBSCAN(eps=EPS, min_samples=MS, n_jobs=-1, check_symmetric=True).fit(J)
    assert np.array_equal(cluster.labels_, want) and np.array_equal(cluster.core_sample_indices_, want_core)


def test_check_symmetric(dev):
    from clustercontrast.utils.dbscan import DBSCAN
    from rg_hip import ops
    x = GOLD["a_x"]
    J = _cjd(x, k1=20, k2=6, return_device=True)
    assert ops.dbscan_asymmetry(J) == 0
    want = DBSCAN(eps=EPS, min_samples=MS, check_symmetric=True).fit_predict(J)
    assert np.array_equal(want, GOLD["a_dbscan"])
    bad = J.clone()
    bad[5, 130] = torch.nextafter(bad[5, 130], torch.tensor(2.0, device=dev))
    assert ops.dbscan_asymmetry(bad) == 1
    with pytest.raises(ValueError, match="not symmetric"):
        DBSCAN(eps=EPS, min_samples=MS, check_symmetric=True).fit(bad)
    DBSCAN(eps=EPS, min_samples=MS).fit(bad)             # unchecked by default
    assert ops.dbscan_asymmetry(bad.half()) == int((bad.half() != bad.half().t()).sum().item()) // 2


def test_bad_arguments(dev):
    from rg_hip import ops
    d = torch.zeros((64, 64), device=dev)
    with pytest.raises(ValueError, match="contiguous"):
        ops.dbscan_neighbors(d.t()[::2, ::2], 0.5, 2)
    with pytest.raises(TypeError, match="float32"):
        ops.dbscan_neighbors(d.double(), 0.5, 2)
    with pytest.raises(ValueError, match="square"):
        ops.dbscan_neighbors(d[:, :32].contiguous(), 0.5, 2)
    with pytest.raises(ValueError, match="min_samples"):
        ops.dbscan_neighbors(d, 0.5, 0)
    rowptr, nbr, core = ops.dbscan_neighbors(d, 0.5, 2)
    with pytest.raises(TypeError, match="int32"):
        ops.dbscan_components(rowptr.long(), nbr, core)
    with pytest.raises(ValueError, match="disagree"):
        ops.dbscan_components(rowptr[:-1].contiguous(), nbr, core)
    with pytest.raises(ValueError, match="disagree"):
        ops.dbscan_labels(rowptr, nbr, core, core[:-1].contiguous())
    # the C ABI itself: status + message, no launch
    from rg_hip.lib import lib
    p = rowptr.data_ptr()
    with pytest.raises(RuntimeError, match="rg_dbscan_count"):
        lib.rg_dbscan_count(None, 0, 64, 64, 0.5, p, p, 0)
    with pytest.raises(RuntimeError, match="rg_dbscan_count"):
        lib.rg_dbscan_count(d.data_ptr(), 0, 1 << 20, 1 << 20, 0.5, p, p, 0)
    with pytest.raises(RuntimeError, match="rg_dbscan_fill"):
        lib.rg_dbscan_fill(d.data_ptr(), 0, 64, 32, 0.5, 2, p, p, p, 0)
    with pytest.raises(RuntimeError, match="min_samples"):
        lib.rg_dbscan_fill(d.data_ptr(), 0, 64, 64, 0.5, 0, p, p, p, 0)
    with pytest.raises(RuntimeError, match="rg_dbscan_components"):
        lib.rg_dbscan_components(p, p, p, 0, p, 0)
    with pytest.raises(RuntimeError, match="rg_dbscan_labels"):
        lib.rg_dbscan_labels(p, p, None, 64, p, p, p, 0)
    with pytest.raises(RuntimeError, match="rg_dbscan_asymmetry"):
        lib.rg_dbscan_asymmetry(d.data_ptr(), 2, 64, 64, p, 0)
