"""The blocked search of rg_hip.search at the smallest sizes that have a block boundary, through every recipe that uses it, and the
shared epilogue of the pseudo-labelling recipes.

The search inputs are small integers, so every inner product, squared norm and combination of them is exact in fp32 whatever tile
or split-K plan the GEMM picks for a block height: a 1-row, a 32-row and a 70-row block must give the same bits, and the tables are
compared entry for entry with an int64 numpy model (score descending, column ascending: a stable argsort of the negated score)."""
import numpy as np
import pytest
import torch

from rg_hip import search
from tests import infomap_hostmodel as IM
from tests.golden import cases_rerank as C

pytestmark = pytest.mark.gpu

N, D, K = 70, 16, 5
BLOCKS = (70, 32, 1)          # one block; two full blocks and a ragged one of 6 rows; a block per row


def _rows():
    x = np.random.RandomState(0).randint(-3, 4, size=(N, D)).astype(np.int64)
    x[40], x[69] = x[10], x[11]          # exact ties that straddle the 32-row blocks
    return x


X = _rows()
DOT = X @ X.T
L2_SCORE = 2 * DOT - np.diag(DOT)[None, :]


def _top(score, k):
    return np.argsort(-score, axis=1, kind="stable")[:, :k]


@pytest.mark.parametrize("rows", BLOCKS)
def test_l2_rank_across_block_boundaries(dev, monkeypatch, rows):
    from clustercontrast.utils.faiss_rerank import l2_rank
    monkeypatch.setattr(search, "BLOCK_ROWS", rows)
    rank = l2_rank(torch.from_numpy(X.astype(np.float32)).to(dev), K)
    assert rank.dtype == torch.int32 and tuple(rank.shape) == (N, K)
    want = _top(L2_SCORE, K)
    assert want[10, :2].tolist() == [10, 40] and want[69, :2].tolist() == [11, 69]          # the ties are in the table
    assert np.array_equal(rank.cpu().numpy(), want)


@pytest.mark.parametrize("rows", BLOCKS)
def test_knn_faiss_across_block_boundaries(dev, monkeypatch, rows):
    from clustercontrast.utils.infomap_cluster import get_dist_nbr, knn_faiss
    monkeypatch.setattr(search, "BLOCK_ROWS", rows)
    x = X.astype(np.float32)
    index = knn_faiss(x, K, verbose=False)
    want = _top(DOT, K)
    sims = np.take_along_axis(DOT, want, axis=1)
    assert index.nbrs.dtype == torch.int32 and np.array_equal(index.nbrs.cpu().numpy(), want)
    assert index.sims.dtype == torch.float32 and np.array_equal(index.sims.cpu().numpy().astype(np.int64), sims)
    assert np.array_equal(index.sims.cpu().numpy(), sims.astype(np.float32))
    dists, nbrs = get_dist_nbr(x, K, return_device=True)
    assert np.array_equal(nbrs.cpu().numpy(), want) and np.array_equal(dists.cpu().numpy(), (1 - sims).astype(np.float32))


def test_rank_topk_blocked_equals_unblocked(dev, monkeypatch):
    from reid.evaluators import rank_topk
    g = np.random.RandomState(1)
    d = np.stack([g.permutation(23) for _ in range(9)]).astype(np.float32)
    d[8, 17] = d[8, 4] = -1.0                 # two equal minima: the lower column comes first
    want = np.argsort(d, axis=1, kind="stable")[:, :7]
    assert want[8, :2].tolist() == [4, 17]
    got = {}
    for rows in (4, 2048):
        monkeypatch.setattr(search, "BLOCK_ROWS", rows)
        got[rows] = rank_topk(d, 7)
        assert got[rows].dtype == torch.int64 and got[rows].is_cuda
        assert np.array_equal(got[rows].cpu().numpy(), want)
    assert torch.equal(got[4], got[2048])


def test_re_ranking_blocked_equals_unblocked(dev, monkeypatch):
    from clustercontrast.utils.rerank import re_ranking
    x = C.make_features(6, 4, 16, 0.35, seed=0)
    dist = np.sqrt(C.sq_l2(x)).astype(np.float32)
    Q = 5
    q_g, q_q, g_g = dist[:Q, Q:].copy(), dist[:Q, :Q].copy(), dist[Q:, Q:].copy()
    assert q_g.shape == (5, 19)
    got = {}
    for rows in (8, 2048):
        monkeypatch.setattr(search, "BLOCK_ROWS", rows)
        got[rows] = re_ranking(q_g, q_q, g_g, k1=6, k2=3, return_device=True)
    assert got[8].is_cuda and tuple(got[8].shape) == (5, 19) and torch.equal(got[8], got[2048])


def test_pseudo_labels_without_a_cluster(dev):
    from clustercontrast.utils.pseudo_labels import dbscan_pseudo_labels
    x = 10.0 * torch.eye(8, 12)               # with k1 = 1 every row's neighbour set is itself: Jaccard distance 1 to all others
    labels, num_cluster, centroids = dbscan_pseudo_labels(x, k1=1, k2=1, eps=0.6, min_samples=4)
    assert isinstance(labels, np.ndarray) and labels.dtype == np.int64 and labels.tolist() == [-1] * 8 and num_cluster == 0
    assert centroids.is_cuda and centroids.dtype == torch.float32 and tuple(centroids.shape) == (0, 12)


def test_pseudo_labels_centroids_equal_the_host_loop(dev):
    from clustercontrast.utils.infomap_cluster import generate_cluster_features
    from clustercontrast.utils.pseudo_labels import dbscan_pseudo_labels, infomap_pseudo_labels, kmeans_pseudo_labels
    x, planted = IM.blobs(8, 10, 32, 0.05, seed=1)
    xt = torch.from_numpy(x)
    labels, num_cluster, centroids = dbscan_pseudo_labels(xt, k1=8, k2=3, eps=0.6, min_samples=4)
    assert num_cluster >= 1 and labels.dtype == np.int64 and labels.shape == (80,)
    assert tuple(centroids.shape) == (num_cluster, 32) and torch.equal(centroids, generate_cluster_features(labels, xt))
    labels, centroids, info = infomap_pseudo_labels(xt, k=8, min_sim=0.5, cluster_num=4)
    assert info["n_clusters"] >= 1 and labels.dtype == np.int64
    xn = torch.nn.functional.normalize(xt.to(dev), dim=1)          # the recipe clusters and averages the normalised rows
    assert tuple(centroids.shape) == (info["n_clusters"], 32) and torch.equal(centroids, generate_cluster_features(labels, xn))
    labels, centroids, info = kmeans_pseudo_labels(xt, num_classes=8)
    assert labels.dtype == np.int64 and labels.min() >= 0 and centroids.is_cuda
    assert tuple(centroids.shape) == (len(np.unique(labels)), 32) and torch.equal(centroids, generate_cluster_features(labels, xt))
