"""The numpy model of the two-level Infomap (tests/infomap_hostmodel.py), pinned without a GPU: the cross-check values of the
definition on the ring-of-cliques fixtures, the link rules, the post-processing, and the refusal of
cluster_by_infomap off the GPU."""
import numpy as np
import pytest
import torch

from tests import infomap_hostmodel as M


def _ring(c, s):
    nbrs, dists, planted = M.ring_of_cliques(c, s)
    src, dst, w, single = M.links(nbrs, dists, 0.5)
    node_flow, q, iters = M.flow(c * s, src, dst, w)
    return nbrs, dists, planted, src, dst, w, single, node_flow, q, iters


@pytest.mark.parametrize("c,s", M.RINGS)
def test_ring_table(c, s):
    n_links, l_planted, l_one, l_single, l_merge = M.RING_TABLE[(c, s)]
    nbrs, dists, planted, src, dst, w, single, node_flow, q, iters = _ring(c, s)
    N = c * s
    assert nbrs.shape == (N, s + 2) and len(src) == n_links and not single.any() and iters < M.FLOW_MAX_ITERS
    assert abs(q.sum() - 1.0) < 1e-12 and abs(node_flow.sum() - 1.0) < 1e-12

    def L(lab):
        return M.codelength(src, dst, q, node_flow, lab)
    assert round(L(planted), 4) == l_planted
    assert round(L(np.zeros(N, dtype=np.int64)), 4) == l_one
    assert round(L(np.arange(N)), 4) == l_single
    merges = [L(np.where(planted == (g + 1) % c, g, planted)) for g in range(c)]
    assert round(min(merges), 4) == l_merge
    # every single-node move out of the planted partition costs at least 0.11 bits: exact recovery is a fair demand
    adj = M._adjacency(N, src, dst)
    base = L(planted)
    for i in range(N):
        for b in sorted({int(planted[j]) for j in adj[i]} - {int(planted[i])}):
            trial = planted.copy()
            trial[i] = b
            assert L(trial) - base >= 0.11


@pytest.mark.parametrize("c,s", M.RINGS)
def test_sequential_search_recovers_rings(c, s):
    nbrs, dists, planted = M.ring_of_cliques(c, s)
    labels, info = M.cluster_by_infomap(nbrs, dists, 0.5, cluster_num=2, return_info=True)
    assert labels.dtype == np.float64 and np.array_equal(labels, M.postprocess(planted, 2))
    assert np.array_equal(labels, planted.astype(np.float64))            # cliques are already numbered by smallest member
    assert not M.violating_moves(info["src"], info["dst"], info["q"], info["node_flow"], info["modules"])


@pytest.mark.parametrize("args,min_sim", [((10, 8, 32, 0.08, 10), 0.5), ((20, 8, 64, 0.1, 12), 0.5)])
def test_sequential_search_recovers_blobs(args, min_sim):
    nbrs, dists, planted = M.blob_table(*args)
    assert np.array_equal(M.cluster_by_infomap(nbrs, dists, min_sim, cluster_num=0), M.postprocess(planted, 0))


def test_link_rules():
    thr = np.float32(1.0 - 0.5)
    lo, hi = np.nextafter(thr, np.float32(0.0)), np.nextafter(thr, np.float32(1.0))
    nbrs = np.array([[0, 1, 2, 3],        # self first
                     [2, 1, 3, 0],        # self in the middle is skipped and does not end the walk
                     [0, 1, 3, 2],        # unsorted: the failing second entry ends the row although the third would pass
                     [3, 3, 3, 3],        # only self: a single
                     [0, 1, 2, 3],        # one ulp either side of the threshold
                     [1, 0, 2, 3]], dtype=np.int32)
    dists = np.array([[0.0, 0.1, 0.2, 0.9],
                      [0.1, 0.0, 0.2, 0.3],
                      [0.1, 0.8, 0.2, 0.0],
                      [0.0, 0.0, 0.0, 0.0],
                      [thr, lo, hi, 0.1],
                      [hi, 0.1, 0.1, 0.1]], dtype=np.float32)
    single, links = M.get_links(nbrs, dists, 0.5)
    f = lambda v: float(np.float32(1.0) - np.float32(v))                 # noqa: E731
    assert single == [3, 5]
    assert links == {(0, 1): f(0.1), (0, 2): f(0.2), (1, 2): f(0.1), (1, 3): f(0.2), (1, 0): f(0.3), (2, 0): f(0.1),
                     (4, 0): f(thr), (4, 1): f(lo)}
    # the threshold is float32(1 - min_sim): float32(0.3) lies above the double 1.0 - 0.7 and still links, compared in fp32
    d = np.array([[0.0, 0.3], [0.0, 0.3]], dtype=np.float32)
    assert float(d[0, 1]) > 1.0 - 0.7
    assert sorted(M.get_links(np.array([[0, 1], [1, 0]], dtype=np.int32), d, 0.7)[1]) == [(0, 1), (1, 0)]
    # a neighbour index outside [0, N) ends the row
    assert M.get_links(np.array([[7, 1], [0, 1]], dtype=np.int32), np.zeros((2, 2), dtype=np.float32), 0.5) == ([0], {(1, 0): 1.0})


def test_postprocess():
    modules = np.array([5, 5, 9, 2, 9, 5, 7, 2, 9, 9])
    assert np.array_equal(M.postprocess(modules, 0), [0, 0, 1, 2, 1, 0, 3, 2, 1, 1])       # numbered by smallest member
    assert np.array_equal(M.postprocess(modules, 1), [0, 0, 1, 2, 1, 0, -1, 2, 1, 1])      # singles -> -1
    assert np.array_equal(M.postprocess(modules, 2), [0, 0, 1, -1, 1, 0, -1, -1, 1, 1])
    assert np.array_equal(M.postprocess(modules, 3), [-1, -1, 0, -1, 0, -1, -1, -1, 0, 0])
    assert np.array_equal(M.postprocess(modules, 4), [-1] * 10) and M.postprocess(modules, 4).dtype == np.float64
    # rows without a link are modules of their own: with cluster_num >= 1 they are dropped, with 0 they are clusters
    nbrs = np.array([[0, 1], [1, 0], [2, 0]], dtype=np.int32)
    dists = np.array([[0.0, 0.1], [0.0, 0.1], [0.0, 0.9]], dtype=np.float32)
    assert np.array_equal(M.cluster_by_infomap(nbrs, dists, 0.5, cluster_num=1), [0, 0, -1])
    assert np.array_equal(M.cluster_by_infomap(nbrs, dists, 0.5, cluster_num=0), [0, 0, 1])


def test_dangling_node_keeps_its_module():
    # node 15 has in-links from clique 0 and no out-link, node 16 out-links only (no flow reaches it), node 17 no link at all
    nbrs, dists, planted = M.ring_with_extras(3, 5)
    labels, info = M.cluster_by_infomap(nbrs, dists, 0.5, cluster_num=2, return_info=True)
    assert np.nonzero(info["single"])[0].tolist() == [15, 17]
    assert info["node_flow"][15] > 0 and info["node_flow"][16] == 0 and info["node_flow"][17] == 0
    assert np.array_equal(labels, [0] * 5 + [1] * 5 + [2] * 5 + [0, -1, -1])
    assert np.array_equal(labels, M.postprocess(planted, 2))


def test_no_cpu_fallback():
    from clustercontrast.utils.infomap_cluster import cluster_by_infomap, get_links
    from clustercontrast.utils.pseudo_labels import infomap_pseudo_labels
    from rg_hip import ops
    nbrs, dists, _ = M.ring_of_cliques(3, 5)
    tn, td = torch.from_numpy(nbrs), torch.from_numpy(dists)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cluster_by_infomap(tn, td, 0.5, cluster_num=2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        get_links([], {}, tn, td, 0.5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.infomap_links(tn, td, 0.5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.infomap(tn, td, 0.5, 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.infomap_labels(torch.zeros(4, dtype=torch.int32), 2)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            cluster_by_infomap(nbrs, dists, 0.5, cluster_num=2)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            infomap_pseudo_labels(torch.zeros(8, 4))
    with pytest.raises(ValueError, match="cluster_num"):
        cluster_by_infomap(tn, td, 0.5, cluster_num=-1)
    for bad in (0.0, -0.1, 1.01):
        with pytest.raises(ValueError, match="min_sim"):
            cluster_by_infomap(tn, td, bad)
        with pytest.raises(ValueError, match="min_sim"):
            get_links([], {}, tn, td, bad)
