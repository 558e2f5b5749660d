"""Two-level Infomap on the device (csrc/infomap.hip) through ops.infomap*, clustercontrast.utils.infomap_cluster and
clustercontrast.utils.pseudo_labels, against the numpy fp64 model of the definition (tests/infomap_hostmodel.py, pinned by
tests/test_infomap_cpu.py).  Link lists are compared for equality (weights bit for bit); flows to an L1 difference of 1e-11
(both sides stop at an L1 change of 1e-13 under a 0.85 contraction, so each is within 6e-13 of the fixed point; the rest is
summation order); codelengths to 1e-10 bits on the device's own flow (only summation order differs); labels for equality."""
import functools

import numpy as np
import pytest
import torch

from tests import infomap_hostmodel as M

pytestmark = pytest.mark.gpu

BLOBS = {"b10": ((10, 8, 32, 0.08, 10), 0.5), "b20": ((20, 8, 64, 0.1, 12), 0.5)}
NOISY = ((12, 6, 16, 0.15, 8), 0.6)


@functools.lru_cache(maxsize=None)
def _fixture(name):
    """(nbrs, dists, planted, min_sim) — computed once, never written to"""
    if name.startswith("ring"):
        c, s = (int(v) for v in name[4:].split("x"))
        return M.ring_of_cliques(c, s) + (0.5,)
    if name == "extras":
        return M.ring_with_extras(3, 5) + (0.5,)
    if name == "noisy":
        return M.blob_table(*NOISY[0]) + (NOISY[1],)
    args, min_sim = BLOBS[name]
    return M.blob_table(*args) + (min_sim,)


@functools.lru_cache(maxsize=None)
def _model(name):
    nbrs, dists, planted, min_sim = _fixture(name)
    src, dst, w, single = M.links(nbrs, dists, min_sim)
    node_flow, q, iters = M.flow(nbrs.shape[0], src, dst, w)
    return src, dst, w, single, node_flow, q, iters


RING_NAMES = ["ring%dx%d" % cs for cs in M.RINGS]
GRAPHS = RING_NAMES + ["b10", "b20", "extras"]


def _up(nbrs, dists, dev):
    return torch.from_numpy(np.ascontiguousarray(nbrs)).to(dev), torch.from_numpy(np.ascontiguousarray(dists)).to(dev)


def _check_links(nbrs, dists, min_sim, dev):
    from rg_hip import ops
    src, dst, w, single = M.links(nbrs, dists, min_sim)
    N = nbrs.shape[0]
    g = ops.infomap_links(*_up(nbrs, dists, dev), min_sim)
    assert g["N"] == N and g["E"] == len(src)
    h = {k: v.cpu().numpy() for k, v in g.items() if torch.is_tensor(v)}
    assert np.array_equal(h["rowptr"], np.concatenate([[0], np.cumsum(np.bincount(src, minlength=N))]))
    assert np.array_equal(h["src"], src) and np.array_equal(h["dst"], dst)
    assert h["w"].dtype == np.float64 and np.array_equal(h["w"], w)                  # bit-equal doubles
    assert np.array_equal(h["single"].astype(bool), single)
    perm = np.argsort(dst, kind="stable")                                           # the transpose: ascending source
    assert np.array_equal(h["in_rowptr"], np.concatenate([[0], np.cumsum(np.bincount(dst, minlength=N))]))
    assert np.array_equal(h["in_eid"], perm) and np.array_equal(h["in_src"], src[perm])
    return g


def _random_table(N, k, seed):
    """rows with self entries at arbitrary positions, unsorted, values on and beside the threshold, rows that pass throughout"""
    rng = np.random.default_rng(seed)
    thr = np.float32(0.5)
    nbrs = np.stack([rng.permutation(N)[:k] if k <= N else rng.integers(0, N, size=k) for _ in range(N)]).astype(np.int32)
    scale = rng.choice(np.array([0.45, 0.52, 0.6, 1.0], dtype=np.float32), size=(N, 1))
    dists = (rng.random((N, k), dtype=np.float32) * scale).astype(np.float32)
    put_self = rng.random(N) < 0.5
    nbrs[put_self, rng.integers(0, k, size=N)[put_self]] = np.nonzero(put_self)[0]
    edge = rng.random((N, k)) < 0.02
    dists[edge] = rng.choice(np.array([thr, np.nextafter(thr, np.float32(0)), np.nextafter(thr, np.float32(1))]), size=int(edge.sum()))
    return nbrs, dists


@pytest.mark.parametrize("name", RING_NAMES + ["extras"])
def test_links_fixtures(dev, name):
    from clustercontrast.utils.infomap_cluster import get_links
    nbrs, dists, _, min_sim = _fixture(name)
    _check_links(nbrs, dists, min_sim, dev)
    want_single, want_links = M.get_links(nbrs, dists, min_sim)
    single, links = get_links([], {}, nbrs, dists, min_sim)
    assert single == want_single and links == want_links
    single, links = get_links([], {}, *_up(nbrs, dists, dev), min_sim)
    assert single == want_single and links == want_links


@pytest.mark.parametrize("N", [1, 2, 63, 64, 65, 257])
def test_links_random_tables(dev, N):
    from clustercontrast.utils.infomap_cluster import get_links
    for k in (1, 2, 15, 64, 65, 128):
        nbrs, dists = _random_table(N, k, seed=1000 * N + k)
        g = _check_links(nbrs, dists, 0.5, dev)
        if N >= 65 and k == 128:
            assert int((g["rowptr"][1:] - g["rowptr"][:-1]).max().item()) > 64           # a row that runs past one wavefront
        if k == 65:
            assert get_links([], {}, nbrs, dists, 0.5) == M.get_links(nbrs, dists, 0.5)


@pytest.mark.parametrize("name", GRAPHS)
def test_flow(dev, name):
    from rg_hip import ops
    nbrs, dists, _, min_sim = _fixture(name)
    src, dst, w, single, node_flow, q, iters = _model(name)
    g = ops.infomap_flow(ops.infomap_links(*_up(nbrs, dists, dev), min_sim))
    assert g["flow_converged"] and abs(g["flow_iterations"] - iters) <= 1
    got_flow, got_q = g["flow"].cpu().numpy(), g["q"].cpu().numpy()
    print("flow L1", np.abs(got_flow - node_flow).sum(), "link flow L1", np.abs(got_q - q).sum(), "iterations", g["flow_iterations"], iters)
    assert np.abs(got_flow - node_flow).sum() <= 1e-11
    assert np.abs(got_q - q).sum() <= 1e-11
    assert np.array_equal(g["iq"].cpu().numpy(), got_q[g["in_eid"].cpu().numpy()])
    if name == "extras":
        assert got_flow[15] > 0 and got_flow[16] == 0 and got_flow[17] == 0


@pytest.mark.parametrize("name", GRAPHS)
def test_codelength(dev, name):
    from rg_hip import ops
    nbrs, dists, planted, min_sim = _fixture(name)
    N = nbrs.shape[0]
    g = ops.infomap_flow(ops.infomap_links(*_up(nbrs, dists, dev), min_sim))
    src, dst = g["src"].cpu().numpy().astype(np.int64), g["dst"].cpu().numpy().astype(np.int64)
    q, node_flow = g["q"].cpu().numpy(), g["flow"].cpu().numpy()           # the device's own flow goes to the model
    rng = np.random.default_rng(7)
    labellings = [planted, np.zeros(N, dtype=np.int64), np.arange(N, dtype=np.int64)]
    labellings += [rng.integers(0, int(rng.integers(2, N + 1)), size=N) * 3 - 5 for _ in range(20)]
    worst = 0.0
    for lab in labellings:
        got = ops.infomap_codelength(g, torch.from_numpy(np.ascontiguousarray(lab, dtype=np.int64)).to(dev))
        worst = max(worst, abs(got - M.codelength(src, dst, q, node_flow, lab)))
    print("codelength: worst |device - model| = %.3g bits" % worst)
    assert worst <= 1e-10
    if name.startswith("ring"):
        c, s = (int(v) for v in name[4:].split("x"))
        want = M.RING_TABLE[(c, s)]
        for lab, v in zip(labellings[:3], want[1:4]):
            assert round(ops.infomap_codelength(g, torch.from_numpy(lab).to(dev)), 4) == v


@pytest.mark.parametrize("name", RING_NAMES + ["b10", "b20", "extras"])
def test_exact_recovery(dev, name):
    from clustercontrast.utils.infomap_cluster import cluster_by_infomap
    nbrs, dists, planted, min_sim = _fixture(name)
    labels, info = cluster_by_infomap(nbrs, dists, min_sim, cluster_num=2, return_info=True)
    print(name, info)
    assert isinstance(labels, np.ndarray) and labels.dtype == np.float64 and labels.shape == (nbrs.shape[0],)
    assert np.array_equal(labels, M.postprocess(planted, 2))
    assert info["converged"] is True
    src, dst, w, single, node_flow, q, iters = _model(name)
    assert abs(info["codelength"] - M.codelength(src, dst, q, node_flow, planted)) <= 1e-9       # flow 1e-11 apart, not the same
    assert abs(info["codelength_one_module"] - M.codelength(src, dst, q, node_flow, np.zeros(len(planted), dtype=np.int64))) <= 1e-9
    assert info["n_singles"] == int(single.sum()) and info["n_clusters"] == int(labels.max()) + 1


NOISY_GRAPHS = {"noisy": NOISY + (0,), "n35": ((15, 10, 16, 0.35, 10), 0.4, 0), "n25": ((30, 6, 8, 0.25, 8), 0.3, 0),
                "rollback": ((5, 8, 4, 0.7, 10), 0.05, 4)}


@pytest.mark.parametrize("name", list(NOISY_GRAPHS))
def test_noisy_blobs_properties(dev, name):
    """Blob graphs where exact recovery is not owed; asserted is what any correct search gives.

    "noisy" is the issue's setting (12 x 6 in 16-d, sigma 0.15, k 8, min_sim 0.6).  The issue quotes 2.8373 (sequential model)
    against 2.9549 (planted) for it; with this file's generator (tests/infomap_hostmodel.py:blobs, default_rng(0): centres
    first, then the noise) those figures do not reproduce: 352 links, planted L 2.892089, and both the model and the device
    return the planted partition.  So the search is also run where it ends away from the planted labels: "n35" (15 x 10 in
    16-d, sigma 0.35, k 10, min_sim 0.4: 1226 links, 7 levels) and "n25" (30 x 6 in 8-d, sigma 0.25, k 8, min_sim 0.3: 1260
    links, 6 levels), where neither the device nor the model returns the planted partition and the two end in different
    partitions, and "rollback" (5 x 8 in 4-d, sigma 0.7, k 10, min_sim 0.05, seed 4: 360 links), found by running a numpy
    emulation of the synchronous sweeps over 48 small graphs: the only one on which a sweep's admitted moves together did not
    lower L, so that the sweep is rolled back and its single best move applied."""
    from rg_hip import ops
    args, min_sim, seed = NOISY_GRAPHS[name]
    nbrs, dists, planted = M.blob_table(*args, seed=seed)
    N = nbrs.shape[0]
    labels, info = ops.infomap(*_up(nbrs, dists, dev), min_sim, 0)
    assert info["converged"] is True
    g = ops.infomap_flow(ops.infomap_links(*_up(nbrs, dists, dev), min_sim))
    src, dst = g["src"].cpu().numpy().astype(np.int64), g["dst"].cpu().numpy().astype(np.int64)
    q, node_flow = g["q"].cpu().numpy(), g["flow"].cpu().numpy()
    modules = info["modules"].cpu().numpy().astype(np.int64)
    assert np.array_equal(labels.cpu().numpy().astype(np.float64), M.postprocess(modules, 0))
    L = M.codelength(src, dst, q, node_flow, modules)
    ref = {"planted": M.codelength(src, dst, q, node_flow, planted), "one module": M.codelength(src, dst, q, node_flow, np.zeros(N, dtype=int)),
           "singletons": M.codelength(src, dst, q, node_flow, np.arange(N))}
    print("%s: %d links, device L %.6f, model L of its labels %.6f, %s, sweeps %d levels %d rollbacks %d modules %d"
          % (name, len(src), info["codelength"], L, ref, info["sweeps"], info["levels"], info["rollbacks"], info["n_modules"]))
    assert abs(info["codelength"] - L) <= 1e-10
    for what, v in ref.items():
        assert info["codelength"] <= v, what
    assert M.violating_moves(src, dst, q, node_flow, modules) == []
    comp = M.weak_components(N, src, dst)
    for m in np.unique(modules):
        assert len(set(comp[modules == m].tolist())) == 1
    if name != "noisy":                  # the search ends away from the planted labels, on the device and in the model
        assert not np.array_equal(M.postprocess(modules, 0), M.postprocess(planted, 0))
        seq = M.search(N, src, dst, q, node_flow)
        assert not np.array_equal(M.postprocess(seq, 0), M.postprocess(planted, 0))
        print("%s: sequential model L %.6f, ratio %.6f" % (name, M.codelength(src, dst, q, node_flow, seq),
                                                           L / M.codelength(src, dst, q, node_flow, seq)))
    if name in ("n35", "n25"):
        assert info["levels"] > 3
    if name == "rollback":
        assert info["rollbacks"] >= 1


def test_edges(dev):
    from clustercontrast.utils.infomap_cluster import cluster_by_infomap
    from rg_hip import ops
    # k = 1 (only self): all singles, all -1
    n = 9
    nbrs, dists = np.arange(n, dtype=np.int32)[:, None], np.zeros((n, 1), dtype=np.float32)
    labels, info = cluster_by_infomap(nbrs, dists, 0.5, cluster_num=2, return_info=True)
    assert np.array_equal(labels, [-1.0] * n) and info["n_singles"] == n and info["sweeps"] == 0 and info["converged"]
    # cluster_num = 0 keeps singles as clusters
    assert np.array_equal(cluster_by_infomap(nbrs, dists, 0.5, cluster_num=0), np.arange(n, dtype=np.float64))
    # min_sim = 0.999: all singles
    rn, rd, _, _ = _fixture("ring5x4")
    labels, info = cluster_by_infomap(rn, rd, 0.999, cluster_num=2, return_info=True)
    assert np.array_equal(labels, [-1.0] * 20) and info["n_singles"] == 20 and info["n_modules"] == 20
    # one clique of 40: one module
    nb = np.array([[i] + [j for j in range(40) if j != i] for i in range(40)], dtype=np.int32)
    dd = np.full(nb.shape, 0.3, dtype=np.float32)
    dd[:, 0] = 0.0
    labels, info = cluster_by_infomap(nb, dd, 0.5, cluster_num=2, return_info=True)
    assert np.array_equal(labels, [0.0] * 40) and info["n_modules"] == 1 and info["converged"]
    assert abs(info["codelength"] - info["codelength_one_module"]) <= 1e-12 and abs(info["codelength"] - np.log2(40)) <= 1e-9
    # two nodes pointing at each other
    nb2, dd2 = np.array([[0, 1], [1, 0]], dtype=np.int32), np.array([[0.0, 0.2], [0.0, 0.3]], dtype=np.float32)
    labels, info = cluster_by_infomap(nb2, dd2, 0.5, cluster_num=1, return_info=True)
    assert np.array_equal(labels, [0.0, 0.0]) and info["n_modules"] == 1 and info["codelength"] == 1.0
    assert np.array_equal(labels, M.cluster_by_infomap(nb2, dd2, 0.5, cluster_num=1))
    dd2[1, 1] = 0.9                                                      # a one-way pair ties at 0 bits and stays apart
    assert np.array_equal(cluster_by_infomap(nb2, dd2, 0.5, cluster_num=0), M.cluster_by_infomap(nb2, dd2, 0.5, cluster_num=0))
    assert np.array_equal(cluster_by_infomap(nb2, dd2, 0.5, cluster_num=0), [0.0, 1.0])
    # a star: the only node with an in-link has no out-link, so no flow reaches a link and every node stays alone
    nbs = np.array([[0, 1, 2], [1, 0, 2], [2, 0, 1], [3, 0, 1], [4, 0, 1]], dtype=np.int32)
    dds = np.array([[0.0, 0.9, 0.9]] + [[0.0, 0.2, 0.9]] * 4, dtype=np.float32)
    labels, info = cluster_by_infomap(nbs, dds, 0.5, cluster_num=0, return_info=True)
    assert np.array_equal(labels, np.arange(5.0)) and info["n_singles"] == 1 and info["sweeps"] == 0
    assert np.array_equal(labels, M.cluster_by_infomap(nbs, dds, 0.5, cluster_num=0))
    # N = 1
    assert np.array_equal(cluster_by_infomap(np.zeros((1, 3), dtype=np.int32), np.zeros((1, 3), dtype=np.float32), 0.5, cluster_num=0), [0.0])
    assert np.array_equal(cluster_by_infomap(np.zeros((1, 1), dtype=np.int32), np.zeros((1, 1), dtype=np.float32), 0.5), [-1.0])
    # the limits and wrong dtype, device or contiguity are refused before any launch
    big = torch.zeros((65537, 1), dtype=torch.int32, device=dev)
    with pytest.raises(ValueError, match="65536"):
        ops.infomap(big, torch.zeros((65537, 1), dtype=torch.float32, device=dev), 0.5, 2)
    with pytest.raises(ValueError, match="65536"):
        cluster_by_infomap(np.zeros((65537, 1), dtype=np.int32), np.zeros((65537, 1), dtype=np.float32), 0.5)
    tn, td = _up(rn, rd, dev)
    with pytest.raises(ValueError, match="128"):
        ops.infomap_links(torch.zeros((4, 129), dtype=torch.int32, device=dev), torch.zeros((4, 129), dtype=torch.float32, device=dev), 0.5)
    with pytest.raises(TypeError, match="int32"):
        ops.infomap_links(tn.long(), td, 0.5)
    with pytest.raises(TypeError, match="float32"):
        ops.infomap_links(tn, td.double(), 0.5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.infomap_links(tn.cpu(), td, 0.5)
    with pytest.raises(ValueError, match="contiguous"):
        ops.infomap_links(tn.t().contiguous().t(), td, 0.5)
    with pytest.raises(ValueError, match="contiguous"):
        cluster_by_infomap(tn, td.t().contiguous().t(), 0.5)
    with pytest.raises(ValueError, match="disagree"):
        ops.infomap_links(tn, td[:, :-1].contiguous(), 0.5)
    g = ops.infomap_flow(ops.infomap_links(tn, td, 0.5))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.infomap_codelength(g, torch.zeros(20, dtype=torch.int64))
    with pytest.raises(ValueError, match="labels"):
        ops.infomap_codelength(g, torch.zeros(19, dtype=torch.int64, device=dev))
    for bad in (0.0, -0.5, 1.5, float("nan")):                           # a link weight 1 - dist has to be positive
        with pytest.raises(ValueError, match="min_sim"):
            ops.infomap_links(tn, td, bad)
        with pytest.raises(ValueError, match="min_sim"):
            cluster_by_infomap(rn, rd, bad)
    assert np.array_equal(cluster_by_infomap(rn, rd, 1.0), [-1.0] * 20)   # min_sim = 1: only dist <= 0 links, none here
    with pytest.raises(ValueError, match="no link"):
        ops.infomap_flow(ops.infomap_links(tn, td, 0.999))


def test_host_and_device_tables_agree(dev):
    """get_dist_nbr's host tables and its return_device=True tables, entry for entry, where no row has a tie"""
    from clustercontrast.utils.infomap_cluster import get_dist_nbr, knn_faiss
    x = torch.from_numpy(_clustered(700, 40, 32, 0.25, seed=11)).to(dev)
    for k in (1, 15, 40):
        dd, dn = get_dist_nbr(x, k=k, return_device=True)
        hd, hn = get_dist_nbr(x, k=k)
        assert dd.is_cuda and dn.is_cuda and tuple(dd.shape) == (700, k) and dd.is_contiguous() and dn.is_contiguous()
        assert hn.dtype == np.int32 and isinstance(hd, np.ndarray)
        dd, dn = dd.cpu().numpy(), dn.cpu().numpy()
        assert (np.diff(dd, axis=1) > 0).all() or k == 1                 # strictly ascending rows: no tie to permute
        assert np.array_equal(hn, dn) and np.array_equal(hd, dd.astype(hd.dtype))
    index = knn_faiss(x, 15)
    assert index._knns is None                                           # nothing copied to the host until `.knns` is asked for
    assert len(index.knns) == 700 and index.knns[3][0].dtype == np.int32 and index.knns[3][1].dtype == np.float32
    assert np.array_equal(index.knns[3][1], 1 - index.sims[3].cpu().numpy())


def _clustered(n, n_ids, dim, sigma, seed):
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((n_ids, dim)).astype(np.float32)
    ids = rng.integers(0, n_ids, size=n)
    x = centres[ids] + sigma * rng.standard_normal((n, dim)).astype(np.float32)
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def test_reproducible(dev):
    from clustercontrast.utils.infomap_cluster import cluster_by_infomap, get_dist_nbr
    x = torch.from_numpy(_clustered(5000, 300, 32, 0.25, seed=3)).to(dev)
    dists, nbrs = get_dist_nbr(x, k=15, return_device=True)
    assert dists.is_cuda and nbrs.is_cuda and dists.dtype == torch.float32 and nbrs.dtype == torch.int32
    a, ia = cluster_by_infomap(nbrs, dists, 0.5, cluster_num=4, return_device=True, return_info=True)
    b, ib = cluster_by_infomap(nbrs, dists, 0.5, cluster_num=4, return_device=True, return_info=True)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        c, ic = cluster_by_infomap(nbrs, dists, 0.5, cluster_num=4, return_device=True, return_info=True)
    side.synchronize()
    print("5000 nodes:", ia)
    assert a.dtype == torch.int64 and a.is_cuda and ia["converged"] and ia["n_clusters"] > 100
    assert torch.equal(a, b) and torch.equal(a, c)
    assert ia == ib and ia == ic                                         # codelength and every count bit-equal
    host = cluster_by_infomap(nbrs, dists, 0.5, cluster_num=4)
    assert host.dtype == np.float64 and np.array_equal(host, a.cpu().numpy().astype(np.float64))


def test_market_size(dev):
    from clustercontrast.utils.infomap_cluster import cluster_by_infomap, get_dist_nbr
    x = torch.from_numpy(_clustered(12936, 751, 64, 0.3, seed=5)).to(dev)
    dists, nbrs = get_dist_nbr(x, k=15, return_device=True)
    assert tuple(nbrs.shape) == (12936, 15)
    labels, info = cluster_by_infomap(nbrs, dists, 0.5, cluster_num=4, return_device=True, return_info=True)
    print("market size:", info)
    lab = labels.cpu().numpy()
    C = info["n_clusters"]
    assert lab.min() >= -1 and lab.max() == C - 1 and C > 0
    counts = np.bincount(lab[lab >= 0], minlength=C)
    assert (counts > 4).all()                                            # every label used, every kept cluster above cluster_num
    assert info["converged"] is True
    assert info["codelength"] < info["codelength_one_module"]
    again, info2 = cluster_by_infomap(nbrs, dists, 0.5, cluster_num=4, return_device=True, return_info=True)
    assert torch.equal(labels, again) and info == info2


def test_end_to_end(dev):
    from clustercontrast.utils.infomap_cluster import cluster_by_infomap, generate_cluster_features, get_dist_nbr
    from clustercontrast.utils.pseudo_labels import infomap_pseudo_labels
    x, planted = M.blobs(20, 8, 64, 0.1, seed=0)
    xt = torch.from_numpy(x)
    labels, centroids, info = infomap_pseudo_labels(xt, k=12, min_sim=0.5, cluster_num=4)
    assert labels.dtype == np.int64 and np.array_equal(labels, planted) and info["converged"] and info["n_clusters"] == 20
    xn = torch.nn.functional.normalize(xt.to(dev), dim=1)
    want = generate_cluster_features(labels, xn)
    assert centroids.is_cuda and tuple(centroids.shape) == (20, 64) and torch.equal(centroids, want)
    # the two lines of examples/cluster_contrast_gan_train_usl_infomap.py:321-325, on numpy inputs
    features_array = xn.cpu().numpy()
    feat_dists, feat_nbrs = get_dist_nbr(features=features_array, k=12, knn_method='faiss-gpu')
    pseudo_labels = cluster_by_infomap(feat_nbrs, feat_dists, min_sim=0.5, cluster_num=4)
    assert isinstance(pseudo_labels, np.ndarray) and pseudo_labels.dtype == np.float64
    assert np.array_equal(pseudo_labels.astype(np.intp), planted)


@pytest.mark.parametrize("single", [0, 1])
def test_one_sweep_from_singletons(dev, single):
    """one propose + apply on ring 8x6: the admitted moves touch disjoint modules, the totals the movers wrote equal the
    totals recomputed from scratch, and with the single best move alone the drop of L is that move's gain exactly"""
    from rg_hip import ops
    from rg_hip.lib import lib
    nbrs, dists, _, min_sim = _fixture("ring8x6")
    g = ops.infomap_flow(ops.infomap_links(*_up(nbrs, dists, dev), min_sim))
    ug, U, p = ops._infomap_leaf_units(g), g["N"], ops._p
    mod = torch.arange(U, dtype=torch.int32, device=dev)
    tot = list(ops._infomap_totals(ug, mod))
    cl, cl2 = torch.empty(2, dtype=torch.float64, device=dev), torch.empty(2, dtype=torch.float64, device=dev)
    ops._infomap_codelength_of(tot, g["scal"], cl)
    tgt = torch.empty(U, dtype=torch.int32, device=dev)
    key, claim, best = (torch.empty(n, dtype=torch.int64, device=dev) for n in (U, U, 1))
    vals, nmoved = torch.empty(4 * U, dtype=torch.float64, device=dev), torch.empty(1, dtype=torch.int32, device=dev)
    lib.rg_infomap_propose(p(ug["orp"]), p(ug["odst"]), p(ug["oq"]), p(ug["irp"]), p(ug["isrc"]), p(ug["iq"]), p(ug["pu"]), p(mod),
                           p(tot[0]), p(tot[1]), p(tot[2]), p(tot[3]), U, p(cl), p(tgt), p(key), p(vals), p(claim), p(best), p(nmoved),
                           ops._stream())
    before, tgt_h, key_h = mod.cpu().numpy(), tgt.cpu().numpy(), key.cpu().numpy()
    lib.rg_infomap_apply(p(tgt), p(key), p(vals), p(claim), p(best), p(ug["pu"]), U, single, p(mod), p(tot[0]), p(tot[1]), p(tot[2]),
                         p(tot[3]), p(nmoved), ops._stream())
    ops._infomap_codelength_of(tot, g["scal"], cl2)
    after = mod.cpu().numpy()
    moved = np.nonzero(after != before)[0]
    assert int(nmoved.item()) == len(moved) >= 1 and (tgt_h >= 0).all()      # from singletons every clique node has a gainful move
    assert np.array_equal(after[moved], tgt_h[moved])
    touched = np.concatenate([before[moved], after[moved]])
    assert len(set(touched.tolist())) == 2 * len(moved)                  # at most one move per module, as source or target
    fresh = ops._infomap_totals(ug, mod)
    for a, b in zip(tot[:3], fresh[:3]):
        assert float((a - b).abs().max().item()) <= 1e-15
    assert torch.equal(tot[3], fresh[3])
    src, dst = g["src"].cpu().numpy().astype(np.int64), g["dst"].cpu().numpy().astype(np.int64)
    q, node_flow = g["q"].cpu().numpy(), g["flow"].cpu().numpy()
    L0, L1 = float(cl[0].item()), float(cl2[0].item())
    assert abs(L0 - M.codelength(src, dst, q, node_flow, before)) <= 1e-10 and abs(L1 - M.codelength(src, dst, q, node_flow, after)) <= 1e-10
    assert L1 < L0
    if single:
        assert len(moved) == 1 and key_h[moved[0]] == key_h.max() == int(best.item())
        gain = np.array([key_h[moved[0]] & ~0xFFFF], dtype=np.int64).view(np.float64)[0]      # the gain with its low 16 bits cut
        assert 0 <= (L0 - L1) - gain <= 1e-10 + (L0 - L1) * 2.0 ** -36
        assert 0xFFFF - (int(key_h[moved[0]]) & 0xFFFF) == moved[0]
