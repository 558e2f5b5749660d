"""k-means on the device (csrc/kmeans.hip) through ops.kmeans*, clustercontrast.models.kmeans and
clustercontrast.utils.pseudo_labels, against the numpy fp64 model of the definition (tests/kmeans_hostmodel.py, pinned by
tests/test_kmeans_cpu.py).

Labels are compared for equality on every row whose fp64 margin (best against second-best score) reaches tau = 8 * D * 2^-24 *
(|x_i|^2 + max_j |c_j|^2), the worst-case fp32 accumulation error of the two scores compared with a factor 8 of room; a row below
it is "excused", and a case may excuse at most 1 % of its rows, which is asserted from the model alone before the device is
touched.  Scores are held to tau / 2, counts and member lists to equality, centroids per element to one fp32 ulp of the mean plus
the fp64 accumulation error (the header documents fp64 accumulation and a single rounding)."""
import functools

import numpy as np
import pytest
import torch

from tests import kmeans_hostmodel as M

pytestmark = pytest.mark.gpu

CAP = 0.01


def _up(a, dev, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(dev)


# ---- assignment, one step ----------------------------------------------------------------------------------------------------
# N in {1, 63, 129, 300} x K in {1, 2, 127, 129, 500} (K <= N) x D in {1, 7, 16, 17, 70, 2048}: tails on all three axes, one and
# two column tiles.  K = 500 (four column tiles) needs N >= 500, which the four row counts do not reach: N = 509 is added for it.
# The three largest (N, K) pairs take every D, the others alternate between two triples: 45 cases.
def _assign_grid():
    pairs = [(n, k) for n in (1, 63, 129, 300) for k in (1, 2, 127, 129, 500) if k <= n] + [(509, 500)]
    full = {(300, 129), (129, 129), (509, 500)}
    cases = []
    for i, (n, k) in enumerate(pairs):
        ds = (1, 7, 16, 17, 70, 2048) if (n, k) in full else ((1, 17, 2048) if i % 2 == 0 else (7, 16, 70))
        cases += [(n, k, d) for d in ds]
    return cases


@functools.lru_cache(maxsize=None)
def _assign_case(N, K, D):
    """(x, c fp32, model labels, model scores, excused mask, tau): Gaussian rows, centroids drawn from the rows.  Two depths
    cannot keep the cap that way and get other inputs: at D = 1 a row that is its own centroid has a squared gap as its margin
    and one in six would be excused, and on a line 500 random centroids are closer than tau allows, so the centroids are a
    shuffled even grid on [-3, 3] and the rows lie around them (0.15 of the spacing); at D = 2048 all squared distances of
    Gaussian rows lie within a few tau of each other (4096 +- 128 against tau = 4), so the rows are drawn around the centroids
    (0.5 * randn).  The first seed whose excused share is within the cap is used."""
    for seed in range(64):
        r = np.random.RandomState(1000 * seed + N + 7 * K + 13 * D)
        x = r.randn(N, D).astype(np.float32)
        if D == 1:
            c = r.permutation(np.linspace(-3.0, 3.0, K + 2)[1:-1]).reshape(K, 1).astype(np.float32)
            x = (c[r.randint(0, K, size=N)] + 0.15 * (6.0 / (K + 1)) * x).astype(np.float32)
        elif D == 2048:
            c = r.randn(K, D).astype(np.float32)
            x = (c[r.randint(0, K, size=N)] + 0.5 * x).astype(np.float32)
        else:
            c = x[r.permutation(N)[:K]].copy()
        ex = M.excused(x, c)
        if ex.mean() <= CAP:
            lab, sc = M.assign(x, c)
            return x, c, lab, sc, ex, M.tau(x, c, D)
    raise AssertionError("no seed keeps the excused rows of N=%d K=%d D=%d within %.0f %%" % (N, K, D, 100 * CAP))


@pytest.mark.parametrize("N,K,D", _assign_grid())
def test_assign_against_the_model(dev, N, K, D):
    from rg_hip import ops
    x, c, lab, sc, ex, tau = _assign_case(N, K, D)
    assert ex.mean() <= CAP
    xd, cd = _up(x, dev), _up(c, dev)
    label, score = ops.kmeans_assign(xd, cd, ops.row_sqsum(cd))
    assert label.dtype == torch.int32 and score.dtype == torch.float32
    got, gs = label.cpu().numpy().astype(np.int64), score.cpu().numpy().astype(np.float64)
    assert got.min() >= 0 and got.max() < K
    assert np.array_equal(got[~ex], lab[~ex]), "rows %s" % np.nonzero((got != lab) & ~ex)[0][:8]
    err = np.abs(gs - sc)
    print("assign N=%d K=%d D=%d: %d excused, score error / (tau / 2) max %.3g" % (N, K, D, int(ex.sum()), (err / (tau / 2)).max()))
    assert (err <= tau / 2).all()


# ---- exact ties, exact arithmetic --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,K,D,far", [(200, 6, 5, 1), (333, 140, 7, 130), (129, 260, 4, 128)])
def test_exact_ties_go_to_the_lowest_index(dev, N, K, D, far):
    """small integers in fp32: every product and sum is exact in fp32 and in fp64, so the labels are the model's on every row.
    Centroid `far` duplicates centroid 0 (far >= 128: the pair sits in different column tiles), centroids 1 and 2 are mirror
    images around rows that are therefore equidistant from both."""
    from rg_hip import ops
    if N < K:
        N = K + 40
    r = np.random.RandomState(N + K)
    x = r.randint(-3, 4, size=(N, D)).astype(np.float32)
    c = r.randint(-3, 4, size=(K, D)).astype(np.float32)
    c[far] = c[0]
    c[1], c[2] = c[1] * 0 + 1, c[2] * 0 + 1
    c[1, 0], c[2, 0] = 3, -3
    x[:40, 0] = 0                                                 # equidistant from centroids 1 and 2
    x[40:60] = c[0]                                               # on the duplicated centroid
    lab, sc = M.assign(x, c)
    s = M.scores(x, c)
    assert (np.sort(s, axis=1)[:, 0] == np.sort(s, axis=1)[:, 1]).sum() >= 20          # the case holds exact ties
    assert (lab[40:60] == 0).all()
    xd, cd = _up(x, dev), _up(c, dev)
    label, score = ops.kmeans_assign(xd, cd, ops.row_sqsum(cd))
    assert np.array_equal(label.cpu().numpy(), lab)
    assert np.array_equal(score.cpu().numpy().astype(np.float64), sc)


# ---- tally, update, split ----------------------------------------------------------------------------------------------------
TALLY_CASES = [(5, 1, 0), (40, 7, 3), (1024, 9, 2), (1025, 130, 40), (2500, 37, 5), (3000, 3000, 0)]


@pytest.mark.parametrize("N,K,empty", TALLY_CASES)
def test_tally_against_the_model(dev, N, K, empty):
    from rg_hip import ops
    r = np.random.RandomState(N + K)
    used = np.sort(r.permutation(K)[:K - empty])
    labels = used[r.randint(0, len(used), size=N)] if K < N else r.permutation(N)
    prev = np.where(r.rand(N) < 0.3, (labels + 1) % K, labels)
    xsq, score = r.rand(N).astype(np.float32) * 50, (r.randn(N) * 20).astype(np.float32)
    cnt, rowptr, order = M.tally(labels, K)
    out = ops.kmeans_tally(_up(labels, dev, torch.int32), _up(prev, dev, torch.int32), _up(xsq, dev), _up(score, dev), K)
    assert np.array_equal(out["cnt"].cpu().numpy(), cnt) and (cnt == 0).sum() >= empty
    assert np.array_equal(out["rowptr"].cpu().numpy(), rowptr)
    assert np.array_equal(out["order"].cpu().numpy(), order)
    assert int(out["changed"].item()) == int((labels != prev).sum())
    want = float((xsq.astype(np.float64) + score.astype(np.float64)).sum())
    assert abs(float(out["obj"].item()) - want) <= 1e-6 * abs(want)


@pytest.mark.parametrize("N,K,D,empty", [(40, 7, 3, 3), (300, 1, 70, 0), (1500, 37, 130, 5), (700, 130, 257, 20)])
def test_update_against_the_model(dev, N, K, D, empty):
    from rg_hip import ops
    r = np.random.RandomState(N + K + D)
    used = np.sort(r.permutation(K)[:K - empty])
    labels = used[r.randint(0, len(used), size=N)]
    x = (r.randn(N, D) * 3).astype(np.float32)
    c_prev = r.randn(K, D).astype(np.float32)
    cnt, rowptr, order = M.tally(labels, K)
    want = M.update(x, labels, c_prev)
    c, csq = _up(c_prev, dev), torch.full((K,), -7.0, device=dev)
    ops.kmeans_update(_up(x, dev), _up(order, dev, torch.int32), _up(rowptr, dev, torch.int32), c, csq)
    got, gsq = c.cpu().numpy().astype(np.float64), csq.cpu().numpy().astype(np.float64)
    assert (np.abs(got - want) <= M.centroid_bound(x, labels, want)).all()
    assert np.array_equal(got[cnt == 0], c_prev[cnt == 0].astype(np.float64)) and (gsq[cnt == 0] == -7.0).all()     # kept
    sq = (got * got).sum(1)
    assert (np.abs(gsq - sq)[cnt > 0] <= 2.0 ** -23 * sq[cnt > 0]).all()


@pytest.mark.parametrize("K,D,cnt", [(5, 3, [10, 0, 3, 10, 0]), (9, 5, [0, 4, 0, 9, 9, 1, 0, 2, 5]), (1, 4, [6]), (3, 2, [1, 0, 1]),
                                      (200, 6, None)])
def test_split_is_exact_on_the_lattice(dev, K, D, cnt):
    from rg_hip import ops
    r = np.random.RandomState(K + D)
    c = r.randint(-3, 4, size=(K, D)).astype(np.float32)
    cnt = np.array(cnt) if cnt is not None else np.where(r.rand(K) < 0.3, 0, r.randint(1, 40, size=K))
    want_c, want_cnt, ns = M.split(c, cnt)
    cd, cntd = _up(c, dev), _up(cnt, dev, torch.int32)
    csq = ops.row_sqsum(cd)
    nsplit = torch.full((1,), 5, dtype=torch.int32, device=dev)
    ops.kmeans_split(cd, csq, cntd, nsplit)
    assert int(nsplit.item()) == 5 + ns
    assert np.array_equal(cntd.cpu().numpy(), want_cnt)
    assert np.array_equal(cd.cpu().numpy().astype(np.float64), want_c)           # integers times 1 +- 2^-10: exact in fp32
    assert np.array_equal(csq.cpu().numpy(), (want_c * want_c).sum(1).astype(np.float32))


# ---- whole runs ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _blob_run(seed):
    x, planted = M.blobs(seed)
    c0 = x[M.init_perm(x.shape[0], 6, 1234)].astype(np.float64)
    return x, planted, M.lloyd(x, c0, 300, trace=True)


@pytest.mark.parametrize("seed", [0, 2, 4, 5])
def test_blob_runs_follow_the_model_exactly(dev, seed):
    from rg_hip import ops
    x, _, r = _blob_run(seed)
    assert all(not M.excused(x, c).any() for _, c in r["steps"]) and not M.excused(x, r["centroids"]).any()
    assert r["converged"] and (r["n_split"] == 1) == (seed == 4)
    labels, c, info = ops.kmeans(_up(x, dev), 6)
    assert labels.dtype == torch.int64 and c.dtype == torch.float32 and tuple(c.shape) == (6, 24)
    assert (info["iterations"], info["n_split"], info["converged"], info["n_train"]) == (r["iterations"], r["n_split"], True, 600)
    assert np.array_equal(labels.cpu().numpy(), r["labels"])
    assert (np.abs(c.cpu().numpy().astype(np.float64) - r["centroids"]) <= M.centroid_bound(x, r["labels"], r["centroids"])).all()
    assert len(info["obj"]) == r["iterations"] and np.allclose(info["obj"], r["obj"], rtol=1e-5, atol=0)


def test_lattice_run_follows_the_model_exactly(dev):
    from rg_hip import ops
    x, c0 = M.lattice(20)
    r = M.lloyd(x, c0, 300)
    assert (r["iterations"], r["n_split"], r["converged"]) == (15, 6, True) and r["cnt"].min() > 0
    labels, c, info = ops.kmeans(_up(x, dev), 8, init_centroids=_up(c0, dev), debug=True)
    assert (info["iterations"], info["n_split"], info["converged"]) == (15, 6, True)
    assert np.array_equal(labels.cpu().numpy(), r["labels"])
    assert np.array_equal(info["cnt"].cpu().numpy(), r["cnt"])
    cnt, rowptr, order = M.tally(r["labels"], 8)
    assert np.array_equal(info["rowptr"].cpu().numpy(), rowptr) and np.array_equal(info["order"].cpu().numpy(), order)
    assert info["score"].shape == (300,)


# ---- invariants where the trajectory may fork ---------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _gauss():
    return np.random.RandomState(11).randn(1000, 70).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _gauss_run():
    from rg_hip import ops
    labels, c, info = ops.kmeans(torch.from_numpy(_gauss()).to("cuda:0"), 37)
    return labels.cpu().numpy(), c.cpu().numpy(), info


def test_invariants_on_gaussian_rows(dev):
    x = _gauss()
    labels, c, info = _gauss_run()
    K = 37
    assert labels.min() >= 0 and labels.max() < K
    assert info["converged"] and info["iterations"] <= 300 and len(info["obj"]) == info["iterations"] == len(info["splits"])
    ex = M.excused(x, c)
    assert ex.mean() <= CAP
    assert np.array_equal(labels[~ex], M.assign(x, c)[0][~ex])
    obj = info["obj"]
    for t in range(len(obj) - 1):
        if info["splits"][t] == 0:
            assert obj[t + 1] <= obj[t] + 1e-6 * obj[0], (t, obj[t], obj[t + 1])
    # the objective is the sum of squared distances to the nearest centroid of the iteration's start
    assert abs(obj[-1] - float(((x.astype(np.float64) - c.astype(np.float64)[labels]) ** 2).sum())) <= 1e-5 * obj[-1]


def test_runs_are_bit_identical(dev):
    from rg_hip import ops
    labels, c, info = _gauss_run()
    xd = _up(_gauss(), dev)

    def same(run):
        l2, c2, i2 = run
        return np.array_equal(l2.cpu().numpy(), labels) and np.array_equal(c2.cpu().numpy(), c) and i2["obj"] == info["obj"] \
            and (i2["iterations"], i2["n_split"], i2["converged"]) == (info["iterations"], info["n_split"], info["converged"])

    assert same(ops.kmeans(xd, 37))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run = ops.kmeans(xd, 37)
    side.synchronize()
    assert same(run)
    for ce in (1, 300):                                           # 8 is the default of the runs above
        assert same(ops.kmeans(xd, 37, check_every=ce)), ce
    assert same(ops.kmeans(xd, 37, niter=info["iterations"]))
    short = ops.kmeans(xd, 37, niter=info["iterations"] - 1)
    assert not short[2]["converged"] and short[2]["obj"] == info["obj"][:-1]


# ---- driver edges -------------------------------------------------------------------------------------------------------------
def test_driver_edges(dev):
    from rg_hip import ops
    r = np.random.RandomState(5)
    x = r.randn(200, 9).astype(np.float32)
    xd = _up(x, dev)
    # N == K: the rows are the centroids
    labels, c, info = ops.kmeans(xd[:17], 17)
    assert np.array_equal(labels.cpu().numpy(), np.arange(17)) and torch.equal(c, xd[:17]) and info["converged"] and info["iterations"] == 0
    # given centroids
    c0 = x[[3, 50, 120, 199]].astype(np.float64)
    m = M.lloyd(x, c0, 300, trace=True)
    assert all(not M.excused(x, cc).any() for _, cc in m["steps"])
    labels, c, info = ops.kmeans(xd, 4, init_centroids=_up(c0.astype(np.float32), dev))
    assert np.array_equal(labels.cpu().numpy(), m["labels"]) and info["iterations"] == m["iterations"]
    # subsampling: 20 training rows, labels for all 200, each the nearest returned centroid
    labels, c, info = ops.kmeans(xd, 5, max_points_per_centroid=4)
    assert info["n_train"] == 20 and labels.shape == (200,)
    cc = c.cpu().numpy()
    ex = M.excused(x, cc)
    assert np.array_equal(labels.cpu().numpy()[~ex], M.assign(x, cc)[0][~ex]) and ex.mean() <= CAP
    rows = M.rand_perm(200, 20, 1234)
    m = M.lloyd(x[rows], x[rows][M.init_perm(20, 5, 1234)].astype(np.float64), 300)
    assert info["iterations"] == m["iterations"] and np.abs(cc - m["centroids"]).max() <= 1e-5
    # rejected inputs
    for bad in (float("nan"), float("inf")):
        y = xd.clone()
        y[7, 3] = bad
        with pytest.raises(ValueError):
            ops.kmeans(y, 4)
    with pytest.raises(ValueError):
        ops.kmeans(xd[:3], 4)
    with pytest.raises(ValueError):
        ops.kmeans_assign(xd, xd[:4], torch.zeros(5, device=dev))
    with pytest.raises(ValueError):
        ops.kmeans_assign(xd[:3], xd[:4].contiguous(), torch.zeros(4, device=dev))           # K > N


def test_no_score_matrix_is_materialised(dev):
    from rg_hip import ops
    N, K, D = 4096, 512, 64
    x = torch.from_numpy(np.random.RandomState(2).randn(N, D).astype(np.float32)).to(dev)
    ops.kmeans(x[:600].contiguous(), 8, niter=2)                   # the per-stream workspace exists before the measurement
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated(dev)
    torch.cuda.reset_peak_memory_stats(dev)
    labels, c, info = ops.kmeans(x, K, niter=20)
    torch.cuda.synchronize()
    grown = torch.cuda.max_memory_allocated(dev) - base
    outputs = labels.numel() * 8 + c.numel() * 4
    print("kmeans N=%d K=%d D=%d: peak grows by %.2f MB over the inputs, outputs %.2f MB, a score matrix would be %.2f MB"
          % (N, K, D, grown / 1e6, outputs / 1e6, N * K * 4 / 1e6))
    assert grown - outputs < N * K * 4
    assert info["iterations"] >= 1 and labels.shape == (N,)


# ---- public interface ---------------------------------------------------------------------------------------------------------
def test_label_generator_kmeans(dev):
    from clustercontrast.models.kmeans import label_generator_kmeans
    x, planted, r = _blob_run(0)
    labels, centers, k, extra = label_generator_kmeans(torch.from_numpy(x), num_classes=6)
    assert isinstance(labels, np.ndarray) and labels.dtype == np.int64 and labels.shape == (600,) and -1 not in labels
    assert torch.is_tensor(centers) and not centers.is_cuda and centers.dtype == torch.float32 and tuple(centers.shape) == (6, 24)
    assert k == 6 and extra is None
    assert np.array_equal(labels, r["labels"])
    dl, dc, k, extra = label_generator_kmeans(torch.from_numpy(x).to(dev), 6, cuda=False, return_device=True)
    assert dl.is_cuda and dl.dtype == torch.int64 and dc.is_cuda and np.array_equal(dl.cpu().numpy(), labels) and torch.equal(dc.cpu(), centers)
    warm = label_generator_kmeans(x, 6, init_centroids=centers, niter=5)
    assert np.array_equal(warm[0], labels)
    with pytest.raises(AssertionError):
        label_generator_kmeans(torch.from_numpy(x), num_classes=0)


def test_kmeans_pseudo_labels_end_to_end(dev):
    from clustercontrast.utils.pseudo_labels import kmeans_pseudo_labels
    x, planted, r = _blob_run(4)           # Lloyd's iteration from these initial rows ends in the planted partition (seeds 2 and 5 do not)
    assert len(set(zip(planted.tolist(), r["labels"].tolist()))) == 6
    pseudo, feats, info = kmeans_pseudo_labels(torch.from_numpy(x), num_classes=6)
    assert isinstance(pseudo, np.ndarray) and pseudo.dtype == np.int64 and pseudo.shape == (600,)
    assert feats.is_cuda and tuple(feats.shape) == (6, 24) and info["converged"]
    # the planted partition up to renaming: the pairs (planted, found) form a bijection
    pairs = set(zip(planted.tolist(), pseudo.tolist()))
    assert len(pairs) == 6 and len({a for a, _ in pairs}) == 6 and len({b for _, b in pairs}) == 6
    means = M.update(x, pseudo, np.zeros((6, 24)))
    b = 2.0 ** -24 * np.stack([np.abs(x[pseudo == j]).sum(0) for j in range(6)]) + 2.0 ** -23 * np.abs(means)   # fp32 segment_mean
    assert (np.abs(feats.cpu().numpy().astype(np.float64) - means) <= b).all()


# ---- Market-1501 size ---------------------------------------------------------------------------------------------------------
def test_market_size_run(dev):
    from rg_hip import ops
    g = torch.Generator(device=dev).manual_seed(7)
    ids = torch.randint(0, 751, (12936,), generator=g, device=dev)
    x = torch.randn((751, 2048), generator=g, device=dev)[ids] + 0.7 * torch.randn((12936, 2048), generator=g, device=dev)
    x = torch.nn.functional.normalize(x, dim=1).contiguous()
    labels, c, info = ops.kmeans(x, 500)
    lab = labels.cpu().numpy()
    print("market size: %d iterations, converged %s, %d splits" % (info["iterations"], info["converged"], info["n_split"]))
    assert lab.min() >= 0 and lab.max() < 500 and np.bincount(lab, minlength=500).min() > 0
    l2, c2, i2 = ops.kmeans(x, 500)
    assert torch.equal(l2, labels) and torch.equal(c2, c) and i2["obj"] == info["obj"] and i2["iterations"] == info["iterations"]
