"""k-means (csrc/kmeans.hip): the four entry-point wrappers and the host loop over them ("Widened row: k-means")."""
from __future__ import absolute_import

import numpy as np
import torch

from ._base import _chk, _chk_rr, _p, _stream, _ws_query, lib, workspace


# ------------------------------------------------------------------------------------------------
# Lloyd's k-means on fp32 features (csrc/kmeans.hip): assign, tally, update, split
# ------------------------------------------------------------------------------------------------
KMEANS_MAX_N, KMEANS_MAX_K, KMEANS_MAX_D = 1 << 20, 8192, 8192


def _chk_kmeans_shape(N, K, D):
    if not (1 <= K <= KMEANS_MAX_K and K <= N <= KMEANS_MAX_N and 1 <= D <= KMEANS_MAX_D):
        raise ValueError("rg_hip: kmeans needs 1 <= K <= %d, K <= N <= %d and 1 <= D <= %d, got N=%d K=%d D=%d"
                         % (KMEANS_MAX_K, KMEANS_MAX_N, KMEANS_MAX_D, N, K, D))


def kmeans_rand_perm(n, m, seed):
    """the first m entries (int64 numpy) of faiss's rand_perm(n, seed): from the identity, for i = 0 .. n - 2 swap perm[i] and
    perm[i + mt() % (n - i)] with mt = std::mt19937(seed); entry i is final after swap i, so m swaps are enough.  numpy's
    legacy seeding of MT19937 is std::mt19937's, and random_raw hands out its 32-bit draws."""
    n, m = int(n), int(m)
    if not 0 <= m <= n:
        raise ValueError("rg_hip: kmeans_rand_perm needs 0 <= m <= n, got n=%d m=%d" % (n, m))
    perm = np.arange(n, dtype=np.int64)
    steps = min(m, n - 1)
    if steps > 0:
        draws = np.random.RandomState(int(seed))._bit_generator.random_raw(steps)
        for i in range(steps):
            j = i + int(draws[i]) % (n - i)
            perm[i], perm[j] = perm[j], perm[i]
    return perm[:m].copy()


def kmeans_assign(x, c, csq, label=None, score=None):
    """(label int32 [N], score fp32 [N]): label[i] = argmin_j (csq[j] - 2 x_i . c_j) with ties to the lowest j, score[i] = the
    minimum.  x [N, D], c [K, D], csq [K] (= |c_j|^2 for nearest-centroid labels).  The [N, K] scores are never stored."""
    x, c, csq = _chk_rr(x, "x", torch.float32, 2), _chk_rr(c, "c", torch.float32, 2), _chk_rr(csq, "csq", torch.float32, 1)
    (N, D), K = x.shape, c.shape[0]
    if c.shape[1] != D or csq.numel() != K:
        raise ValueError("rg_hip: kmeans_assign: x %s, c %s and csq %s disagree" % (tuple(x.shape), tuple(c.shape), tuple(csq.shape)))
    _chk_kmeans_shape(N, K, D)
    if label is None:
        label = torch.empty((N,), dtype=torch.int32, device=x.device)
    if score is None:
        score = torch.empty((N,), dtype=torch.float32, device=x.device)
    nbytes = _ws_query("rg_kmeans_assign_workspace", N, K, D)
    ws = workspace(nbytes, x.device) if nbytes else None
    lib.rg_kmeans_assign(_p(x), _p(c), _p(csq), N, K, D, _p(label), _p(score), _p(ws), nbytes, _stream())
    return label, score


def kmeans_tally(label, prev, xsq, score, K, out=None):
    """{"cnt" int32 [K], "rowptr" int32 [K + 1], "order" int32 [N], "changed" int32 [1], "obj" fp64 [1]} of the labels: member
    counts, their exclusive prefix sum, the members cluster by cluster in ascending row index, the number of rows whose label
    differs from prev, and sum_i (xsq[i] + score[i]) in fp64.  `out` reuses the tensors of an earlier call."""
    label, prev = _chk_rr(label, "label", torch.int32, 1), _chk_rr(prev, "prev", torch.int32, 1)
    xsq, score = _chk_rr(xsq, "xsq", torch.float32, 1), _chk_rr(score, "score", torch.float32, 1)
    N, K = label.numel(), int(K)
    if prev.numel() != N or xsq.numel() != N or score.numel() != N:
        raise ValueError("rg_hip: kmeans_tally: label, prev, xsq and score must have the same length")
    _chk_kmeans_shape(N, K, 1)
    dev = label.device
    if out is None:
        out = dict(cnt=torch.empty((K,), dtype=torch.int32, device=dev), rowptr=torch.empty((K + 1,), dtype=torch.int32, device=dev),
                   order=torch.empty((N,), dtype=torch.int32, device=dev), changed=torch.empty((1,), dtype=torch.int32, device=dev),
                   obj=torch.empty((1,), dtype=torch.float64, device=dev))
    nbytes = _ws_query("rg_kmeans_tally_workspace", N, K)
    ws = workspace(nbytes, dev)
    lib.rg_kmeans_tally(_p(label), _p(prev), _p(xsq), _p(score), N, K, _p(out["cnt"]), _p(out["rowptr"]), _p(out["order"]),
                        _p(out["changed"]), _p(out["obj"]), _p(ws), nbytes, _stream())
    return out


def kmeans_update(x, order, rowptr, c, csq):
    """c[j] = mean of the rows x[order[rowptr[j] : rowptr[j + 1]]] (fp64 accumulation in list order, one rounding to fp32),
    csq[j] = |c[j]|^2, both in place; a cluster without a member keeps its row."""
    x, c, csq = _chk_rr(x, "x", torch.float32, 2), _chk_rr(c, "c", torch.float32, 2), _chk_rr(csq, "csq", torch.float32, 1)
    order, rowptr = _chk_rr(order, "order", torch.int32, 1), _chk_rr(rowptr, "rowptr", torch.int32, 1)
    (N, D), K = x.shape, c.shape[0]
    if c.shape[1] != D or csq.numel() != K or order.numel() != N or rowptr.numel() != K + 1:
        raise ValueError("rg_hip: kmeans_update: the arrays disagree with N=%d K=%d D=%d" % (N, K, D))
    _chk_kmeans_shape(N, K, D)
    lib.rg_kmeans_update(_p(x), _p(order), _p(rowptr), N, K, D, _p(c), _p(csq), _stream())
    return c, csq


def kmeans_split(c, csq, cnt, nsplit):
    """the deterministic split of empty clusters, in place on c [K, D], csq [K], cnt int32 [K]; nsplit int32 [1] is incremented
    by the number of splits (include/reidgan_hip.h states the rule)."""
    c, csq = _chk_rr(c, "c", torch.float32, 2), _chk_rr(csq, "csq", torch.float32, 1)
    cnt, nsplit = _chk_rr(cnt, "cnt", torch.int32, 1), _chk_rr(nsplit, "nsplit", torch.int32, 1)
    K, D = c.shape
    if csq.numel() != K or cnt.numel() != K or nsplit.numel() < 1:
        raise ValueError("rg_hip: kmeans_split: the arrays disagree with K=%d" % K)
    if not (1 <= K <= KMEANS_MAX_K and 1 <= D <= KMEANS_MAX_D):
        raise ValueError("rg_hip: kmeans_split needs 1 <= K <= %d and 1 <= D <= %d, got K=%d D=%d" % (KMEANS_MAX_K, KMEANS_MAX_D, K, D))
    lib.rg_kmeans_split(_p(c), _p(csq), _p(cnt), K, D, _p(nsplit), _stream())
    return c, csq, cnt


def _row_sqsum(x):
    out = torch.empty((x.shape[0],), dtype=torch.float32, device=x.device)
    lib.rg_row_sqsum(_p(x), _p(out), x.shape[0], x.shape[1], _stream())
    return out


def kmeans(x, k, niter=300, seed=1234, init_centroids=None, *, max_points_per_centroid=256, check_every=8, debug=False):
    """(labels int64 [N], centroids fp32 [k, D], info) — both on the device — of Lloyd's k-means on the rows of x fp32 [N, D]:
    faiss's Clustering::train (spherical = False, nredo = 1) with a deterministic split rule, so faiss's objective and iteration,
    not its seeded labels.

    Initial centroids: init_centroids [k, D] (e.g. last epoch's centres), else the training rows perm[:k] of faiss's
    rand_perm(n_train, seed + 1).  With N > k * max_points_per_centroid the iterations run on the rows
    rand_perm(N, seed)[:k * max_points_per_centroid]; the returned labels cover all N rows.  N == k returns the rows as centroids
    and labels = arange (faiss's shortcut).  Every iteration is assign, tally, update, split on the device; the loop stops at the
    first iteration whose labels equal the previous iteration's (a fixed point: further iterations reproduce the same centroids
    bit for bit), which the host learns every `check_every` iterations — any value gives the same labels, centroids and info.
    The returned labels are the assignment against the final centroids (at a fixed point: the last assignment).

    info: iterations (the one that found no change included), converged, obj (list of the per-iteration objectives
    sum_i min_j |x_i - c_j|^2), n_split, splits (per iteration), n_train; with
    debug=True also the device tensors cnt (after the split), rowptr, order and score of the last iteration that ran.
    N < k, a non-finite feature and a non-2-D input raise ValueError."""
    if not torch.is_tensor(x):
        raise TypeError("rg_hip: kmeans: x must be a tensor, got %s" % type(x).__name__)
    k, niter, check_every = int(k), int(niter), int(check_every)
    if x.dim() != 2:
        raise ValueError("rg_hip: kmeans: x must be [N, D], got shape %s" % (tuple(x.shape),))
    N, D = x.shape
    if k < 1 or N < k:
        raise ValueError("rg_hip: kmeans needs 1 <= k <= N, got N=%d k=%d" % (N, k))
    _chk_kmeans_shape(N, k, D)
    if niter < 0 or check_every < 1 or int(max_points_per_centroid) < 1:
        raise ValueError("rg_hip: kmeans needs niter >= 0, check_every >= 1 and max_points_per_centroid >= 1")
    x = _chk(x, "x")
    if not bool(torch.isfinite(x).all().item()):
        raise ValueError("rg_hip: kmeans: x holds a non-finite value")
    dev = x.device
    if init_centroids is not None:
        init_centroids = _chk(init_centroids, "init_centroids")
        if tuple(init_centroids.shape) != (k, D):
            raise ValueError("rg_hip: kmeans: init_centroids must be [%d, %d], got %s" % (k, D, tuple(init_centroids.shape)))
        if not bool(torch.isfinite(init_centroids).all().item()):
            raise ValueError("rg_hip: kmeans: init_centroids holds a non-finite value")
    info = dict(iterations=0, converged=False, obj=[], n_split=0, splits=[], n_train=N)
    if N == k and init_centroids is None:
        info["converged"] = True
        labels = torch.arange(N, dtype=torch.int64, device=dev)
        if debug:
            info.update(cnt=torch.ones((k,), dtype=torch.int32, device=dev), rowptr=torch.arange(k + 1, dtype=torch.int32, device=dev),
                        order=torch.arange(N, dtype=torch.int32, device=dev), score=-_row_sqsum(x))
        return labels, x.clone(), info

    n_train = min(N, k * int(max_points_per_centroid))
    if n_train < N:
        rows = torch.from_numpy(kmeans_rand_perm(N, n_train, seed)).to(dev)
        xt = x[rows].contiguous()
    else:
        xt = x
    info["n_train"] = n_train
    if init_centroids is not None:
        c = init_centroids.clone()
    else:
        c = xt[torch.from_numpy(kmeans_rand_perm(n_train, k, int(seed) + 1)).to(dev)].contiguous()
    csq = _row_sqsum(c)
    xsq = _row_sqsum(xt)

    # labels of the previous / the current iteration alternate between two buffers; iteration t writes its changed count, its
    # objective and its number of splits into slot t of three device arrays, so nothing is read back inside a batch
    i32 = lambda n: torch.empty((n,), dtype=torch.int32, device=dev)          # noqa: E731
    labs = [torch.full((n_train,), -1, dtype=torch.int32, device=dev), i32(n_train)]
    score = torch.empty((n_train,), dtype=torch.float32, device=dev)
    cnt, rowptr, order = i32(k), i32(k + 1), i32(n_train)
    slots = max(niter, 1)
    hist_changed, hist_split = torch.zeros((slots,), dtype=torch.int32, device=dev), torch.zeros((slots,), dtype=torch.int32, device=dev)
    hist_obj = torch.zeros((slots,), dtype=torch.float64, device=dev)
    a_bytes, t_bytes = _ws_query("rg_kmeans_assign_workspace", n_train, k, D), _ws_query("rg_kmeans_tally_workspace", n_train, k)
    ws = workspace(max(a_bytes, t_bytes), dev)
    s = _stream()
    ran, stop = 0, None
    while ran < niter and stop is None:
        batch = min(check_every, niter - ran)
        for t in range(ran, ran + batch):
            prev, cur = labs[t & 1], labs[(t + 1) & 1]
            lib.rg_kmeans_assign(_p(xt), _p(c), _p(csq), n_train, k, D, _p(cur), _p(score), _p(ws) if a_bytes else None, a_bytes, s)
            lib.rg_kmeans_tally(_p(cur), _p(prev), _p(xsq), _p(score), n_train, k, _p(cnt), _p(rowptr), _p(order),
                                hist_changed.data_ptr() + 4 * t, hist_obj.data_ptr() + 8 * t, _p(ws), t_bytes, s)
            lib.rg_kmeans_update(_p(xt), _p(order), _p(rowptr), n_train, k, D, _p(c), _p(csq), s)
            lib.rg_kmeans_split(_p(c), _p(csq), _p(cnt), k, D, hist_split.data_ptr() + 4 * t, s)
        ran += batch
        same = torch.nonzero(hist_changed[:ran] == 0).flatten()
        if same.numel():
            stop = int(same[0].item())
    iterations = ran if stop is None else stop + 1
    splits = hist_split[:iterations].cpu().tolist()
    info.update(iterations=iterations, converged=stop is not None, obj=hist_obj[:iterations].cpu().tolist(), n_split=sum(splits),
                splits=splits)
    if stop is not None and n_train == N:
        labels = labs[ran & 1].to(torch.int64)            # the last assignment: the labels of the fixed point
    else:
        labels = kmeans_assign(x, c, csq)[0].to(torch.int64)
    if debug:
        if ran == 0:
            raise ValueError("rg_hip: kmeans: debug=True needs niter >= 1")
        info.update(cnt=cnt, rowptr=rowptr, order=order, score=score)
    return labels, c, info
