"""The per-epoch Infomap pseudo-labelling on the MI355X: kNN search and community detection, without faiss or `infomap`.

Mirror of CC/clustercontrast/utils/infomap_cluster.py: `knn_faiss` (:51-111), `knns2ordered_nbrs` (:114-125), `get_links`
(:129-144), `cluster_by_infomap` (:147-227), `get_dist_nbr` (:230-234) — same names, arguments and return formats — so

    feat_dists, feat_nbrs = get_dist_nbr(features=features_array, k=opt.k1, knn_method='faiss-gpu')
    pseudo_labels = cluster_by_infomap(feat_nbrs, feat_dists, min_sim=opt.eps, cluster_num=opt.k2)

(examples/cluster_contrast_gan_train_usl_infomap.py:321-325) run unchanged.  The brute-force inner-product search is the
MFMA GEMM (row blocks of X X^T) followed by `rg_topk_rows`; `knn_method` is accepted and ignored.  Result order: similarity
descending, ties by lower index (faiss leaves ties unspecified).

`cluster_by_infomap` runs on the device (csrc/infomap.hip through `ops.infomap`): link construction, PageRank flow, a
deterministic two-level map-equation search and the reference's post-processing.  It minimises the objective the `infomap`
package minimises under "--two-level --directed" (DESIGN §6 has the definition); the package's search is seeded and
stochastic, so equality with its labels is not claimed.  The labels are bit-reproducible: every rank of a data-parallel run
reaches the same ones without a broadcast.  Departures from the reference's function: kept clusters are numbered by
ascending smallest member (the reference enumerates a Python set, an unspecified order; the scripts use labels as identities
only), and a node with in-links but no out-links keeps the module the search gives it (the reference would trip its own
`idx_len == node_count` assert there).  Rows must be free of duplicate neighbours, as a kNN search gives them.

`generate_cluster_features` is the nested helper of the example script (:332-348).
"""
from __future__ import absolute_import

import collections

import numpy as np
import torch

from rg_hip import ops, search


class knn_faiss(object):
    """Brute-force inner-product kNN (for L2-normalised features: cosine similarity)."""

    def __init__(self, feats, k, knn_method='faiss-cpu', verbose=True):
        self.verbose = verbose
        x = search.to_device(feats, "knn_faiss: feats")
        # [rows, n] inner products per block
        self.nbrs, self.sims = search.blocked_topk(x.shape[0], k, lambda r0, r1: ops.linear_fwd(x[r0:r1], x), want_values=True)
        self._knns = None

    @property
    def knns(self):
        """the reference's list of (nbrs int32 [k], 1 - similarity fp32 [k]) per row, copied from the device when first asked
        for: a caller that stays on the device (`.nbrs` / `.sims`, get_dist_nbr(..., return_device=True)) never pays for it"""
        if self._knns is None:
            nb, sm = self.nbrs.cpu().numpy(), self.sims.cpu().numpy()
            self._knns = [(np.array(a, dtype=np.int32), 1 - np.array(s, dtype=np.float32)) for a, s in zip(nb, sm)]
        return self._knns

    def filter_by_th(self, i):
        th_nbrs, th_dists = [], []
        nbrs, dists = self.knns[i]
        for n, dist in zip(nbrs, dists):
            if 1 - dist < self.th:
                continue
            th_nbrs.append(n)
            th_dists.append(dist)
        return np.array(th_nbrs), np.array(th_dists)

    def get_knns(self, th=None):
        if th is None or th <= 0.:
            return self.knns
        self.th = th
        return [self.filter_by_th(i) for i in range(len(self.knns))]


def knns2ordered_nbrs(knns, sort=True):
    if isinstance(knns, list):
        knns = np.array(knns)
    nbrs = knns[:, 0, :].astype(np.int32)
    dists = knns[:, 1, :]
    if sort:
        nb_idx = np.argsort(dists, axis=1)
        idxs = np.arange(nb_idx.shape[0]).reshape(-1, 1)
        dists = dists[idxs, nb_idx]
        nbrs = nbrs[idxs, nb_idx]
    return dists, nbrs


def get_dist_nbr(features, k=80, knn_method='faiss-cpu', return_device=False):
    """(dists [n, k], nbrs int32 [n, k]) as the reference (dists: fp32 values in the float64 array its np.array(knns) makes);
    return_device=True (not in the reference) returns the tables as fp32 / int32 device tensors and copies nothing to the
    host.  Both are in ascending distance.  The device tables keep the search's order among equal distances (lower index
    first); the host path re-sorts every row with the reference's np.argsort, which is not stable, so rows with exactly
    equal distances may come out permuted there — where a row has no tie the two tables are equal entry for entry."""
    index = knn_faiss(feats=features, k=k, knn_method=knn_method)
    if return_device:
        return (1 - index.sims).contiguous(), index.nbrs.contiguous()
    knns = index.get_knns()
    dists, nbrs = knns2ordered_nbrs(knns)
    return dists, nbrs


@torch.no_grad()
def generate_cluster_features(labels, features):
    """centroid of every pseudo-label (label -1 = outlier skipped), rows ordered by ascending label
    (examples/cluster_contrast_gan_train_usl_infomap.py:332-348); `features` [n, D] tensor, returns a device tensor."""
    labels = np.asarray(labels)
    groups = collections.defaultdict(list)
    for i, lb in enumerate(labels.tolist()):
        if lb == -1:
            continue
        groups[lb].append(i)
    keys = sorted(groups.keys())
    if not keys:
        raise ValueError("generate_cluster_features: every sample is an outlier")
    order = [i for kk in keys for i in groups[kk]]
    offsets = np.cumsum([0] + [len(groups[kk]) for kk in keys])
    x = search.to_device(features, "generate_cluster_features: features", rows_ok=True)
    return ops.segment_mean(x, torch.tensor(order, dtype=torch.int64).to(x.device), torch.tensor(offsets, dtype=torch.int64).to(x.device))


@torch.no_grad()
def generate_cluster_features_device(labels, features):
    """`generate_cluster_features` for int64 labels that already live on the device (ops.dbscan's): the member lists are
    built there by a stable sort of the non-negative labels, so every cluster is summed in ascending sample index like the
    host loop above and the centroids equal its result bit for bit.  No label leaves the device; returns a device tensor
    [number of distinct labels, D]."""
    if not torch.is_tensor(labels) or not labels.is_cuda or labels.dtype != torch.int64 or labels.dim() != 1:
        raise TypeError("generate_cluster_features_device: labels must be a 1-D int64 device tensor")
    x = search.as_matrix(features, "generate_cluster_features_device: features", rows_ok=True).to(labels.device).contiguous()
    if x.shape[0] != labels.numel():
        raise ValueError("generate_cluster_features_device: features %s do not match %d labels" % (tuple(x.shape), labels.numel()))
    keep = torch.nonzero(labels != -1).flatten()                  # ascending sample index
    if keep.numel() == 0:
        raise ValueError("generate_cluster_features_device: every sample is an outlier")
    _, perm, offsets = ops.sorted_segments(labels[keep], ptr_dtype=torch.int64)
    return ops.segment_mean(x, keep[perm].contiguous(), offsets)


def _check_min_sim(min_sim, who):
    if not 0.0 < float(min_sim) <= 1.0:
        raise ValueError("%s: min_sim must lie in (0, 1] (a link weight 1 - dist has to be positive), got %r" % (who, min_sim))


def _table_on_device(nbrs, dists, who):
    """the kNN table as contiguous int32 / fp32 device tensors; numpy arrays are copied over, host tensors are refused"""
    if not torch.cuda.is_available():
        raise RuntimeError("%s: nbrs / dists must live on the GPU; the HIP path has no CPU fallback" % who)
    out = []
    for t, name, dtype in ((nbrs, "nbrs", torch.int32), (dists, "dists", torch.float32)):
        if torch.is_tensor(t):
            if not t.is_cuda:
                raise RuntimeError("%s: %s must live on the GPU (got %s); the HIP path has no CPU fallback" % (who, name, t.device))
            if t.dtype != dtype:
                raise TypeError("%s: %s must be %s on the device, got %s" % (who, name, dtype, t.dtype))
            if not t.is_contiguous():
                raise ValueError("%s: %s must be contiguous (shape %s, strides %s)" % (who, name, tuple(t.shape), t.stride()))
        else:
            a = np.asarray(t)
            if a.ndim != 2:
                raise ValueError("%s: %s must be an [N, k] table, got shape %s" % (who, name, a.shape))
            t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32 if dtype == torch.int32 else np.float32))
        out.append(t)
    nbrs, dists = out
    if nbrs.dim() != 2 or tuple(nbrs.shape) != tuple(dists.shape):
        raise ValueError("%s: nbrs %s and dists %s must be equal [N, k] tables" % (who, tuple(nbrs.shape), tuple(dists.shape)))
    if not (1 <= nbrs.shape[0] <= ops.INFOMAP_MAX_N and 1 <= nbrs.shape[1] <= ops.INFOMAP_MAX_K):
        raise ValueError("%s needs 1 <= N <= %d and 1 <= k <= %d, got N=%d k=%d"
                         % (who, ops.INFOMAP_MAX_N, ops.INFOMAP_MAX_K, nbrs.shape[0], nbrs.shape[1]))
    dev = search.device()
    return nbrs.to(dev), dists.to(dev)


def get_links(single, links, nbrs, dists, min_sim):
    """the reference's get_links (:129-144): appends the rows without a link to `single`, adds (i, j) -> float(1 - dist) to
    `links`, returns both; filled from the device's link lists.  0 < min_sim <= 1, so that every link weight is positive."""
    _check_min_sim(min_sim, "get_links")
    nbrs, dists = _table_on_device(nbrs, dists, "get_links")
    g = ops.infomap_links(nbrs, dists, float(min_sim))
    single.extend(int(i) for i in torch.nonzero(g["single"]).flatten().cpu().numpy())
    src, dst, w = g["src"].cpu().numpy(), g["dst"].cpu().numpy(), g["w"].cpu().numpy()
    for a, b, c in zip(src.tolist(), dst.tolist(), w.tolist()):
        links[(a, b)] = c
    return single, links


@torch.no_grad()
def cluster_by_infomap(nbrs, dists, min_sim, cluster_num=2, *, return_device=False, return_info=False):
    """float64 numpy [N] pseudo-labels of the reference's cluster_by_infomap (-1: the sample's cluster has <= cluster_num
    members), from nbrs / dists [N, k] as get_dist_nbr returns them (numpy) or as int32 / fp32 device tensors.
    return_device=True: int64 device labels instead, and nothing but scalars leaves the device.  return_info=True: also a
    dict with codelength, codelength_one_module (bits), n_modules, n_singles, levels, sweeps, flow_iterations, converged, and
    beyond the reference-shaped list n_clusters (kept clusters) and rollbacks (sweeps undone for their single best move); the
    same keys on every path.  0 < min_sim <= 1."""
    if int(cluster_num) != cluster_num or int(cluster_num) < 0:
        raise ValueError("cluster_by_infomap: cluster_num must be an integer >= 0, got %r" % (cluster_num,))
    _check_min_sim(min_sim, "cluster_by_infomap")
    nbrs, dists = _table_on_device(nbrs, dists, "cluster_by_infomap")
    labels, info = ops.infomap(nbrs, dists, float(min_sim), int(cluster_num))
    info = {k: info[k] for k in ("codelength", "codelength_one_module", "n_modules", "n_singles", "levels", "sweeps",
                                 "flow_iterations", "converged", "n_clusters", "rollbacks")}
    out = labels if return_device else labels.cpu().numpy().astype(np.float64)
    return (out, info) if return_info else out
