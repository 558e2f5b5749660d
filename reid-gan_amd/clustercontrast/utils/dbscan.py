"""DBSCAN on a precomputed distance matrix on the MI355X, with scikit-learn's labels.

Stands in for `sklearn.cluster.DBSCAN` in the pseudo-labelling step of examples/cluster_contrast_train_usl.py:157-161,
    cluster = DBSCAN(eps=eps, min_samples=4, metric='precomputed', n_jobs=-1)
    pseudo_labels = cluster.fit_predict(rerank_dist)
with one changed import line: `from clustercontrast.utils.dbscan import DBSCAN`.  The matrix may be the numpy array
`compute_jaccard_distance` returns (it is uploaded) or, with `return_device=True`, the device tensor itself, which then
never leaves the device (csrc/dbscan.hip through `ops.dbscan`).

The labels are the ones scikit-learn computes for a symmetric matrix: j is a neighbour of i where d[i, j] <= eps (the
diagonal is read like any other entry), a point with at least min_samples neighbours is a core point, clusters are the
connected components of the core points, numbered in ascending order of their lowest core index, and a non-core point
with core neighbours gets the lowest cluster number among them; every other point is -1.

Differences, all outside what the training scripts do:
  * only metric='precomputed' (raw features with a metric or a spatial index are not implemented);
  * the threshold is compared in float32 against float32(eps), float16 entries being widened first — what scikit-learn does
    for a float32 matrix with numpy >= 2; numpy 1.x compares in float64, which differs only for entries within one float32
    rounding of eps;
  * an asymmetric matrix makes scikit-learn's search directed, which is not reproduced: `check_symmetric=True` verifies bit
    symmetry on the device and raises ValueError (off by default: the Jaccard matrix is bit-symmetric by construction);
  * scikit-learn refuses negative entries; here a negative entry is simply <= eps;
  * no sample_weight; `n_jobs` is accepted and ignored.
"""
from __future__ import absolute_import

import numpy as np
import torch

from rg_hip import ops, search


class DBSCAN(object):
    def __init__(self, eps=0.5, *, min_samples=5, metric='precomputed', n_jobs=None, check_symmetric=False):
        self.eps = eps
        self.min_samples = min_samples
        self.metric = metric
        self.n_jobs = n_jobs
        self.check_symmetric = check_symmetric

    def _validated(self, X):
        """argument checks that need no device; returns X as a host or device tensor, float32 or float16"""
        if self.metric != 'precomputed':
            raise ValueError("DBSCAN: only metric='precomputed' is implemented on the device (an [N, N] distance matrix), "
                             "got metric=%r" % (self.metric,))
        if not float(self.eps) > 0.0:
            raise ValueError("DBSCAN: eps must be positive, got %r" % (self.eps,))
        if int(self.min_samples) != self.min_samples or int(self.min_samples) < 1:
            raise ValueError("DBSCAN: min_samples must be an integer >= 1, got %r" % (self.min_samples,))
        if not torch.is_tensor(X):
            X = np.asarray(X)
            if X.dtype not in (np.float32, np.float16):
                X = X.astype(np.float32)
            X = torch.from_numpy(np.ascontiguousarray(X))
        if X.dim() != 2 or X.shape[0] != X.shape[1] or X.shape[0] < 1:
            raise ValueError("DBSCAN: a precomputed distance matrix must be square [N, N], got shape %s" % (tuple(X.shape),))
        if X.dtype not in (torch.float32, torch.float16):
            X = X.float()
        return X

    def fit(self, X, y=None, sample_weight=None):
        if sample_weight is not None:
            raise ValueError("DBSCAN: sample_weight is not implemented")
        X = self._validated(X)
        d = X.detach().to(search.device()).contiguous()
        if self.check_symmetric:
            bad = ops.dbscan_asymmetry(d)
            if bad:
                raise ValueError("DBSCAN: the distance matrix is not symmetric (%d entries differ from their mirror)" % bad)
        labels, n_clusters, dbg = ops.dbscan(d, float(self.eps), int(self.min_samples), debug=True)
        self.labels_device_ = labels
        self.n_clusters_ = n_clusters
        self.labels_ = labels.cpu().numpy()
        self.core_sample_indices_ = torch.nonzero(dbg["core"]).flatten().cpu().numpy()
        return self

    def fit_predict(self, X, y=None, sample_weight=None):
        return self.fit(X, sample_weight=sample_weight).labels_
