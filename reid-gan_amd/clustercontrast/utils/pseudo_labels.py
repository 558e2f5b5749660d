"""The per-epoch pseudo-labelling of examples/cluster_contrast_train_usl.py:146-200 as one call that stays on the device:

    rerank_dist = compute_jaccard_distance(features, k1=args.k1, k2=args.k2)          # [N, N]
    pseudo_labels = DBSCAN(eps, min_samples=4, metric='precomputed').fit_predict(rerank_dist)
    cluster_features = generate_cluster_features(pseudo_labels, features)

becomes `pseudo_labels, num_cluster, cluster_features = dbscan_pseudo_labels(features, k1, k2, eps)`.  The [N, N] matrix is
neither copied to the host nor duplicated; only the N labels come back, because the caller builds its dataset list from them
(:195-198).  `cluster_features` is the un-normalised per-cluster mean in ascending label order, ready for
`F.normalize(cluster_features, dim=1)` into `ClusterMemory.features`.
"""
from __future__ import absolute_import, print_function

import time

import torch

from rg_hip import ops
from .faiss_rerank import compute_jaccard_distance
from .infomap_cluster import generate_cluster_features_device


@torch.no_grad()
def dbscan_pseudo_labels(features, k1=30, k2=6, eps=0.6, min_samples=4, print_flag=False):
    """(pseudo_labels numpy int64 [N], num_cluster int, cluster_features device tensor [num_cluster, D]) of `features` [N, D]
    (host or device tensor).  Labels are scikit-learn's DBSCAN(eps, min_samples, metric='precomputed') labels of the
    k-reciprocal Jaccard distance; -1 marks an outlier.  With no cluster at all, cluster_features is an empty [0, D] tensor."""
    if not float(eps) > 0.0:
        raise ValueError("dbscan_pseudo_labels: eps must be positive, got %r" % (eps,))
    if int(min_samples) < 1:
        raise ValueError("dbscan_pseudo_labels: min_samples must be >= 1, got %r" % (min_samples,))
    end = time.time()
    dist = compute_jaccard_distance(features, k1=k1, k2=k2, print_flag=print_flag, return_device=True)
    labels, num_cluster = ops.dbscan(dist, float(eps), int(min_samples))
    del dist
    x = features if torch.is_tensor(features) else torch.as_tensor(features)
    if num_cluster:
        cluster_features = generate_cluster_features_device(labels, x)
    else:
        cluster_features = torch.empty((0, x.shape[1]), dtype=torch.float32, device=labels.device)
    pseudo_labels = labels.cpu().numpy()
    if print_flag:
        print("DBSCAN pseudo labels: {} clusters, {} outliers, time cost: {}".format(
            num_cluster, int((pseudo_labels == -1).sum()), time.time() - end))
    return pseudo_labels, num_cluster, cluster_features
