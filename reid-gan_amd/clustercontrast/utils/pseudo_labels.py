"""The per-epoch pseudo-labelling of examples/cluster_contrast_train_usl.py:146-200 as one call that stays on the device:

    rerank_dist = compute_jaccard_distance(features, k1=args.k1, k2=args.k2)          # [N, N]
    pseudo_labels = DBSCAN(eps, min_samples=4, metric='precomputed').fit_predict(rerank_dist)
    cluster_features = generate_cluster_features(pseudo_labels, features)

becomes `pseudo_labels, num_cluster, cluster_features = dbscan_pseudo_labels(features, k1, k2, eps)`.  The [N, N] matrix is
neither copied to the host nor duplicated; only the N labels come back, because the caller builds its dataset list from them
(:195-198).  `cluster_features` is the un-normalised per-cluster mean in ascending label order, ready for
`F.normalize(cluster_features, dim=1)` into `ClusterMemory.features`.

`infomap_pseudo_labels` is the same for examples/cluster_contrast_gan_train_usl_infomap.py:318-348 (normalise, get_dist_nbr,
cluster_by_infomap, generate_cluster_features): kNN table, Infomap and centroids stay on the device.

`kmeans_pseudo_labels` is the fixed-K recipe: `label_generator_kmeans` (clustercontrast/models/kmeans.py, k-means with
num_classes centroids on `ops.kmeans`) followed by generate_cluster_features; it has no outliers, so every row carries a label.
"""
from __future__ import absolute_import, print_function

import time

import torch

from rg_hip import ops, search
from .faiss_rerank import compute_jaccard_distance
from .infomap_cluster import cluster_by_infomap, generate_cluster_features_device, get_dist_nbr


def _finish(labels, x, any_cluster, print_flag, line, end):
    """the shared epilogue: (labels as numpy, per-cluster means of x [N, D] in ascending label order — an empty [0, D] tensor
    without a cluster); `line(pseudo_labels, cluster_features)` is the recipe's progress line without its time"""
    if any_cluster:
        cluster_features = generate_cluster_features_device(labels, x)
    else:
        cluster_features = torch.empty((0, x.shape[1]), dtype=torch.float32, device=labels.device)
    pseudo_labels = labels.cpu().numpy()
    if print_flag:
        print("{}, time cost: {}".format(line(pseudo_labels, cluster_features), time.time() - end))
    return pseudo_labels, cluster_features


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
    pseudo_labels, cluster_features = _finish(
        labels, search.as_matrix(features, "dbscan_pseudo_labels: features"), num_cluster, print_flag,
        lambda pl, cf: "DBSCAN pseudo labels: {} clusters, {} outliers".format(num_cluster, int((pl == -1).sum())), end)
    return pseudo_labels, num_cluster, cluster_features


@torch.no_grad()
def infomap_pseudo_labels(features, k=15, min_sim=0.5, cluster_num=4, print_flag=False):
    """(pseudo_labels numpy int64 [N], cluster_features device tensor [C, D], info) of `features` [N, D] (host or device
    tensor): the rows are L2-normalised, searched for their k nearest neighbours and clustered by the two-level Infomap of
    cluster_by_infomap; -1 marks a sample whose cluster has <= cluster_num members.  cluster_features is the un-normalised
    mean of the normalised rows of every cluster in ascending label order (an empty [0, D] tensor without a cluster).  Only
    the N labels are copied out.  The defaults are the scripts' --k1 15 --eps 0.5 --k2 4."""
    end = time.time()
    x = search.to_device(features, "infomap_pseudo_labels: features", refuse_without_gpu=True)
    x = torch.nn.functional.normalize(x, dim=1).contiguous()
    dists, nbrs = get_dist_nbr(x, k=int(k), knn_method='faiss-gpu', return_device=True)
    labels, info = cluster_by_infomap(nbrs, dists, min_sim=min_sim, cluster_num=cluster_num, return_device=True, return_info=True)
    pseudo_labels, cluster_features = _finish(
        labels, x, info["n_clusters"], print_flag,
        lambda pl, cf: "Infomap pseudo labels: {} clusters, {} outliers, codelength {:.4f} bits".format(
            info["n_clusters"], int((pl == -1).sum()), info["codelength"]), end)
    return pseudo_labels, cluster_features, info


@torch.no_grad()
def kmeans_pseudo_labels(features, num_classes=500, niter=300, print_flag=False):
    """(pseudo_labels numpy int64 [N], cluster_features device tensor [C, D], info) of `features` [N, D] (host or device
    tensor), used as given — the caller normalises, as the scripts do before clustering.  The labels are those of
    `ops.kmeans` with num_classes centroids (info is its info); cluster_features is the un-normalised mean of the rows of every
    label that occurs, in ascending label order: C == num_classes unless the final assignment leaves a centroid without a
    row.  Only the N labels are copied out."""
    end = time.time()
    x = search.to_device(features, "kmeans_pseudo_labels: features", refuse_without_gpu=True)
    labels, _, info = ops.kmeans(x, int(num_classes), niter=int(niter))
    pseudo_labels, cluster_features = _finish(
        labels, x, True, print_flag,
        lambda pl, cf: "k-means pseudo labels: {} clusters, {} iterations, objective {:.4f}".format(
            cf.shape[0], info["iterations"], info["obj"][-1] if info["obj"] else float("nan")), end)
    return pseudo_labels, cluster_features, info
