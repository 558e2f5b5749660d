"""k-means pseudo-labels (the fixed-K recipe): `label_generator_kmeans`, whose faiss.Kmeans(niter=300) becomes `ops.kmeans`
(csrc/kmeans.hip): faiss's objective and iteration under a deterministic split rule, not its seeded labels."""
from __future__ import absolute_import

import torch

from rg_hip import ops, search

__all__ = ["label_generator_kmeans"]


@torch.no_grad()
def label_generator_kmeans(features, num_classes=500, cuda=True, *, niter=300, seed=1234, init_centroids=None, return_device=False):
    """(labels numpy int64 [N], centers CPU float tensor [num_classes, D], num_classes, None) of `features` [N, D] (host or
    device tensor, or a numpy array); with return_device=True labels and centers are device tensors.  `cuda` is accepted and
    ignored: there is no CPU path.  init_centroids [num_classes, D] warm-starts from given centres."""
    assert num_classes, "num_classes for kmeans is null"
    x = search.to_device(features, "label_generator_kmeans: features", refuse_without_gpu=True)
    if init_centroids is not None:
        init_centroids = search.to_device(init_centroids, "label_generator_kmeans: init_centroids")
    labels, centers, _ = ops.kmeans(x, int(num_classes), niter=niter, seed=seed, init_centroids=init_centroids)
    if return_device:
        return labels, centers, num_classes, None
    labels = labels.cpu().numpy()          # every row has a nearest centroid: no -1
    return labels, centers.cpu(), num_classes, None
