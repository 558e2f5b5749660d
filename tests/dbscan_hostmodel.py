"""numpy model of scikit-learn's DBSCAN labels on a symmetric dense precomputed matrix — the yardstick of the device tests
(tests/test_dbscan_cpu.py ties it to scikit-learn itself and to the reference's recorded labels):

  adj[i][j] = d[i][j] <= eps, the diagonal included as it stands; core[i] = |adj[i]| >= min_samples;
  clusters = connected components of the core points under adj, numbered 0, 1, ... by ascending lowest core index;
  a non-core point gets the lowest cluster number among its core neighbours, -1 without one.
"""
import numpy as np


def neighbor_lists(d, eps):
    """per row the ascending columns with d[i][j] <= eps; a float32 / float16 matrix is compared in float32 against float32(eps)"""
    d = np.asarray(d)
    if d.dtype in (np.float32, np.float16):
        d, eps = d.astype(np.float32), np.float32(eps)
    return [np.nonzero(row <= eps)[0] for row in d]


def labels_from_lists(lists, min_samples):
    """(labels int64 [N], core_sample_indices int64, parent int64 [N]) from the neighbour lists; parent[i] = lowest core
    index of i's cluster for a core point, -1 otherwise"""
    n = len(lists)
    core = np.array([len(nb) >= min_samples for nb in lists], dtype=bool)
    labels = np.full(n, -1, dtype=np.int64)
    parent = np.full(n, -1, dtype=np.int64)
    n_clusters = 0
    for i in range(n):                       # ascending: a cluster is opened at its lowest core index
        if not core[i] or labels[i] >= 0:
            continue
        labels[i], parent[i] = n_clusters, i
        todo = [i]
        while todo:
            a = todo.pop()
            for b in lists[a]:
                if core[b] and labels[b] < 0:
                    labels[b], parent[b] = n_clusters, i
                    todo.append(b)
        n_clusters += 1
    for i in np.nonzero(~core)[0]:
        near = [labels[b] for b in lists[i] if core[b]]
        if near:
            labels[i] = min(near)
    return labels, np.nonzero(core)[0].astype(np.int64), parent


def dbscan(d, eps, min_samples):
    """(labels, core_sample_indices, n_clusters)"""
    labels, core_idx, _ = labels_from_lists(neighbor_lists(d, eps), min_samples)
    return labels, core_idx, int(labels.max()) + 1 if len(labels) else 0


def shared_border_points(d, eps, min_samples):
    """number of non-core points whose core neighbours lie in more than one cluster (where the lowest-number rule decides)"""
    lists = neighbor_lists(d, eps)
    labels, core_idx, _ = labels_from_lists(lists, min_samples)
    core = np.zeros(len(lists), dtype=bool)
    core[core_idx] = True
    return sum(1 for i in np.nonzero(~core)[0] if len({int(labels[b]) for b in lists[i] if core[b]}) > 1)


def random_case(seed):
    """(d float32 [n, n], eps, min_samples): Euclidean distances of n uniform points of the unit square, n in 20..119"""
    g = np.random.RandomState(seed)
    n = int(g.randint(20, 120))
    eps = float(g.choice([0.05, 0.08, 0.1, 0.125]))
    min_samples = int(g.choice([3, 4, 5]))
    pts = g.rand(n, 2)
    d = np.sqrt(((pts[:, None, :] - pts[None, :, :]) ** 2).sum(-1)).astype(np.float32)
    d = np.maximum(d, d.T)
    near = np.abs(d - np.float32(eps)) <= 1e-2       # keep every entry further than 1e-2 from eps: no rounding can matter
    d[near & (d <= eps)] -= np.float32(2e-2)
    d[near & (d > eps)] += np.float32(2e-2)
    return np.ascontiguousarray(np.maximum(d, 0)), eps, min_samples
