"""Plain numpy model of the staged re-ranking pipeline (csrc/rerank.hip), for the tests: the same stages on the same
intermediate objects (ranking -> expanded sets -> weights -> query expansion -> Jaccard rows), dense and slow."""
import numpy as np


def expand_sets(rank, kf, kh):
    """list of sorted unique int arrays: R(i, kf) united with every R(c, kh), c in R(i, kf), that lies to more than two
    thirds inside R(i, kf);  R(i, k) = { j in rank[i, :k] : i in rank[j, :k] }"""
    n = rank.shape[0]

    def recip(i, k):
        fwd = rank[i, :k]
        return fwd[(rank[fwd, :k] == i).any(axis=1)]

    full = [recip(i, kf) for i in range(n)]
    half = [recip(i, kh) for i in range(n)]
    out = []
    for i in range(n):
        members = set(full[i].tolist())
        grown = set(members)
        for c in full[i]:
            h = half[c]
            if len(members.intersection(h.tolist())) > 2. / 3 * len(h):
                grown.update(h.tolist())
        out.append(np.array(sorted(grown), dtype=np.int64))
    return out


def dense_weights(sets, x=None, orig=None):
    """fp32 [N, N]: row i holds softmax(-(2 - 2 x_i . x_e)) (features) or exp(-orig[i, e]) / sum (distances) on its set"""
    n = len(sets)
    V = np.zeros((n, n), dtype=np.float32)
    for i, s in enumerate(sets):
        if x is not None:
            d = -(2.0 - 2.0 * (x[s].astype(np.float64) @ x[i].astype(np.float64)))
            e = np.exp(d - d.max())
        else:
            e = np.exp(-orig[i, s].astype(np.float64))
        V[i, s] = (e / e.sum()).astype(np.float32)
    return V


def query_expand(V, rank, k2):
    if k2 == 1:
        return V
    acc = np.zeros_like(V)
    for l in range(k2):
        acc += V[rank[:, l]]
    return acc / np.float32(k2)


def jaccard_rows(V, rows):
    """fp32 [len(rows), N]: 1 - m / (2 - m), m[j] = sum_c min(V[i, c], V[j, c]) over the non-zero columns of row i"""
    out = np.empty((len(rows), V.shape[0]), dtype=np.float32)
    for t, i in enumerate(rows):
        nz = np.nonzero(V[i])[0]
        m = np.minimum(V[i, nz][None, :], V[:, nz]).astype(np.float64).sum(axis=1)
        out[t] = (1.0 - m / (2.0 - m)).astype(np.float32)
    return out
