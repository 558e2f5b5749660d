"""Cases and helpers shared by make_golden_rerank.py (reference side) and the re-ranking tests (fixture / device side).

Ranks are discrete, so the fixture is a fair yardstick only where the reference's own neighbour sets do not hinge on fp32
noise: every case satisfies the gap condition below (asserted by the generator, re-asserted from the stored inputs by
tests/test_rerank_fixture_cpu.py).  The sizes are about a third below the first draft's 256 / 320 / 288 rows so that the
stored features, the reference's outputs and the upper triangles of its (bit-symmetric) Jaccard matrices stay under 300 KB.
"""
import numpy as np

# name -> identities x copies, feature width, noise (relative to the unit centre), k1, k2
CASES = {
    "a": dict(n_id=21, per=8, D=64, noise=0.35, k1=20, k2=6),      # the function's defaults
    "b": dict(n_id=27, per=8, D=64, noise=0.35, k1=5, k2=1),       # k2 == 1 skips the expansion; round(5 / 2) = 2 (half to even)
    "c": dict(n_id=32, per=6, D=128, noise=0.30, k1=30, k2=6),     # the training script's defaults
}
SEEDS = range(300)
GAP = 1e-5            # ~30x the 3e-7 absolute error of an fp32 distance of order 1
LAMBDA = 0.3
DBSCAN_EPS, DBSCAN_MIN_SAMPLES = 0.6, 4


def make_features(n_id, per, D, noise, seed, scale=None):
    """fp32 [n_id * per, D]: `per` noisy copies (centre + noise * gaussian / sqrt(D)) of n_id random unit centres,
    L2-normalised, rows shuffled; scale = (lo, hi) multiplies every row by a factor drawn from that range afterwards"""
    g = np.random.RandomState(seed)
    c = g.randn(n_id, D)
    c /= np.linalg.norm(c, axis=1, keepdims=True)
    x = np.repeat(c, per, axis=0) + noise * g.randn(n_id * per, D) / np.sqrt(D)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    x = x[g.permutation(len(x))]
    if scale is not None:
        x = x * g.uniform(scale[0], scale[1], size=(len(x), 1))
    return np.ascontiguousarray(x, dtype=np.float32)


def half_k(k1):
    return int(np.around(k1 / 2.))


def sq_l2(x):
    """fp64 [N, N] squared L2 distances of the fp32 rows"""
    x = np.asarray(x, dtype=np.float64)
    n, out = len(x), np.empty((len(x), len(x)))
    step = max(1, (1 << 24) // max(1, n * x.shape[1]))          # differences of a row block: at most 128 MB
    for r0 in range(0, n, step):
        d = x[r0:r0 + step, None, :] - x[None, :, :]
        out[r0:r0 + step] = np.einsum("ijk,ijk->ij", d, d)
    return out


def euclid_inputs(x):
    """(q_g, q_q, g_g) fp32 Euclidean distance matrices, the first quarter of the rows being the queries"""
    d = np.sqrt(sq_l2(x)).astype(np.float32)
    q = len(x) // 4
    return d[:q, q:].copy(), d[:q, :q].copy(), d[q:, q:].copy()


def normalised_dist64(q_g, q_q, g_g):
    """re_ranking's transpose(d^2 / max(d^2, axis=0)) of the fp32 inputs, in fp64"""
    a = np.block([[q_q, q_g], [q_g.T, g_g]]).astype(np.float64) ** 2
    return np.transpose(a / a.max(axis=0))


def cut_gap(dist, k1, k2):
    """smallest gap, over all rows of the fp64 matrix `dist`, between consecutive sorted entries at the positions where a
    neighbour set is cut: k1-1|k1 and k1|k1+1, r|r+1 with r = round(k1 / 2), k2-1|k2"""
    s = np.sort(dist, axis=1)
    cuts = sorted({k1 - 1, k1, half_k(k1), k2 - 1})
    return min(float((s[:, c + 1] - s[:, c]).min()) for c in cuts)


def rank_of(dist, k):
    """first k columns of the row-wise ascending order (stable: ties by lower index)"""
    return np.argsort(dist, axis=1, kind="stable")[:, :k].astype(np.int32)


def pack_upper(m):
    i, j = np.triu_indices(m.shape[0])
    return np.ascontiguousarray(m[i, j])


def unpack_upper(v, n):
    m = np.empty((n, n), dtype=v.dtype)
    i, j = np.triu_indices(n)
    m[i, j] = v
    m[j, i] = v
    return m
