"""numpy fp64 model of the k-means definition (include/reidgan_hip.h): faiss's Clustering::train with spherical =
False, nredo = 1 and the deterministic split rule.  Pinned by tests/test_kmeans_cpu.py, compared with the device by
tests/test_kmeans_gpu.py."""
import numpy as np

EPS = 1.0 / 1024.0


def mt19937_raw(seed, n):
    """the first n 32-bit draws of std::mt19937(seed) (numpy's legacy seeding is the same initialisation)"""
    return np.random.RandomState(int(seed))._bit_generator.random_raw(int(n))


def rand_perm(n, m, seed):
    """the first m entries of faiss's rand_perm(n, seed)"""
    perm = np.arange(n, dtype=np.int64)
    steps = min(m, n - 1)
    draws = mt19937_raw(seed, steps) if steps > 0 else []
    for i in range(steps):
        j = i + int(draws[i]) % (n - i)
        perm[i], perm[j] = perm[j], perm[i]
    return perm[:m].copy()


def init_perm(n, k, seed):
    """the rows that become the initial centroids: rand_perm(n, seed + 1)[:k]"""
    return rand_perm(n, k, seed + 1)


def scores(x, c):
    x, c = np.asarray(x, np.float64), np.asarray(c, np.float64)
    return (c * c).sum(1)[None, :] - 2.0 * (x @ c.T)


def assign(x, c):
    """(labels int64 [N], score fp64 [N]): argmin_j (|c_j|^2 - 2 x_i . c_j), ties to the lowest j (np.argmin's rule)"""
    s = scores(x, c)
    lab = np.argmin(s, axis=1)
    return lab.astype(np.int64), s[np.arange(s.shape[0]), lab]


def margin(x, c):
    """gap between the best and the second-best score per row (inf with one centroid)"""
    s = np.sort(scores(x, c), axis=1)
    return s[:, 1] - s[:, 0] if s.shape[1] > 1 else np.full(s.shape[0], np.inf)


def tau(x, c, D):
    """8 * D * 2^-24 * (|x_i|^2 + max_j |c_j|^2): the worst-case fp32 accumulation error D * 2^-24 * sum_d |x_d c_d| <=
    D * 2^-24 * (|x|^2 + |c|^2) / 2 on each of the two scores compared (the score is twice the product), with a factor 8 of
    room.  A row whose fp64 margin reaches it cannot legitimately get another label."""
    x, c = np.asarray(x, np.float64), np.asarray(c, np.float64)
    return 8.0 * D * 2.0 ** -24 * ((x * x).sum(1) + (c * c).sum(1).max())


def excused(x, c):
    return margin(x, c) < tau(x, c, np.asarray(x).shape[1])


def tally(labels, K):
    """(cnt [K], rowptr [K + 1], order [N]): members cluster by cluster in ascending row index"""
    labels = np.asarray(labels, np.int64)
    cnt = np.bincount(labels, minlength=K).astype(np.int64)
    rowptr = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    return cnt, rowptr, np.argsort(labels, kind="stable").astype(np.int64)


def update(x, labels, c_prev):
    """member means; a cluster without a member keeps its row"""
    x = np.asarray(x, np.float64)
    c = np.array(c_prev, np.float64, copy=True)
    for j in range(c.shape[0]):
        m = labels == j
        if m.any():
            c[j] = x[m].mean(0)
    return c


def split(c, cnt):
    """(c, cnt, n_split) after the deterministic split: empties in ascending index, donor = largest count (lowest index on ties)"""
    c, cnt = np.array(c, np.float64, copy=True), np.array(cnt, np.int64, copy=True)
    s = np.where(np.arange(c.shape[1]) % 2 == 0, EPS, -EPS)
    ns = 0
    for e in range(c.shape[0]):
        if cnt[e] != 0:
            continue
        donor = int(np.argmax(cnt))
        if cnt[donor] <= 0 or donor == e:
            break
        c[e] = c[donor] * (1.0 + s)
        c[donor] = c[donor] * (1.0 - s)
        cnt[e] = cnt[donor] // 2
        cnt[donor] -= cnt[e]
        ns += 1
    return c, cnt, ns


def lloyd(x, c0, niter, trace=False):
    """dict(labels, centroids, iterations, converged, obj, n_split, cnt): every iteration is assign, tally, update, split; the
    loop stops after the first iteration whose labels equal the previous iteration's.  labels = the assignment against the final
    centroids; cnt = the counts after the last split.  trace=True adds `steps`: the (labels, centroids before the assignment) of
    every iteration."""
    x = np.asarray(x, np.float64)
    c = np.array(c0, np.float64, copy=True)
    K = c.shape[0]
    xsq = (x * x).sum(1)
    prev = np.full(x.shape[0], -1, np.int64)
    out = dict(iterations=0, converged=False, obj=[], n_split=0, cnt=None, steps=[])
    for it in range(niter):
        lab, sc = assign(x, c)
        if trace:
            out["steps"].append((lab, c.copy()))
        out["obj"].append(float((xsq + sc).sum()))
        changed = int((lab != prev).sum())
        cnt = np.bincount(lab, minlength=K)
        c = update(x, lab, c)
        c, cnt, ns = split(c, cnt)
        out["n_split"] += ns
        out["cnt"] = cnt
        out["iterations"] = it + 1
        prev = lab
        if changed == 0:
            out["converged"] = True
            break
    out["labels"] = assign(x, c)[0]
    out["centroids"] = c
    return out


def centroid_bound(x, labels, c):
    """per-element bound of a centroid computed as the device does (fp64 accumulation, one rounding to fp32) against the fp64
    mean: one fp32 ulp of the mean (a sum that differs in the last fp64 bits can round to the neighbouring float) plus the fp64
    accumulation error"""
    x, c = np.asarray(x, np.float64), np.asarray(c, np.float64)
    b = 2.0 ** -23 * np.abs(c)
    for j in range(c.shape[0]):
        m = labels == j
        if m.any():
            b[j] += 2.0 ** -45 * np.abs(x[m]).sum(0)
    return b


def blobs(seed, K=6, D=24, N=600):
    """(x fp32 [N, D], planted labels): K centres 4 * randn, unit noise"""
    r = np.random.RandomState(seed)
    centres = 4.0 * r.randn(K, D)
    planted = r.randint(0, K, size=N)
    x = centres[planted] + r.randn(N, D)
    return x.astype(np.float32), planted


def lattice(seed=0, N=300, D=5):
    """(x fp32 [N, D] of integers in [-3, 3], c0 = the first four rows each duplicated)"""
    r = np.random.RandomState(seed)
    x = r.randint(-3, 4, size=(N, D)).astype(np.float32)
    c0 = np.repeat(x[:4], 2, axis=0).copy()
    return x, c0
