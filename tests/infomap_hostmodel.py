"""numpy fp64 model of the two-level Infomap the device computes — the yardstick of tests/test_infomap_gpu.py,
itself pinned by tests/test_infomap_cpu.py.  Written from the definition, not from any implementation:

  links       row i of nbrs / dists [N, k] left to right; an entry with nbrs[i][j] == i is skipped; an entry with
              float32(dists[i][j]) <= float32(1.0 - min_sim) is the link i -> nbrs[i][j] of weight double(1.0f - dist); the first
              other entry (or a neighbour index outside [0, N)) ends the row.  A row without a link is a single.
  flow        PageRank in fp64, alpha = 0.15, teleportation to node j proportional to its in-link weight, a node without
              out-links teleports with probability 1: p <- normalise((1 - a) p W~ + (a sum_nondangling p + sum_dangling p) t)
              from uniform p over the nodes that occur in a link, until the L1 change is <= 1e-13 or 1000 iterations ran.
              Link flow q_ij = p_i w_ij / w_i^out normalised to sum 1, node flow p_j = sum_i q_ij.  (If no node with an
              out-link has an in-link no flow reaches a link; every node then stays a module of its own.)
  codelength  L = plogp(sum enter) - sum plogp(enter) - sum plogp(exit) + sum plogp(exit + p) - sum_nodes plogp(p_node), bits.
  search      sequential: units in index order move to the best module of a linked unit (gain > 1e-10 bits, ties to the
              lower module id), modules become units, repeat until nothing merges, then a leaf-level fine-tune sweep; coarse and
              fine rounds repeat until neither changes anything.  Every candidate is scored by a full recomputation of L.
  labels      every node that occurs in no link is a module of its own; modules with <= cluster_num members get -1; the rest
              are numbered 0 .. C-1 in ascending order of their smallest member.
"""
import numpy as np

ALPHA, FLOW_TOL, FLOW_MAX_ITERS, MIN_GAIN = 0.15, 1e-13, 1000, 1e-10


def links(nbrs, dists, min_sim):
    """(src int64 [E], dst int64 [E], w float64 [E], single bool [N]), links in row order"""
    nbrs, dists = np.asarray(nbrs), np.asarray(dists, dtype=np.float32)
    N, k = nbrs.shape
    thr = np.float32(1.0 - float(min_sim))
    src, dst, w = [], [], []
    single = np.zeros(N, dtype=bool)
    for i in range(N):
        count = 0
        for j in range(k):
            nb = int(nbrs[i, j])
            if nb == i:
                continue
            if 0 <= nb < N and dists[i, j] <= thr:
                src.append(i)
                dst.append(nb)
                w.append(float(np.float32(1.0) - dists[i, j]))
                count += 1
            else:
                break
        single[i] = count == 0
    return np.array(src, dtype=np.int64), np.array(dst, dtype=np.int64), np.array(w, dtype=np.float64), single


def get_links(nbrs, dists, min_sim):
    """the reference's return format: (list of singles, {(i, j): weight})"""
    src, dst, w, single = links(nbrs, dists, min_sim)
    return [int(i) for i in np.nonzero(single)[0]], {(int(a), int(b)): float(c) for a, b, c in zip(src, dst, w)}


def flow(N, src, dst, w):
    """(node flow [N], link flow [E], iterations); nodes in no link have flow 0"""
    wout = np.bincount(src, weights=w, minlength=N)
    win = np.bincount(dst, weights=w, minlength=N)
    hasout = np.bincount(src, minlength=N) > 0
    ingraph = hasout | (np.bincount(dst, minlength=N) > 0)
    tele = win / win.sum()
    p = ingraph / float(ingraph.sum())
    iters = 0
    while iters < FLOW_MAX_ITERS:
        s = np.bincount(dst, weights=p[src] * w / wout[src], minlength=N)
        raw = (1.0 - ALPHA) * s + (ALPHA * p[hasout].sum() + p[~hasout].sum()) * tele
        pn = raw / raw.sum()
        diff = np.abs(pn - p).sum()
        p = pn
        iters += 1
        if diff <= FLOW_TOL:
            break
    q = p[src] * w / wout[src]
    if q.sum() > 0:                      # 0: no node with an out-link has an in-link, no flow reaches a link
        q = q / q.sum()
    return np.bincount(dst, weights=q, minlength=N), q, iters


def plogp(x):
    x = np.asarray(x, dtype=np.float64)
    out = np.zeros_like(x)
    pos = x > 0
    out[pos] = x[pos] * np.log2(x[pos])
    return out


def codelength(src, dst, q, node_flow, labels):
    """L in bits of the partition `labels` (any integers) given link flow q and node flow"""
    _, lab = np.unique(np.asarray(labels), return_inverse=True)
    M = int(lab.max()) + 1
    cross = lab[src] != lab[dst]
    ex = np.bincount(lab[src][cross], weights=q[cross], minlength=M)
    en = np.bincount(lab[dst][cross], weights=q[cross], minlength=M)
    pm = np.bincount(lab, weights=node_flow, minlength=M)
    return float(plogp(en.sum()) - plogp(en).sum() - plogp(ex).sum() + plogp(ex + pm).sum() - plogp(node_flow).sum())


def _adjacency(N, src, dst):
    adj = [set() for _ in range(N)]
    for a, b in zip(src.tolist(), dst.tolist()):
        adj[a].add(b)
        adj[b].add(a)
    return adj


def best_move(unit, labels, adj, src, dst, q, node_flow, L0=None):
    """(gain, target module) of the best move of the nodes `unit` (all in one module) to the module of a linked node"""
    a = labels[unit[0]]
    cands = sorted({int(labels[j]) for i in unit for j in adj[i]} - {int(a)})
    if L0 is None:
        L0 = codelength(src, dst, q, node_flow, labels)
    best_gain, best_b = 0.0, None
    for b in cands:
        trial = labels.copy()
        trial[unit] = b
        gain = L0 - codelength(src, dst, q, node_flow, trial)
        if gain > MIN_GAIN and gain > best_gain:
            best_gain, best_b = gain, b
    return best_gain, best_b


def _sweeps(units, labels, adj, src, dst, q, node_flow, cap=100):
    any_move = False
    for _ in range(cap):
        moved = False
        for unit in units:
            L0 = codelength(src, dst, q, node_flow, labels)
            gain, b = best_move(unit, labels, adj, src, dst, q, node_flow, L0)
            if b is not None:
                labels[unit] = b
                moved = any_move = True
        if not moved:
            break
    return any_move


def _modules_as_units(labels):
    order = np.argsort(labels, kind="stable")
    cuts = np.nonzero(np.diff(labels[order]))[0] + 1
    groups = np.split(order, cuts)
    return sorted(groups, key=lambda g: int(g[0]))


def search(N, src, dst, q, node_flow, rounds=16):
    """module id int64 [N] of the sequential search (ids are arbitrary; nodes in no link stay alone)"""
    labels = np.arange(N, dtype=np.int64)
    adj = _adjacency(N, src, dst)
    for _ in range(rounds):
        changed = False
        while True:                                   # coarse: modules as units until nothing merges
            if not _sweeps(_modules_as_units(labels), labels, adj, src, dst, q, node_flow):
                break
            changed = True
        if _sweeps([np.array([i]) for i in range(N)], labels, adj, src, dst, q, node_flow):      # fine-tune
            changed = True
        if not changed:
            break
    return labels


def postprocess(modules, cluster_num):
    """float64 [N]: modules with <= cluster_num members -> -1, the rest numbered by ascending smallest member"""
    modules = np.asarray(modules)
    N = modules.shape[0]
    _, inv, counts = np.unique(modules, return_inverse=True, return_counts=True)
    first = np.full(counts.shape[0], N, dtype=np.int64)
    np.minimum.at(first, inv, np.arange(N))
    keep = counts > cluster_num
    number = np.full(counts.shape[0], -1, dtype=np.int64)
    kept = np.nonzero(keep)[0]
    number[kept[np.argsort(first[kept], kind="stable")]] = np.arange(kept.shape[0])
    return number[inv].astype(np.float64)


def cluster_by_infomap(nbrs, dists, min_sim, cluster_num=2, return_info=False):
    nbrs = np.asarray(nbrs)
    N = nbrs.shape[0]
    src, dst, w, single = links(nbrs, dists, min_sim)
    if src.shape[0] == 0:
        labels = postprocess(np.arange(N), cluster_num)
        return (labels, dict(codelength=0.0, modules=np.arange(N))) if return_info else labels
    node_flow, q, iters = flow(N, src, dst, w)
    modules = search(N, src, dst, q, node_flow) if q.sum() > 0 else np.arange(N)
    labels = postprocess(modules, cluster_num)
    if return_info:
        return labels, dict(codelength=codelength(src, dst, q, node_flow, modules), modules=modules, flow_iterations=iters,
                            src=src, dst=dst, w=w, q=q, node_flow=node_flow, single=single)
    return labels


def violating_moves(src, dst, q, node_flow, modules):
    """single-node moves to a linked module that gain more than MIN_GAIN (a finished search leaves none)"""
    modules = np.asarray(modules, dtype=np.int64).copy()
    adj = _adjacency(modules.shape[0], src, dst)
    L0 = codelength(src, dst, q, node_flow, modules)
    out = []
    for i in range(modules.shape[0]):
        gain, b = best_move(np.array([i]), modules, adj, src, dst, q, node_flow, L0)
        if b is not None:
            out.append((i, b, gain))
    return out


def weak_components(N, src, dst):
    parent = list(range(N))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for a, b in zip(src.tolist(), dst.tolist()):
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
    return np.array([find(i) for i in range(N)])


# ---------------------------------------------------------------------------------------------- fixtures
def ring_of_cliques(c, s):
    """(nbrs int32 [c s, s + 2], dists float32, planted int64): a ring of c cliques of s nodes, k = s + 2.  Row i (group
    g = i // s): self at 0; its s - 1 clique mates in ascending index at 0.2 + 0.001 x; for i % s == 0 a bridge to node
    ((g + 1) % c) s + s - 1 at 0.35; padding with the lowest-index nodes not yet in the row at 0.9."""
    N, k = c * s, s + 2
    nbrs = np.zeros((N, k), dtype=np.int32)
    dists = np.zeros((N, k), dtype=np.float32)
    for i in range(N):
        g = i // s
        row, d = [i], [0.0]
        for x, m in enumerate(j for j in range(g * s, g * s + s) if j != i):
            row.append(m)
            d.append(0.2 + 0.001 * x)
        if i % s == 0:
            row.append(((g + 1) % c) * s + s - 1)
            d.append(0.35)
        j = 0
        while len(row) < k:
            if j not in row:
                row.append(j)
                d.append(0.9)
            j += 1
        nbrs[i], dists[i] = row, d
    return nbrs, dists, np.arange(N, dtype=np.int64) // s


RINGS = ((8, 6), (5, 4), (3, 5), (16, 6))
# c x s: links, L planted, L one module, L singletons, lowest L over merges of two adjacent cliques
RING_TABLE = {(8, 6): (248, 2.8142, 5.5837, 7.5837, 3.0343), (5, 4): (65, 2.4232, 4.3191, 6.3191, 2.7348),
              (3, 5): (63, 2.5878, 3.9051, 5.9050, 3.1632), (16, 6): (496, 2.8375, 6.5837, 8.5837, 2.9460)}


def blobs(n_clusters, per, dim, sigma, seed=0):
    """(x float32 [n, dim] unit rows, planted int64 [n]): unit-norm centres, x = centre + sigma noise, renormalised"""
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((n_clusters, dim))
    centres /= np.linalg.norm(centres, axis=1, keepdims=True)
    planted = np.repeat(np.arange(n_clusters, dtype=np.int64), per)
    x = centres[planted] + sigma * rng.standard_normal((n_clusters * per, dim))
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    return x.astype(np.float32), planted


def knn_table(x, k):
    """(nbrs int32 [n, k], dists float32 [n, k]) by a stable descending sort of the fp32 inner products"""
    x = np.asarray(x, dtype=np.float32)
    sims = x @ x.T
    order = np.argsort(-sims, axis=1, kind="stable")[:, :k]
    return order.astype(np.int32), (np.float32(1.0) - np.take_along_axis(sims, order, axis=1)).astype(np.float32)


def blob_table(n_clusters, per, dim, sigma, k, seed=0):
    x, planted = blobs(n_clusters, per, dim, sigma, seed)
    nbrs, dists = knn_table(x, k)
    return nbrs, dists, planted


def ring_with_extras(c, s):
    """ring_of_cliques(c, s) plus three nodes: N = c s without an out-link (its row fails at once) that rows 1 and 2 link to
    at 0.3 (a dangling node with in-links), N + 1 that links to the first three nodes of clique 1 at 0.3 and has no in-link,
    N + 2 that occurs in no link.  (nbrs, dists, planted): the dangling node planted in clique 0, the other two alone."""
    nbrs, dists, planted = ring_of_cliques(c, s)
    N, k = nbrs.shape
    nbrs = np.concatenate([nbrs, np.zeros((3, k), dtype=np.int32)])
    dists = np.concatenate([dists, np.full((3, k), 0.9, dtype=np.float32)])
    for i in (1, 2):
        nbrs[i, s], dists[i, s] = N, 0.3
    for i in (N, N + 2):
        nbrs[i] = [i] + list(range(k - 1))
        dists[i, 0] = 0.0
    nbrs[N + 1] = [N + 1, s, s + 1, s + 2] + list(range(k - 4))
    dists[N + 1, :4] = [0.0, 0.3, 0.3, 0.3]
    return nbrs, dists, np.concatenate([planted, [0, c, c + 1]])
