"""Two-level Infomap (csrc/infomap.hip): the entry-point wrappers and the host-driven search over them."""
from __future__ import absolute_import

import torch

from ._base import _chk_rr, _eps32, _list_total, _p, _stream, lib
from .retrieval import compact_labels, sorted_segments


# ------------------------------------------------------------------------------------------------
# Two-level Infomap on a kNN table (csrc/infomap.hip): links, PageRank flow, codelength, search, labels
# ------------------------------------------------------------------------------------------------
INFOMAP_MAX_N, INFOMAP_MAX_K = 65536, 128
INFOMAP_FLOW_MAX_ITERS = 1000        # power iterations (the definition's cap)
INFOMAP_FLOW_BATCH = 16              # iterations enqueued per readback of the done flag
INFOMAP_SWEEP_CAP = 200              # sweeps per level
INFOMAP_LEVEL_CAP = 32               # aggregations per coarse phase
INFOMAP_ROUND_CAP = 16               # coarse + fine rounds


def _chk_infomap_table(nbrs, dists):
    nbrs, dists = _chk_rr(nbrs, "nbrs", torch.int32, 2), _chk_rr(dists, "dists", torch.float32, 2)
    if tuple(nbrs.shape) != tuple(dists.shape):
        raise ValueError("rg_hip: infomap: nbrs %s and dists %s disagree" % (tuple(nbrs.shape), tuple(dists.shape)))
    N, k = nbrs.shape
    if not (1 <= N <= INFOMAP_MAX_N and 1 <= k <= INFOMAP_MAX_K):
        raise ValueError("rg_hip: infomap needs 1 <= N <= %d and 1 <= k <= %d, got N=%d k=%d" % (INFOMAP_MAX_N, INFOMAP_MAX_K, N, k))
    return nbrs, dists


def _chk_infomap_graph(g, flow=False):
    if not isinstance(g, dict) or "rowptr" not in g or (flow and "q" not in g):
        raise TypeError("rg_hip: infomap: expected the graph of infomap_links%s" % (" with the flow of infomap_flow" if flow else ""))
    for name in ("rowptr", "src", "dst", "in_rowptr", "in_src", "in_eid", "single"):
        _chk_rr(g[name], name, torch.int32, 1)
    _chk_rr(g["w"], "w", torch.float64, 1)
    if flow:
        for name in ("q", "iq", "flow", "scal"):
            _chk_rr(g[name], name, torch.float64, 1)
    N, E = g["N"], g["E"]
    if not (1 <= N <= INFOMAP_MAX_N) or g["rowptr"].numel() != N + 1 or g["in_rowptr"].numel() != N + 1 or \
            any(g[n].numel() != E for n in ("src", "dst", "w", "in_src", "in_eid")):
        raise ValueError("rg_hip: infomap: the graph's arrays disagree with N=%d, E=%d" % (N, E))
    return g


def infomap_links(nbrs, dists, min_sim):
    """The link graph of a kNN table nbrs int32 / dists fp32 [N, k] (rows free of duplicate neighbours, as a kNN search gives
    them): row i left to right, an entry with nbrs == i is skipped, an entry with dists <= float32(1 - min_sim) is the link
    i -> nbrs[i][j] of weight double(1.0f - dist), the first other entry (or an index outside [0, N)) ends the row.  Returns
    {"N", "E", "rowptr" [N + 1], "src", "dst" int32 [E], "w" fp64 [E] (row order), "single" int32 [N], "in_rowptr" [N + 1],
    "in_src", "in_eid" int32 [E]}: the in-list of a node holds its sources in ascending order and the position of each link
    in the out list.  Reads one integer back (E)."""
    nbrs, dists = _chk_infomap_table(nbrs, dists)
    if not 0.0 < float(min_sim) <= 1.0:      # a link has dist <= 1 - min_sim < 1, so every weight 1 - dist is positive
        raise ValueError("rg_hip: infomap needs 0 < min_sim <= 1, got %r" % (min_sim,))
    N, k = nbrs.shape
    thr = _eps32(1.0 - float(min_sim))
    dev = nbrs.device
    cnt = torch.empty((N,), dtype=torch.int32, device=dev)
    rowptr = torch.empty((N + 1,), dtype=torch.int32, device=dev)
    lib.rg_infomap_links_count(_p(nbrs), _p(dists), N, k, thr, _p(cnt), _p(rowptr), _stream())
    E = _list_total(rowptr, cnt, N, N * k, "infomap_links")
    src = torch.empty((E,), dtype=torch.int32, device=dev)
    dst = torch.empty((E,), dtype=torch.int32, device=dev)
    w = torch.empty((E,), dtype=torch.float64, device=dev)
    if E == 0:
        return dict(N=N, E=0, rowptr=rowptr, src=src, dst=dst, w=w, single=torch.ones((N,), dtype=torch.int32, device=dev),
                    in_rowptr=torch.zeros((N + 1,), dtype=torch.int32, device=dev), in_src=src.clone(), in_eid=src.clone())
    single = torch.empty((N,), dtype=torch.int32, device=dev)
    incnt = torch.empty((N,), dtype=torch.int32, device=dev)
    in_rowptr = torch.empty((N + 1,), dtype=torch.int32, device=dev)
    lib.rg_infomap_links_fill(_p(nbrs), _p(dists), N, k, thr, _p(rowptr), _p(src), _p(dst), _p(w), _p(single), _p(incnt), _p(in_rowptr),
                              _stream())
    # the transpose: a stable sort of the targets keeps the sources of a node ascending (the out list is in source order)
    _, perm = torch.sort(dst, stable=True)
    in_eid = perm.to(torch.int32)
    return dict(N=N, E=E, rowptr=rowptr, src=src, dst=dst, w=w, single=single, in_rowptr=in_rowptr, in_src=src[perm].contiguous(),
                in_eid=in_eid)


def infomap_flow(graph):
    """Adds the flow of the definition to the graph of infomap_links (which must have a link) and returns it: "p" the
    PageRank vector, "q" fp64 [E] link flow (sum 1), "iq" the same in in-list order, "flow" fp64 [N] node flow (in-flow),
    "flow_iterations", "flow_converged", "link_flow_total" (the sum before normalising; 0 when no node with an out-link has
    an in-link: no flow reaches a link and q is undefined), "scal" (device scalars; [7] = sum_nodes plogp(flow)).  The host loops over batches of
    INFOMAP_FLOW_BATCH iterations and reads the done flag back after each; iterations after the stop change nothing."""
    g = _chk_infomap_graph(graph)
    N, E = g["N"], g["E"]
    if E < 1:
        raise ValueError("rg_hip: infomap_flow: the graph has no link")
    dev = g["w"].device
    f64 = lambda n: torch.empty((n,), dtype=torch.float64, device=dev)          # noqa: E731
    wout, win, p, tele, raw, scal = f64(N), f64(N), f64(N), f64(N), f64(N), torch.zeros((16,), dtype=torch.float64, device=dev)
    lib.rg_infomap_flow_start(_p(g["rowptr"]), _p(g["w"]), _p(g["in_rowptr"]), _p(g["in_eid"]), N, E, _p(wout), _p(win), _p(p), _p(tele),
                              _p(scal), _stream())
    iters, done = 0, False
    for _ in range(-(-INFOMAP_FLOW_MAX_ITERS // INFOMAP_FLOW_BATCH)):
        lib.rg_infomap_flow_iterate(_p(g["rowptr"]), _p(g["in_rowptr"]), _p(g["in_src"]), _p(g["in_eid"]), _p(g["w"]), _p(wout), _p(tele),
                                    N, E, INFOMAP_FLOW_BATCH, INFOMAP_FLOW_MAX_ITERS, _p(p), _p(raw), _p(scal), _stream())
        sh = scal.cpu()
        iters, done = int(sh[5].item()), bool(sh[6].item() != 0.0)
        if done:
            break
    q, iq, flow = f64(E), f64(E), f64(N)
    lib.rg_infomap_flow_finish(_p(g["src"]), _p(g["in_rowptr"]), _p(g["in_eid"]), _p(g["w"]), _p(wout), _p(p), N, E, _p(q), _p(iq),
                               _p(flow), _p(scal), _stream())
    out = dict(g)
    out.update(p=p, q=q, iq=iq, flow=flow, scal=scal, flow_iterations=iters,
               flow_converged=bool(done and float(sh[4].item()) <= 1e-13), link_flow_total=float(scal[8].item()))
    return out


def _infomap_leaf_units(g):
    return dict(U=g["N"], E=g["E"], orp=g["rowptr"], odst=g["dst"], oq=g["q"], irp=g["in_rowptr"], isrc=g["in_src"], iq=g["iq"],
                pu=g["flow"])


def _infomap_totals(ug, mod):
    """(exit, enter, flow fp64 [U], nunits int32 [U]) of the modules mod int32 [U] (values in [0, U)) of a unit graph, every
    module summed over its units in ascending index (segments of a stable sort)"""
    U, dev = ug["U"], mod.device
    _, order, segptr = sorted_segments(mod)
    S, order = segptr.numel() - 1, order.to(torch.int32)
    xo, xi = torch.empty((U,), dtype=torch.float64, device=dev), torch.empty((U,), dtype=torch.float64, device=dev)
    mexit, menter, mflow = (torch.zeros((U,), dtype=torch.float64, device=dev) for _ in range(3))
    nunits = torch.zeros((U,), dtype=torch.int32, device=dev)
    lib.rg_infomap_totals(_p(ug["orp"]), _p(ug["odst"]), _p(ug["oq"]), _p(ug["irp"]), _p(ug["isrc"]), _p(ug["iq"]), _p(ug["pu"]), _p(mod),
                          _p(order), _p(segptr), U, S, _p(xo), _p(xi), _p(mexit), _p(menter), _p(mflow), _p(nunits), _stream())
    return mexit, menter, mflow, nunits


def _infomap_codelength_of(tot, scal, out):
    lib.rg_infomap_codelength(_p(tot[0]), _p(tot[1]), _p(tot[2]), tot[0].numel(), scal.data_ptr() + 7 * 8, _p(out), _stream())


def infomap_codelength(graph, labels):
    """L in bits (a Python float) of the partition `labels` (integer device tensor [N], any values) under the flow of
    infomap_flow; module sums in ascending node index.  Reads one number back."""
    g = _chk_infomap_graph(graph, flow=True)
    if not torch.is_tensor(labels):
        raise TypeError("rg_hip: labels must be a tensor, got %s" % type(labels).__name__)
    if not labels.is_cuda:
        raise RuntimeError("rg_hip: labels must live on the GPU (got %s); the HIP path has no CPU fallback" % (labels.device,))
    if labels.dtype not in (torch.int32, torch.int64) or labels.dim() != 1 or labels.numel() != g["N"]:
        raise ValueError("rg_hip: infomap_codelength: labels must be an int32 / int64 vector of %d entries" % g["N"])
    mod, _ = compact_labels(labels)
    tot = _infomap_totals(_infomap_leaf_units(g), mod)
    out = torch.empty((2,), dtype=torch.float64, device=mod.device)
    _infomap_codelength_of(tot, g["scal"], out)
    return float(out[0].item())


def _infomap_level(ug, mod, scal, stats):
    """local-move sweeps over the units of `ug` from the partition mod (changed in place); True if a unit moved.  Every
    accepted sweep lowers L (recomputed from the module totals); a sweep that does not is rolled back and only its single
    best move applied; if that does not lower L either the level ends."""
    U, dev = ug["U"], mod.device
    if ug["E"] == 0 or U < 2:
        return False
    tot = list(_infomap_totals(ug, mod))
    cl, cl2 = torch.empty((2,), dtype=torch.float64, device=dev), torch.empty((2,), dtype=torch.float64, device=dev)
    _infomap_codelength_of(tot, scal, cl)
    L = float(cl[0].item())
    tgt = torch.empty((U,), dtype=torch.int32, device=dev)
    key, claim = torch.empty((U,), dtype=torch.int64, device=dev), torch.empty((U,), dtype=torch.int64, device=dev)
    best = torch.empty((1,), dtype=torch.int64, device=dev)
    vals = torch.empty((4 * U,), dtype=torch.float64, device=dev)
    nmoved = torch.empty((1,), dtype=torch.int32, device=dev)
    moved_any = False

    def apply(single):
        lib.rg_infomap_apply(_p(tgt), _p(key), _p(vals), _p(claim), _p(best), _p(ug["pu"]), U, single, _p(mod), _p(tot[0]), _p(tot[1]),
                             _p(tot[2]), _p(tot[3]), _p(nmoved), _stream())
        _infomap_codelength_of(tot, scal, cl2)
        return float(cl2[0].item()), int(nmoved.item())

    for _ in range(INFOMAP_SWEEP_CAP):
        stats["sweeps"] += 1
        lib.rg_infomap_propose(_p(ug["orp"]), _p(ug["odst"]), _p(ug["oq"]), _p(ug["irp"]), _p(ug["isrc"]), _p(ug["iq"]), _p(ug["pu"]),
                               _p(mod), _p(tot[0]), _p(tot[1]), _p(tot[2]), _p(tot[3]), U, _p(cl), _p(tgt), _p(key), _p(vals), _p(claim),
                               _p(best), _p(nmoved), _stream())
        backup = [mod.clone()] + [t.clone() for t in tot]
        Ln, n = apply(0)
        if n == 0:
            return moved_any
        if not Ln < L:
            mod.copy_(backup[0])
            for t, b in zip(tot, backup[1:]):
                t.copy_(b)
            stats["rollbacks"] += 1
            Ln, n = apply(1)
            if n == 0 or not Ln < L:
                mod.copy_(backup[0])
                return moved_any
        L, moved_any = Ln, True
        stats["moves"] += n
        cl, cl2 = cl2, cl
    return moved_any                     # the sweep cap: the partition is valid, the caller's next level or round goes on


def _infomap_aggregate(g, leaf_mod):
    """(unit graph of the modules of leaf_mod int32 [N], leaf_mod compacted to [0, M)): link flow between two modules = the
    sum of the leaf links between them in ascending link index (segments of a stable sort of the module pairs), unit flow =
    the module's node flow in ascending node index"""
    N, dev = g["N"], leaf_mod.device
    lm, M = compact_labels(leaf_mod)
    leaf = _infomap_leaf_units(g)
    pu = _infomap_totals(leaf, lm)[2][:M].contiguous()
    ms, md = lm[g["src"].long()].long(), lm[g["dst"].long()].long()
    cross = torch.nonzero(ms != md).flatten()
    ug = dict(U=M, E=int(cross.numel()), pu=pu)
    if ug["E"] == 0:
        return ug, lm
    lists = []
    for a, b in ((ms[cross], md[cross]), (md[cross], ms[cross])):      # out lists by (source, target), in lists by (target, source)
        pairs, perm, segptr = sorted_segments(a * M + b)
        S, eidx = pairs.numel(), cross[perm].to(torch.int32)
        val = torch.empty((S,), dtype=torch.float64, device=dev)
        lib.rg_infomap_segment_sum(_p(g["q"]), g["E"], _p(eidx), _p(segptr), S, eidx.numel(), _p(val), _stream())
        row = torch.div(pairs, M, rounding_mode="floor")
        rp = torch.searchsorted(row, torch.arange(M + 1, dtype=torch.int64, device=dev)).to(torch.int32)
        lists.append((rp, (pairs - row * M).to(torch.int32), val))
    ug.update(orp=lists[0][0], odst=lists[0][1], oq=lists[0][2], irp=lists[1][0], isrc=lists[1][1], iq=lists[1][2])
    return ug, lm


def infomap_search(graph):
    """(modules int32 [N] compact in [0, n_modules), info) — the deterministic two-level search on the flow of infomap_flow,
    driven from here: leaf sweeps from singletons, then modules become units and are swept until nothing merges, then a leaf
    fine-tune from the found partition; coarse and fine rounds repeat until the fine-tune moves nothing.  Caps:
    INFOMAP_SWEEP_CAP sweeps per level, INFOMAP_LEVEL_CAP aggregations per coarse phase, INFOMAP_ROUND_CAP rounds.  A level that
    reaches its cap hands its (valid) partition on; converged = a fine-tune moved nothing before the round cap.  Nodes in no link stay modules of their own."""
    g = _chk_infomap_graph(graph, flow=True)
    N, dev = g["N"], g["w"].device
    stats = dict(sweeps=0, levels=0, rounds=0, moves=0, rollbacks=0)
    leaf = _infomap_leaf_units(g)
    leaf_mod = torch.arange(N, dtype=torch.int32, device=dev)
    converged = False
    for rnd in range(INFOMAP_ROUND_CAP):
        stats["rounds"] += 1
        settled = False
        for lvl in range(INFOMAP_LEVEL_CAP):
            if rnd == 0 and lvl == 0:
                ug, mod = leaf, leaf_mod.clone()
            else:
                ug, leaf_mod = _infomap_aggregate(g, leaf_mod)
                mod = torch.arange(ug["U"], dtype=torch.int32, device=dev)
            stats["levels"] += 1
            if not _infomap_level(ug, mod, g["scal"], stats):
                settled = True
                break
            leaf_mod = mod[leaf_mod.long()].contiguous()
        leaf_mod, _ = compact_labels(leaf_mod)
        stats["levels"] += 1
        if not _infomap_level(leaf, leaf_mod, g["scal"], stats) and settled:      # the last coarse level moved nothing either
            converged = True
            break
    leaf_mod, stats["n_modules"] = compact_labels(leaf_mod)
    stats["converged"] = converged
    return leaf_mod, stats


def infomap_labels(modules, cluster_num):
    """(labels int64 [N], n_clusters): modules int32 [N] (values in [0, N)) with more than cluster_num members numbered
    0 .. C-1 in ascending order of their smallest member, -1 for the rest.  Reads one integer back (C)."""
    modules = _chk_rr(modules, "modules", torch.int32, 1)
    N, cluster_num = modules.numel(), int(cluster_num)
    if not 1 <= N <= INFOMAP_MAX_N or cluster_num < 0:
        raise ValueError("rg_hip: infomap_labels needs 1 <= N <= %d and cluster_num >= 0, got N=%d cluster_num=%d"
                         % (INFOMAP_MAX_N, N, cluster_num))
    dev = modules.device
    size, minm, head = (torch.empty((N,), dtype=torch.int32, device=dev) for _ in range(3))
    num = torch.empty((N + 1,), dtype=torch.int32, device=dev)
    labels = torch.empty((N,), dtype=torch.int64, device=dev)
    lib.rg_infomap_labels(_p(modules), N, cluster_num, _p(size), _p(minm), _p(head), _p(num), _p(labels), _stream())
    return labels, int(num[N].item())


def infomap(nbrs, dists, min_sim, cluster_num=2):
    """(labels int64 [N] on the device, info) of the two-level Infomap clustering of a kNN table: links, flow,
    search, labels.  info (the same keys on every path): codelength, codelength_one_module, n_modules, n_singles, levels,
    sweeps, flow_iterations, converged, rollbacks, moves, rounds, n_clusters, modules (int32 device tensor).  0 < min_sim <= 1.  A table without a link, and N <= 2, return without a search (two nodes that link each other form
    one module: L = 1 bit against 3 bits apart; a one-way pair ties at 0 bits and stays apart)."""
    nbrs, dists = _chk_infomap_table(nbrs, dists)
    if int(cluster_num) < 0:
        raise ValueError("rg_hip: infomap needs cluster_num >= 0, got %r" % (cluster_num,))
    N, dev = nbrs.shape[0], nbrs.device
    g = infomap_links(nbrs, dists, min_sim)
    info = dict(codelength=0.0, codelength_one_module=0.0, n_modules=N, n_singles=N, levels=0, sweeps=0, flow_iterations=0,
                converged=True, rollbacks=0, moves=0, rounds=0)          # the same keys whichever path is taken
    modules = torch.arange(N, dtype=torch.int32, device=dev)
    if g["E"] == 0:
        pass
    elif N == 2:
        info.update(n_singles=2 - g["E"])
        if g["E"] == 2:
            modules.zero_()
            info.update(codelength=1.0, codelength_one_module=1.0, n_modules=1)
    else:
        g = infomap_flow(g)
        info.update(n_singles=int(g["single"].sum().item()), flow_iterations=g["flow_iterations"])
        if g["link_flow_total"] > 0.0:       # otherwise no flow reaches a link: nothing to search, every node stays alone
            modules, stats = infomap_search(g)
            info.update(codelength=infomap_codelength(g, modules), codelength_one_module=infomap_codelength(g, torch.zeros_like(modules)),
                        n_modules=stats["n_modules"], levels=stats["levels"], sweeps=stats["sweeps"],
                        converged=bool(stats["converged"] and g["flow_converged"]), rollbacks=stats["rollbacks"],
                        moves=stats["moves"], rounds=stats["rounds"])
    labels, n_clusters = infomap_labels(modules, cluster_num)
    info["n_clusters"] = n_clusters
    info["modules"] = modules
    return labels, info
