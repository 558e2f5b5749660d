"""Cluster memory, kNN and row helpers of the pseudo-labelling code, k-reciprocal re-ranking, CMC / mAP scoring, the second stage
of the cascade evaluation: csrc/cm.hip, csrc/retrieval.hip, csrc/rerank.hip, csrc/rank_eval.hip, csrc/cmc_shot.hip, csrc/cascade.hip."""
from __future__ import absolute_import

import numpy as np
import torch

from ._base import _chk, _chk_rr, _list_total, _p, _stream, lib


# ------------------------------------------------------------------------------------------------
# cluster memory
# ------------------------------------------------------------------------------------------------
def cm_update(inputs, targets, features, momentum, hard=False, normalize_eps=False):
    inputs = _chk(inputs, "inputs")
    targets = _chk(targets, "targets", torch.int64)
    if not (features.is_cuda and features.is_contiguous() and features.dtype == torch.float32):
        raise RuntimeError("cm_update: the memory bank must be a contiguous fp32 GPU tensor (updated in place)")
    B, D = inputs.shape
    K = features.shape[0]
    if hard:
        lib.rg_cm_update_hard(_p(inputs), _p(targets), _p(features), B, D, K, float(momentum), _stream())
    else:
        lib.rg_cm_update(_p(inputs), _p(targets), _p(features), B, D, K, float(momentum), int(normalize_eps), _stream())
    return features


# ------------------------------------------------------------------------------------------------
# row helpers of the pseudo-labelling front half: kNN, distances, cluster centres (csrc/cm.hip, csrc/retrieval.hip)
# ------------------------------------------------------------------------------------------------
def normalize_listed_rows(g, ids, eps=1e-16):
    """in place: g[id] /= |g[id]| + eps for the listed (int64, device) row ids"""
    g = _chk(g, "g")
    ids = _chk(ids, "ids", torch.int64)
    lib.rg_normalize_listed_rows(_p(g), _p(ids), ids.numel(), g.shape[0], g.shape[1], eps, _stream())
    return g


def topk_rows(s, k):
    """(idx int32 [rows, k], val [rows, k]) of the k largest entries per row, ties by lower index"""
    s = _chk(s, "s")
    rows, cols = s.shape
    idx = torch.empty((rows, k), dtype=torch.int32, device=s.device)
    val = torch.empty((rows, k), dtype=torch.float32, device=s.device)
    lib.rg_topk_rows(_p(s), rows, cols, k, _p(idx), _p(val), _stream())
    return idx, val


def row_sqsum(x):
    x = _chk(x, "x")
    out = torch.empty(x.shape[0], dtype=torch.float32, device=x.device)
    lib.rg_row_sqsum(_p(x), _p(out), x.shape[0], x.shape[1], _stream())
    return out


def add_outer_terms(m, rowv=None, colv=None, alpha=1.0, a=1.0, b=1.0):
    m = _chk(m, "m")
    lib.rg_add_outer_terms(_p(m), _p(rowv), _p(colv), alpha, a, b, m.shape[0], m.shape[1], _stream())
    return m


def segment_mean(x, order, offsets):
    x = _chk(x, "x")
    order, offsets = _chk(order, "order", torch.int64), _chk(offsets, "offsets", torch.int64)
    out = torch.empty((offsets.numel() - 1, x.shape[1]), dtype=torch.float32, device=x.device)
    lib.rg_segment_mean(_p(x), _p(order), _p(offsets), _p(out), offsets.numel() - 1, x.shape[1], _stream())
    return out


def sorted_segments(keys, ptr_dtype=torch.int32):
    """(uniq, perm, ptr) of a stable sort of the 1-D `keys`: the distinct keys ascending, the sorting permutation (int64: equal
    keys keep their order, so a segment lists its members in ascending position) and ptr [S + 1] in ptr_dtype, the exclusive
    prefix sum of the segment sizes: segment s is perm[ptr[s]:ptr[s + 1]].  Pure torch, on the device of `keys`."""
    skeys, perm = torch.sort(keys, stable=True)
    uniq, counts = torch.unique_consecutive(skeys, return_counts=True)
    ptr = torch.zeros((uniq.numel() + 1,), dtype=ptr_dtype, device=keys.device)
    ptr[1:] = torch.cumsum(counts, dim=0)
    return uniq, perm, ptr


def compact_labels(t):
    """(inverse int32 contiguous, count): every entry of `t` replaced by the rank of its value among the `count` distinct ones"""
    uniq, inv = torch.unique(t, return_inverse=True)
    return inv.to(torch.int32).contiguous(), uniq.numel()


# ------------------------------------------------------------------------------------------------
# k-reciprocal re-ranking (csrc/rerank.hip): sparse encodings as row lists, see include/reidgan_hip.h
# ------------------------------------------------------------------------------------------------
def rerank_expand(rank, kf, kh, cap=None):
    """(sets int32 [N, cap], counts int32 [N]): expanded k-reciprocal set of every row of the ranking `rank` int32 [N, R]
    (kf / kh = columns read for the full / the half sets).  The default cap is the worst case kf * (kh + 1), capped at N."""
    rank = _chk_rr(rank, "rank", torch.int32, 2)
    N, R = rank.shape
    kf, kh = int(kf), int(kh)
    if not (1 <= kh <= kf <= R):
        raise ValueError("rg_hip: rerank_expand needs 1 <= kh <= kf <= rank.shape[1], got kf=%d kh=%d R=%d" % (kf, kh, R))
    cap = min(N, kf * (kh + 1)) if cap is None else int(cap)
    sets = torch.empty((N, cap), dtype=torch.int32, device=rank.device)
    counts = torch.empty((N,), dtype=torch.int32, device=rank.device)
    lib.rg_rerank_expand(_p(rank), N, R, kf, kh, _p(sets), _p(counts), cap, _stream())
    return sets, counts


def rerank_weights(sets, counts, x=None, orig=None):
    """w [N, cap]: softmax of -(2 - 2 x_i . x_e) over each row's set (x [N, D]), or exp(-orig[i, e]) / sum (orig [N, N])"""
    sets, counts = _chk_rr(sets, "sets", torch.int32, 2), _chk_rr(counts, "counts", torch.int32, 1)
    if (x is None) == (orig is None):
        raise ValueError("rg_hip: rerank_weights takes exactly one of x and orig")
    N, cap = sets.shape
    w = torch.empty((N, cap), dtype=torch.float32, device=sets.device)      # entries beyond counts[i] are never read
    if x is not None:
        x = _chk_rr(x, "x", torch.float32, 2)
        if x.data_ptr() & 15:            # the kernel reads the gathered rows as 16-byte vectors
            x = x.clone()
        if x.shape[0] != N or counts.numel() != N:
            raise ValueError("rg_hip: rerank_weights: x %s, sets %s, counts %s disagree" % (tuple(x.shape), tuple(sets.shape), tuple(counts.shape)))
        lib.rg_rerank_weights_feat(_p(x), N, x.shape[1], _p(sets), _p(counts), cap, _p(w), _stream())
    else:
        orig = _chk_rr(orig, "orig", torch.float32, 2)
        if tuple(orig.shape) != (N, N) or counts.numel() != N:
            raise ValueError("rg_hip: rerank_weights: orig %s must be [%d, %d]" % (tuple(orig.shape), N, N))
        lib.rg_rerank_weights_dist(_p(orig), N, _p(sets), _p(counts), cap, _p(w), _stream())
    return w


def rerank_query_expand(sets, w, counts, rank=None, k2=1):
    """CSR (rowptr int32 [N + 1], cols int32 [nnz], vals [nnz]) of the encodings after the local query expansion: row i = mean of
    the rows rank[i, :k2]; rank None (k2 == 1) keeps every row.  Reads one integer back (nnz) to size the arrays."""
    sets, counts, w = _chk_rr(sets, "sets", torch.int32, 2), _chk_rr(counts, "counts", torch.int32, 1), _chk_rr(w, "w", torch.float32, 2)
    N, cap = sets.shape
    if tuple(w.shape) != (N, cap) or counts.numel() != N:
        raise ValueError("rg_hip: rerank_query_expand: sets %s, w %s, counts %s disagree" % (tuple(sets.shape), tuple(w.shape), tuple(counts.shape)))
    k2, R = int(k2), 0
    if rank is not None:
        rank = _chk_rr(rank, "rank", torch.int32, 2)
        R = rank.shape[1]
        if rank.shape[0] != N or not (1 <= k2 <= min(R, 64)):
            raise ValueError("rg_hip: rerank_query_expand needs rank [N, R] and 1 <= k2 <= min(R, 64), got %s, k2=%d" % (tuple(rank.shape), k2))
    elif k2 != 1:
        raise ValueError("rg_hip: rerank_query_expand without a ranking is the identity (k2 == 1), got k2=%d" % k2)
    rowcnt = torch.empty((N,), dtype=torch.int32, device=sets.device)
    rowptr = torch.empty((N + 1,), dtype=torch.int32, device=sets.device)
    lib.rg_rerank_qe_count(_p(rank), R, k2, N, _p(sets), _p(counts), cap, _p(rowcnt), _p(rowptr), _stream())
    nnz = _list_total(rowptr, rowcnt, N, N * min(N, k2 * cap), "rerank_query_expand")
    if nnz == 0:
        raise RuntimeError("rg_hip: rerank_query_expand: every expanded set is empty")
    cols = torch.empty((nnz,), dtype=torch.int32, device=sets.device)
    vals = torch.empty((nnz,), dtype=torch.float32, device=sets.device)
    lib.rg_rerank_qe_fill(_p(rank), R, k2, N, _p(sets), _p(w), _p(counts), cap, _p(rowptr), _p(cols), _p(vals), _stream())
    return rowptr, cols, vals


def rerank_columns(rowptr, cols, vals):
    """column lists (colptr int32 [N + 1], crow int32 [nnz], cval [nnz]) of a CSR matrix; order inside a column unspecified"""
    rowptr, cols, vals = _chk_rr(rowptr, "rowptr", torch.int32, 1), _chk_rr(cols, "cols", torch.int32, 1), _chk_rr(vals, "vals", torch.float32, 1)
    N, nnz = rowptr.numel() - 1, cols.numel()
    if N < 1 or vals.numel() != nnz:
        raise ValueError("rg_hip: rerank_columns: rowptr %s, cols %s, vals %s disagree" % (tuple(rowptr.shape), tuple(cols.shape), tuple(vals.shape)))
    colptr = torch.empty((N + 1,), dtype=torch.int32, device=cols.device)
    cursor = torch.empty((N,), dtype=torch.int32, device=cols.device)
    crow, cval = torch.empty_like(cols), torch.empty_like(vals)
    lib.rg_rerank_columns(_p(rowptr), _p(cols), _p(vals), N, nnz, _p(colptr), _p(cursor), _p(crow), _p(cval), _stream())
    return colptr, crow, cval


def rerank_jaccard(csr, csc, rows=None, col_off=0, orig=None, lambda_value=0.0, clamp=True, chunk=0):
    """[rows, N - col_off] Jaccard distances of the sparse encodings (csr / csc as returned above); with `orig` [N, N]:
    (1 - lambda) * jaccard + lambda * orig.  chunk = columns accumulated per workgroup, 0 = automatic; same bits either way."""
    rowptr, cols, vals = csr
    colptr, crow, cval = csc
    rowptr, colptr = _chk_rr(rowptr, "rowptr", torch.int32, 1), _chk_rr(colptr, "colptr", torch.int32, 1)
    cols, crow = _chk_rr(cols, "cols", torch.int32, 1), _chk_rr(crow, "crow", torch.int32, 1)
    vals, cval = _chk_rr(vals, "vals", torch.float32, 1), _chk_rr(cval, "cval", torch.float32, 1)
    N = rowptr.numel() - 1
    rows = N if rows is None else int(rows)
    col_off, chunk = int(col_off), int(chunk)
    if colptr.numel() != N + 1 or not (cols.numel() == vals.numel() == crow.numel() == cval.numel()):
        raise ValueError("rg_hip: rerank_jaccard: row and column lists disagree")
    if not (1 <= rows <= N and 0 <= col_off < N) or chunk < 0:
        raise ValueError("rg_hip: rerank_jaccard: rows=%d col_off=%d chunk=%d outside N=%d" % (rows, col_off, chunk, N))
    if orig is not None:
        orig = _chk_rr(orig, "orig", torch.float32, 2)
        if orig.shape[1] != N or orig.shape[0] < rows:
            raise ValueError("rg_hip: rerank_jaccard: orig %s must be [>= %d, %d]" % (tuple(orig.shape), rows, N))
    out = torch.empty((rows, N - col_off), dtype=torch.float32, device=cols.device)
    lib.rg_rerank_jaccard(_p(rowptr), _p(cols), _p(vals), _p(colptr), _p(crow), _p(cval), N, rows, col_off, _p(orig),
                          float(lambda_value), int(bool(clamp)), _p(out), chunk, _stream())
    return out


def rerank_orig_dist(q_g, q_q, g_g):
    """transpose(A^2 / max(A^2, axis 0)) [Q + G, Q + G] of A = [[q_q, q_g], [q_g^T, g_g]] (re_ranking's normalised matrix)"""
    q_g, q_q, g_g = _chk_rr(q_g, "q_g_dist", torch.float32, 2), _chk_rr(q_q, "q_q_dist", torch.float32, 2), _chk_rr(g_g, "g_g_dist", torch.float32, 2)
    Q, G = q_g.shape
    if tuple(q_q.shape) != (Q, Q) or tuple(g_g.shape) != (G, G):
        raise ValueError("rg_hip: rerank_orig_dist: q_g %s needs q_q [%d, %d] and g_g [%d, %d], got %s and %s"
                         % (tuple(q_g.shape), Q, Q, G, G, tuple(q_q.shape), tuple(g_g.shape)))
    colmax = torch.empty((Q + G,), dtype=torch.float32, device=q_g.device)
    orig = torch.empty((Q + G, Q + G), dtype=torch.float32, device=q_g.device)
    lib.rg_rerank_orig_dist(_p(q_g), _p(q_q), _p(g_g), Q, G, _p(colmax), _p(orig), _stream())
    return orig


def rerank_from_rank(rank, kf, kh, k2, x=None, orig=None, rows=None, col_off=0, lambda_value=0.0, clamp=True, chunk=0, debug=False):
    """Stages 2-6 of the re-ranking on an initial ranking `rank` int32 [N, R]: expanded k-reciprocal sets, their weights (from
    the features x or the normalised distances orig), local query expansion over rank[:, :k2], column lists, Jaccard rows.
    debug=True also returns {"rank", "sets", "counts", "w", "rowptr", "cols", "vals"} (device tensors)."""
    sets, counts = rerank_expand(rank, kf, kh)
    w = rerank_weights(sets, counts, x=x) if orig is None else rerank_weights(sets, counts, orig=orig)
    csr = rerank_query_expand(sets, w, counts, rank=rank if k2 != 1 else None, k2=k2)
    csc = rerank_columns(*csr)
    out = rerank_jaccard(csr, csc, rows=rows, col_off=col_off, orig=orig, lambda_value=lambda_value, clamp=clamp, chunk=chunk)
    if debug:
        return out, dict(rank=rank, sets=sets, counts=counts, w=w, rowptr=csr[0], cols=csr[1], vals=csr[2])
    return out


# ------------------------------------------------------------------------------------------------
# CMC / mAP scoring of a query x gallery distance matrix (csrc/rank_eval.hip)
# ------------------------------------------------------------------------------------------------
def rank_eval(dist, query_ids, gallery_ids, query_cams, gallery_cams, topk=100, separate_camera_set=False, chunk=0, debug=False):
    """Scores the ranking every row of dist [Q, G] (fp32 or fp64, on the device) defines, without sorting it:
    {"status", "num_valid", "ap_sum", "first_hist" int64 [topk], "allshots" fp64 [topk]} — the number of queries with a
    positive, the sum of their average precisions, the histogram of the first-match rank and sum_i hits[i, k] / npos[i]
    (cumsum / num_valid of the last two are the reference's `market1501` and `allshots` CMC curves, ap_sum / num_valid its
    mAP).  ids / cams are int32 device vectors.  Two small tensors (topk + 2 and topk + 1 numbers) are read back.  A NaN in
    the matrix raises ValueError.  chunk = positives per pass held in LDS (0 = automatic), same bits for any value.
    debug=True adds the per-query device tensors "npos", "ap", "first", "hits"."""
    if not torch.is_tensor(dist) or dist.dtype not in (torch.float32, torch.float64):
        raise TypeError("rg_hip: rank_eval: dist must be an fp32 or fp64 tensor, got %s"
                        % (dist.dtype if torch.is_tensor(dist) else type(dist).__name__))
    dist = _chk_rr(dist, "dist", dist.dtype, 2)
    Q, G = dist.shape
    topk, chunk = int(topk), int(chunk)
    if Q < 1 or G < 1:
        raise ValueError("rg_hip: rank_eval: dist must be a non-empty [Q, G] matrix, got shape %s" % (tuple(dist.shape),))
    if topk < 1 or Q * topk >= 2 ** 31:
        raise ValueError("rg_hip: rank_eval needs topk >= 1 and Q * topk < 2^31, got Q=%d topk=%d" % (Q, topk))
    if not 0 <= chunk <= 1024:
        raise ValueError("rg_hip: rank_eval: chunk must be 0 (automatic) or 1 .. 1024, got %d" % chunk)
    vecs = []
    for t, name, n in ((query_ids, "query_ids", Q), (gallery_ids, "gallery_ids", G), (query_cams, "query_cams", Q),
                       (gallery_cams, "gallery_cams", G)):
        t = _chk_rr(t, name, torch.int32, 1)
        if t.numel() != n:
            raise ValueError("rg_hip: rank_eval: %s has %d entries, dist %s needs %d" % (name, t.numel(), tuple(dist.shape), n))
        vecs.append(t)
    dev = dist.device
    npos = torch.empty((Q,), dtype=torch.int32, device=dev)
    ap = torch.empty((Q,), dtype=torch.float64, device=dev)
    first = torch.empty((Q,), dtype=torch.int32, device=dev)
    hits = torch.empty((Q, topk), dtype=torch.int32, device=dev)
    counts = torch.empty((topk + 2,), dtype=torch.int32, device=dev)
    sums = torch.empty((topk + 1,), dtype=torch.float64, device=dev)
    lib.rg_rank_eval(_p(dist), int(dist.dtype == torch.float64), Q, G, G, _p(vecs[0]), _p(vecs[1]), _p(vecs[2]), _p(vecs[3]),
                     int(bool(separate_camera_set)), topk, chunk, _p(npos), _p(ap), _p(first), _p(hits), _p(counts), _p(sums), _stream())
    counts_h, sums_h = counts.cpu().numpy(), sums.cpu().numpy()
    if counts_h[0] != 0:
        raise ValueError("rg_hip: rank_eval: the distance matrix holds a NaN")
    res = dict(status=int(counts_h[0]), num_valid=int(counts_h[1]), ap_sum=float(sums_h[0]),
               first_hist=counts_h[2:].astype("int64"), allshots=sums_h[1:].copy())
    if debug:
        res.update(npos=npos, ap=ap, first=first, hits=hits)
    return res


# ------------------------------------------------------------------------------------------------
# single-gallery-shot CMC, the reference's `cuhk03` protocol (csrc/cmc_shot.hip): order pass, host draws, rank pass
# ------------------------------------------------------------------------------------------------
CMC_SHOT_MAX_IDS, CMC_SHOT_MAX_REPEAT, CMC_SHOT_DRAW_BYTES = 4096, 64, 32 << 20
CMC_SHOT_GLOBAL, CMC_SHOT_LDS_ROW = 0, 1      # values of cmc_shot_regime


def cmc_shot_regime(G, nid, is_double):
    """where the rank pass gathers a row's entries from at this shape: CMC_SHOT_LDS_ROW (the row staged in LDS with 16-byte loads)
    or CMC_SHOT_GLOBAL; -1 outside the limits"""
    return int(lib.rg_cmc_shot_regime(int(G), int(nid), int(bool(is_double))))


def _cmc_shot_dist(dist, who):
    if not torch.is_tensor(dist) or dist.dtype not in (torch.float32, torch.float64):
        raise TypeError("rg_hip: %s: dist must be an fp32 or fp64 tensor, got %s"
                        % (who, dist.dtype if torch.is_tensor(dist) else type(dist).__name__))
    dist = _chk_rr(dist, "dist", dist.dtype, 2)
    if dist.shape[0] < 1 or dist.shape[1] < 1:
        raise ValueError("rg_hip: %s: dist must be a non-empty [Q, G] matrix, got shape %s" % (who, tuple(dist.shape)))
    return dist


def cmc_shot_order(dist, query_ids, gallery_ids, query_cams, gallery_cams, separate_camera_set=False):
    """Order pass of the single-gallery-shot CMC on dist [Q, G] (fp32 or fp64, on the device; ids / cams int32 device vectors as
    for rank_eval).  Groups the gallery by identity on the host (O(G); the two id vectors are read back for it), then per query:
    n = identities with a valid entry (0: no valid match, the query is skipped), slot[q, :n] = their indices in the order the
    reference draws for them (first appearance in the row's stable (d, j) order), high[q, :n] = their valid counts.
    Returns the plan the rank pass takes: {"dist", "Q", "G", "nid", "separate", "seg_ptr", "seg_perm", "gallery_cams", "query_seg",
    "query_cams", "n", "slot", "high" (device), "n_host" [Q], "high_host" [Q, nid] (numpy int32)}.  More than 4096 identities
    raise ValueError before anything is enqueued; a NaN in the matrix raises ValueError."""
    dist = _cmc_shot_dist(dist, "cmc_shot_order")
    Q, G = dist.shape
    vecs = []
    for t, name, n in ((query_ids, "query_ids", Q), (gallery_ids, "gallery_ids", G), (query_cams, "query_cams", Q),
                       (gallery_cams, "gallery_cams", G)):
        t = _chk_rr(t, name, torch.int32, 1)
        if t.numel() != n:
            raise ValueError("rg_hip: cmc_shot_order: %s has %d entries, dist %s needs %d" % (name, t.numel(), tuple(dist.shape), n))
        vecs.append(t)
    qid, gid = vecs[0].cpu().numpy(), vecs[1].cpu().numpy()
    uniq, counts = np.unique(gid, return_counts=True)
    nid = int(uniq.size)
    if nid > CMC_SHOT_MAX_IDS:
        raise ValueError("rg_hip: cmc_shot_order: at most %d gallery identities (their keys are sorted in LDS), got %d"
                         % (CMC_SHOT_MAX_IDS, nid))
    if Q * nid >= 2 ** 31:
        raise ValueError("rg_hip: cmc_shot_order needs Q * nid < 2^31, got Q=%d nid=%d" % (Q, nid))
    seg_ptr = np.zeros(nid + 1, dtype=np.int32)
    seg_ptr[1:] = np.cumsum(counts)
    seg_perm = np.argsort(gid, kind="stable").astype(np.int32)          # ids ascending, the entries of one in ascending j
    pos = np.minimum(np.searchsorted(uniq, qid), nid - 1)
    qseg = np.where(uniq[pos] == qid, pos, -1).astype(np.int32)
    dev = dist.device
    seg_ptr_d, seg_perm_d, qseg_d = (torch.from_numpy(a).to(dev) for a in (seg_ptr, seg_perm, qseg))
    n = torch.empty((Q,), dtype=torch.int32, device=dev)
    slot = torch.empty((Q, nid), dtype=torch.int32, device=dev)
    high = torch.empty((Q, nid), dtype=torch.int32, device=dev)
    status = torch.empty((1,), dtype=torch.int32, device=dev)
    sep = int(bool(separate_camera_set))
    lib.rg_cmc_shot_order(_p(dist), int(dist.dtype == torch.float64), Q, G, G, nid, _p(seg_ptr_d), _p(seg_perm_d), _p(vecs[3]),
                          _p(qseg_d), _p(vecs[2]), sep, _p(n), _p(slot), _p(high), _p(status), _stream())
    st = int(status.cpu().numpy()[0])
    if st & 1:
        raise ValueError("rg_hip: cmc_shot_order: the distance matrix holds a NaN")
    if st:
        raise RuntimeError("rg_hip: cmc_shot_order: broken segment list (status %d)" % st)
    return dict(dist=dist, Q=Q, G=G, nid=nid, separate=sep, seg_ptr=seg_ptr_d, seg_perm=seg_perm_d, gallery_cams=vecs[3],
                query_seg=qseg_d, query_cams=vecs[2], n=n, slot=slot, high=high, n_host=n.cpu().numpy(),
                high_host=high.cpu().numpy())


def cmc_shot_rank(plan, draws, q0, q1, repeat, topk, rank, hist):
    """Rank pass for the queries [q0, q1) of a cmc_shot_order plan.  draws: host int32 vector, for the valid queries of the range
    in query order the [repeat, n[q]] block of draws u[r, p] in [0, high[q, p]).  Writes rank[q0:q1] (int32 [Q, repeat] on the
    device: the rank of the own identity among the sampled entries, -1 for a skipped query) and adds the ranks below topk into
    hist (int32 [topk] on the device, zeroed by the caller)."""
    Q, nid, repeat, topk, q0, q1 = plan["Q"], plan["nid"], int(repeat), int(topk), int(q0), int(q1)
    dist = plan["dist"]
    if not 0 <= q0 < q1 <= Q:
        raise ValueError("rg_hip: cmc_shot_rank: queries [%d, %d) outside the %d rows" % (q0, q1, Q))
    if not 1 <= repeat <= CMC_SHOT_MAX_REPEAT or topk < 1 or Q * repeat >= 2 ** 31:
        raise ValueError("rg_hip: cmc_shot_rank needs 1 <= repeat <= %d, topk >= 1 and Q * repeat < 2^31, got repeat=%d topk=%d Q=%d"
                         % (CMC_SHOT_MAX_REPEAT, repeat, topk, Q))
    rank, hist = _chk_rr(rank, "rank", torch.int32, 2), _chk_rr(hist, "hist", torch.int32, 1)
    if tuple(rank.shape) != (Q, repeat) or hist.numel() != topk:
        raise ValueError("rg_hip: cmc_shot_rank: rank %s must be [%d, %d] and hist %s [%d]"
                         % (tuple(rank.shape), Q, repeat, tuple(hist.shape), topk))
    draws = np.ascontiguousarray(draws)
    off = np.zeros(q1 - q0 + 1, dtype=np.int64)
    np.cumsum(plan["n_host"][q0:q1].astype(np.int64) * repeat, out=off[1:])
    if draws.dtype != np.int32 or draws.ndim != 1 or draws.size != off[-1]:
        raise ValueError("rg_hip: cmc_shot_rank: draws must be an int32 vector of %d entries, got %s %s"
                         % (off[-1], draws.dtype, draws.shape))
    dev = dist.device
    draws_d = torch.from_numpy(draws if draws.size else np.zeros(1, dtype=np.int32)).to(dev)
    off_d = torch.from_numpy(off[:-1].copy()).to(dev)
    lib.rg_cmc_shot_rank(_p(dist), int(dist.dtype == torch.float64), Q, q0, q1 - q0, plan["G"], plan["G"], nid, _p(plan["seg_ptr"]),
                         _p(plan["seg_perm"]), _p(plan["gallery_cams"]), _p(plan["query_seg"]), _p(plan["query_cams"]),
                         plan["separate"], _p(plan["n"]), _p(plan["slot"]), _p(draws_d), _p(off_d), repeat, topk, _p(rank), _p(hist),
                         _stream())
    return rank


def cmc_shot(dist, query_ids, gallery_ids, query_cams, gallery_cams, topk=100, separate_camera_set=False, repeat=10,
             random_state=None, chunk=0, debug=False):
    """The whole single-gallery-shot scoring: order pass, host draws, rank pass.  {"hist" int64 [topk] (host): the (query, repeat)
    pairs whose sampled rank is the bin, "num_valid": the queries with a valid match}; debug=True adds the device tensors "n",
    "slot", "high", "rank".  The draws are ONE stream of `random_state.randint(0, highs)` over, for the valid queries in query
    order, np.tile(high[q, :n[q]], repeat) — what the reference's np.random.choice loop consumes, so the generator is left where
    the reference leaves it; random_state None is numpy's global generator.  chunk = queries per rank launch (0: as many as keep
    one launch's draws at or below 32 MB); the stream, the bits and the generator state do not depend on it.  Every check,
    the NaN check included, comes before the first draw."""
    topk, repeat, chunk = int(topk), int(repeat), int(chunk)
    if not 1 <= repeat <= CMC_SHOT_MAX_REPEAT:
        raise ValueError("rg_hip: cmc_shot: repeat must be 1 .. %d, got %d" % (CMC_SHOT_MAX_REPEAT, repeat))
    if topk < 1:
        raise ValueError("rg_hip: cmc_shot: topk must be at least 1, got %d" % topk)
    if chunk < 0:
        raise ValueError("rg_hip: cmc_shot: chunk must be 0 (automatic) or a number of queries, got %d" % chunk)
    rs = np.random if random_state is None else random_state
    if not callable(getattr(rs, "randint", None)):
        raise TypeError("rg_hip: cmc_shot: random_state must be None or a numpy.random.RandomState, got %s" % type(random_state).__name__)
    plan = cmc_shot_order(dist, query_ids, gallery_ids, query_cams, gallery_cams, separate_camera_set)
    Q, dev = plan["Q"], plan["dist"].device
    if Q * repeat >= 2 ** 31:
        raise ValueError("rg_hip: cmc_shot needs Q * repeat < 2^31, got Q=%d repeat=%d" % (Q, repeat))
    n_h, high_h = plan["n_host"], plan["high_host"]
    rank = torch.empty((Q, repeat), dtype=torch.int32, device=dev)
    hist = torch.zeros((topk,), dtype=torch.int32, device=dev)
    per_query = n_h.astype(np.int64) * repeat * 4
    q0 = 0
    while q0 < Q:
        if chunk:
            q1 = min(Q, q0 + chunk)
        else:
            q1 = q0 + max(1, int(np.searchsorted(np.cumsum(per_query[q0:]), CMC_SHOT_DRAW_BYTES, side="right")))
        highs = [np.tile(high_h[q, :n_h[q]], repeat) for q in range(q0, q1) if n_h[q] > 0]
        if highs:
            draws = rs.randint(0, np.concatenate(highs)).astype(np.int32)
        else:
            draws = np.zeros(0, dtype=np.int32)
        cmc_shot_rank(plan, draws, q0, q1, repeat, topk, rank, hist)
        q0 = q1
    res = dict(hist=hist.cpu().numpy().astype(np.int64), num_valid=int((n_h > 0).sum()))
    if debug:
        res.update(n=plan["n"], slot=plan["slot"], high=plan["high"], rank=rank)
    return res


# ------------------------------------------------------------------------------------------------
# second stage of the cascade evaluation (csrc/cascade.hip): the verification head on gathered pairs, the merge of the two stages
# ------------------------------------------------------------------------------------------------
PAIR_SCORE_MAX_C, PAIR_SCORE_MAX_D, PAIR_SCORE_MAX_Q, CASCADE_MERGE_MAX_G = 16, 8192, 32768, 1 << 20
PAIR_VEC4, PAIR_SPLIT_K = 1, 2        # bits of pair_score_regime


def pair_score_regime(Q, k, D, C, aligned=True):
    """the launch regime `pair_score` takes at this shape, bits PAIR_VEC4 (16-byte loads, else 4-byte: D no multiple of 4) and
    PAIR_SPLIT_K (k split over several workgroups per query: Q below the CU count).  `aligned` is always true for tensors that went through the wrapper."""
    return int(lib.rg_pair_score_regime(int(Q), int(k), int(D), int(C), int(bool(aligned))))


def _pair_vec(t, name, n):
    t = _chk_rr(t, name, torch.float32, 1)
    if t.numel() != n:
        raise ValueError("rg_hip: pair_score %s must have %d elements, got %d" % (name, n, t.numel()))
    return t.clone() if t.data_ptr() & 15 else t


def pair_score(probe, gallery, idx, gamma, beta, running_mean, running_var, weight, bias, eps, want_logits=False, want_score=True,
               chunk=PAIR_SCORE_MAX_Q):
    """The eval-mode verification head (Linear(BatchNorm1d((x1 - x2)^2)), running statistics) of probe row q against the gallery
    rows idx[q, :], gathered inside the kernel: probe [Q, D], gallery [G, D], idx int32 [Q, k] with entries in [0, G), weight
    [C, D], bias [C] or None.  -> (logits [Q, k, C] or None, score [Q, k] or None), score = softmax(logits)[..., 0].
    chunk = queries per launch (at most 32 768); the bits do not depend on it."""
    probe, gallery = _chk_rr(probe, "probe", torch.float32, 2), _chk_rr(gallery, "gallery", torch.float32, 2)
    idx, weight = _chk_rr(idx, "idx", torch.int32, 2), _chk_rr(weight, "weight", torch.float32, 2)
    (Q, D), G, (C, k), chunk = probe.shape, gallery.shape[0], (weight.shape[0], idx.shape[1]), int(chunk)
    if gallery.shape[1] != D or weight.shape[1] != D or idx.shape[0] != Q:
        raise ValueError("rg_hip: pair_score: probe %s, gallery %s, idx %s, weight %s disagree"
                         % (tuple(probe.shape), tuple(gallery.shape), tuple(idx.shape), tuple(weight.shape)))
    if not (1 <= C <= PAIR_SCORE_MAX_C and 1 <= D <= PAIR_SCORE_MAX_D and 1 <= k <= G and Q >= 1):
        raise ValueError("rg_hip: pair_score needs 1 <= C <= %d, 1 <= D <= %d, 1 <= k <= G and Q >= 1, got C=%d D=%d k=%d G=%d Q=%d"
                         % (PAIR_SCORE_MAX_C, PAIR_SCORE_MAX_D, C, D, k, G, Q))
    if not (want_logits or want_score):
        raise ValueError("rg_hip: pair_score computes logits, score or both: one of want_logits and want_score")
    if not 1 <= chunk <= PAIR_SCORE_MAX_Q or chunk * k * C >= 2 ** 31:
        raise ValueError("rg_hip: pair_score: chunk must be 1 .. %d with chunk * k * C < 2^31, got %d" % (PAIR_SCORE_MAX_Q, chunk))
    gamma, beta = _pair_vec(gamma, "gamma", D), _pair_vec(beta, "beta", D)
    running_mean, running_var = _pair_vec(running_mean, "running_mean", D), _pair_vec(running_var, "running_var", D)
    bias = None if bias is None else _pair_vec(bias, "bias", C)
    if (probe.data_ptr() | gallery.data_ptr() | weight.data_ptr()) & 15:           # the rows are read as 16-byte vectors
        probe, gallery, weight = (t.clone() if t.data_ptr() & 15 else t for t in (probe, gallery, weight))
    dev = probe.device
    logits = torch.empty((Q, k, C), dtype=torch.float32, device=dev) if want_logits else None
    score = torch.empty((Q, k), dtype=torch.float32, device=dev) if want_score else None
    for q0 in range(0, Q, chunk):
        q1 = min(Q, q0 + chunk)
        lib.rg_pair_score(_p(probe[q0:q1]), _p(gallery), _p(idx[q0:q1]), _p(gamma), _p(beta), _p(running_mean), _p(running_var),
                          _p(weight), _p(bias), _p(None if logits is None else logits[q0:q1]),
                          _p(None if score is None else score[q0:q1]), q1 - q0, G, k, D, C, float(eps), _stream())
    return logits, score


def cascade_merge(dist, idx, score):
    """In place on dist [Q, G] (rows may be strided, columns not): the k columns idx[q, :] (int32, distinct per row) take
    score[q, :], every other column moves up by gap = max((max_j score[q, j] + 1) - min of the other columns, 0), so that the
    re-scored entries rank first (FD/reid/evaluators.py:218-226).  k == G: the overwrite alone.  Returns dist."""
    for t, name, dt in ((dist, "dist", torch.float32), (idx, "idx", torch.int32), (score, "score", torch.float32)):
        if not torch.is_tensor(t) or not t.is_cuda or t.dtype != dt or t.dim() != 2:
            raise ValueError("rg_hip: cascade_merge: %s must be a 2-D %s GPU tensor" % (name, dt))
    idx, score = _chk_rr(idx, "idx", torch.int32, 2), _chk_rr(score, "score", torch.float32, 2)
    _chk_rr(dist[0], "dist rows", torch.float32, 1)
    (Q, G), k = dist.shape, idx.shape[1]
    ld = dist.stride(0) if Q > 1 else max(G, dist.stride(0))
    if tuple(idx.shape) != (Q, k) or tuple(score.shape) != (Q, k) or not 1 <= k <= G or ld < G:
        raise ValueError("rg_hip: cascade_merge: dist %s (row stride %d), idx %s, score %s disagree (1 <= k <= G)"
                         % (tuple(dist.shape), ld, tuple(idx.shape), tuple(score.shape)))
    if G > CASCADE_MERGE_MAX_G:
        raise ValueError("rg_hip: cascade_merge: at most %d gallery columns, got %d" % (CASCADE_MERGE_MAX_G, G))
    lib.rg_cascade_merge(_p(dist), ld, _p(idx), _p(score), Q, G, k, _stream())
    return dist
