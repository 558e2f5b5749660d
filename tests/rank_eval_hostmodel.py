"""numpy model of the CMC / mAP scoring (csrc/rank_eval.hip, clustercontrast/evaluation_metrics/ranking.py), written from
the definitions: a stable argsort by distance (ties by gallery index), the validity rules, scikit-learn's
`average_precision_score` for AP and the hit rule for CMC.  tests/test_rank_eval_cpu.py ties it to the reference's recorded
results (tests/golden/reference_eval.npz); the GPU tests compare the device's per-query outputs with it.

Per query i, with valid_j = (gid_j != qid_i) | (gcam_j != qcam_i) (and gcam_j != qcam_i with separate_camera_set) and
pos_j = valid_j & (gid_j == qid_i), over the valid entries in stable (d, j) order:
  npos   number of positives
  ap     average precision of the scores -d (tied scores grouped), 0 without a positive
  first  valid non-matching entries before the first positive, -1 without a positive
  hits   [topk]: hits[r] = positives with exactly r valid non-matching entries before them
"""
import numpy as np


def ap_formula(match, d):
    """(1 / P) sum_p TP(d <= d_p) / N(d <= d_p) over the positives p of one query's valid entries"""
    match, d = np.asarray(match, dtype=bool), np.asarray(d)
    dp = d[match]
    tp = (dp[None, :] <= dp[:, None]).sum(axis=1)
    n = (d[None, :] <= dp[:, None]).sum(axis=1)
    return float(np.mean(tp / n.astype(np.float64)))


def ap_sklearn(match, d):
    from sklearn.metrics import average_precision_score
    return float(average_precision_score(np.asarray(match, dtype=bool), -np.asarray(d, dtype=np.float64)))


def per_query(dist, query_ids, gallery_ids, query_cams, gallery_cams, topk=100, separate_camera_set=False):
    """(npos int32 [Q], ap fp64 [Q], first int32 [Q], hits int32 [Q, topk]).  AP is scikit-learn's where it accepts the row
    (it refuses infinities) and the closed formula otherwise."""
    dist = np.asarray(dist)
    qid, gid, qcam, gcam = (np.asarray(v) for v in (query_ids, gallery_ids, query_cams, gallery_cams))
    Q, G = dist.shape
    order = np.argsort(dist, axis=1, kind="stable")
    npos, ap = np.zeros(Q, dtype=np.int32), np.zeros(Q)
    first, hits = np.full(Q, -1, dtype=np.int32), np.zeros((Q, topk), dtype=np.int32)
    for i in range(Q):
        idx = order[i]
        valid = (gid[idx] != qid[i]) | (gcam[idx] != qcam[i])
        if separate_camera_set:
            valid &= gcam[idx] != qcam[i]
        kept = idx[valid]
        match = gid[kept] == qid[i]
        npos[i] = match.sum()
        if npos[i] == 0:
            continue
        at = np.nonzero(match)[0]
        r = at - np.arange(len(at))                 # non-matching entries before each positive
        first[i] = r[0]
        hits[i] = np.bincount(r[r < topk], minlength=topk)[:topk]
        dk = dist[i, kept]
        ap[i] = ap_sklearn(match, dk) if np.isfinite(dk).all() else ap_formula(match, dk)
    return npos, ap, first, hits


def summarize(npos, ap, first, hits):
    """(mAP, CMC with first_match_break, CMC counting every positive): the reference's averages over the valid queries"""
    ok = npos > 0
    n = int(ok.sum())
    if n == 0:
        raise RuntimeError("No valid query")
    topk = hits.shape[1]
    f = first[ok]
    cmc_first = np.bincount(f[f < topk], minlength=topk)[:topk].astype(np.float64).cumsum() / n
    cmc_all = (hits[ok] / npos[ok, None].astype(np.float64)).sum(axis=0).cumsum() / n
    return float(ap[ok].mean()), cmc_first, cmc_all
