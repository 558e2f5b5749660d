"""numpy model of the single-gallery-shot CMC (csrc/cmc_shot.hip, ops.cmc_shot, clustercontrast.evaluation_metrics.cmc_single_shot),
written from the definition of the reference's `cmc(single_gallery_shot=True)` rather than from the counting form the device
uses: a stable argsort of the row by (distance, gallery index), the validity rules, per identity the list of its valid entries
in row order, one draw per identity and repeat, and the position of the query's own sampled entry among the sampled ones.
The only departure from the reference's text is that the draws of all queries are ONE `randint(0, highs)` call (`draw`);
tests/test_sgs_hostmodel_cpu.py ties that to a loop of `np.random.choice` and the whole model to the reference's recorded
curves and generator states (tests/golden/reference_sgs.npz).

Per valid query i (one with a valid entry of its own identity; the others are skipped BEFORE any draw):
  n      identities with a valid entry
  ids    those identities in first-appearance order over the row's valid entries (the order the reference's dict iterates in);
         slot = their indices among the sorted distinct gallery identities
  high   their valid counts in that order
  u      [repeat, n] draws, u[r, p] in [0, high[p]): the stream is repeat-major, position-minor
  rank   [repeat]: sampled entries of OTHER identities that precede the own identity's sampled entry
and over the queries hist[k] = #(query, repeat) with rank k < topk; the curve is (hist * w).cumsum() / num_valid with w = 1 under
first_match_break (the reference adds 1 per repeat) and 1 / repeat otherwise.

The steps are methods so that the CPU test can plant a defect in a copy (a subclass) and show that the fixture catches it.
"""
import numpy as np


def draw(random_state, highs):
    """one bounded draw per entry of `highs`, in order: what a loop of np.random.choice over lists of those lengths consumes"""
    rs = np.random if random_state is None else random_state
    highs = np.asarray(highs)
    if highs.size == 0:
        return np.zeros(0, dtype=np.int64)
    return rs.randint(0, highs)


class Model(object):
    def sort_row(self, d_row):
        """gallery indices in (d, j) order"""
        return np.argsort(d_row, kind="stable")

    def id_order(self, kept_ids):
        """the distinct identities of the row's valid entries, by first appearance"""
        uniq, first = np.unique(kept_ids, return_index=True)
        return uniq[np.argsort(first, kind="stable")]

    def highs_of(self, info, repeat):
        """the bounds of the query's draws in stream order; a skipped query draws nothing"""
        if info["skip"]:
            return np.zeros(0, dtype=np.int64)
        return np.tile(info["high"], repeat)

    def draws_of(self, flat, info, repeat):
        """[repeat, n] from the query's slice of the stream"""
        return np.asarray(flat).reshape(repeat, info["n"])

    def rank_of(self, sampled, own):
        """sampled: per position, where that identity's sampled entry sits among the row's valid entries"""
        return int((sampled < sampled[own]).sum())

    # ---- per query ----------------------------------------------------------------------------------------------------------
    def query_order(self, d_row, qid_i, qcam_i, gid, gcam, uniq, separate_camera_set=False):
        order = self.sort_row(np.asarray(d_row))
        valid = (gid[order] != qid_i) | (gcam[order] != qcam_i)
        if separate_camera_set:
            valid &= gcam[order] != qcam_i
        kept_ids = gid[order[valid]]
        ids = self.id_order(kept_ids) if kept_ids.size else np.zeros(0, dtype=gid.dtype)
        lists = [np.nonzero(kept_ids == x)[0] for x in ids]
        skip = not (kept_ids == qid_i).any()
        info = dict(skip=skip, ids=ids, lists=lists, high=np.array([len(v) for v in lists], dtype=np.int64),
                    slot=np.searchsorted(uniq, ids).astype(np.int32), own=-1 if skip else int(np.nonzero(ids == qid_i)[0][0]))
        info["n"] = 0 if skip else len(ids)
        return info

    def query_ranks(self, info, u):
        """ranks [repeat] of one valid query given its draws u [repeat, n]"""
        u = np.asarray(u)
        out = np.zeros(u.shape[0], dtype=np.int32)
        for r in range(u.shape[0]):
            sampled = np.array([info["lists"][p][u[r, p]] for p in range(len(info["lists"]))])
            out[r] = self.rank_of(sampled, info["own"])
        return out

    # ---- all queries --------------------------------------------------------------------------------------------------------
    def run(self, dist, query_ids, gallery_ids, query_cams, gallery_cams, topk=100, separate_camera_set=False,
            first_match_break=False, repeat=10, random_state=None):
        """dict: n [Q], slot / high [Q, nid] (-1 / 0 beyond n), rank [Q, repeat] (-1 for a skipped query), hist int64 [topk],
        num_valid, curve, infos"""
        dist = np.asarray(dist)
        qid, gid, qcam, gcam = (np.asarray(v) for v in (query_ids, gallery_ids, query_cams, gallery_cams))
        Q = dist.shape[0]
        uniq = np.unique(gid)
        nid = len(uniq)
        infos = [self.query_order(dist[i], qid[i], qcam[i], gid, gcam, uniq, separate_camera_set) for i in range(Q)]
        blocks = [self.highs_of(info, repeat) for info in infos]
        flat = draw(random_state, np.concatenate(blocks) if blocks else np.zeros(0, dtype=np.int64))
        n = np.zeros(Q, dtype=np.int32)
        slot, high = np.full((Q, nid), -1, dtype=np.int32), np.zeros((Q, nid), dtype=np.int32)
        rank, hist = np.full((Q, repeat), -1, dtype=np.int32), np.zeros(topk, dtype=np.int64)
        at = 0
        for i, (info, block) in enumerate(zip(infos, blocks)):
            mine = flat[at:at + len(block)]
            at += len(block)
            if info["skip"]:
                continue
            n[i] = info["n"]
            slot[i, :n[i]], high[i, :n[i]] = info["slot"], info["high"]
            rank[i] = self.query_ranks(info, self.draws_of(mine, info, repeat))
            hist += np.bincount(rank[i][rank[i] < topk], minlength=topk)[:topk]
        num_valid = int((n > 0).sum())
        res = dict(n=n, slot=slot, high=high, rank=rank, hist=hist, num_valid=num_valid, infos=infos, curve=None)
        if num_valid:
            res["curve"] = curve(hist, num_valid, repeat, first_match_break)
        return res


def curve(hist, num_valid, repeat, first_match_break):
    """the expression clustercontrast.evaluation_metrics.cmc_single_shot returns"""
    w = 1.0 if first_match_break else 1.0 / repeat
    return (np.asarray(hist) * w).cumsum() / num_valid


def run(*args, **kwargs):
    res = Model().run(*args, **kwargs)
    if res["num_valid"] == 0:
        raise RuntimeError("No valid query")
    return res
