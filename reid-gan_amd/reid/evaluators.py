"""Evaluation distances and the cascade re-ranking stage of FD-GAN's evaluators on the MI355X.

Mirror of the numeric part of FD-GAN-master/reid/evaluators.py: `pairwise_distance` (:76-98), `extract_embeddings`
(:19-43) and `CascadeEvaluator` (:183-227, what `baseline.py:103-104` — BASELINE config 1 — calls).  The loader loop
`extract_features` and `evaluate_all` are host code and stay the reference's (inherited at the bottom of this file when its tree
sits behind this one on sys.path); the `cmc` / `mean_ap` they import are this build's (reid/evaluation_metrics/, on the device).

MI355X-first restatement of the second stage: the reference scores one query at a time (one embedding-network call on a
[1, 2048] probe against its top-k gallery rows, 3 368 calls for Market-1501).  Here the first-stage ranking is a device
top-k of the distance matrix (`rg_topk_rows` on the negated distances, ties by lower index like a stable argsort), the
top-k gallery rows of ALL queries are gathered into one [Q * k, 2048] operand and the embedding network (eltwise
(x1 - x2)^2 -> BatchNorm1d -> Linear) runs once.  The merge of the two stages (:215-225) is unchanged arithmetic.

Device-resident counterparts under names of their own, which need no reference tree: `extract_features_device`,
`evaluate_all_device` (and `evaluate_all_single_shot`, which also scores the `cuhk03` column on the device) and
`DeviceCascadeEvaluator`.  Its second stage gathers the pairs inside `ops.pair_score`
(csrc/cascade.hip: no [Q * k, 2048] operand is ever built) and merges in place on the device with `ops.cascade_merge`.
The collection loop behind `extract_features_device` is rg_hip/hostloop.py's and the opening of `evaluate_all_device` is
`clustercontrast.evaluators.score_mean_ap`.
"""
from __future__ import print_function, absolute_import

import numpy as np
import torch

from rg_hip import hostloop, ops, search


def pairwise_distance(features, query=None, gallery=None, metric=None):
    if metric is not None:
        raise NotImplementedError("pairwise_distance: learned metrics (metric.transform) are not on the GAN path")
    return search.pairwise(features, query, gallery)[0].cpu()


def rank_topk(distmat, k):
    """indices [Q, k] of the k smallest distances per row, ascending, ties by lower column (device top-k of -dist)"""
    d = search.to_device(distmat, "rank_topk: distmat")
    return search.blocked_topk(d.shape[0], int(k), lambda r0, r1: ops.scale(d[r0:r1], -1.0)).long()


def extract_embeddings(model, features, alpha, query=None, topk_gallery=None, rerank_topk=0, print_freq=500,
                       topk_indices=None, gallery=None):
    """pairwise scores [Q * rerank_topk, C] of every query against its top-k gallery entries.  Reference signature
    (`topk_gallery`: per query, the list of gallery (fname, pid, cam) triples); `topk_indices` [Q, k] + `gallery` is the
    device form used by CascadeEvaluator (no per-query Python lists)."""
    model.eval()
    probe = search.to_device(search.stack_rows(features, query), "extract_embeddings: query features")
    Q = probe.shape[0]
    if topk_indices is not None:
        gal = search.to_device(search.stack_rows(features, gallery), "extract_embeddings: gallery features")
        x2 = gal.index_select(0, topk_indices.to(gal.device).reshape(-1))
    else:
        x2 = search.to_device(search.stack_rows(features, [e for i in range(Q) for e in topk_gallery[i]]),
                              "extract_embeddings: gallery features")
    x1 = probe.view(Q, 1, -1).expand(Q, rerank_topk, probe.shape[1]).reshape(Q * rerank_topk, -1).contiguous()
    with torch.no_grad():
        score = model(x1, x2.contiguous())
    return score.view(Q * rerank_topk, -1)


class CascadeEvaluator(object):
    def __init__(self, base_model, embed_model, embed_dist_fn=None):
        super(CascadeEvaluator, self).__init__()
        self.base_model = base_model
        self.embed_model = embed_model
        self.embed_dist_fn = embed_dist_fn

    def second_stage(self, distmat, features, query, gallery, alpha=0, rerank_topk=75):
        """first-stage distances [Q, G] -> merged two-stage distances (numpy, as the reference leaves them), :202-225"""
        distmat = np.array(torch.as_tensor(distmat).cpu().numpy(), dtype=np.float32)
        Q, G = distmat.shape
        k = min(int(rerank_topk), G)
        top = rank_topk(distmat, k)
        embeddings = extract_embeddings(self.embed_model, features, alpha, query=query, rerank_topk=k, topk_indices=top,
                                        gallery=gallery)
        if self.embed_dist_fn is not None:
            embeddings = self.embed_dist_fn(embeddings.data)
        emb = torch.as_tensor(embeddings).detach().float().cpu().numpy().reshape(Q, k)
        top_np = top.cpu().numpy()
        rows = np.arange(Q)[:, None]
        if k < G:
            # the first gallery entry OUTSIDE the top-k (:222 `indices[rerank_topk]`): smallest first-stage distance of the rest
            rest = distmat.copy()
            rest[rows, top_np] = np.inf
            nxt = rest.min(axis=1)
        distmat[rows, top_np] = emb
        if k < G:
            bar = emb.max(axis=1)
            gap = np.maximum(bar + 1.0 - nxt, 0.0).astype(np.float32)
            outside = np.ones_like(distmat, dtype=bool)
            outside[rows, top_np] = False
            distmat += outside * gap[:, None]
        return distmat

    def evaluate(self, data_loader, query, gallery, alpha=0, cache_file=None, rerank_topk=75, second_stage=True, dataset=None,
                 top1=True):
        features, _ = extract_features(self.base_model, data_loader)          # noqa: F821  (reference host loop, inherited)
        distmat = pairwise_distance(features, query, gallery)
        print("First stage evaluation:")
        if second_stage:
            evaluate_all(distmat, query=query, gallery=gallery, dataset=dataset, top1=top1)      # noqa: F821
            distmat = self.second_stage(distmat, features, query, gallery, alpha, rerank_topk)
            print("Second stage evaluation:")
        return evaluate_all(distmat, query, gallery, dataset=dataset, top1=top1)                # noqa: F821


# ------------------------------------------------------------------------------------------------
# the device-resident cascade: needs no reference tree, nothing but ids, cameras and the scores crosses to the host
# ------------------------------------------------------------------------------------------------
PAIR_OPERAND_BYTES = 256 << 20      # composed path: the [q * k, D] operand of one chunk of queries stays at or below this


def softmax_class0(x):
    """F.softmax(x, dim=1)[:, 0]: the `embed_dist_fn` of baseline.py:106 and train.py:59 under a name, so that
    DeviceCascadeEvaluator can recognise it and take the score from the pair-scoring kernel"""
    return torch.nn.functional.softmax(x, dim=1)[:, 0]


def extract_features_device(model, data_loader, print_freq=1):
    """The reference's `extract_features` loop (:46-73) with the features kept on the device: (DeviceFeatures, labels).  Reads
    the first three fields of a batch (imgs, fnames, pids), so the 4-tuples of this package's loaders and 5-tuples both work."""
    return hostloop.collect_features(model, data_loader, print_freq)


def evaluate_all_device(distmat, query=None, gallery=None,
                        query_ids=None, gallery_ids=None,
                        query_cams=None, gallery_cams=None,
                        cmc_topk=(1, 5, 10), dataset=None, top1=True):
    """The reference's `evaluate_all` (:101-181): same signature, printed lines and return values, from ONE `ops.rank_eval` pass
    over the (device) matrix, which yields mAP, the `allshots` and the `market1501` CMC together.  top1=False returns the mAP; a
    named dataset other than 'cuhk03' returns (market1501 top-1, mAP).
    The `cuhk03` column (single_gallery_shot=True) by default goes through this build's `cmc`, which hands it to the reference's
    host sampling: with dataset=None and with dataset='cuhk03' a run without the reference tree ends in that function's
    NotImplementedError (after the 'Mean AP' line).  The signature stays the reference's; `evaluate_all_single_shot` is the same
    function with the column scored on the device."""
    return _evaluate_all(distmat, query, gallery, query_ids, gallery_ids, query_cams, gallery_cams, cmc_topk, dataset, top1, False)


def evaluate_all_single_shot(distmat, query=None, gallery=None,
                             query_ids=None, gallery_ids=None,
                             query_cams=None, gallery_cams=None,
                             cmc_topk=(1, 5, 10), dataset=None, top1=True, single_shot=True):
    """`evaluate_all_device` with one more, last keyword, under a name of its own: the `cuhk03` column comes from
    `cmc_single_shot` (the reference's protocol with the ranks counted on the device, separate_camera_set=True as the reference
    configures `cuhk03`), so dataset=None and dataset='cuhk03' need no reference tree.  single_shot=True draws from numpy's
    global generator as the reference does, a `np.random.RandomState` is drawn from instead, False is `evaluate_all_device`."""
    return _evaluate_all(distmat, query, gallery, query_ids, gallery_ids, query_cams, gallery_cams, cmc_topk, dataset, top1, single_shot)


def _evaluate_all(distmat, query, gallery, query_ids, gallery_ids, query_cams, gallery_cams, cmc_topk, dataset, top1, single_shot):
    from clustercontrast.evaluation_metrics import ranking as R
    from clustercontrast.evaluators import score_mean_ap
    res, mAP, (query_ids, gallery_ids, query_cams, gallery_cams) = score_mean_ap(distmat, query, gallery, query_ids, gallery_ids,
                                                                                 query_cams, gallery_cams)
    if not top1:
        return mAP

    def cuhk03():
        if single_shot is not False and single_shot is not None:
            return R.cmc_single_shot(distmat, query_ids, gallery_ids, query_cams, gallery_cams, separate_camera_set=True,
                                     first_match_break=False, random_state=None if single_shot is True else single_shot)
        return R.cmc(distmat, query_ids, gallery_ids, query_cams, gallery_cams, separate_camera_set=True,
                     single_gallery_shot=True, first_match_break=False)
    allshots = res["allshots"].cumsum() / res["num_valid"]
    market = res["first_hist"].astype(np.float64).cumsum() / res["num_valid"]
    if not dataset:
        cmc_scores = {'allshots': allshots, 'cuhk03': cuhk03(), 'market1501': market}
        print('CMC Scores{:>12}{:>12}{:>12}'
              .format('allshots', 'cuhk03', 'market1501'))
        for k in cmc_topk:
            print('  top-{:<4}{:12.1%}{:12.1%}{:12.1%}'
                  .format(k, cmc_scores['allshots'][k - 1],
                          cmc_scores['cuhk03'][k - 1],
                          cmc_scores['market1501'][k - 1]))
        return cmc_scores['allshots'][0]
    name = 'cuhk03' if dataset == 'cuhk03' else 'market1501'
    scores = cuhk03() if name == 'cuhk03' else market
    print('CMC Scores{:>12}'.format(name))
    for k in cmc_topk:
        print('  top-{:<4}{:12.1%}'
              .format(k, scores[k - 1]))
    return scores[0], mAP


class DeviceCascadeEvaluator(object):
    """`CascadeEvaluator` with features, distances, ranking, pair scores and the merged matrix kept on the device; works with no
    reference tree.  The second stage is a device top-k, `ops.pair_score` (the embedding network on pairs gathered inside the
    kernel: no [Q * k, D] operand) and `ops.cascade_merge` (in place).  single_shot is `evaluate_all_single_shot`'s: False keeps the
    `cuhk03` column with the reference's host sampling, True or a `np.random.RandomState` scores it on the device."""

    def __init__(self, base_model, embed_model, embed_dist_fn=softmax_class0, single_shot=False):
        super(DeviceCascadeEvaluator, self).__init__()
        self.base_model = base_model
        self.embed_model = embed_model
        self.embed_dist_fn = embed_dist_fn
        self.single_shot = single_shot
        self.last_path = None           # 'score' / 'logits' (the fused kernel) or 'composed', and the chunks the latter took
        self.last_chunks = 0
        self.last_distmat = None        # the matrix the last `evaluate` scored (device), for callers that go on with it

    def fusable(self, D):
        from reid.models.embedding import EltwiseSubEmbed
        m = self.embed_model
        return isinstance(m, EltwiseSubEmbed) and m.has_fused_loss and D <= ops.PAIR_SCORE_MAX_D

    def pair_scores(self, probe, gallery, top, pair_bytes=PAIR_OPERAND_BYTES):
        """[Q, k] second-stage distances of every query against the gallery rows `top` int32 [Q, k] lists"""
        (Q, D), k, fn = probe.shape, top.shape[1], self.embed_dist_fn
        m = self.embed_model
        m.eval()
        if self.fusable(D):
            bn, fc = m.bn, m.classifier
            fused = fn is softmax_class0
            self.last_path, self.last_chunks = ('score' if fused else 'logits'), 1
            logits, score = ops.pair_score(probe, gallery, top, bn.weight.detach(), bn.bias.detach(), bn.running_mean,
                                           bn.running_var, fc.weight.detach(), None if fc.bias is None else fc.bias.detach(),
                                           bn.eps, want_logits=not fused, want_score=fused)
            if fused:
                return score
            emb = logits.view(Q * k, -1)
            emb = fn(emb) if fn is not None else emb
            return emb.detach().float().reshape(Q, k).contiguous()
        rows = max(1, int(pair_bytes) // (k * D * 4))
        out = torch.empty((Q, k), dtype=torch.float32, device=probe.device)
        self.last_path, self.last_chunks = 'composed', 0
        with torch.no_grad():
            for q0 in range(0, Q, rows):
                q1 = min(Q, q0 + rows)
                x1 = probe[q0:q1].view(q1 - q0, 1, D).expand(q1 - q0, k, D).reshape((q1 - q0) * k, D).contiguous()
                x2 = gallery.index_select(0, top[q0:q1].reshape(-1).long())
                emb = m(x1, x2).view((q1 - q0) * k, -1)
                emb = fn(emb.data) if fn is not None else emb
                out[q0:q1] = emb.detach().float().reshape(q1 - q0, k)
                self.last_chunks += 1
        return out

    def second_stage_device(self, distmat, probe, gallery, rerank_topk=75, pair_bytes=PAIR_OPERAND_BYTES):
        """first-stage distances [Q, G] on the device -> the merged two-stage distances, written over `distmat` and returned
        (:202-225).  probe [Q, D], gallery [G, D]: contiguous fp32 device tensors.  pair_bytes bounds the [q * k, D] operand
        of the composed path (an embed model the kernel does not cover)."""
        Q, G = distmat.shape
        k = min(int(rerank_topk), G)
        top = search.blocked_topk(Q, k, lambda r0, r1: ops.scale(distmat[r0:r1], -1.0))
        score = self.pair_scores(probe, gallery, top, pair_bytes)
        return ops.cascade_merge(distmat, top, score)

    def evaluate(self, data_loader, query, gallery, alpha=0, cache_file=None, rerank_topk=75, second_stage=True, dataset=None,
                 top1=True):
        features, _ = extract_features_device(self.base_model, data_loader)
        probe, gal = features.rows(query), features.rows(gallery)
        distmat = search.dist_block(probe, gal, 1.0, True)
        print("First stage evaluation:")
        if second_stage:
            evaluate_all_single_shot(distmat, query=query, gallery=gallery, dataset=dataset, top1=top1, single_shot=self.single_shot)
            distmat = self.second_stage_device(distmat, probe, gal, rerank_topk)
            print("Second stage evaluation:")
        self.last_distmat = distmat
        return evaluate_all_single_shot(distmat, query, gallery, dataset=dataset, top1=top1, single_shot=self.single_shot)


# `extract_features`, `evaluate_all`, `Evaluator` are the reference's own host code (rg_hip/overlay.py); they score through this
# build's reid.evaluation_metrics
from rg_hip.overlay import inherit as _rg_inherit  # noqa: E402
_rg_inherit(globals())
