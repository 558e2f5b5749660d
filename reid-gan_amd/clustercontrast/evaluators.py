"""Feature extraction and distance matrices of the evaluation / pseudo-labelling loops on the MI355X.

Mirror of the numeric part of CC/clustercontrast/evaluators.py: `extract_cnn_feature` (:16-20), `extract_all_feature`
(:22-27), `pairwise_distance` (:71-88) (FD/reid/evaluators.py:76-98 and FD/reid/feature_extraction/cnn.py:9-16 are the same
functions).  The loader loop `extract_features` (:30-68), `evaluate_all` and the `Evaluator` class keep the reference's names
only when its tree sits behind this one on sys.path: they are inherited at the bottom of this file, call the functions defined
here, and import `cmc` / `mean_ap` from this build's `.evaluation_metrics` (scored on the device) and `re_ranking` from this
build's `.utils.rerank`.  Their device-resident counterparts live here under names of their own — `extract_features_device`,
`evaluate_all_device`, `DeviceEvaluator` — and need no reference tree: features, distance matrices and the re-ranked matrix stay
on the device and one `ops.rank_eval` call scores mAP and the `market1501` CMC.  The collection loop behind
`extract_features_device` and `DeviceFeatures` live in rg_hip/hostloop.py; `score_mean_ap`, the opening of `evaluate_all_device`,
is defined here and serves reid/evaluators.py too.
"""
from __future__ import print_function, absolute_import

import torch

from rg_hip import hostloop, search
from rg_hip.hostloop import DeviceFeatures  # noqa: F401


def _to_torch(x):
    return x if torch.is_tensor(x) else torch.as_tensor(x)


def extract_cnn_feature(model, inputs):
    inputs = _to_torch(inputs).to(search.device(), non_blocking=True)
    with torch.no_grad():
        outputs = model(inputs)
    return outputs.data.cpu()


def extract_all_feature(model, inputs):
    inputs = _to_torch(inputs).to(search.device(), non_blocking=True)
    with torch.no_grad():
        outputs, extra_outputs = model(inputs, test_all=True)
    return outputs.data.cpu(), extra_outputs.data.cpu()


def pairwise_distance(features, query=None, gallery=None, return_device=False):
    """return_device=True: the distance matrix (and, with query / gallery, the two feature blocks) stay device tensors"""
    dist_m, x, y, xd, yd = search.pairwise(features, query, gallery)
    if query is None and gallery is None:
        return dist_m if return_device else dist_m.cpu()
    if return_device:
        return dist_m, xd, yd
    return dist_m.cpu(), x.numpy(), y.numpy()


def extract_features_device(model, data_loader, print_freq=50):
    """The reference's `extract_features` loop (:30-68) with the features kept on the device: (DeviceFeatures, labels)."""
    return hostloop.collect_features(model, data_loader, print_freq)


def pairwise_distance_device(features, query, gallery):
    """[len(query), len(gallery)] squared distances of a DeviceFeatures, on the device"""
    return search.dist_block(features.rows(query), features.rows(gallery), 1.0, True)


def score_mean_ap(distmat, query=None, gallery=None, query_ids=None, gallery_ids=None, query_cams=None, gallery_cams=None):
    """The opening of both `evaluate_all_device`: ids and cameras from the (fname, pid, cam) triples of `query` / `gallery` or
    from the four lists, one `ops.rank_eval` pass over the matrix, the 'Mean AP' line.  Returns the pass's results, the mAP and
    the four lists."""
    from .evaluation_metrics import ranking as R
    if query is not None and gallery is not None:
        query_ids = [pid for _, pid, _ in query]
        gallery_ids = [pid for _, pid, _ in gallery]
        query_cams = [cam for _, _, cam in query]
        gallery_cams = [cam for _, _, cam in gallery]
    else:
        assert (query_ids is not None and gallery_ids is not None
                and query_cams is not None and gallery_cams is not None)
    res = R._score(distmat, query_ids, gallery_ids, query_cams, gallery_cams, 100, False)
    mAP = float(res["ap_sum"] / res["num_valid"])
    print('Mean AP: {:4.1%}'.format(mAP))
    return res, mAP, (query_ids, gallery_ids, query_cams, gallery_cams)


def evaluate_all_device(distmat, query=None, gallery=None,
                        query_ids=None, gallery_ids=None,
                        query_cams=None, gallery_cams=None,
                        cmc_topk=(1, 5, 10), cmc_flag=False):
    """The reference's `evaluate_all` (:91-122, without its two unused feature arguments) from one `ops.rank_eval` call: mAP and
    the `market1501` CMC (first match, cameras not separated) come out of the same pass over the matrix.  Same printed lines
    and return values."""
    import numpy as np
    res, mAP, _ = score_mean_ap(distmat, query, gallery, query_ids, gallery_ids, query_cams, gallery_cams)

    if (not cmc_flag):
        return mAP

    scores = res["first_hist"].astype(np.float64).cumsum() / res["num_valid"]
    print('CMC Scores:')
    for k in cmc_topk:
        print('  top-{:<4}{:12.1%}'.format(k, scores[k - 1]))
    return scores, mAP


class DeviceEvaluator(object):
    """The reference's `Evaluator` (:125-142) with the features, the distance matrices and the re-ranked matrix kept on the
    device; works with no reference tree."""

    def __init__(self, model):
        super(DeviceEvaluator, self).__init__()
        self.model = model

    def evaluate(self, data_loader, query, gallery, cmc_flag=False, rerank=False):
        from .utils.rerank import re_ranking
        features, _ = extract_features_device(self.model, data_loader)
        distmat = pairwise_distance_device(features, query, gallery)
        results = evaluate_all_device(distmat, query=query, gallery=gallery, cmc_flag=cmc_flag)

        if (not rerank):
            return results

        print('Applying person re-ranking ...')
        distmat_qq = pairwise_distance_device(features, query, query)
        distmat_gg = pairwise_distance_device(features, gallery, gallery)
        distmat = re_ranking(distmat, distmat_qq, distmat_gg, return_device=True)
        return evaluate_all_device(distmat, query=query, gallery=gallery, cmc_flag=cmc_flag)


# `extract_features`, `Evaluator` and `evaluate_all` are the reference's own host code: when its tree sits behind this one on
# sys.path they are taken from there, and they call the functions above (rg_hip/overlay.py); the `re_ranking`, `cmc` and `mean_ap`
# they import are this build's (clustercontrast/utils/rerank.py, clustercontrast/evaluation_metrics/, on the device)
from rg_hip.overlay import inherit as _rg_inherit  # noqa: E402
_rg_inherit(globals())
