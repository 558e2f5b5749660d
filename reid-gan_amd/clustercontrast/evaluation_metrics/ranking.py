"""CMC and mAP of a query x gallery distance matrix on the MI355X.

Mirror of CC/clustercontrast/evaluation_metrics/ranking.py (`cmc` :18-79, `mean_ap` :82-115; FD/reid/evaluation_metrics/
ranking.py is the same file): same names, arguments, defaults and return types.  The reference argsorts the whole matrix on
the host (twice per evaluation) and calls scikit-learn's `average_precision_score` once per query; here `ops.rank_eval`
(csrc/rank_eval.hip) counts, per positive, the entries that a stable sort would put before it, and topk + 2 numbers leave the
device.  The distance matrix may be a numpy array, a CPU tensor or a device tensor; a device tensor is used where it is.

Ties: average precision groups equal distances (as scikit-learn does), so mAP does not depend on how ties are ordered; the
CMC ranks are those of a stable sort by (distance, gallery index), where the reference's quicksort leaves them unspecified.
A NaN in the matrix raises ValueError.

`cmc(single_gallery_shot=True)` draws from numpy's global generator in a Python loop and the draws define the result: it is
not moved to the device.  With the reference tree behind this one on sys.path the call is handed to the reference's own
function; without one it raises NotImplementedError.
"""
from __future__ import absolute_import

import os

import numpy as np
import torch

from rg_hip import ops, search

__all__ = ['cmc', 'mean_ap']


def _dist_on_device(distmat):
    t = distmat if torch.is_tensor(distmat) else torch.as_tensor(np.asarray(distmat))
    if t.dim() != 2:
        raise ValueError("distmat must be a [query, gallery] matrix, got shape %s" % (tuple(t.shape),))
    t = t.detach()
    if t.dtype not in (torch.float32, torch.float64):
        t = t.float() if t.dtype in (torch.float16, torch.bfloat16) else t.double()
    if not t.is_cuda:
        t = t.to(search.device())
    return t.contiguous()


def _ids_on_device(v, name, n, dev):
    """int32 device vector of the ids / cameras (any integer sequence, array or tensor), after a range check"""
    if torch.is_tensor(v):
        t = v.detach().reshape(-1)
        if t.dtype.is_floating_point or t.dtype == torch.bool:
            raise ValueError("%s must hold integers, got %s" % (name, t.dtype))
        if t.numel() != n:
            raise ValueError("%s has %d entries, the distance matrix needs %d" % (name, t.numel(), n))
        if t.dtype != torch.int32:
            if t.numel() and (int(t.min()) < -2 ** 31 or int(t.max()) >= 2 ** 31):
                raise ValueError("%s does not fit int32" % name)
            t = t.to(torch.int32)
        return t.to(dev).contiguous()
    a = np.asarray(v).reshape(-1)
    if a.dtype.kind not in "iu":
        raise ValueError("%s must hold integers, got %s" % (name, a.dtype))
    if a.size != n:
        raise ValueError("%s has %d entries, the distance matrix needs %d" % (name, a.size, n))
    if a.size and (int(a.min()) < -2 ** 31 or int(a.max()) >= 2 ** 31):
        raise ValueError("%s does not fit int32" % name)
    return torch.from_numpy(np.ascontiguousarray(a.astype(np.int32))).to(dev)


def _fill_defaults(m, n, query_ids, gallery_ids, query_cams, gallery_cams):
    # the reference's defaults (:26-33)
    if query_ids is None:
        query_ids = np.arange(m)
    if gallery_ids is None:
        gallery_ids = np.arange(n)
    if query_cams is None:
        query_cams = np.zeros(m).astype(np.int32)
    if gallery_cams is None:
        gallery_cams = np.ones(n).astype(np.int32)
    return query_ids, gallery_ids, query_cams, gallery_cams


def _score(distmat, query_ids, gallery_ids, query_cams, gallery_cams, topk, separate_camera_set):
    d = _dist_on_device(distmat)
    m, n = d.shape
    ids = _fill_defaults(m, n, query_ids, gallery_ids, query_cams, gallery_cams)
    names = ("query_ids", "gallery_ids", "query_cams", "gallery_cams")
    qi, gi, qc, gc = (_ids_on_device(v, nm, k, d.device) for v, nm, k in zip(ids, names, (m, n, m, n)))
    res = ops.rank_eval(d, qi, gi, qc, gc, topk=topk, separate_camera_set=separate_camera_set)
    if res["num_valid"] == 0:
        raise RuntimeError("No valid query")
    return res


def _reference_ranking():
    """the reference's ranking.py from the extended package path (rg_hip/overlay.py), loaded the way overlay.inherit loads
    modules; None without a reference tree"""
    import importlib.util
    import sys
    pkg = __name__.rpartition(".")[0]
    ref_name = pkg + "._ref_ranking"
    if ref_name in sys.modules:
        return sys.modules[ref_name]
    own = os.path.abspath(__file__)
    for d in list(getattr(sys.modules.get(pkg), "__path__", [])):
        cand = os.path.join(d, "ranking.py")
        if not os.path.isfile(cand) or os.path.abspath(cand) == own:
            continue
        spec = importlib.util.spec_from_file_location(ref_name, cand)
        ref = importlib.util.module_from_spec(spec)
        ref.__package__ = pkg
        sys.modules[ref_name] = ref
        try:
            spec.loader.exec_module(ref)
        except Exception:
            sys.modules.pop(ref_name, None)
            raise
        return ref
    return None


def cmc(distmat, query_ids=None, gallery_ids=None,
        query_cams=None, gallery_cams=None, topk=100,
        separate_camera_set=False,
        single_gallery_shot=False,
        first_match_break=False):
    if single_gallery_shot:
        ref = _reference_ranking()
        if ref is None:
            raise NotImplementedError("cmc(single_gallery_shot=True) samples the gallery with numpy's global generator on the host "
                                      "and is not implemented on the device; it needs the reference tree behind this one")
        host = distmat.detach().cpu() if torch.is_tensor(distmat) else distmat
        return ref.cmc(host, query_ids, gallery_ids, query_cams, gallery_cams, topk=topk, separate_camera_set=separate_camera_set,
                       single_gallery_shot=True, first_match_break=first_match_break)
    res = _score(distmat, query_ids, gallery_ids, query_cams, gallery_cams, int(topk), bool(separate_camera_set))
    ret = res["first_hist"].astype(np.float64) if first_match_break else res["allshots"]
    return ret.cumsum() / res["num_valid"]


def mean_ap(distmat, query_ids=None, gallery_ids=None,
            query_cams=None, gallery_cams=None):
    res = _score(distmat, query_ids, gallery_ids, query_cams, gallery_cams, 1, False)
    return float(res["ap_sum"] / res["num_valid"])
