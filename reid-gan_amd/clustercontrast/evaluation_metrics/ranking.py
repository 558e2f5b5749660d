"""CMC and mAP of a query x gallery distance matrix on the MI355X.

Mirror of CC/clustercontrast/evaluation_metrics/ranking.py (`cmc` :18-79, `mean_ap` :82-115; FD/reid/evaluation_metrics/
ranking.py is the same file): same names, arguments, defaults and return types.  The reference argsorts the whole matrix on
the host (twice per evaluation) and calls scikit-learn's `average_precision_score` once per query; here `ops.rank_eval`
(csrc/rank_eval.hip) counts, per positive, the entries that a stable sort would put before it, and topk + 2 numbers leave the
device.  The distance matrix may be a numpy array, a CPU tensor or a device tensor; a device tensor is used where it is.

Ties: average precision groups equal distances (as scikit-learn does), so mAP does not depend on how ties are ordered; the
CMC ranks are those of a stable sort by (distance, gallery index), where the reference's quicksort leaves them unspecified.
A NaN in the matrix raises ValueError.

`cmc(single_gallery_shot=True)` draws from numpy's global generator in a Python loop and the draws define the result: that
call is not moved to the device.  With the reference tree behind this one on sys.path it is handed to the reference's own
function; without one it raises NotImplementedError.  The opt-in is `cmc_single_shot`, a name of its own: the same protocol
with the draws made on the host in ONE `randint` call that consumes exactly the stream of the reference's loop (same values,
same generator state afterwards), and the ranks counted on the device (csrc/cmc_shot.hip) — no copy of the matrix, no sort.
"""
from __future__ import absolute_import

import os

import numpy as np
import torch

from rg_hip import ops, search

__all__ = ['cmc', 'mean_ap', 'cmc_single_shot']


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
                                      "and is not implemented on the device; it needs the reference tree behind this one "
                                      "(cmc_single_shot is the device-resident form of the same protocol)")
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


def cmc_single_shot(distmat, query_ids=None, gallery_ids=None, query_cams=None, gallery_cams=None, topk=100,
                    separate_camera_set=False, first_match_break=False, repeat=10, random_state=None, chunk=0, debug=False):
    """The reference's `cmc(single_gallery_shot=True)` (:53-75; `repeat` is its constant 10) without the matrix leaving the
    device: `ops.cmc_shot` finds, per query, the order in which the reference draws for the gallery identities and their valid
    counts, the draws are ONE `randint` call on the host, and the device counts the rank of every (query, repeat).  Inputs are
    coerced as in `cmc`.  random_state None draws from numpy's global generator, so the same `np.random.seed` gives the
    reference's curve and leaves the generator in the reference's state; a `np.random.RandomState` is drawn from instead.
    Returns (hist * w).cumsum() / num_valid, float64 [topk], with w = 1 under first_match_break (the reference then adds 1 per
    repeat, `repeat` per query) and 1 / repeat otherwise.  Ties in a row are ordered by (distance, gallery index).  Every
    argument check and the NaN check (ValueError) come before the first draw.  chunk = queries per rank launch (0 = automatic);
    the result and the generator state do not depend on it.  debug=True returns (curve, {"n", "slot", "high", "rank" (device),
    "hist" (host), "num_valid"})."""
    topk, repeat = int(topk), int(repeat)
    if repeat < 1 or repeat > ops.CMC_SHOT_MAX_REPEAT:
        raise ValueError("cmc_single_shot: repeat must be 1 .. %d, got %d" % (ops.CMC_SHOT_MAX_REPEAT, repeat))
    if topk < 1:
        raise ValueError("cmc_single_shot: topk must be at least 1, got %d" % topk)
    shape = tuple(distmat.shape) if torch.is_tensor(distmat) else np.shape(distmat)
    if len(shape) != 2:
        raise ValueError("distmat must be a [query, gallery] matrix, got shape %s" % (shape,))
    m, n = shape
    ids = _fill_defaults(m, n, query_ids, gallery_ids, query_cams, gallery_cams)
    names = ("query_ids", "gallery_ids", "query_cams", "gallery_cams")
    host = torch.device("cpu")
    ids = [v if torch.is_tensor(v) and v.is_cuda else _ids_on_device(v, nm, k, host) for v, nm, k in zip(ids, names, (m, n, m, n))]
    d = _dist_on_device(distmat)
    qi, gi, qc, gc = (_ids_on_device(v, nm, k, d.device) for v, nm, k in zip(ids, names, (m, n, m, n)))
    res = ops.cmc_shot(d, qi, gi, qc, gc, topk=topk, separate_camera_set=bool(separate_camera_set), repeat=repeat,
                       random_state=random_state, chunk=chunk, debug=debug)
    if res["num_valid"] == 0:
        raise RuntimeError("No valid query")
    w = 1.0 if first_match_break else 1.0 / repeat
    curve = (res["hist"] * w).cumsum() / res["num_valid"]
    return (curve, res) if debug else curve
