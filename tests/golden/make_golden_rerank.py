"""Generates tests/golden/reference_rerank.npz by running the REFERENCE's own re-ranking functions (build container only;
/root/reference does not exist on the GPU box):

  * CC/clustercontrast/utils/rerank.py        `re_ranking` (:32-99), imported as it is (pure numpy)
  * CC/clustercontrast/utils/faiss_rerank.py  `compute_jaccard_distance` (:31-127)

The second module imports `faiss` and `.faiss_utils` at import time; faiss is not installed in this image, so placeholder
modules are registered for those imports whose `search_raw_array_pytorch` is an fp64 brute-force L2 search (distance
ascending, ties by lower index) — the recipe make_golden_datagen.py uses for torchvision.  Nothing from the reference is
copied: the file stores inputs (the features) and the reference's outputs.

For every case of cases_rerank.py the seed is the one of `SEEDS` with the widest cut gap (the smaller of the gap under the
squared L2 distance and the gap under re_ranking's normalised distance); the gap condition (>= GAP for both) is asserted.
The Jaccard matrices are bit-symmetric (asserted) and stored as upper triangles.

Usage:  python tests/golden/make_golden_rerank.py
"""
from __future__ import absolute_import, print_function

import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
from tests.golden import cases_rerank as C  # noqa: E402

CC = "/root/reference/cluster-contrast-reid-main"


def _l2_search(res, xb, xq, k, *a, **kw):
    d = torch.from_numpy(C.sq_l2(xb.cpu().numpy()))
    order = torch.from_numpy(np.argsort(d.numpy(), axis=1, kind="stable")[:, :k])
    return torch.gather(d, 1, order).float(), order


def _placeholders():
    faiss = types.ModuleType("faiss")
    faiss.get_num_gpus = lambda: 0

    class StandardGpuResources(object):
        def setDefaultNullStreamAllDevices(self):
            pass
    faiss.StandardGpuResources = StandardGpuResources
    sys.modules["faiss"] = faiss
    pkg = types.ModuleType("cc_ref_utils")
    pkg.__path__ = [CC + "/clustercontrast/utils"]
    sys.modules["cc_ref_utils"] = pkg
    fu = types.ModuleType("cc_ref_utils.faiss_utils")
    fu.search_raw_array_pytorch = _l2_search
    fu.search_index_pytorch = fu.index_init_gpu = fu.index_init_cpu = None
    sys.modules["cc_ref_utils.faiss_utils"] = fu


def load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def gaps(x, k1, k2):
    return C.cut_gap(C.sq_l2(x), k1, k2), C.cut_gap(C.normalised_dist64(*C.euclid_inputs(x)), k1, k2)


def main():
    _placeholders()
    fr = load(CC + "/clustercontrast/utils/faiss_rerank.py", "cc_ref_utils.faiss_rerank")
    rr = load(CC + "/clustercontrast/utils/rerank.py", "cc_ref_utils.rerank")
    out = {}
    for name, cs in C.CASES.items():
        k1, k2 = cs["k1"], cs["k2"]
        shape = (cs["n_id"], cs["per"], cs["D"], cs["noise"])
        best = max(C.SEEDS, key=lambda s: min(gaps(C.make_features(*shape, seed=s), k1, k2)))
        x = C.make_features(*shape, seed=best)
        g_l2, g_rr = gaps(x, k1, k2)
        assert g_l2 >= C.GAP and g_rr >= C.GAP, (name, best, g_l2, g_rr)
        n = len(x)
        jac = fr.compute_jaccard_distance(torch.from_numpy(x), k1=k1, k2=k2, print_flag=False)
        assert jac.shape == (n, n) and jac.dtype == np.float32 and np.array_equal(jac, jac.T), name
        q_g, q_q, g_g = C.euclid_inputs(x)
        fin = rr.re_ranking(q_g, q_q, g_g, k1=k1, k2=k2, lambda_value=C.LAMBDA)
        assert fin.shape == q_g.shape and fin.dtype == np.float32, name
        out[name + "_x"] = x
        out[name + "_seed"] = np.int64(best)
        out[name + "_gaps"] = np.array([g_l2, g_rr])
        out[name + "_jaccard_upper"] = C.pack_upper(jac)
        out[name + "_final"] = fin
        line = "case %s: N=%d seed=%d gaps l2 %.2e rerank %.2e, support %d, diag max %.1e" % (
            name, n, best, g_l2, g_rr, int((jac < 1).sum()), float(np.abs(np.diag(jac)).max()))
        try:
            from sklearn.cluster import DBSCAN
            lab = DBSCAN(eps=C.DBSCAN_EPS, min_samples=C.DBSCAN_MIN_SAMPLES, metric="precomputed", n_jobs=1).fit_predict(jac)
            off = jac[~np.eye(n, dtype=bool)]
            out[name + "_dbscan"] = lab.astype(np.int32)
            line += ", DBSCAN %d clusters %d outliers, closest entry to eps %.3g" % (
                lab.max() + 1, int((lab < 0).sum()), float(np.abs(off - C.DBSCAN_EPS).min()))
        except ImportError:
            pass
        print(line)
    path = os.path.join(HERE, "reference_rerank.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
