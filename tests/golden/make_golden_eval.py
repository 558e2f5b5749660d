"""Generates tests/golden/reference_eval.npz by running the REFERENCE's own scoring functions (build container only;
/root/reference does not exist on the GPU box):

  * CC/clustercontrast/evaluation_metrics/ranking.py  `cmc` (:18-79) and `mean_ap` (:82-115), loaded by file path

The package `__init__` files above it import torchvision, which is not installed in this image, so placeholder parent
packages are registered (the recipe of make_golden_rerank.py) whose `utils.to_numpy` is numpy's `asarray`.  Nothing from the
reference is copied: the file stores the inputs and the reference's outputs.

For the tie-free cases every row's distances are asserted distinct (the reference's argsort is an unstable quicksort, which
then has no say) and the four CMC configurations without sampling are stored; the quantised case stores mAP only.

Usage:  python tests/golden/make_golden_eval.py
"""
from __future__ import absolute_import, print_function

import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
from tests.golden import cases_eval as C  # noqa: E402

CC = "/root/reference/cluster-contrast-reid-main"


def load_reference_ranking():
    root = types.ModuleType("cc_ref_eval")
    root.__path__ = [CC + "/clustercontrast"]
    utils = types.ModuleType("cc_ref_eval.utils")
    utils.to_numpy = np.asarray
    metrics = types.ModuleType("cc_ref_eval.evaluation_metrics")
    metrics.__path__ = [CC + "/clustercontrast/evaluation_metrics"]
    sys.modules.update({"cc_ref_eval": root, "cc_ref_eval.utils": utils, "cc_ref_eval.evaluation_metrics": metrics})
    name = "cc_ref_eval.evaluation_metrics.ranking"
    spec = importlib.util.spec_from_file_location(name, CC + "/clustercontrast/evaluation_metrics/ranking.py")
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def main():
    R = load_reference_ranking()
    out = {}
    for name in C.CASES:
        d, qid, gid, qcam, gcam = C.make_inputs(name)
        for k, v in zip(("dist", "qid", "gid", "qcam", "gcam"), (d, qid, gid, qcam, gcam)):
            out["%s_%s" % (name, k)] = v
        out[name + "_map"] = np.float64(R.mean_ap(d, qid, gid, qcam, gcam))
        line = "case %s: Q=%d G=%d mAP %.6f" % (name, d.shape[0], d.shape[1], out[name + "_map"])
        if name in C.TIE_FREE:
            assert C.rows_tie_free(d), name
            for cfg, kw in C.CMC_CONFIGS.items():
                out["%s_cmc_%s" % (name, cfg)] = R.cmc(d, qid, gid, qcam, gcam, topk=C.TOPK, single_gallery_shot=False, **kw)
                line += ", %s top-1 %.4f" % (cfg, out["%s_cmc_%s" % (name, cfg)][0])
        else:
            line += ", %d distinct distances" % len(np.unique(d))
        print(line)
    path = os.path.join(HERE, "reference_eval.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
