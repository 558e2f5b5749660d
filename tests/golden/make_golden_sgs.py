"""Generates tests/golden/reference_sgs.npz by running the REFERENCE's own `cmc(single_gallery_shot=True)` (build container
only; /root/reference does not exist on the GPU box):

  * FD-GAN-master/reid/evaluation_metrics/ranking.py  `cmc` (:18-79), loaded by file path

with placeholder parent packages whose `utils.to_numpy` is numpy's `asarray` (the recipe of make_golden_eval.py).  The
reference's `_unique_sample` spells the mask's dtype `np.bool`, which numpy 2 no longer has: the maker provides that alias for
the duration of the run.  Nothing from the reference is copied: the file stores the inputs of the one case that
reference_eval.npz does not hold, and per case, configuration and seed the reference's curve at topk = 20 and numpy's global
generator state after the call.  Every row is asserted tie-free (the reference's argsort is an unstable quicksort).

Usage:  python tests/golden/make_golden_sgs.py
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
from tests.golden import cases_eval as CE  # noqa: E402
from tests.golden import cases_sgs as C  # noqa: E402

FD = "/root/reference/FD-GAN-master"


def load_reference_ranking():
    root = types.ModuleType("fd_ref_sgs")
    root.__path__ = [FD + "/reid"]
    utils = types.ModuleType("fd_ref_sgs.utils")
    utils.to_numpy = np.asarray
    metrics = types.ModuleType("fd_ref_sgs.evaluation_metrics")
    metrics.__path__ = [FD + "/reid/evaluation_metrics"]
    sys.modules.update({"fd_ref_sgs": root, "fd_ref_sgs.utils": utils, "fd_ref_sgs.evaluation_metrics": metrics})
    name = "fd_ref_sgs.evaluation_metrics.ranking"
    spec = importlib.util.spec_from_file_location(name, FD + "/reid/evaluation_metrics/ranking.py")
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def main():
    R = load_reference_ranking()
    if not hasattr(np, "bool"):
        np.bool = bool
    out = {}
    for name in C.CASES:
        d, qid, gid, qcam, gcam = C.make_inputs(name)
        assert CE.rows_tie_free(d), "%s has a row with two equal distances" % name
        if name in C.OWN:
            for k, v in zip(("dist", "qid", "gid", "qcam", "gcam"), (d, qid, gid, qcam, gcam)):
                out["%s_%s" % (name, k)] = v
        sizes = np.bincount(gid - gid.min())
        line = "case %s: Q=%d G=%d ids %d largest segment %d" % (name, d.shape[0], d.shape[1], len(np.unique(gid)), sizes.max())
        for cfg, kw in C.CONFIGS.items():
            for seed in C.SEEDS:
                np.random.seed(seed)
                curve = R.cmc(d, qid, gid, qcam, gcam, topk=C.TOPK, single_gallery_shot=True, **kw)
                state = np.random.get_state()
                out[C.key(name, cfg, seed, "curve")] = np.asarray(curve, dtype=np.float64)
                out[C.key(name, cfg, seed, "key")] = np.asarray(state[1], dtype=np.uint32)
                out[C.key(name, cfg, seed, "pos")] = np.int64(state[2])
            line += ", %s top-1 %.4f" % (cfg, curve[0])
        print(line)
    path = os.path.join(HERE, "reference_sgs.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
