"""Generates tests/golden/reference_bank.npz by running the REFERENCE's own identity samplers (build container only):

  * CC/clustercontrast/utils/data/sampler.py  `RandomMultipleGallerySampler` (:47-107) and `RandomMultipleGallerySamplerNoCam`
    (:110-155), that ONE file loaded by path — it needs only torch and numpy.

Nothing from the reference is copied: the file stores, per toy data set of cases_bank.py, sampler and epoch, the index list the
reference's sampler yields under the case's seeds, and its `len()`.  Two consecutive epochs are drawn without re-seeding in
between, so the fixture also pins how much of each generator one epoch consumes.

Usage:  python tests/golden/make_golden_bank.py [path of the reference's cluster-contrast tree]
"""
from __future__ import absolute_import, print_function

import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
from tests.golden import cases_bank as C  # noqa: E402

CC = sys.argv[1] if len(sys.argv) > 1 else "/root/reference/cluster-contrast-reid-main"


def load_reference_sampler():
    spec = importlib.util.spec_from_file_location("cc_ref_sampler", CC + "/clustercontrast/utils/data/sampler.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    # the reference calls `super().__init__(data_source)`; torch >= 2.2's Sampler takes no argument any more.  In this
    # process only, give the base class the constructor the reference was written against (it stored nothing).
    mod.Sampler.__init__ = lambda self, data_source=None: None
    return mod


def main():
    R = load_reference_sampler()
    out = {}
    for name in C.CASES:
        entries = C.make_entries(name)
        for sampler in C.SAMPLERS:
            s = getattr(R, sampler)(entries, C.NUM_INSTANCES)
            out["%s_%s_len" % (name, sampler)] = np.int64(len(s))
            C.seed_all(name)
            for epoch in range(2):
                out[C.key(name, sampler, epoch)] = np.asarray(list(iter(s)), dtype=np.int64)
            print("case %s %s: %d entries, len %d, epochs of %d and %d indices" % (
                name, sampler, len(entries), len(s), len(out[C.key(name, sampler, 0)]), len(out[C.key(name, sampler, 1)])))
    path = os.path.join(HERE, "reference_bank.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
