"""Toy data sets shared by make_golden_bank.py (reference side) and tests/test_bank_loader_cpu.py (this build's samplers).

Each is a list of (fname, pid, camid) triples in the order the samplers index it; every one holds entries with pid < 0
(unclustered samples, never drawn).  A case fixes the three generators the samplers draw from: torch's default generator,
Python's `random` and `numpy.random`.
"""
import random

import numpy as np
import torch

NUM_INSTANCES = 4
SAMPLERS = ("RandomMultipleGallerySampler", "RandomMultipleGallerySamplerNoCam")


def _entries(spec):
    """spec: [(pid, [camid per image])] -> triples, interleaved so that an identity's entries are not contiguous"""
    rows = [(pid, cam) for pid, cams in spec for cam in cams]
    order = np.random.RandomState(len(rows)).permutation(len(rows))
    return [("%04d_c%ds1_%06d.jpg" % (max(rows[k][0], 0), rows[k][1] + 1, i), rows[k][0], rows[k][1]) for i, k in enumerate(order)]


CASES = {
    # identities with a single image (the anchor alone), next to ordinary ones
    "single": dict(seed=11, spec=[(0, [0]), (1, [0, 1, 2, 0, 1]), (2, [3]), (-1, [0, 1, 2]), (3, [0, 1, 2, 3, 4, 5]), (4, [2]),
                                  (5, [1, 1, 0])]),
    # identities seen by one camera only: companions come from the identity's other entries
    "onecam": dict(seed=12, spec=[(0, [2, 2, 2, 2, 2, 2]), (1, [0, 0]), (-1, [4]), (2, [1, 1, 1]), (3, [5, 5, 5, 5]), (4, [0, 3, 0, 3]),
                                  (-1, [1, 1])]),
    # fewer other-camera images than num_instances: drawn with replacement
    "fewcam": dict(seed=13, spec=[(0, [0, 0, 0, 1]), (1, [0, 1]), (2, [0, 0, 1, 1, 2]), (-1, [0, 0]), (3, [4, 4, 4, 4, 4, 2, 3]),
                                  (7, [1, 0, 0, 0, 0, 0, 0, 0])]),
}


def make_entries(name):
    return _entries(CASES[name]["spec"])


def seed_all(name, epoch=0):
    s = CASES[name]["seed"] + 100 * epoch
    torch.manual_seed(s)
    random.seed(s + 1)
    np.random.seed(s + 2)


def key(name, sampler, epoch):
    return "%s_%s_e%d" % (name, sampler, epoch)
