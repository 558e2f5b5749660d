"""The identity samplers of CC/clustercontrast/utils/data/sampler.py (RandomMultipleGallerySampler :47-107 and its NoCam form
:110-155) as plain host iterables that need no reference tree: same constructor, same `__len__`, and the same sequence of calls
into the three generators the reference uses — one `torch.randperm` over the identities, then per identity one Python
`random.choice` for the anchor and at most one `numpy.random.choice` for its companions — so a run seeded on all three yields the
reference's index list.  (`clustercontrast.utils.data.sampler` still resolves to the reference's file through the overlay.)

Per identity, in the permuted order:
  anchor      random.choice of the identity's entries
  companions  num_instances - 1 draws by numpy.random.choice from the POSITIONS (within the identity's entry list) of
              - with cameras: the entries seen by another camera than the anchor's; if there are none,
              - the entries other than the anchor itself; if there are none either, the identity contributes the anchor alone;
              without replacement when there are at least num_instances candidates, with replacement otherwise.
Entries with pid < 0 (unclustered) are never drawn.  `__len__` is identities x num_instances, an upper bound as in the reference.
"""
from __future__ import absolute_import

import random

import numpy as np
import torch


class _IdentitySampler(object):
    use_cameras = True

    def __init__(self, data_source, num_instances=4):
        self.data_source = data_source
        self.num_instances = num_instances
        self.rows = {}                                   # pid -> [entry index], in data_source order (dicts keep insertion order)
        self.cams = {}                                   # pid -> [camera of that entry]
        for i, (_, pid, cam) in enumerate(data_source):
            if pid < 0:
                continue
            self.rows.setdefault(pid, []).append(i)
            self.cams.setdefault(pid, []).append(cam)
        self.pids = list(self.rows)
        self.num_samples = len(self.pids)

    def __len__(self):
        return self.num_samples * self.num_instances

    def _companions(self, positions):
        k = self.num_instances
        return np.random.choice(positions, size=k - 1, replace=len(positions) < k)

    def __iter__(self):
        out = []
        for p in torch.randperm(len(self.pids)).tolist():
            pid = self.pids[p]
            rows = self.rows[pid]
            anchor = random.choice(rows)
            out.append(anchor)
            positions = []
            if self.use_cameras:
                cam = self.data_source[anchor][2]
                positions = [k for k, c in enumerate(self.cams[pid]) if c != cam]
            if not positions:
                positions = [k for k, r in enumerate(rows) if r != anchor]
            if not positions:
                continue
            out.extend(rows[k] for k in self._companions(positions))
        return iter(out)


class RandomMultipleGallerySampler(_IdentitySampler):
    use_cameras = True


class RandomMultipleGallerySamplerNoCam(_IdentitySampler):
    use_cameras = False
