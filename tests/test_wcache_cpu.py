"""rg_hip/wcache.py on CPU tensors: the key of a weight-derived cache, the refresh rule while a network program is being captured, the
once-per-capture rule of a group, and which filters get an (r,s)-major copy.  The refresh functions are stubs that count."""
import torch

from rg_hip import ops, wcache


class _Arena(object):
    epoch = 0


def test_weight_key_follows_version_arena_epoch_and_address():
    w, b = torch.zeros(4, 3), torch.zeros(4)
    k0 = wcache.weight_key(w, b)
    assert len(k0) == 2 and k0 == wcache.weight_key(w, b)
    assert k0[0] == (0, w._version, w.data_ptr()) and k0[1] == (0, b._version, b.data_ptr())
    w.add_(1)
    k1 = wcache.weight_key(w, b)
    assert k1 != k0 and k1[1] == k0[1] and k1 == wcache.weight_key(w, b)
    w._rg_arena = _Arena()
    assert wcache.weight_key(w, b) == k1               # a fresh arena's epoch is the 0 of "no arena"
    w._rg_arena.epoch += 1
    k2 = wcache.weight_key(w, b)
    assert k2 != k1 and k2[0][0] == 1 and k2 == wcache.weight_key(w, b)
    keep = w.data                                      # keeps the old storage alive: the new one cannot land on its address
    w.data = torch.zeros(4, 3)
    k3 = wcache.weight_key(w, b)
    assert k3 != k2 and k3[0][2] == w.data_ptr() != keep.data_ptr() and k3 == wcache.weight_key(w, b)


class _Cache(object):
    """a single cache driven the way nn.conv._KrscCache._krsc and lowp.F8Layer.weights drive theirs"""

    def __init__(self, w):
        self.w, self.stamp, self.refreshes = w, wcache.Stamp(), 0

    def get(self):
        key = wcache.weight_key(self.w)
        if self.stamp.stale(key):
            self.refreshes += 1
            self.stamp.set(key)
        return self.refreshes


def test_stamp_is_stale_and_stays_unstamped_while_capturing():
    c = _Cache(torch.zeros(4, 3))
    assert [c.get(), c.get()] == [1, 1]                # eager: refreshed once, then a hit
    c.w.add_(1)
    assert [c.get(), c.get()] == [2, 2]
    ops.CAPTURING[0] += 1
    try:
        assert c.stamp.key == wcache.weight_key(c.w) and c.stamp.stale(c.stamp.key)      # an equal key is still stale
        assert [c.get(), c.get()] == [3, 4]            # every use inside the capture records a refresh ...
        assert c.stamp.key is None                     # ... and stamps nothing
    finally:
        ops.CAPTURING[0] -= 1
    assert c.stamp.stale(wcache.weight_key(c.w))       # so the first eager check afterwards is stale again
    assert [c.get(), c.get()] == [5, 5]


class _Group(object):
    """a group driven the way nn.conv.KrscGroup.get / refresh drive theirs: one refresh serves (and stamps) every member"""

    def __init__(self, ws):
        self.ws, self.stamps, self.stamp, self.refreshes = ws, [wcache.Stamp() for _ in ws], wcache.GroupStamp(), 0

    def get(self, i):
        if self.stamp.stale(self.stamps[i], wcache.weight_key(self.ws[i])):
            self.refreshes += 1
            self.stamp.set(self.stamps, [wcache.weight_key(w) for w in self.ws])
        return self.refreshes


def test_group_refreshes_once_per_capture_and_eagerly_only_for_a_changed_member():
    g = _Group([torch.zeros(4, 3), torch.zeros(2, 3)])
    assert [g.get(0), g.get(1), g.get(0)] == [1, 1, 1]                 # the first member's refresh served both
    g.ws[1].add_(1)
    assert [g.get(0), g.get(1), g.get(1)] == [1, 2, 2]                 # eager: only the member whose key changed asks for one
    for expect in (3, 4):                                              # two captures (netgraph._capture_mode bumps both counters)
        ops.CAPTURING[0] += 1
        ops.CAPTURE_GEN[0] += 1                                        # (only ever counts up: it is not put back)
        try:
            assert [g.get(0), g.get(1), g.get(0)] == [expect] * 3      # two members, one CAPTURE_GEN: one refresh
            assert all(s.key is None for s in g.stamps)
        finally:
            ops.CAPTURING[0] -= 1
    assert [g.get(1), g.get(0), g.get(1)] == [5, 5, 5]                 # eager after the captures: stale once, for real


def test_krsc_wanted():
    K = 16
    assert [wcache.krsc_wanted(s) for s in ((K, 8, 1, 1), (K, 6, 3, 3), (K, 8, 3, 3))] == [False, False, True]
    assert wcache.krsc_wanted(torch.zeros(K, 4, 1, 3).shape) and not wcache.krsc_wanted(torch.Size((K, 3, 7, 7)))
