"""Data derived from weights — (r,s)-major filter copies, fp8 filters, BatchNorm folds — is cached under a key of the weights it
was made from.  This module states the key, the rule for refreshing such a cache while a network program is being captured
(rg_hip.netgraph), and which filters get an (r,s)-major copy; rg_hip.nn and rg_hip.lowp hold the caches themselves.
"""
from __future__ import absolute_import

from . import ops


class _NoArena(object):
    epoch = 0


def weight_key(*tensors):
    """per tensor (arena epoch, version, address): the fused optimizers write parameters behind torch's version counters and bump
    their arena's epoch instead; the address changes with load_state_dict / .to()"""
    return tuple([(getattr(t, "_rg_arena", _NoArena).epoch, t._version, t.data_ptr()) for t in tensors])


def krsc_wanted(shape):
    """does a [K][C][KH][KW] filter tensor get an (r,s)-major copy (the kernels that read their filters tap by tap)"""
    return shape[2] * shape[3] > 1 and shape[1] % 4 == 0


class Stamp(object):
    """The weight_key a cached derivation was last refreshed for.  Inside a capture a refresh is recorded, not run (and its result
    lives in the capture's pool): every check is stale there, so the refresh becomes a node of the program, and nothing is
    stamped, so eager code after the capture — the fallback of a capture that FAILED included — refreshes for real."""
    __slots__ = ("key",)

    def __init__(self):
        self.key = None

    def stale(self, key):
        return self.key != key or ops.CAPTURING[0] > 0

    def set(self, key):
        self.key = None if ops.CAPTURING[0] else key


class GroupStamp(object):
    """ONE launch refreshes every member of a group and stamps them all.  Eagerly it is due when the asking member is stale (after
    an optimizer step every member is); inside a capture once per captured program (ops.CAPTURE_GEN)."""
    __slots__ = ("gen",)

    def __init__(self):
        self.gen = -1

    def stale(self, member, key):
        if ops.CAPTURING[0]:
            return self.gen != ops.CAPTURE_GEN[0]
        return member.key != key

    def set(self, members, keys):
        self.gen = ops.CAPTURE_GEN[0]
        for m, k in zip(members, keys):
            m.set(k)
