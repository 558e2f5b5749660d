"""The per-launch event profiler of the library."""
from __future__ import absolute_import

import ctypes

from ..lib import FAMILIES
from ._base import lib


# ------------------------------------------------------------------------------------------------
# profiler
# ------------------------------------------------------------------------------------------------
_PROFILING = [False]


def profile_enable(on=True):
    _PROFILING[0] = bool(on)
    lib.rg_profile_enable(int(on))


def check_not_profiling():
    """the per-launch event profiler records timing events on the launch stream: not capturable / meaningless under replay"""
    if _PROFILING[0]:
        raise RuntimeError("rg_hip: the launch profiler is on; switch it off (ops.profile_enable(False)) before capturing or "
                           "replaying a step graph")


def profile_reset():
    lib.rg_profile_reset()


def profile_collect():
    n =lib.rg_family_count()
    ms = (ctypes.c_double * n)()
    fl = (ctypes.c_double * n)()
    by = (ctypes.c_double * n)()
    calls = (ctypes.c_longlong * n)()
    lib.rg_profile_collect(ctypes.addressof(ms), ctypes.addressof(fl), ctypes.addressof(by), ctypes.addressof(calls))
    return {FAMILIES[i]: {"ms": ms[i], "flops": fl[i], "bytes": by[i], "calls": calls[i]} for i in range(n)}
