"""Running mean of a logged quantity with the attribute interface the trainers' progress lines read
(`.val`, `.avg`, `.sum`, `.count`, `reset()`, `update(value, n)`; CC/clustercontrast/utils/meters.py).  Host-side
bookkeeping only.  The class lives in rg_hip/hostloop.py, next to the loops that use it."""
from __future__ import absolute_import

from rg_hip.hostloop import AverageMeter  # noqa: F401
