"""Drop-in `reid.evaluation_metrics` (FD/reid/evaluation_metrics/__init__.py): the reference's ranking.py is the same file in
both trees, so `cmc` and `mean_ap` are clustercontrast.evaluation_metrics' (scored on the MI355X); `accuracy` stays the
reference's and resolves when its tree sits behind this one on sys.path; without one it is the restatement in `_accuracy.py`."""
from __future__ import absolute_import

from rg_hip.overlay import extend as _rg_extend  # noqa: E402
_rg_extend(globals())                      # see rg_hip/overlay.py

from .ranking import cmc, mean_ap, cmc_single_shot  # noqa: E402

__all__ = ['accuracy', 'cmc', 'mean_ap', 'cmc_single_shot']

try:
    from .classification import accuracy  # noqa: E402,F401
except ImportError:                        # no reference tree behind this one: the local restatement
    from ._accuracy import accuracy  # noqa: E402,F401
