"""Drop-in `clustercontrast.evaluation_metrics` (CC/clustercontrast/evaluation_metrics/__init__.py): `cmc` and `mean_ap`
score on the MI355X (ranking.py); `accuracy` (classification.py, host code that no loop here calls) stays the reference's
and resolves when its tree sits behind this one on sys.path."""
from __future__ import absolute_import

from rg_hip.overlay import extend as _rg_extend  # noqa: E402
_rg_extend(globals())                      # see rg_hip/overlay.py: reference-only sub-modules (classification) stay importable

from .ranking import cmc, mean_ap, cmc_single_shot  # noqa: E402

__all__ = ['cmc', 'mean_ap', 'cmc_single_shot']

try:
    from .classification import accuracy  # noqa: E402,F401
    __all__.insert(0, 'accuracy')
except ImportError:                        # no reference tree behind this one
    pass
