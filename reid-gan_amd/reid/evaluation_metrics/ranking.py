"""FD/reid/evaluation_metrics/ranking.py is CC/clustercontrast/evaluation_metrics/ranking.py: one implementation serves both."""
from __future__ import absolute_import

from clustercontrast.evaluation_metrics.ranking import cmc, mean_ap, cmc_single_shot  # noqa: F401

__all__ = ['cmc', 'mean_ap', 'cmc_single_shot']
