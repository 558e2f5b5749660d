"""Model registry — mirrors CC/clustercontrast/models/__init__.py:6-59 for the ResNet family, the IBN-a ResNets (the
encoder of the reference's published cluster-contrast recipe) and the multi-part encoder `resnet_mp50` (the one its flagship script
builds); the two-branch (bip / bipd) variants registered there are outside the hot path, SURVEY §2 row 20.  Domain-specific
BatchNorm is no registered model but a conversion of one: `clustercontrast.models.dsbn` (convert_dsbn / convert_bn, as
examples/test.py --dsbn uses them) on the fused two-domain layer rg_hip.nn.DSBN2d / DSBN1d."""
from __future__ import absolute_import

from rg_hip.overlay import extend as _rg_extend  # noqa: E402
_rg_extend(globals(), run_init=False)       # see rg_hip/overlay.py: the reference tree may sit behind this one on sys.path


from .resnet import *  # noqa: F401,F403
from .resnet import resnet18, resnet34, resnet50, resnet101, resnet152
from .resnet_ibn import *  # noqa: F401,F403
from .resnet_ibn import resnet_ibn50a, resnet_ibn101a
from .resnet_mp import *  # noqa: F401,F403
from .resnet_mp import resnet_mp50

__factory = {
    'resnet18': resnet18,
    'resnet34': resnet34,
    'resnet50': resnet50,
    'resnet101': resnet101,
    'resnet152': resnet152,
    'resnet_ibn50a': resnet_ibn50a,
    'resnet_ibn101a': resnet_ibn101a,
    'resnet_mp50': resnet_mp50,
}


def names():
    return sorted(__factory.keys())


def create(name, *args, **kwargs):
    """create(name, pretrained=True, cut_at_pooling=False, num_features=0, norm=False, dropout=0, num_classes=0,
    pooling_type='avg') — CC/clustercontrast/models/__init__.py:26-59; 'resnet_mp50' takes num_proj and need_predictor in place
    of num_classes."""
    if name not in __factory:
        raise KeyError("Unknown model:", name)
    return __factory[name](*args, **kwargs)
