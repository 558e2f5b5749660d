from __future__ import absolute_import

from rg_hip.overlay import extend as _rg_extend  # noqa: E402
_rg_extend(globals(), run_init=True)       # see rg_hip/overlay.py: the reference tree may sit behind this one on sys.path
from .device_pipeline import PoseMapGenerator, flip_images  # noqa: F401,E402
from .device_pairs import (DeviceFDTestLoader, DevicePairLoader, FDRandomErase, RandomPairSampler, get_data_device,  # noqa: F401,E402
                           read_landmarks, stage_landmarks)
from .device_stage1 import DeviceStage1Loader, FDRandomSizedRectCrop, get_data_stage1_device  # noqa: F401,E402
