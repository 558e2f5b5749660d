"""The toy data shared by make_golden_fdstage1.py (reference side) and the FD-GAN stage-I loader tests (this build's side).

Ten images of four identities at five sizes: 128x64 (the recipe's source), 150x70 (odd ratios), 64x64 (every box of
RandomSizedRectCrop is at least 72 high, so every draw falls back to the whole image, and the fallback's resize to 64x32 leaves
one axis as it is), 64x32 (a fallback is the identity at the item size) and 80x40.  The generator writes them as PNG (lossless:
what PIL decodes is `source_image(k)` itself, so the fixture stores only a checksum of them).
"""
import random

import numpy as np
import torch

H, W = 64, 32                                              # the item size of the Preprocessor runs
PIDS = [2, 2, 2, 10, 10, 100, 100, 100, 7, 7]
CAMS = [0, 1, 0, 2, 0, 1, 1, 3, 0, 2]
SIZES = [(128, 64), (150, 70), (64, 64), (64, 32), (80, 40), (80, 40), (64, 32), (150, 70), (64, 32), (80, 40)]   # (height, width)
NAMES = ["%08d_%02d_%04d.jpg" % (p, c, k) for k, (p, c) in enumerate(zip(PIDS, CAMS))]
TRAIN = [(n, p, c) for n, p, c in zip(NAMES, PIDS, CAMS)]

# box sequences of RandomSizedRectCrop: name -> (source height, source width, draws, seed)
BOXES = {"128x64": (128, 64, 240, 11), "150x70": (150, 70, 80, 12), "64x64": (64, 64, 12, 13), "256x128": (256, 128, 60, 14)}
# crop outputs: name -> (toy image, output height, output width, draws, how many are stored whole, seed)
CROPS = {"recipe": (0, 256, 128, 24, 2, 21), "down": (1, 64, 32, 40, 4, 22), "fallback": (2, 64, 32, 3, 1, 23)}
RATIO = 1
SAMPLER_SEED = 33
ITEM_SEED = 51
ITEM_PAIRS, ITEM_FULL = 8, 3                               # pairs run through the Preprocessor / pairs whose items are stored whole


def source_image(k):
    """uint8 [h, w, 3]: blocks, ramps and noise that tell images, channels, rows and columns apart"""
    h, w = SIZES[k]
    g = np.random.RandomState(300 + k)
    y, x = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    blocks = g.randint(0, 256, size=(h // 8 + 1, w // 8 + 1, 3))[y // 8, x // 8]
    ramp = np.stack([2 * y + k * 7, 3 * x + 40, y + x + 11 * k], axis=2)
    return np.clip(blocks * 0.5 + ramp * 0.4 + g.randint(0, 40, size=(h, w, 3)), 0, 255).astype(np.uint8)


def images_sum():
    return int(sum(int(source_image(k).astype(np.uint64).sum()) * (k + 1) for k in range(len(SIZES))))


def byte_sum(a):
    """position-weighted 64-bit sum of an array's bytes"""
    b = np.frombuffer(np.ascontiguousarray(a).tobytes(), dtype=np.uint8).astype(np.uint64)
    return np.uint64((b * (np.arange(b.size, dtype=np.uint64) % np.uint64(251) + np.uint64(1))).sum())


def seed_sampler():
    np.random.seed(SAMPLER_SEED)


def seed_items():
    random.seed(ITEM_SEED)
    torch.manual_seed(ITEM_SEED + 1000)
