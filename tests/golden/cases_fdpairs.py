"""The toy data set shared by make_golden_fdpairs.py (reference side) and the FD-GAN pair-loader tests (this build's side).

Ten images of four identities whose pids have 1, 2 and 3 digits (the reference sorts the pid column as STRINGS), originals partly at
the map size 64x32 (RectScale returns them as they are) and partly 80x40 (RectScale resamples them), one landmark file of J = 10
lines per image with fractional, negative and border values.  The generator writes the images as JPEG and stores what PIL decodes;
the tests write those decoded arrays back losslessly.
"""
import random

import numpy as np
import torch

H, W, J = 64, 32, 10
MAP_STRIDE = 2
PIDS = [2, 2, 2, 10, 10, 100, 100, 100, 7, 7]
CAMS = [0, 1, 0, 2, 0, 1, 1, 3, 0, 2]
SIZES = [(64, 32), (80, 40), (80, 40), (64, 32), (80, 40), (80, 40), (64, 32), (80, 40), (64, 32), (80, 40)]
NAMES = ["%08d_%02d_%04d.jpg" % (p, c, k) for k, (p, c) in enumerate(zip(PIDS, CAMS))]
TRAINVAL = [(n, p, c) for n, p, c in zip(NAMES, PIDS, CAMS)]
PID_IMGS = {}
for _n, _p in zip(NAMES, PIDS):
    PID_IMGS.setdefault(_p, []).append(_n)

RATIOS = (1, 3)
SAMPLER_SEED = 31
ERASE_SEED, ERASE_CALLS = 5, 40
AUGS = ("no", "erase", "gauss")
ITEM_PAIRS = {"no": 2, "erase": 1, "gauss": 1}       # the first pairs of epoch 0 at ratio 3 are the stored items
ITEM_SEEDS = {"no": 41, "erase": 42, "gauss": 43}


def source_image(k):
    """uint8 [h, w, 3]: blocks and ramps that tell images, channels, rows and columns apart and survive JPEG recognisably"""
    h, w = SIZES[k]
    g = np.random.RandomState(100 + k)
    y, x = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    blocks = g.randint(0, 256, size=(h // 16 + 1, w // 16 + 1, 3))[y // 16, x // 16]
    ramp = np.stack([2 * y + k * 7, 3 * x + 40, y + x + 11 * k], axis=2)
    return np.clip(blocks * 0.5 + ramp * 0.5, 0, 255).astype(np.uint8)


def landmark_lines(k):
    """the text of image k's landmark file: 'row col' per joint in the ORIGINAL image's pixels"""
    h, w = SIZES[k]
    g = np.random.RandomState(200 + k)
    rows = [[g.uniform(0, h - 1), g.uniform(0, w - 1)] for _ in range(J)]
    rows[0] = [0.0, 0.0]                                   # the corners
    rows[1] = [h - 1, w - 1]
    rows[2] = [-1.0, -1.0]                                 # not detected
    rows[3] = [-0.4, 3.7] if k % 2 else [5.25, -7.0]       # int() truncates -0.32 to 0; a negative column alone
    rows[4] = [h - 0.01, w / 2.0] if k % 3 == 0 else rows[4]      # the last row after scaling, by a hair
    rows[5] = [-3.5, -0.2]
    rows[6] = [h / 2.0 + 0.5, w - 1.0]                     # on the right border
    return ["%r %r" % (float(r), float(c)) for r, c in rows]


def seed_sampler(ratio):
    np.random.seed(SAMPLER_SEED + ratio)


def seed_items(aug):
    random.seed(ITEM_SEEDS[aug])
    torch.manual_seed(ITEM_SEEDS[aug] + 1000)
