"""Host model of FD-GAN stage I's input pipeline on the raw image bank (csrc/databank.hip: rg_bank_fd_crop_batch), in plain
integer numpy, restated from the description of PIL's bilinear resampling and written apart from the code under test:

  * `coeffs(n, m)`      the (lo, cnt, k) of one axis with input length n and output length m, one output index at a time;
  * `resample(a, H, W)` the two passes (horizontal first, a uint8 intermediate) of an HWC uint8 array;
  * `fd_crop_model`     the whole kernel: crop -> two passes -> the eraser's patch -> flip -> the byte table;
  * `crop_draw`         RandomSizedRectCrop's draws on Python's `random`;
  * `item` / `pair_list`  one loader item and the sampler's pairs in the reference's order.

`defect=` plants one known mistake (tests/test_fd_stage1_cpu.py shows that each is told apart):
  'vertical_first'    the vertical pass runs before the horizontal one
  'fp32_coeffs'       the weights are computed in float32
  'no_half'           the accumulator starts at 0 instead of 2^21
  'round_bounds'      lo / hi are rounded instead of truncated
  'erase_after_flip'  the patch is pasted in post-flip coordinates
  'origin_ignored'    the crop is taken at (0, 0)
"""
import math
import random

import numpy as np
import torch

from tests.fd_pairs_hostmodel import REID_MEAN, REID_STD, bank_lut, erase_draw, pair_list  # noqa: F401  (shared with stage II)

BITS = 22


def coeffs(n, m, defect=None):
    """[(lo, cnt, [k_0 .. k_cnt-1])] for the m output indices of an axis of input length n"""
    f = np.float32 if defect == "fp32_coeffs" else float          # Python's float is the C double
    scale = f(n) / f(m)
    fs = max(scale, f(1.0))
    support = fs
    inv = f(1.0) / fs
    out = []
    for j in range(m):
        centre = (f(j) + f(0.5)) * scale
        if defect == "round_bounds":
            lo, hi = int(round(float(centre - support + f(0.5)))), int(round(float(centre + support + f(0.5))))
        else:
            lo, hi = int(centre - support + f(0.5)), int(centre + support + f(0.5))
        lo, hi = max(lo, 0), min(hi, n)
        cnt = hi - lo
        w, ww = [], f(0.0)
        for x in range(cnt):
            a = abs((f(x + lo) - centre + f(0.5)) * inv)
            wx = f(1.0) - a if a < 1 else f(0.0)
            w.append(wx)
            ww = ww + wx
        out.append((lo, cnt, [int(f(0.5) + (wx / ww) * f(1 << BITS)) for wx in w]))
    return out


def _pass_rows(a, m, defect=None):
    """resample axis 1 of a uint8 array [rows, n, C] to length m"""
    rows, n, C = a.shape
    out = np.empty((rows, m, C), dtype=np.uint8)
    half = 0 if defect == "no_half" else 1 << (BITS - 1)
    src = a.astype(np.int64)
    for j, (lo, cnt, k) in enumerate(coeffs(n, m, defect)):
        acc = np.full((rows, C), half, dtype=np.int64)
        for x in range(cnt):
            acc += src[:, lo + x, :] * k[x]
        out[:, j, :] = np.clip(acc >> BITS, 0, 255)
    return out


def resample(a, H, W, defect=None):
    """HWC uint8 [h, w, 3] -> [H, W, 3] as Image.fromarray(a).resize((W, H), BILINEAR)"""
    a = np.ascontiguousarray(a, dtype=np.uint8)
    if defect == "vertical_first":
        t = _pass_rows(a.transpose(1, 0, 2), H, defect).transpose(1, 0, 2)
        return _pass_rows(t, W, defect)
    t = _pass_rows(a, W, defect)                                           # horizontal: [h, W, 3], uint8
    return _pass_rows(t.transpose(1, 0, 2), H, defect).transpose(1, 0, 2)  # vertical over the intermediate


def crop_bytes(img, draw, H, W, defect=None):
    """the bytes [H, W, 3] of one draw (x1, y1, w, h, flip, er0, ec0, eh, ew, rgb) on the HWC image: crop, resample, patch, flip"""
    x1, y1, w, h, flip, er0, ec0, eh, ew, rgb = [int(v) for v in draw]
    if defect == "origin_ignored":
        x1 = y1 = 0
    out = resample(img[y1:y1 + h, x1:x1 + w], H, W, defect).copy()
    colour = [(rgb >> (8 * c)) & 255 for c in range(3)]
    if defect == "erase_after_flip":
        if flip:
            out = out[:, ::-1].copy()
        if eh > 0:
            out[er0:er0 + eh, ec0:ec0 + ew] = colour
        return out
    if eh > 0:
        out[er0:er0 + eh, ec0:ec0 + ew] = colour
    return out[:, ::-1].copy() if flip else out


def fd_crop_model(images, rows, draws, lut, H, W, defect=None):
    """fp32 [N, 3, H, W]: what rg_bank_fd_crop_batch writes for the bank rows `rows` and the draws [N][10] (as crop_bytes)"""
    out = np.empty((len(rows), 3, H, W), dtype=np.float32)
    for n, (m, d) in enumerate(zip(rows, draws)):
        b = crop_bytes(images[int(m)], d, H, W, defect)
        for c in range(3):
            out[n, c] = lut[c][b[:, :, c]]
    return out


def crop_draw(W_src, H_src):
    """RandomSizedRectCrop's draws on an image W_src wide and H_src high -> (x1, y1, w, h); the whole image after ten misses"""
    for _ in range(10):
        area = W_src * H_src
        target = random.uniform(0.64, 1.0) * area
        ratio = random.uniform(2, 3)
        h = int(round(math.sqrt(target * ratio)))
        w = int(round(math.sqrt(target / ratio)))
        if w <= W_src and h <= H_src:
            x1 = random.randint(0, W_src - w)
            y1 = random.randint(0, H_src - h)
            return x1, y1, w, h
    return 0, 0, W_src, H_src


def item_draw(img, H, W, generator=None):
    """one item's draws in the reference's num_workers=0 order: crop, eraser, flip -> the draw row of crop_bytes"""
    x1, y1, w, h = crop_draw(img.shape[1], img.shape[0])
    rect = erase_draw(H, W)
    flip = 1 if float(torch.rand(1, generator=generator)) < 0.5 else 0
    er0, ec0, eh, ew, rgb = (0, 0, 0, 0, 0) if rect is None else rect
    return (x1, y1, w, h, flip, er0, ec0, eh, ew, rgb)


def item(images, index, H, W, lut, defect=None):
    """fp32 [3, H, W] of data-set item `index` (= bank row here)"""
    return fd_crop_model(images, [index], [item_draw(images[index], H, W)], lut, H, W, defect)[0]
