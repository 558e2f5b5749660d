"""Host model of FD-GAN stage II's pair pipeline (include/reidgan_hip.h: rg_bank_fd_image_batch, rg_bank_fd_pose_batch;
reid/utils/data/device_pairs.py), index by index in numpy and in the reference's draw order — TEST INFRASTRUCTURE ONLY.

    fd_image_model     rg_bank_fd_image_batch: paste (on bytes, through the table), flip, table look-up
    fd_pose_model      rg_bank_fd_pose_batch through oracle.ref_datagen.o_generate_pose_map (scipy) + flip
    erase_draw         RandomSizedEarser's draws and where the patch lands
    pair_list          RandomPairSampler's epoch
    item               one `_get_single_item_with_pose` from the RectScale planes and the landmark table
    ordered_batch      the test-time transform

`defect=` plants one wrong reading of the reference in an otherwise unchanged model; tests/test_fd_pairs_cpu.py shows that the
fixture (tests/golden/reference_fdpairs.npz, the reference's own outputs) tells every one of them from the model:
    'paste_at_x1y1'           the patch lands on the box it was sized from, not at (column pw, row ph)
    'rect_after_flip'         the patch's coordinates are taken in the flipped image
    'colour_after_normalize'  the patch holds colour / 255, written after Normalize
    'numeric_pid_order'       the sampler sorts the pids as numbers
    'partner_first'           the partner image is drawn before the eraser's draws and the origin's flip
    'tflip_before_partner'    the target's flip is drawn before the partner
"""
import math
import os.path as osp
import random

import numpy as np
import torch

from oracle import ref_datagen as OD
from tests.bank_hostmodel import REID_MEAN, REID_STD, bank_lut  # noqa: F401


def fd_image_model(bank, idx, params, lut, defect=None):
    """bank uint8 [M, H, W, 3]; params [N, 8] = (flip, -, -, er0, ec0, eh, ew, rgb) -> float32 [N, 3, H, W]"""
    M, H, W, _ = bank.shape
    N = len(idx)
    out = np.empty((N, 3, H, W), dtype=np.float32)
    for n in range(N):
        flip, _, _, er0, ec0, eh, ew, rgb = [int(v) for v in params[n]]
        m = int(idx[n])
        assert 0 <= m < M
        for c in range(3):
            byte = (rgb >> (8 * c)) & 255
            for y in range(H):
                for x in range(W):
                    xs = W - 1 - x if flip else x                       # the eraser runs before the flip
                    xr = x if defect == "rect_after_flip" else xs
                    if eh > 0 and er0 <= y < er0 + eh and ec0 <= xr < ec0 + ew:
                        out[n, c, y, x] = np.float32(byte) / np.float32(255) if defect == "colour_after_normalize" else lut[c][byte]
                    else:
                        out[n, c, y, x] = lut[c][bank[m][y][xs][c]]
    return out


def fd_pose_model(landmarks, idx, pose_params, H, W):
    """landmarks int [M, J, 2]; pose_params [N, 4] = (flip, sigma, erased joint or -1, -) -> float32 [N, J, H, W]"""
    landmarks = np.asarray(landmarks)
    out = []
    for n in range(len(idx)):
        flip, sigma, erased = [int(v) for v in pose_params[n][:3]]
        lm = landmarks[int(idx[n])].astype(np.int64).copy()
        for j in range(lm.shape[0]):
            if j == erased or not (0 <= lm[j, 0] < H and 0 <= lm[j, 1] < W):
                lm[j] = -1
        maps = OD.o_generate_pose_map(lm, H, W, "no", gauss_sigma=sigma)
        if flip:
            maps = np.flip(maps, 2)
        out.append(maps.astype(np.float32))
    return np.stack(out)


def erase_draw(H, W, sl=0.02, sh=0.2, asratio=0.3, p=0.5, rnd=random, defect=None):
    """None or (er0, ec0, eh, ew, rgb), consuming `rnd` as RandomSizedEarser does"""
    if rnd.uniform(-1, 1.0) > p:
        return None
    area = H * W
    while True:
        Se = rnd.uniform(sl, sh) * area
        re = rnd.uniform(asratio, 1 / asratio)
        He, We = np.sqrt(Se * re), np.sqrt(Se / re)
        xe, ye = rnd.uniform(0, W - We), rnd.uniform(0, H - He)
        if xe + We <= W and ye + He <= H and xe > 0 and ye > 0:
            break
    x1, y1 = int(math.ceil(xe)), int(math.ceil(ye))
    x2, y2 = int(math.floor(x1 + We)), int(math.floor(y1 + He))
    r, g, b = rnd.randint(0, 255), rnd.randint(0, 255), rnd.randint(0, 255)
    pw, ph = x2 - x1, y2 - y1
    left, top = (x1, y1) if defect == "paste_at_x1y1" else (pw, ph)      # img.paste(I, part1.size): the box is the SIZE
    eh, ew = min(H, top + ph) - top, min(W, left + pw) - left
    rgb = r | g << 8 | b << 16
    if pw <= 0 or ph <= 0 or eh <= 0 or ew <= 0:
        return 0, 0, 0, 0, rgb
    return top, left, eh, ew, rgb


def pair_list(trainval, ratio, defect=None):
    """(index_map, [(anchor, other)] of one epoch) from numpy's global generator"""
    pids = np.asarray(trainval)[:, 1]
    if defect == "numeric_pid_order":
        pids = pids.astype(np.int64)
    index_map = [int(v) for v in np.argsort(pids)]
    n = len(trainval)
    span = {}
    for pos, j in enumerate(index_map):
        lo, hi = span.get(trainval[j][1], (pos, pos))
        span[trainval[j][1]] = (min(lo, pos), max(hi, pos))
    pairs = []
    for i in np.random.permutation(n):
        anchor = index_map[i]
        lo, hi = span[trainval[anchor][1]]
        k = np.random.choice(hi - lo, size=1, replace=False) + lo
        k += (k >= i) * 1
        pairs.append((anchor, index_map[int(k[0])]))
        ks = np.random.choice(n - (hi - lo + 1), size=ratio, replace=False)
        ks += (ks >= lo) * (hi - lo + 1)
        pairs += [(anchor, index_map[int(v)]) for v in ks]
    return index_map, pairs


def item(planes, landmarks, trainval, pid_imgs, index, pose_aug, lut, defect=None):
    """one item of the reference's Preprocessor from the RectScale planes [M, H, W, 3] (row m = trainval[m]) and the landmark table;
    draws from `random` and torch's default generator"""
    M, H, W, _ = planes.shape
    row = {f: m for m, (f, _, _) in enumerate(trainval)}
    fname, pid, _ = trainval[index]

    def partner():
        names = list(pid_imgs[pid])
        if fname in names and len(names) > 1:
            names.remove(fname)
        return row[osp.splitext(random.choice(names))[0] + ".jpg"]
    t = partner() if defect == "partner_first" else None
    rect = erase_draw(H, W, defect=defect)
    flip = 1 if float(torch.rand(1)) < 0.5 else 0
    tflip = None
    if defect == "tflip_before_partner":
        tflip = 1 if random.choice([True, False]) else 0
    if t is None:
        t = partner()
    erased, sigma = -1, 5
    if pose_aug == "erase":
        erased = random.randrange(landmarks.shape[1])
    elif pose_aug == "gauss":
        sigma = random.randint(4, 6)
    if tflip is None:
        tflip = 1 if random.choice([True, False]) else 0
    er0, ec0, eh, ew, rgb = (0, 0, 0, 0, 0) if rect is None else rect
    imgs = fd_image_model(planes, [index, t], [(flip, 0, 0, er0, ec0, eh, ew, rgb), (tflip, 0, 0, 0, 0, 0, 0, 0)], lut, defect)
    maps = fd_pose_model(landmarks, [t], [(tflip, sigma, erased, 0)], H, W)
    return {"origin": imgs[0], "target": imgs[1], "posemap": maps[0], "pid": np.asarray([pid], dtype=np.int64)}


def ordered_batch(planes, rows, lut):
    """RectScale -> ToTensor -> Normalize of the rows, unflipped"""
    return fd_image_model(planes, rows, np.zeros((len(rows), 8), dtype=np.int64), lut)

