"""Host model of the three batch definitions of csrc/databank.hip (include/reidgan_hip.h), index by index in numpy: no
vectorised cleverness, one Python loop level per output dimension, so that each line can be read against the header.

    bank_lut            the [3, 256] table, built by torch with the reference's arithmetic (the entry points take it as an input)
    reid_batch_model    rg_bank_reid_batch
    gan_batch_model     rg_bank_gan_batch
    pose_batch_model    rg_bank_pose_batch in the reference's own form, exp(-(dy^2 + dx^2) / (2 sigma^2)) in float64 rounded to
                        float32 (`cords_to_map`).  The kernel evaluates the product of two float64 exponentials, as
                        rg_pose_maps mode 1 does; the GPU tests compare it bit for bit with THAT entry on the gathered centres,
                        and this function ties the gather and the flip to the reference's formula on the CPU.

tests/test_bank_hostmodel_cpu.py ties the model to the reference's transform composition, to planted defects and to the
elementwise table expression; tests/test_bank_gpu.py compares the kernels with it bit for bit.
"""
import numpy as np
import torch

REID_MEAN, REID_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
GAN_MEAN, GAN_STD = (0.5, 0.5, 0.5), (0.5, 0.5, 0.5)
MISSING = -2 ** 31


def bank_lut(mean, std):
    """[3, 256] float32: ((arange(256, dtype=float32) / 255) - mean[c]) / std[c] in fp32, by torch"""
    rows = []
    for c in range(3):
        m = torch.tensor(mean[c], dtype=torch.float32)
        s = torch.tensor(std[c], dtype=torch.float32)
        rows.append(((torch.arange(256, dtype=torch.float32) / 255) - m) / s)
    return torch.stack(rows).numpy()


def reid_batch_model(bank, idx, params, lut, fill, H, W, pad):
    """bank uint8 [M, Hs, Ws, 3]; idx [N]; params [N, >= 7] = (flip, top, left, er0, ec0, eh, ew); -> float32 [N, 3, H, W]"""
    M, Hs, Ws, _ = bank.shape
    N = len(idx)
    out = np.empty((N, 3, H, W), dtype=np.float32)
    for n in range(N):
        flip, top, left, er0, ec0, eh, ew = [int(v) for v in params[n][:7]]
        m = int(idx[n])
        assert 0 <= m < M
        for c in range(3):
            for y in range(H):
                for x in range(W):
                    xs = W - 1 - x if flip else x
                    if eh > 0 and er0 <= y < er0 + eh and ec0 <= xs < ec0 + ew:
                        out[n, c, y, x] = fill[c]
                        continue
                    r, q = top + y - pad, left + xs - pad
                    if r < 0 or r >= Hs or q < 0 or q >= Ws:
                        out[n, c, y, x] = lut[c][0]
                    else:
                        out[n, c, y, x] = lut[c][bank[m][r][q][c]]
    return out


def gan_batch_model(bank, idx, flips, lut):
    """bank uint8 [M, Hg, Wg, 3]; -> float32 [N, 3, Hg, Wg]"""
    M, Hg, Wg, _ = bank.shape
    N = len(idx)
    out = np.empty((N, 3, Hg, Wg), dtype=np.float32)
    for n in range(N):
        m = int(idx[n])
        assert 0 <= m < M
        for c in range(3):
            for y in range(Hg):
                for x in range(Wg):
                    xs = Wg - 1 - x if int(flips[n]) else x
                    out[n, c, y, x] = lut[c][bank[m][y][xs][c]]
    return out


def pose_batch_model(centres, idx, flips, sigma, Hg, Wg):
    """centres int [M, J, 2] = (row, col), MISSING for an absent joint; -> float32 [N, J, Hg, Wg]"""
    M, J, _ = centres.shape
    N = len(idx)
    out = np.zeros((N, J, Hg, Wg), dtype=np.float32)
    for n in range(N):
        m = int(idx[n])
        assert 0 <= m < M
        for j in range(J):
            cy, cx = int(centres[m][j][0]), int(centres[m][j][1])
            if cy == MISSING or cx == MISSING:
                continue
            for y in range(Hg):
                for x in range(Wg):
                    xs = Wg - 1 - x if int(flips[n]) else x
                    out[n, j, y, x] = np.float32(np.exp(-((y - cy) ** 2 + (xs - cx) ** 2) / (2 * sigma ** 2)))
    return out
