"""FD-GAN stage II's input pipeline on the device image bank (csrc/databank.hip: rg_bank_fd_image_batch / rg_bank_fd_pose_batch).

The reference (FD/train.py:21-44) feeds its training step from `DataLoader(Preprocessor(trainval, with_pose=True, ...),
sampler=RandomPairSampler(trainval, 3))`: per drawn sample a JPEG decode, `RectScale`, `RandomSizedEarser`, a flip, a second
decode for the target image and eighteen scipy Gaussian filters for its pose maps, all on the host.  `RectScale(height, width)` is
stage II's only resize; it is deterministic and precedes every draw.  So the planes are resized ONCE with the reference's own PIL
call when the bank is built (`DeviceImageBank.from_files(reid_resample='bilinear', pose_root=...)`), the landmarks of every image
are scaled once into an int32 table, and a batch is two gathers: one launch for the four image tensors, one for the two map
tensors, with nothing but the packed rows and draws (one int32 buffer) and the pids crossing from the host.

Draw order (the reference's at num_workers=0; its worker processes have generator states of their own, so only this order is
reproducible).  Pairs come from `RandomPairSampler` (numpy's global generator); a batch is `batch_size` pairs in sampler order, the
short last one kept; a pair (a, b) is item(a) then item(b); an item draws
  1. `FDRandomErase.draw` (Python `random`): uniform(-1, 1), and unless it exceeds p: (Se, re, xe, ye) until the box fits, then
     three randint(0, 255);
  2. the origin's flip: `torch.rand(1) < 0.5` on `generator` (None: torch's default) — what torchvision's current
     RandomHorizontalFlip does; torchvision is not installed next to this build, so this was NOT verified against a run of it;
  3. the partner image: `random.choice` over the identity's file names without the sample's own (if others are left);
  4. the landmark augmentation: 'erase' `random.randrange(J)`, 'gauss' `random.randint(4, 6)`, anything else nothing;
  5. `random.choice([True, False])`: the flip of target image and maps together.

The paste rule.  The reference's eraser ends in `img.paste(I, part1.size)`: the box argument is the patch's SIZE (pw, ph), so the
patch lands with its upper-left corner at column pw, row ph — not at the box it was sized from — and PIL clips it to the image.
That is reproduced as it is: rows [ph, min(H, 2 ph)), columns [pw, min(W, 2 pw)), in the coordinates before the flip.

Still the reference's, on the host: JPEG decoding (once, at build time) and the data sets' directory parsing.  Stage I's
`RandomSizedRectCrop` resamples a fresh box per draw, so it cannot gather from these planes: `baseline.py`'s loader is
device_stage1.py, on a raw bank with the resampling in the kernel; it shares the sampler, the eraser and the test loader of this file.

Importable without a reference tree and without torchvision; there is deliberately no sampler.py / preprocessor.py / transforms.py
next to this file — those names resolve to the reference's modules behind the overlay.
"""
from __future__ import absolute_import

import os.path as osp
import random

import numpy as np
import torch

from clustercontrast.utils.data.device_bank import REID_MEAN, REID_STD, DeviceImageBank, _OrderedLoader, stage_files


# ---- landmarks ------------------------------------------------------------------------------------------------------------------
def read_landmarks(path, scale_h, scale_w):
    """One landmark file ('row col' per line, in the original image's pixels) -> int32 [J, 2] as `_load_landmark`
    (preprocessor.py:100-112): int(float(s) * scale) in float64, truncated towards zero, every negative result -1."""
    out = []
    with open(path, "r") as f:
        for line in f.readlines():
            parts = line.strip().split(" ")
            if parts == [""]:
                continue
            h0, w0 = int(float(parts[0]) * scale_h), int(float(parts[1]) * scale_w)
            out.append((-1 if h0 < 0 else h0, -1 if w0 < 0 else w0))
    return np.asarray(out, dtype=np.int32).reshape(-1, 2)


def stage_landmarks(fnames, pose_root, old_sizes, size, only=None):
    """int32 [M, J, 2]: `read_landmarks` of splitext(fname) + '.txt' under `pose_root` for every image, scaled by
    size / old_sizes[m] ((height, width) both; Python float division, as the reference).  `only`: a set of file names — the others
    get a row of -1 without their file being opened (images that never serve as a target)."""
    height, width = int(size[0]), int(size[1])
    rows, J = [], None
    for m, fname in enumerate(fnames):
        if only is not None and fname not in only:
            rows.append(None)
            continue
        path = osp.splitext(fname)[0] + ".txt"
        if pose_root is not None:
            path = osp.join(pose_root, path)
        lm = read_landmarks(path, height / int(old_sizes[m][0]), width / int(old_sizes[m][1]))
        if J is None:
            J = lm.shape[0]
        if lm.shape[0] != J or J == 0:
            raise ValueError("stage_landmarks: %s holds %d landmarks, the files before it %d" % (path, lm.shape[0], J))
        rows.append(lm)
    if J is None:
        raise ValueError("stage_landmarks: no landmark file was read")
    return np.stack([np.full((J, 2), -1, dtype=np.int32) if r is None else r for r in rows])


# ---- the pair sampler -----------------------------------------------------------------------------------------------------------
def _choose_from(start, end, excluded, size):
    """`size` distinct positions of [start, end] outside excluded = (first, last), by the reference's numpy call"""
    n_ex = excluded[1] - excluded[0] + 1
    inds = np.random.choice(end - start + 1 - n_ex, size=size, replace=False) + start
    inds += (inds >= excluded[0]) * n_ex
    return inds


class RandomPairSampler(object):
    """FD/reid/utils/data/sampler.py's RandomPairSampler: per anchor (one `np.random.permutation` per epoch) one positive and
    `neg_pos_ratio` negatives, as (anchor index, other index) pairs; `len()` = M (1 + ratio).  Same numpy calls in the same order,
    so the pairs are the reference's under the same numpy seed — including its sort of the pid column of
    `np.asarray(data_source)`, which is a column of STRINGS ('10' < '100' < '2')."""

    def __init__(self, data_source, neg_pos_ratio=1):
        self.data_source = data_source
        self.num_samples = len(data_source)
        self.neg_pos_ratio = int(neg_pos_ratio)
        order = np.argsort(np.asarray(data_source)[:, 1])
        self.index_map = [int(j) for j in order]                    # sorted position -> index
        self.index_range = {}                                       # pid -> [first, last] sorted position
        for pos, j in enumerate(self.index_map):
            pid = data_source[j][1]
            r = self.index_range.setdefault(pid, [pos, pos])
            r[0], r[1] = min(r[0], pos), max(r[1], pos)
        for pid, (first, last) in self.index_range.items():
            if last == first:
                raise ValueError("RandomPairSampler: identity %r has a single image, no positive pair can be drawn" % (pid,))
            if self.num_samples - (last - first + 1) < self.neg_pos_ratio:
                raise ValueError("RandomPairSampler: fewer than %d images outside identity %r" % (self.neg_pos_ratio, pid))

    def __len__(self):
        return self.num_samples * (1 + self.neg_pos_ratio)

    def __iter__(self):
        for i in np.random.permutation(self.num_samples):
            i = int(i)
            anchor = self.index_map[i]
            first, last = self.index_range[self.data_source[anchor][1]]
            pos = _choose_from(first, last, (i, i), 1)[0]
            yield anchor, self.index_map[int(pos)]
            for k in _choose_from(0, self.num_samples - 1, (first, last), self.neg_pos_ratio):
                yield anchor, self.index_map[int(k)]


# ---- the eraser -----------------------------------------------------------------------------------------------------------------
class FDRandomErase(object):
    """The draws of FD/reid/utils/data/transforms.py's RandomSizedEarser and where its patch really lands (module docstring)."""

    def __init__(self, sl=0.02, sh=0.2, asratio=0.3, p=0.5):
        self.sl, self.sh, self.asratio, self.p = sl, sh, asratio, p

    def draw(self, H, W):
        """None (image unchanged) or (er0, ec0, eh, ew, rgb): the patch's rows [er0, er0 + eh), columns [ec0, ec0 + ew) inside the
        H x W image (eh = 0: it fell outside) and its colour R | G << 8 | B << 16.  Consumes `random` exactly as the reference."""
        if random.uniform(-1, 1.0) > self.p:
            return None
        area = H * W
        while True:
            Se = random.uniform(self.sl, self.sh) * area
            re = random.uniform(self.asratio, 1 / self.asratio)
            He, We = np.sqrt(Se * re), np.sqrt(Se / re)
            xe = random.uniform(0, W - We)
            ye = random.uniform(0, H - He)
            if xe + We <= W and ye + He <= H and xe > 0 and ye > 0:
                break
        x1, y1 = int(np.ceil(xe)), int(np.ceil(ye))
        pw, ph = int(np.floor(x1 + We)) - x1, int(np.floor(y1 + He)) - y1
        rgb = random.randint(0, 255)
        rgb |= random.randint(0, 255) << 8
        rgb |= random.randint(0, 255) << 16
        eh, ew = min(H, 2 * ph) - ph, min(W, 2 * pw) - pw           # paste at (column pw, row ph), clipped to the image
        if ph <= 0 or pw <= 0 or eh <= 0 or ew <= 0:
            return 0, 0, 0, 0, rgb
        return ph, pw, eh, ew, rgb


# ---- loaders --------------------------------------------------------------------------------------------------------------------
class DevicePairLoader(object):
    """`train.py`'s train_loader on the bank: iterating it is one epoch of (dict, dict) batches, each dict {'origin', 'target'
    fp32 [B, 3, H, W], 'posemap' fp32 [B, J, H, W], 'pid' int64 [B, 1]} on the device — the form FDGANModel.set_input's device
    branch takes.  The four image tensors are views of one allocation, the two map tensors of another.

    bank: built with reid_resample='bilinear' and pose_root (its `reid` planes are RectScale's, `landmarks` the table).  trainval:
    [(fname, pid, camid)], the list the sampler's indices refer to; pid_imgs: {pid: [fname]} (dataset.trainval_query).  Every name
    of pid_imgs is resolved to a bank row here (splitext(name) + '.jpg'), a KeyError names a file the bank lacks.

    One batch is two launches, one host->device copy of the packed draws (ops.fd_draws) and the copy of the pids."""

    def __init__(self, bank, trainval, pid_imgs, batch_size, neg_pos_ratio=3, pose_aug='no', generator=None, sampler=None,
                 erase=None, ops=None):
        if ops is None:
            from rg_hip import ops
        self.ops, self.bank = ops, bank
        if bank.landmarks is None:
            raise ValueError("DevicePairLoader: the bank holds no landmark table (build it with pose_root=)")
        self.trainval = list(trainval)
        self.batch_size = int(batch_size)
        if self.batch_size <= 0:
            raise ValueError("batch_size must be positive")
        self.pose_aug, self.generator = pose_aug, generator
        self.sampler = RandomPairSampler(self.trainval, neg_pos_ratio) if sampler is None else sampler
        self.erase = FDRandomErase() if erase is None else erase
        self.height, self.width = bank.reid_size
        self.joints = int(bank.landmarks.shape[1])

        def row(name):
            try:
                return bank.row[name]
            except KeyError:
                raise KeyError("%s is not in the bank" % (name,))
        self._rows = [row(f) for f, _, _ in self.trainval]
        self._pids = [int(p) for _, p, _ in self.trainval]
        self._query = {pid: (list(names), [row(osp.splitext(n)[0] + ".jpg") for n in names]) for pid, names in pid_imgs.items()}
        self._lut = ops.bank_lut(REID_MEAN, REID_STD).to(bank.device)

    def __len__(self):
        return -(-len(self.sampler) // self.batch_size)

    def _item(self, index):
        """one item's draws, in the reference's order -> (origin row, origin params, target row, pose params)"""
        fname, pid, _ = self.trainval[index]
        rect = self.erase.draw(self.height, self.width)
        flip = 1 if float(torch.rand(1, generator=self.generator)) < 0.5 else 0
        names, rows = self._query[pid]
        if fname in names and len(names) > 1:
            k = names.index(fname)
            rows = rows[:k] + rows[k + 1:]
        target = random.choice(rows)
        erased, sigma = -1, 5
        if self.pose_aug == 'erase':
            erased = random.randrange(self.joints)
        elif self.pose_aug == 'gauss':
            sigma = random.randint(4, 6)
        tflip = 1 if random.choice([True, False]) else 0
        er0, ec0, eh, ew, rgb = (0, 0, 0, 0, 0) if rect is None else rect
        return self._rows[index], (flip, 0, 0, er0, ec0, eh, ew, rgb), target, (tflip, sigma, erased, 0)

    def _batch(self, pairs):
        B = len(pairs)
        items = [[self._item(a), self._item(b)] for a, b in pairs]          # a pair is item(a), then item(b)
        idx, params, pidx, pparams, pids = [], [], [], [], []
        for side in (0, 1):
            it = [items[k][side] for k in range(B)]
            idx += [t[0] for t in it] + [t[2] for t in it]                  # origins, then targets
            params += [t[1] for t in it] + [(t[3][0], 0, 0, 0, 0, 0, 0, 0) for t in it]
            pidx += [t[2] for t in it]
            pparams += [t[3] for t in it]
            pids.append([self._pids[p[side]] for p in pairs])
        draws = self.ops.fd_draws(torch.tensor(idx, dtype=torch.int64), torch.tensor(params, dtype=torch.int64),
                                  torch.tensor(pidx, dtype=torch.int64), torch.tensor(pparams, dtype=torch.int64),
                                  device=self.bank.device)
        pid = torch.tensor(pids, dtype=torch.int64).to(self.bank.device, non_blocking=True)
        imgs = self.ops.bank_fd_image_batch(self.bank.reid, draws, self._lut)
        maps = self.ops.bank_fd_pose_batch(self.bank.landmarks, draws, self.height, self.width)
        return tuple({'origin': imgs[2 * s * B:(2 * s + 1) * B], 'target': imgs[(2 * s + 1) * B:(2 * s + 2) * B],
                      'posemap': maps[s * B:(s + 1) * B], 'pid': pid[s].view(B, 1)} for s in (0, 1))

    def __iter__(self):
        chunk = []
        for pair in self.sampler:
            chunk.append((int(pair[0]), int(pair[1])))
            if len(chunk) == self.batch_size:
                yield self._batch(chunk)
                chunk = []
        if chunk:
            yield self._batch(chunk)


class DeviceFDTestLoader(_OrderedLoader):
    """`train.py`'s test_loader on the bank: RectScale -> ToTensor -> Normalize of `entries` in order, as (imgs, fnames, pids,
    camids) batches, the last one short — the ReID gather (rg_bank_reid_batch) with zero draws."""

    def __iter__(self):
        for indices, draws, meta in self._chunks():
            imgs = self.ops.bank_reid_batch(self.bank.reid, draws, self._lut, self._fill0, self.bank.reid_size, 0)
            yield imgs, [self._fnames[i] for i in indices], meta[0], meta[1]


def get_data_device(dataset, height, width, batch_size, pose_aug, workers=None, device=None):
    """`get_data` of FD/train.py on the device: (dataset, train_loader, test_loader) from a loaded data set object (`trainval`,
    `trainval_query`, `query`, `gallery`, `images_dir`, `poses_dir`; the directory parsing stays the reference's).  ONE bank over
    trainval, query and gallery; landmark files are read for the trainval images only (nothing else serves as a target)."""
    test_entries = list(set(dataset.query) | set(dataset.gallery))
    entries, seen = [], set()
    for e in list(dataset.trainval) + test_entries:
        if e[0] not in seen:
            seen.add(e[0])
            entries.append(e)
    staged = stage_files(entries, dataset.images_dir, (height, width), None, None, workers, reid_resample="bilinear")
    targets = set(osp.splitext(n)[0] + ".jpg" for names in dataset.trainval_query.values() for n in names)
    staged["landmarks"] = stage_landmarks(staged["fnames"], dataset.poses_dir, staged["old_sizes"], (height, width), only=targets)
    bank = DeviceImageBank.from_arrays(device=device, **staged)
    train_loader = DevicePairLoader(bank, dataset.trainval, dataset.trainval_query, batch_size, neg_pos_ratio=3, pose_aug=pose_aug)
    return dataset, train_loader, DeviceFDTestLoader(bank, test_entries, batch_size)
