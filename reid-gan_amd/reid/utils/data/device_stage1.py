"""FD-GAN stage I's input pipeline on a raw device image bank (csrc/databank.hip: rg_bank_fd_crop_batch).

The reference (FD/baseline.py:28-71) feeds `SiameseTrainer` from `DataLoader(Preprocessor(train_set, transform=Compose([
RandomSizedRectCrop(height, width), RandomSizedEarser(), RandomHorizontalFlip(), ToTensor(), Normalize])),
sampler=RandomPairSampler(train_set, np_ratio))`: per drawn sample a JPEG decode, a crop of random area and aspect ratio resampled
to height x width with PIL's bilinear filter, the eraser's patch, a flip.  The resize FOLLOWS the draw here, so no once-resized
plane can serve; but the crop precedes the resize (`img.crop(box).resize(...)`), so the resample box is always the whole crop and
PIL's coefficients depend on (crop length, output length) alone.  `DeviceRawBank` keeps every decoded image at its own size in HBM
with the coefficient tables for every length that can occur, built once on the host in float64, and a batch is ONE launch that
resamples the drawn boxes in PIL's own integer arithmetic, pastes, flips and normalises — nothing but the packed draws (one int32
buffer) and the ids cross from the host.

Draw order (the reference's at num_workers=0, as device_pairs.py).  Pairs come from `RandomPairSampler`; a batch is `batch_size`
pairs in sampler order, the short last one kept; a pair (a, b) is item(a) then item(b); an item draws
  1. `FDRandomSizedRectCrop.draw` (Python `random`): up to ten times uniform(0.64, 1) * area and uniform(2, 3), and for the first
     box that fits randint(0, W - w), randint(0, H - h); after ten misses the whole image (the reference's RectScale fallback is the
     same resample of the full box, and the identity when the sizes already match);
  2. `FDRandomErase.draw(height, width)` (Python `random`), placed by the reference's `paste(I, part1.size)` rule;
  3. the flip: `torch.rand(1, generator) < 0.5` — torchvision's current rule, not verified against a torchvision run
     (device_pairs.py has the same caveat).

Still the reference's, on the host: JPEG decoding (once, when the bank is built) and the data sets' directory parsing.

There is deliberately no sampler.py / preprocessor.py / transforms.py next to this file — those names resolve to the reference's
modules behind the overlay.
"""
from __future__ import absolute_import

import math
import random

import torch

from clustercontrast.utils.data.device_bank import REID_MEAN, REID_STD, DeviceImageBank, DeviceRawBank, stage_files

from .device_pairs import DeviceFDTestLoader, FDRandomErase, RandomPairSampler


class FDRandomSizedRectCrop(object):
    """The draws of FD/reid/utils/data/transforms.py's RandomSizedRectCrop(height, width)."""

    def __init__(self, height, width):
        self.height, self.width = int(height), int(width)

    def draw(self, W_src, H_src):
        """(x1, y1, w, h): the box cut out of a W_src x H_src image before it is resampled to width x height.  Consumes `random`
        exactly as the reference; after ten boxes that do not fit, the whole image."""
        area = W_src * H_src
        for _ in range(10):
            target = random.uniform(0.64, 1.0) * area
            ratio = random.uniform(2, 3)
            h = int(round(math.sqrt(target * ratio)))
            w = int(round(math.sqrt(target / ratio)))
            if w <= W_src and h <= H_src:
                x1 = random.randint(0, W_src - w)
                y1 = random.randint(0, H_src - h)
                return x1, y1, w, h
        return 0, 0, W_src, H_src


class DeviceStage1Loader(object):
    """`baseline.py`'s train_loader on the raw bank: iterating it is one epoch of ((imgs1, fnames1, pids1, camids1), (imgs2, fnames2,
    pids2, camids2)) batches — what SiameseTrainer._parse_data unpacks — with imgs fp32 [B, 3, H, W] (the two halves of ONE
    [2B, 3, H, W] device allocation), pids / camids int64 device tensors and fnames lists of str.

    train_set: [(fname, pid, camid)], the list the sampler's indices refer to.  One batch is one launch, one host->device copy of the
    packed draws (ops.fd_crop_draws) and one copy of the ids."""

    def __init__(self, raw_bank, train_set, batch_size, neg_pos_ratio=1, generator=None, sampler=None, crop=None, erase=None,
                 ops=None):
        if ops is None:
            from rg_hip import ops
        self.ops, self.bank = ops, raw_bank
        self.train_set = list(train_set)
        self.batch_size = int(batch_size)
        if self.batch_size <= 0:
            raise ValueError("batch_size must be positive")
        self.generator = generator
        self.sampler = RandomPairSampler(self.train_set, neg_pos_ratio) if sampler is None else sampler
        self.height, self.width = raw_bank.size
        self.crop = FDRandomSizedRectCrop(self.height, self.width) if crop is None else crop
        self.erase = FDRandomErase() if erase is None else erase
        try:
            self._rows = [raw_bank.row[f] for f, _, _ in self.train_set]
        except KeyError as e:
            raise KeyError("%s is not in the bank" % (e.args[0],))
        self._fnames = [f for f, _, _ in self.train_set]
        self._ids = torch.tensor([[int(p) for _, p, _ in self.train_set], [int(c) for _, _, c in self.train_set]], dtype=torch.int64)
        self._lut = ops.bank_lut(REID_MEAN, REID_STD).to(raw_bank.device)

    def __len__(self):
        return -(-len(self.sampler) // self.batch_size)

    def _item(self, index):
        """one item's draws, in the reference's order -> (bank row, x1, y1, w, h, flip, er0, ec0, eh, ew, rgb)"""
        m = self._rows[index]
        hs, ws = int(self.bank.sizes_host[m][0]), int(self.bank.sizes_host[m][1])
        box = self.crop.draw(ws, hs)
        rect = self.erase.draw(self.height, self.width)
        flip = 1 if float(torch.rand(1, generator=self.generator)) < 0.5 else 0
        return (m,) + tuple(box) + (flip,) + ((0, 0, 0, 0, 0) if rect is None else tuple(rect))

    def _batch(self, pairs):
        B = len(pairs)
        items = [(self._item(a), self._item(b)) for a, b in pairs]          # a pair is item(a), then item(b)
        order = [p[0] for p in pairs] + [p[1] for p in pairs]
        draws = self.ops.fd_crop_draws(torch.tensor([it[0] for it in items] + [it[1] for it in items], dtype=torch.int64),
                                       device=self.bank.device)
        ids = self._ids[:, torch.tensor(order, dtype=torch.int64)].to(self.bank.device, non_blocking=True)
        imgs = self.ops.bank_fd_crop_batch(self.bank, draws, self._lut)
        names = [self._fnames[i] for i in order]
        return ((imgs[:B], names[:B], ids[0, :B], ids[1, :B]), (imgs[B:], names[B:], ids[0, B:], ids[1, B:]))

    def __iter__(self):
        chunk = []
        for pair in self.sampler:
            chunk.append((int(pair[0]), int(pair[1])))
            if len(chunk) == self.batch_size:
                yield self._batch(chunk)
                chunk = []
        if chunk:
            yield self._batch(chunk)


def get_data_stage1_device(dataset, height, width, batch_size, combine_trainval, np_ratio, workers=None, device=None):
    """`get_data` of FD/baseline.py on the device: (dataset, train_loader, val_loader, test_loader) from a loaded data set object
    (`trainval`, `train`, `val`, `query`, `gallery`, `images_dir`; the directory parsing stays the reference's).  The train loader
    runs on a raw bank over trainval or train; the val and test loaders are RectScale -> ToTensor -> Normalize (DeviceFDTestLoader)
    on a resized bank over val and query | gallery."""
    train_set = dataset.trainval if combine_trainval else dataset.train
    raw = DeviceRawBank.from_files(train_set, dataset.images_dir, workers, device, (height, width))
    train_loader = DeviceStage1Loader(raw, train_set, batch_size, neg_pos_ratio=np_ratio)
    test_entries = list(set(dataset.query) | set(dataset.gallery))
    entries, seen = [], set()
    for e in list(dataset.val) + test_entries:
        if e[0] not in seen:
            seen.add(e[0])
            entries.append(e)
    staged = stage_files(entries, dataset.images_dir, (height, width), None, None, workers, reid_resample="bilinear")
    bank = DeviceImageBank.from_arrays(device=device, **staged)
    return dataset, train_loader, DeviceFDTestLoader(bank, list(dataset.val), batch_size), DeviceFDTestLoader(bank, test_entries,
                                                                                                              batch_size)
