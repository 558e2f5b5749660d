"""A device-resident image bank and the loaders that draw finished batches from it (csrc/databank.hip).

The reference's input pipeline (CC/examples/cluster_contrast_gan_train_usl_infomap.py:71-186 with
CC/clustercontrast/utils/data/preprocessor.py) decodes, resizes, augments and normalises every sample on the host each time it is
drawn, and copies fp32 batches to the device.  Its two resizes — `T.Resize((h, w), BICUBIC)` for the ReID view,
`F.resize(Xs, load_size)` (bilinear) for the GAN image — are deterministic and precede every random draw, so they are done ONCE
here, when the bank is built, with the same PIL calls; the resized uint8 planes then stay in HBM (98 304 + 24 576 bytes per image
at 256x128 / 128x64: Market-1501's 35 585 images are 4.4 GB, MSMT17's 126 441 are 15.5 GB), and a batch is one gather kernel per
view with nothing but the row indices and the draws crossing from the host.  The pose centres (`cords_to_map`'s per-point
arithmetic, device_pose._centres) are likewise computed once per image into an int32 device table.

One loader's resize FOLLOWS its draw (FD-GAN stage I's RandomSizedRectCrop): `DeviceRawBank` keeps the decoded images at their own
size with PIL's bilinear coefficients as integer tables (`pil_bilinear_table`), and the batch kernel resamples the drawn box
(reid/utils/data/device_stage1.py).

Not here, still the reference's: JPEG decoding itself (PIL, at build time) and the data sets' directory parsing.

Importable without a reference tree, without torchvision and without pandas; PIL is needed by `from_files` only.
"""
from __future__ import absolute_import

import csv
import json
import os
import os.path as osp
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from .device_pose import _SENTINEL, _centres
from .device_transforms import PadRandomCropFlip, RandomErasing

REID_MEAN, REID_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
GAN_MEAN, GAN_STD = (0.5, 0.5, 0.5), (0.5, 0.5, 0.5)


def default_workers():
    """decode threads: the CPUs this process may run on, at most 16 (never the machine's CPU count)"""
    try:
        n = len(os.sched_getaffinity(0))
    except AttributeError:                                  # platforms without affinity masks
        n = 1
    return max(1, min(16, n))


# ---- host staging (no device needed) ------------------------------------------------------------------------------------------
def read_pose_csv(path):
    """The reference's pose annotation file (`pd.read_csv(path, sep=':')`, columns name / keypoints_y / keypoints_x, the
    coordinates as JSON lists, -1 for a missing joint) -> {name: int64 [J, 2] = (y, x)} (`load_pose_cords_from_strings`)."""
    out = {}
    with open(path, "r", newline="") as f:
        reader = csv.reader(f, delimiter=":")
        header = [h.strip() for h in next(reader)]
        try:
            ci, cy, cx = header.index("name"), header.index("keypoints_y"), header.index("keypoints_x")
        except ValueError:
            raise ValueError("read_pose_csv: %s has no name / keypoints_y / keypoints_x columns (header %s)" % (path, header))
        for row in reader:
            if not row:
                continue
            ys, xs = json.loads(row[cy]), json.loads(row[cx])
            if len(ys) != len(xs):
                raise ValueError("read_pose_csv: %s has %d y and %d x coordinates" % (row[ci], len(ys), len(xs)))
            out[row[ci]] = np.stack([np.asarray(ys, dtype=np.int64), np.asarray(xs, dtype=np.int64)], axis=1)
    return out


def stage_centres(cords, old_sizes, gan_size):
    """int32 [M, J, 2] centre table of `cords_to_map(cords[m], gan_size, old_sizes[m])`: device_pose._centres per image
    (INT32_MIN marks a missing joint), clipped to int32 as cords_to_map_batch does."""
    cords = np.asarray(cords)
    if cords.ndim != 3 or cords.shape[2] != 2:
        raise ValueError("stage_centres: cords must be [M, J, 2]")
    size = (int(gan_size[0]), int(gan_size[1]))
    c = np.stack([_centres(cords[m], size, None if old_sizes is None else (int(old_sizes[m][0]), int(old_sizes[m][1])), None)
                  for m in range(cords.shape[0])])
    return np.clip(c, _SENTINEL, 2 ** 31 - 1).astype(np.int32)


def _decode(path, reid_size, gan_size, reid_resample="bicubic"):
    from PIL import Image
    img = Image.open(path).convert("RGB")
    old = (img.size[1], img.size[0])
    # T.Resize((h, w), interpolation=BICUBIC) on a PIL image is img.resize((w, h), BICUBIC); F.resize(Xs, (hg, wg)) is
    # img.resize((wg, hg), BILINEAR).  An image that already has the size is taken as it is: PIL's resize to the same
    # size over the full box returns a copy, so this is what torchvision's call gives too
    bicubic = getattr(Image, "Resampling", Image).BICUBIC
    bilinear = getattr(Image, "Resampling", Image).BILINEAR
    # reid_resample 'bilinear': FD-GAN's RectScale(height, width) (FD/reid/utils/data/transforms.py:9-19), the same rule with
    # PIL's BILINEAR
    reid = img if (img.size[1], img.size[0]) == tuple(reid_size) else \
        img.resize((reid_size[1], reid_size[0]), bicubic if reid_resample == "bicubic" else bilinear)
    out_r = np.asarray(reid, dtype=np.uint8)
    out_g = None
    if gan_size is not None:
        gan = img if (img.size[1], img.size[0]) == tuple(gan_size) else img.resize((gan_size[1], gan_size[0]), bilinear)
        out_g = np.asarray(gan, dtype=np.uint8)
    return out_r, out_g, old


def _decode_pool(one, M, workers):
    """one(m) for every m in [0, M) on `workers` threads (PIL releases the GIL while it decodes and resamples)"""
    if workers == 1:
        for m in range(M):
            one(m)
    else:
        with ThreadPoolExecutor(max_workers=workers) as pool:
            list(pool.map(one, range(M), chunksize=1))


def stage_files(entries, root=None, reid_size=(256, 128), gan_size=(128, 64), pose_file=None, workers=None, reid_resample="bicubic",
                pose_root=None):
    """Decode every file of `entries` = [(fname, pid, camid)] ONCE and resize it to both plane sizes on the host.  Returns the
    keyword arguments of DeviceImageBank.from_arrays as numpy arrays / lists; nothing here touches a device.

    reid_resample: 'bicubic' (T.Resize(..., BICUBIC)) or 'bilinear' (FD-GAN's RectScale).  pose_root: the directory of FD-GAN's
    landmark files (splitext(fname) + '.txt'); adds `landmarks`, the int32 [M, J, 2] table of `_load_landmark` at reid_size
    (reid.utils.data.device_pairs.stage_landmarks)."""
    entries = list(entries)
    if not entries:
        raise ValueError("stage_files: no entries")
    if reid_resample not in ("bicubic", "bilinear"):
        raise ValueError("stage_files: reid_resample must be 'bicubic' or 'bilinear', got %r" % (reid_resample,))
    reid_size = (int(reid_size[0]), int(reid_size[1]))
    gan_size = None if gan_size is None else (int(gan_size[0]), int(gan_size[1]))
    paths = [f if root is None else osp.join(root, f) for f, _, _ in entries]
    workers = default_workers() if workers is None else max(1, int(workers))
    M = len(entries)
    reid = np.empty((M,) + reid_size + (3,), dtype=np.uint8)
    gan = None if gan_size is None else np.empty((M,) + gan_size + (3,), dtype=np.uint8)
    old = np.empty((M, 2), dtype=np.int64)

    def one(m):
        r, g, o = _decode(paths[m], reid_size, gan_size, reid_resample)
        reid[m] = r
        if gan is not None:
            gan[m] = g
        old[m] = o

    _decode_pool(one, M, workers)
    cords = None
    if pose_file is not None:
        table = read_pose_csv(pose_file)
        cords = np.stack([table[osp.split(p)[-1]] for p in paths])
    out = dict(reid_u8=reid, fnames=[e[0] for e in entries], pids=[int(e[1]) for e in entries],
               camids=[int(e[2]) for e in entries], gan_u8=gan, cords=cords, old_sizes=old)
    if pose_root is not None:
        from reid.utils.data.device_pairs import stage_landmarks
        out["landmarks"] = stage_landmarks([e[0] for e in entries], pose_root, old, reid_size)
    return out


# ---- the bank -----------------------------------------------------------------------------------------------------------------
class DeviceImageBank(object):
    """uint8 planes of every image of a data set on the device: `reid` [M, Hs, Ws, 3], `gan` [M, Hg, Wg, 3] or None, `centres`
    int32 [M, J, 2] or None, `landmarks` int32 [M, J, 2] or None (FD-GAN's `_load_landmark` at the ReID plane's size), plus the host bookkeeping (`fnames`, `pids`, `camids`, `old_sizes`, `row`: fname -> bank row)."""

    def __init__(self, reid, gan, centres, fnames, pids, camids, old_sizes, landmarks=None):
        self.reid, self.gan, self.centres, self.landmarks = reid, gan, centres, landmarks
        self.fnames, self.pids, self.camids, self.old_sizes = list(fnames), list(pids), list(camids), old_sizes
        self.row = {f: m for m, f in enumerate(self.fnames)}
        if len(self.row) != len(self.fnames):
            raise ValueError("DeviceImageBank: duplicate file names")
        self.device = reid.device

    def __len__(self):
        return len(self.fnames)

    @property
    def nbytes(self):
        return sum(t.numel() * t.element_size() for t in (self.reid, self.gan, self.centres, self.landmarks) if t is not None)

    @property
    def reid_size(self):
        return (self.reid.shape[1], self.reid.shape[2])

    @property
    def gan_size(self):
        return None if self.gan is None else (self.gan.shape[1], self.gan.shape[2])

    @classmethod
    def from_arrays(cls, reid_u8, fnames, pids, camids, gan_u8=None, cords=None, old_sizes=None, centres=None, device=None,
                    landmarks=None):
        """From already-resized uint8 arrays [M, H, W, 3] (numpy or torch).  `cords` [M, J, 2] = (y, x) in the ORIGINAL image's
        pixels with `old_sizes` [M, 2] = (height, width) of the originals (None: the GAN plane's size), or a ready `centres`
        table; the upload is the only device work."""
        if device is None:
            device = torch.device("cuda", torch.cuda.current_device())
        device = torch.device(device)

        def plane(a, name):
            t = torch.as_tensor(a)
            if t.dtype != torch.uint8 or t.dim() != 4 or t.shape[3] != 3:
                raise ValueError("DeviceImageBank: %s must be uint8 [M, H, W, 3], got %s %s" % (name, t.dtype, tuple(t.shape)))
            if t.shape[0] != len(fnames):
                raise ValueError("DeviceImageBank: %s holds %d images for %d names" % (name, t.shape[0], len(fnames)))
            return t.contiguous().to(device)

        if not (len(fnames) == len(pids) == len(camids)) or not len(fnames):
            raise ValueError("DeviceImageBank: fnames, pids and camids must be non-empty and of one length")
        reid = plane(reid_u8, "reid_u8")
        gan = None if gan_u8 is None else plane(gan_u8, "gan_u8")
        if centres is None and cords is not None:
            if gan is None:
                raise ValueError("DeviceImageBank: poses need the GAN planes (their size is the map size)")
            centres = stage_centres(cords, old_sizes, (gan.shape[1], gan.shape[2]))
        if centres is not None:
            centres = torch.as_tensor(centres)
            if centres.dtype != torch.int32 or centres.dim() != 3 or centres.shape[0] != len(fnames) or centres.shape[2] != 2:
                raise ValueError("DeviceImageBank: centres must be int32 [M, J, 2]")
            centres = centres.contiguous().to(device)
        if landmarks is not None:
            landmarks = torch.as_tensor(landmarks)
            if landmarks.dtype != torch.int32 or landmarks.dim() != 3 or landmarks.shape[0] != len(fnames) or landmarks.shape[2] != 2:
                raise ValueError("DeviceImageBank: landmarks must be int32 [M, J, 2]")
            landmarks = landmarks.contiguous().to(device)
        return cls(reid, gan, centres, fnames, pids, camids, None if old_sizes is None else np.asarray(old_sizes), landmarks)

    @classmethod
    def from_files(cls, entries, root=None, reid_size=(256, 128), gan_size=(128, 64), pose_file=None, workers=None, device=None,
                   reid_resample="bicubic", pose_root=None):
        """Decode each file of the reference's (fname, pid, camid) triples once with PIL, resize it to both plane sizes on the
        host (`stage_files`) and upload."""
        return cls.from_arrays(device=device, **stage_files(entries, root, reid_size, gan_size, pose_file, workers, reid_resample,
                                                            pose_root))


# ---- the raw bank (FD-GAN stage I) ----------------------------------------------------------------------------------------------
PIL_PRECISION_BITS = 22
RAW_MAX_RATIO = 8                                           # input length / output length: keeps a table row at 17 taps


def pil_bilinear_table(nmax, m):
    """int32 [nmax + 1, m, 2 + K]: PIL's BILINEAR coefficients of an axis resampled from input length n (the first index; row 0 is
    unused) to output length m over its WHOLE extent, as rows (lo, cnt, k_0 .. k_{K-1}) — the taps in[lo .. lo + cnt) with
    integer weights k_x (zero beyond cnt), K the longest row.  The rule, in float64 throughout (checked against PIL's output, byte for byte):
        scale = n / m; fs = max(scale, 1); support = fs; centre = (j + 0.5) * scale
        lo = max(int(centre - support + 0.5), 0); hi = min(int(centre + support + 0.5), n)          (int truncates)
        w_x = 1 - a if a < 1 else 0,  a = |(x + lo - centre + 0.5) * (1 / fs)|;  ww = sum of w_x in increasing x
        k_x = int(0.5 + (w_x / ww) * 2^22)
    and a resampled byte is min(255, (2^21 + sum_x in[lo + x] * k_x) >> 22).  All input lengths at once; only the sum runs over
    x in order."""
    nmax, m = int(nmax), int(m)
    if nmax < 1 or m < 1 or nmax > RAW_MAX_RATIO * m:
        raise ValueError("pil_bilinear_table: input lengths up to %d for output length %d (at most %d times as long)"
                         % (nmax, m, RAW_MAX_RATIO))
    n = np.arange(1, nmax + 1, dtype=np.int64)[:, None]
    scale = n.astype(np.float64) / np.float64(m)
    fs = np.maximum(scale, 1.0)
    centre = (np.arange(m, dtype=np.float64)[None, :] + 0.5) * scale
    lo = np.maximum((centre - fs + 0.5).astype(np.int64), 0)
    hi = np.minimum((centre + fs + 0.5).astype(np.int64), n)
    cnt = hi - lo
    K = int(cnt.max())
    x = np.arange(K, dtype=np.int64)[None, None, :]
    a = np.abs(((x + lo[:, :, None]).astype(np.float64) - centre[:, :, None] + 0.5) * (1.0 / fs)[:, :, None])
    w = np.where((a < 1.0) & (x < cnt[:, :, None]), 1.0 - a, 0.0)
    ww = np.zeros_like(centre)
    for i in range(K):                                      # PIL sums in increasing x; adding the zeros beyond cnt changes nothing
        ww = ww + w[:, :, i]
    k = (0.5 + (w / ww[:, :, None]) * np.float64(1 << PIL_PRECISION_BITS)).astype(np.int64)
    table = np.zeros((nmax + 1, m, 2 + K), dtype=np.int32)
    table[1:, :, 0], table[1:, :, 1], table[1:, :, 2:] = lo, cnt, k
    return table


class DeviceRawBank(object):
    """Every image of a data set at its OWN size on the device, for loaders whose resize follows the draw (FD-GAN stage I's
    RandomSizedRectCrop): `data` uint8 [sum H_m W_m 3] (HWC images one after the other), `offsets` int64 [M] (bytes), `sizes` int32
    [M, 2] = (H_m, W_m) with its host copy `sizes_host`, and PIL's bilinear coefficient tables `table_x` / `table_y`
    (pil_bilinear_table) for every input length up to the widest / highest image at the output `size` = (height, width); plus the
    host bookkeeping of DeviceImageBank (`fnames`, `pids`, `camids`, `row`: fname -> bank row).  Market-1501's trainval (12 936
    images of 128x64) is 318 MB."""

    def __init__(self, data, offsets, sizes, sizes_host, table_x, table_y, size, fnames, pids, camids):
        self.data, self.offsets, self.sizes, self.sizes_host = data, offsets, sizes, sizes_host
        self.table_x, self.table_y, self.size = table_x, table_y, (int(size[0]), int(size[1]))
        self.fnames, self.pids, self.camids = list(fnames), list(pids), list(camids)
        self.row = {f: m for m, f in enumerate(self.fnames)}
        if len(self.row) != len(self.fnames):
            raise ValueError("DeviceRawBank: duplicate file names")
        self.device = data.device

    def __len__(self):
        return len(self.fnames)

    @property
    def nbytes(self):
        return sum(t.numel() * t.element_size() for t in (self.data, self.offsets, self.sizes, self.table_x, self.table_y))

    @classmethod
    def from_arrays(cls, images, fnames, pids, camids, device=None, size=(256, 128)):
        """From decoded images, a list of HWC uint8 arrays [H_m, W_m, 3]; size = (height, width) of the batches.  An image more
        than 8 times as high or wide as the output is refused by name (its coefficient rows would outgrow the kernel's)."""
        if device is None:
            device = torch.device("cuda", torch.cuda.current_device())
        device = torch.device(device)
        height, width = int(size[0]), int(size[1])
        if height < 1 or width < 1:
            raise ValueError("DeviceRawBank: output size %r" % (size,))
        if not (len(images) == len(fnames) == len(pids) == len(camids)) or not len(fnames):
            raise ValueError("DeviceRawBank: images, fnames, pids and camids must be non-empty and of one length")
        arrays = []
        for a, f in zip(images, fnames):
            a = np.asarray(a)
            if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3 or a.shape[0] < 1 or a.shape[1] < 1:
                raise ValueError("DeviceRawBank: %s must be uint8 [H, W, 3], got %s %s" % (f, a.dtype, a.shape))
            if a.shape[0] > RAW_MAX_RATIO * height or a.shape[1] > RAW_MAX_RATIO * width:
                raise ValueError("DeviceRawBank: %s is %dx%d, more than %d times the %dx%d output"
                                 % (f, a.shape[0], a.shape[1], RAW_MAX_RATIO, height, width))
            arrays.append(a)
        sizes = np.asarray([a.shape[:2] for a in arrays], dtype=np.int32)
        nbytes = sizes[:, 0].astype(np.int64) * sizes[:, 1] * 3
        offsets = np.concatenate([[0], np.cumsum(nbytes)[:-1]]).astype(np.int64)
        data = np.concatenate([a.reshape(-1) for a in arrays])
        table_x = pil_bilinear_table(int(sizes[:, 1].max()), width)
        table_y = pil_bilinear_table(int(sizes[:, 0].max()), height)
        return cls(torch.from_numpy(data).to(device), torch.from_numpy(offsets).to(device), torch.from_numpy(sizes).to(device),
                   sizes, torch.from_numpy(table_x).to(device), torch.from_numpy(table_y).to(device), (height, width), fnames, pids,
                   camids)

    @classmethod
    def from_files(cls, entries, root=None, workers=None, device=None, size=(256, 128)):
        """Decode each file of the reference's (fname, pid, camid) triples once, with the reference's call
        (`Image.open(path).convert('RGB')`) on the decode threads of `stage_files`, and upload the images as they are."""
        entries = list(entries)
        if not entries:
            raise ValueError("DeviceRawBank: no entries")
        paths = [f if root is None else osp.join(root, f) for f, _, _ in entries]
        images = [None] * len(entries)

        def one(m):
            from PIL import Image
            images[m] = np.asarray(Image.open(paths[m]).convert("RGB"), dtype=np.uint8)

        _decode_pool(one, len(entries), default_workers() if workers is None else max(1, int(workers)))
        return cls.from_arrays(images, [e[0] for e in entries], [int(e[1]) for e in entries], [int(e[2]) for e in entries], device,
                               size)


# ---- loaders ------------------------------------------------------------------------------------------------------------------
def _gt_label(fname):
    """`int(Xs_name.split('_', 1)[0])` of preprocessor.py:175"""
    return int(osp.split(fname)[-1].split("_", 1)[0])


class _BankLoader(object):
    """What the three loaders share: the bank rows and labels of their entry list, the tables, and the batch builders."""

    def __init__(self, bank, entries, batch_size, ops=None):
        if ops is None:
            from rg_hip import ops
        self.ops, self.bank = ops, bank
        self.entries = list(entries)
        self.batch_size = int(batch_size)
        if self.batch_size <= 0:
            raise ValueError("batch_size must be positive")
        try:
            self._rows = [bank.row[f] for f, _, _ in self.entries]
        except KeyError as e:
            raise KeyError("%s is not in the bank" % (e.args[0],))
        self._fnames = [f for f, _, _ in self.entries]
        self._names = [osp.split(f)[-1] for f in self._fnames]
        # (pid, camid, index, gt_label) per entry as int64 rows: one host gather and one copy per batch
        self._meta = torch.tensor([[int(p) for _, p, _ in self.entries], [int(c) for _, _, c in self.entries],
                                   list(range(len(self.entries))), [0] * len(self.entries)], dtype=torch.int64)
        self._lut = ops.bank_lut(REID_MEAN, REID_STD).to(bank.device)
        self._fill0 = torch.zeros(3, dtype=torch.float32).to(bank.device)      # no rectangle is ever drawn with it
        self._lut_gan = None

    def _need_gan(self):
        if self.bank.gan is None:
            raise ValueError("the bank holds no GAN planes")
        if self._lut_gan is None:
            self._lut_gan = self.ops.bank_lut(GAN_MEAN, GAN_STD).to(self.bank.device)
            self._meta[3] = torch.tensor([_gt_label(f) for f in self._fnames], dtype=torch.int64)

    def _labels(self, indices):
        return self._meta[:, torch.as_tensor(indices, dtype=torch.int64)].to(self.bank.device, non_blocking=True)

    def _gan_dict(self, draws, indices, meta, sigma):
        d = {"Xs": self.ops.bank_gan_batch(self.bank.gan, draws, self._lut_gan)}
        if self.bank.centres is not None:
            hg, wg = self.bank.gan_size
            d["Ps"] = self.ops.bank_pose_batch(self.bank.centres, draws, hg, wg, sigma)
        d["Xs_path"] = [self._names[i] for i in indices]
        d["gt_label"] = meta[3]
        return d


class DeviceTrainLoader(_BankLoader):
    """`get_train_loader`'s IterLoader(DataLoader(Preprocessor(...))) on the bank: `next()`, `new_epoch()`, `__len__`, `__iter__`.

    trainset: the epoch's [(fname, pseudo_label, camid)] list, in the order the sampler's indices refer to (the reference passes
    `sorted(trainset)` to both); the labels live here, not in the bank.  `next()` returns the reference's batch,
    [imgs, fnames, pids, camids, indexes] or, with_gan, ([...], {'Xs', 'Ps' (bank with poses), 'Xs_path', 'gt_label'}): imgs /
    Xs / Ps fp32 device tensors, pids / camids / indexes / gt_label int64 device tensors, fnames / Xs_path lists of str.

    Draw order.  An epoch's index list is `list(sampler)` (None: `torch.randperm(len(trainset), generator=generator)`), cut into
    batches of `batch_size` (`drop_last` drops the short one).  For each batch, per sample in batch order: the flip
    (`torch.rand(1, generator) < 0.5` when flip_all), then PadRandomCropFlip.draw (top, then left, torch.randint on the same
    generator), then RandomErasing.draw (Python `random`).  The reference makes the same draws per sample in the same order, but in
    worker processes with their own generator states, so its sequence is not reproducible; this one is, from the seeds of `random`,
    `numpy.random` (sampler), torch's default generator (sampler) and `generator`.  `draws(indices) -> [N][7]` replaces the
    per-sample draws (tests).

    One `next()` is one kernel launch, three with_gan on a bank with poses; only the packed indices / draws (int32 [9 N]) and the
    labels (int64 [4, N]) cross from the host."""

    def __init__(self, bank, trainset, batch_size, sampler=None, length=None, height=None, width=None, padding=10,
                 erasing=RandomErasing(0.5, mean=[0.485, 0.456, 0.406]), flip_all=True, with_gan=False, generator=None,
                 drop_last=True, draws=None, sigma=6.0, ops=None):
        super(DeviceTrainLoader, self).__init__(bank, trainset, batch_size, ops)
        hs, ws = bank.reid_size
        self.height, self.width = int(hs if height is None else height), int(ws if width is None else width)
        self.padding = int(padding)
        self.sampler, self.length, self.drop_last = sampler, length, bool(drop_last)
        self.erasing, self.flip_all, self.with_gan, self.generator = erasing, bool(flip_all), bool(with_gan), generator
        self.draws, self.sigma = draws, float(sigma)
        self._crop = PadRandomCropFlip((self.height, self.width), self.padding, 0.0, generator=generator)
        if self.height > hs + 2 * self.padding or self.width > ws + 2 * self.padding:
            raise ValueError("crop %dx%d larger than the padded %dx%d plane" % (self.height, self.width, hs, ws))
        mean = [0.0, 0.0, 0.0] if erasing is None else [float(v) for v in erasing.mean]
        if len(mean) != 3:
            raise ValueError("erasing.mean must have three values")
        self._fill = torch.tensor(mean, dtype=torch.float32).to(bank.device)
        if self.with_gan:
            self._need_gan()
        self.iter = None

    def _epoch_indices(self):
        if self.sampler is not None:
            return [int(i) for i in self.sampler]
        return torch.randperm(len(self.entries), generator=self.generator).tolist()

    def _epoch_batches(self):
        order, bs = self._epoch_indices(), self.batch_size
        for s in range(0, len(order), bs):
            chunk = order[s:s + bs]
            if len(chunk) < bs and self.drop_last:
                return
            yield self._batch(chunk)

    def __len__(self):
        if self.length is not None:
            return self.length
        n = len(self.sampler) if self.sampler is not None else len(self.entries)
        return n // self.batch_size if self.drop_last else -(-n // self.batch_size)

    def __iter__(self):
        return self._epoch_batches()

    def new_epoch(self):
        self.iter = self._epoch_batches()

    def next(self):
        if self.iter is not None:
            try:
                return next(self.iter)
            except StopIteration:
                pass
        self.iter = self._epoch_batches()
        return next(self.iter)

    def _draw(self, n):
        hs, ws = self.bank.reid_size
        rows = []
        for _ in range(n):
            flip = 0
            if self.flip_all:
                flip = 1 if float(torch.rand(1, generator=self.generator)) < 0.5 else 0
            _, top, left = self._crop.draw(hs, ws)
            rect = (0, 0, 0, 0) if self.erasing is None else self.erasing.draw(3, self.height, self.width)
            rows.append((flip, top, left) + tuple(rect))
        return rows

    def _batch(self, indices):
        params = self._draw(len(indices)) if self.draws is None else self.draws(indices)
        params = torch.as_tensor(np.asarray(params, dtype=np.int64).reshape(len(indices), -1))
        draws = self.ops.bank_draws([self._rows[i] for i in indices], params, device=self.bank.device)
        meta = self._labels(indices)
        imgs = self.ops.bank_reid_batch(self.bank.reid, draws, self._lut, self._fill, (self.height, self.width), self.padding)
        reid = [imgs, [self._fnames[i] for i in indices], meta[0], meta[1], meta[2]]
        if not self.with_gan:
            return reid
        return reid, self._gan_dict(draws, indices, meta, self.sigma)


class _OrderedLoader(_BankLoader):
    def __len__(self):
        return -(-len(self.entries) // self.batch_size)

    def _chunks(self):
        for s in range(0, len(self.entries), self.batch_size):
            indices = list(range(s, min(s + self.batch_size, len(self.entries))))
            yield indices, self.ops.bank_draws([self._rows[i] for i in indices], None, device=self.bank.device), \
                self._labels(indices)


class DeviceTestLoader(_OrderedLoader):
    """`get_test_loader` on the bank: Resize -> ToTensor -> Normalize of `testset` in order, as (imgs, fnames, pids, camids,
    indexes) batches (the last one short) — what extract_features_device, DeviceEvaluator and DeviceCascadeEvaluator read."""

    def __iter__(self):
        for indices, draws, meta in self._chunks():
            imgs = self.ops.bank_reid_batch(self.bank.reid, draws, self._lut, self._fill0, self.bank.reid_size, 0)
            yield imgs, [self._fnames[i] for i in indices], meta[0], meta[1], meta[2]


class DeviceGanLoader(_OrderedLoader):
    """`get_gan_loader` (only_gan) on the bank: (gan_dict, pid, index) batches in order, unflipped, for `get_conf_weight`."""

    def __init__(self, bank, testset, batch_size, sigma=6.0, ops=None):
        super(DeviceGanLoader, self).__init__(bank, testset, batch_size, ops)
        self.sigma = float(sigma)
        self._need_gan()

    def __iter__(self):
        for indices, draws, meta in self._chunks():
            yield self._gan_dict(draws, indices, meta, self.sigma), meta[0], meta[2]
