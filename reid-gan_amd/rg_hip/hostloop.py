"""The host side of a training epoch and of a feature-extraction pass, stated once for clustercontrast/trainers.py,
reid/trainers.py and the two evaluators.py: the meter, the epoch loop shell with its deferred readback, the single-optimizer
update tail, the host->device copy of a batch and the feature collection loop.  Imports nothing from the model packages."""
from __future__ import print_function, absolute_import

import time
from collections import OrderedDict

import torch

from . import search
from .tape import backward as _backward

try:                                    # optional observability, never on the hot path
    import wandb as _wandb
except Exception:                       # pragma: no cover
    _wandb = None


class AverageMeter(object):
    __slots__ = ("val", "sum", "count")

    def __init__(self):
        self.val, self.sum, self.count = 0, 0, 0

    reset = __init__

    @property
    def avg(self):
        return self.sum / self.count if self.count else 0

    def update(self, value, n=1):
        self.val = value
        self.sum = self.sum + value * n
        self.count = self.count + n


def wandb_log(values):
    if _wandb is not None and getattr(_wandb, "run", None) is not None:
        _wandb.log(values)


LOSS = (("Loss", "{:.3f} ({:.3f})"),)


def run_epoch(epoch, batches, n_iters, shown, step, print_freq=10, sync_every_step=False, columns=LOSS, tail="", wandb_key=None):
    """The loop shell of every trainer's epoch: the reference's meters and `Epoch: [..][../..]` line, with `loss.item()` (a device
    sync per step there) deferred to one stacked device->host transfer per flush.  A flush is due at every step when
    `sync_every_step`, else at a print interval and at iteration `n_iters`.

    batches: iterable of batches; shown: the denominator of the line (`len(data_loader)`); step(batch): a 0-d device tensor, or
    (one 0-d device tensor per column, weight); columns: (name, format of `val, avg`) pairs; wandb_key: the first column is
    logged under it, value by value.  Returns the columns' meters."""
    batch_time, data_time = AverageMeter(), AverageMeter()
    meters = [AverageMeter() for _ in columns]
    line = "Epoch: [{}][{}/{}]\tTime {:.3f} ({:.3f})\tData {:.3f} ({:.3f})" + "".join("\t%s %s" % c for c in columns) + tail
    pending = []
    end = time.time()
    for i, batch in enumerate(batches):
        data_time.update(time.time() - end)

        out = step(batch)
        pending.append((torch.stack(out[0]), out[1]) if isinstance(out, tuple) else (out.reshape(1), 1))
        if sync_every_step or (i + 1) % print_freq == 0 or i + 1 == n_iters:
            rows = torch.stack([r for r, _ in pending]).tolist()        # one device->host transfer for the interval
            for row, (_, n) in zip(rows, pending):
                for m, v in zip(meters, row):
                    m.update(v, n)
                if wandb_key is not None:
                    wandb_log({wandb_key: row[0]})
            pending = []

        batch_time.update(time.time() - end)
        end = time.time()

        if (i + 1) % print_freq == 0:
            print(line.format(epoch, i + 1, shown, batch_time.val, batch_time.avg, data_time.val, data_time.avg,
                              *[x for m in meters for x in (m.val, m.avg)]))
    return meters


def update(loss, optimizer, reducer=None):
    """The tail of a single-optimizer step; returns the detached device loss.  `reducer` (rg_hip.parallel.GradReducer) was
    fetched by the caller BEFORE its first forward: creating it broadcasts rank 0's replica."""
    optimizer.zero_grad()
    _backward(loss)
    if reducer is not None:
        reducer.reduce()
    optimizer.step()
    return loss.detach()


def to_device(*tensors):
    """non-blocking host->device copies of a batch's tensors, in order"""
    dev = search.device()
    return tuple(t.to(dev, non_blocking=True) for t in tensors)


class DeviceFeatures(object):
    """What `extract_features_device` returns: all features as one [N, D] device tensor plus fname -> row.  `features[fname]`
    is a row view, so the object also serves where the reference's OrderedDict of features is read."""

    def __init__(self, matrix, index):
        self.matrix, self.index = matrix, index

    def __getitem__(self, fname):
        return self.matrix[self.index[fname]]

    def __len__(self):
        return len(self.index)

    def rows(self, entries):
        """[len(entries), D] device block of the (fname, pid, cam) triples, one gather"""
        idx = torch.as_tensor([self.index[f] for f, _, _ in entries], dtype=torch.int64).to(self.matrix.device)
        return self.matrix.index_select(0, idx).view(len(entries), -1).float().contiguous()


def collect_features(model, data_loader, print_freq):
    """The reference's `extract_features` loop with the features kept on the device: (DeviceFeatures, labels).  Reads the first
    three fields of a batch (imgs, fnames, pids), so the loaders' 4-tuples and 5-tuples both work."""
    model.eval()
    batch_time, data_time = AverageMeter(), AverageMeter()
    blocks, index, labels, base = [], OrderedDict(), OrderedDict(), 0
    end = time.time()
    with torch.no_grad():
        for i, batch in enumerate(data_loader):
            data_time.update(time.time() - end)
            outputs = model(to_device(torch.as_tensor(batch[0]))[0]).data
            blocks.append(outputs.reshape(outputs.shape[0], -1))
            for k, (fname, pid) in enumerate(zip(batch[1], batch[2])):
                index[fname] = base + k
                labels[fname] = pid
            base += outputs.shape[0]
            batch_time.update(time.time() - end)
            end = time.time()
            if (i + 1) % print_freq == 0:
                print('Extract Features: [{}/{}]\t'
                      'Time {:.3f} ({:.3f})\t'
                      'Data {:.3f} ({:.3f})\t'
                      .format(i + 1, len(data_loader),
                              batch_time.val, batch_time.avg,
                              data_time.val, data_time.avg))
    return DeviceFeatures(torch.cat(blocks, 0), index), labels
