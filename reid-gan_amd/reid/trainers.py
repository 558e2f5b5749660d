"""Stage-I step driver — restates FD-GAN-master/reid/trainers.py (BaseTrainer :11-60, SiameseTrainer :62-73) on the HIP runtime:
the trainer of `baseline.py`, which produces the checkpoint FD-GAN's stages II and III load into `net_E`.

Same constructor, method names, arguments and printed line.  Differences that are scheduling only (the ones
clustercontrast/trainers.py documents):
  * host->device copies are non-blocking and go to `rg_hip.search.device()`;
  * loss and precision stay on the device and reach the meters once per print interval (`loss.data[0]`, a device sync per step
    in the reference, :34) unless `sync_every_step=True`;
  * `step(imgs1, imgs2, targets, optimizer)` is the loop body, `train` a loop over it: the epoch loop, the update tail of a step
    and the batch's host->device copy are rg_hip/hostloop.py's, shared with clustercontrast/trainers.py;
  * `_forward` runs SiameseNet.forward_loss — both trunk passes, the verification head, nn.CrossEntropyLoss() and `accuracy` as
    one tape program with the head on csrc/verif_head.hip — when the model is a SiameseNet (bare or as `.module` of a
    DataParallel wrapper) whose embed model has BatchNorm and classifier, and the criterion is an nn.CrossEntropyLoss with default
    settings.  Anything else, or `fused_head=False`, runs the reference's three lines on the composed layers.  Both return
    (loss, prec) with the same meaning; `prec` counts a tie of the two logits for class 0 on the fused path, where torch.topk
    leaves it unspecified.  The two differ for a target outside [0, num_classes) (possible only with a head of one class): the
    criterion raises, or for -100 averages over the kept rows; the fused path gives such a row loss 0 and no gradient and still
    divides by the batch size (the rule of rg_softmax_ce_fwd).  Pair targets are 0 / 1 and `baseline.py`'s head has two classes.

Data parallelism over torch.distributed is not built: a SiameseNet in train mode runs its trunk twice on one tape, and the
stage-hook gradient reducer takes a stage's first gradient of a step for its final one.  With a world size
above 1 the trainer raises before the first forward.
"""
from __future__ import print_function, absolute_import

import torch.distributed as dist
from torch import nn

from rg_hip import hostloop, parallel

from .evaluation_metrics import accuracy
from .models.multi_branch import SiameseNet


def _plain_cross_entropy(criterion):
    return (type(criterion) is nn.CrossEntropyLoss and criterion.weight is None and criterion.reduction == 'mean'
            and criterion.ignore_index == -100 and getattr(criterion, "label_smoothing", 0.0) == 0.0)


class BaseTrainer(object):
    def __init__(self, model, criterion, num_classes=0, num_instances=4, fused_head=True):
        super(BaseTrainer, self).__init__()
        self.model = model
        self.criterion = criterion
        self.num_classes = num_classes
        self.num_instances = num_instances
        self.fused_head = fused_head
        self.sync_every_step = False

    def train(self, epoch, data_loader, optimizer, base_lr=0.1, print_freq=1):
        self.model.train()

        def step(inputs):
            inputs, targets = self._parse_data(inputs)
            return self.step(inputs[0], inputs[1], targets, optimizer), targets.size(0)
        n_batches = len(data_loader)
        hostloop.run_epoch(epoch, data_loader, n_batches, n_batches, step, print_freq, self.sync_every_step,
                           columns=hostloop.LOSS + (("Prec", "{:.2%} ({:.2%})"),), tail="\t")

    def step(self, imgs1, imgs2, targets, optimizer):
        """One training step (reference loop body :32-39); returns the detached device (loss, prec), both 0-d."""
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            raise NotImplementedError(
                "reid.trainers: stage I under torch.distributed is not built — a SiameseNet in train mode runs its trunk twice on "
                "one tape, which the stage-hook gradient reducer does not reduce correctly (ADVICE.md item 1); run one process")
        loss, prec1 = self._forward([imgs1, imgs2], targets)
        return hostloop.update(loss, optimizer), prec1.detach().reshape(())

    def _parse_data(self, inputs):
        raise NotImplementedError

    def _forward(self, inputs, targets):
        raise NotImplementedError


class SiameseTrainer(BaseTrainer):
    def _parse_data(self, inputs):
        (imgs1, _, pids1, _), (imgs2, _, pids2, _) = inputs
        targets, imgs1, imgs2 = hostloop.to_device((pids1 == pids2).long(), imgs1, imgs2)
        return [imgs1, imgs2], targets

    def _siamese(self):
        """the SiameseNet whose fused program `_forward` may take, or None"""
        if not self.fused_head or not _plain_cross_entropy(self.criterion):
            return None
        net = self.model
        if isinstance(net, (nn.DataParallel, parallel.DataParallel)):
            net = net.module
        if isinstance(net, SiameseNet) and getattr(net.embed_model, "has_fused_loss", False):
            return net
        return None

    def _forward(self, inputs, targets):
        net = self._siamese()
        if net is not None:
            _, _, _, loss, prec1 = net.forward_loss(inputs[0], inputs[1], targets)
            return loss, prec1
        _, _, outputs = self.model(*inputs)
        loss = self.criterion(outputs, targets)
        prec1, = accuracy(outputs.data, targets.data)
        return loss, prec1[0]
