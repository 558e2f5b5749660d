"""Step drivers — restates CC/clustercontrast/trainers.py (ClusterContrastTrainer :213-270,
ClusterContrastWithGANTrainer :15-210, GANTrainer :273-335), the joint ReID + GAN step that only exists in
CC/clustercontrast/trainers_b.py:617-814 (`train_all`) and the ReID warm-up loop of :1087-1138 (`train_reid`), on the HIP runtime.
`ClusterContrastWithGANTrainer.train` is the hard-mix loop of trainers.py:34-127 (`hard_mix_step`) when the memory is a
ClusterMemory_Gradient, the only memory its `ex_f=` call is valid for.

Same constructors, method names and arguments.  Differences that are scheduling only:
  * host->device copies are non-blocking; `loss.item()` (a device sync per step in the reference, :247)
    is deferred to the print interval unless `sync_every_step=True`;
  * the optimizer's gradient arena is all-reduced over RCCL (rg_hip.parallel.GradReducer) when
    torch.distributed is initialised — the reference used single-process DataParallel;
  * wandb / tensorboard writers are optional (not installed on the target machines).
The encoder's train-mode tuple output is accepted everywhere.

The epoch loop (meters, deferred readback, print line, wandb), the update tail of a single-optimizer step (`zero_grad`, backward,
reduce, `step`) and the batch's host->device copy are rg_hip/hostloop.py's, shared with reid/trainers.py; every loop here is
`_EncoderTrainer._epoch` over a step.  `joint_step` and `GANTrainer.train_gan` keep sequences of their own.
"""
from __future__ import print_function, absolute_import

import inspect
import time

import torch
import torch.nn as nn

from rg_hip import functional as RF, hostloop
from rg_hip.hostloop import AverageMeter
from rg_hip.nn import invalidate_folds
from rg_hip.parallel import GradReducer, attach_stage_hooks
from rg_hip.tape import backward as _backward

from .utils.data.diff_augs import my_transform


def _first(out):
    return out[0] if isinstance(out, (tuple, list)) else out


class _ReducerCache(object):
    """one GradReducer per optimizer object (created at the top of the first step — the trainers receive the optimizer per call,
    not at construction — so rank 0's broadcast precedes the first forward; no-op without torch.distributed)."""

    def __init__(self):
        self._r = {}

    def get(self, optimizer, modules=None):
        """`modules`: the networks this optimizer trains — rank 0's parameters and buffers are broadcast once when the
        reducer is created, so user-built replicas need not share a seed (rg_hip.parallel.GradReducer)."""
        r = self._r.get(id(optimizer))
        if r is None:
            r = self._r[id(optimizer)] = GradReducer(optimizer, modules=modules)
            if modules is not None:
                # the encoder's arena is reduced stage by stage from inside its backward program (layer4 first), not after it
                attach_stage_hooks(r, *(modules if isinstance(modules, (list, tuple)) else [modules]))
        return r


def intra_cl(q, k, temperature, group_size=16):
    """group contrast of trainers.py:200-210: logits[n, g] = sum over the g-th group of k of <q_n, k_m> / T."""
    from clustercontrast.models.cm import _MatmulT
    q = RF.normalize_rows(q)
    k = RF.normalize_rows(k)
    logits = _MatmulT.apply(q, k)
    qs, ks = logits.shape
    ones = torch.zeros(ks // group_size, ks, device=q.device)
    ones[torch.arange(ks, device=q.device) // group_size, torch.arange(ks, device=q.device)] = 1.0
    grouped = _MatmulT.apply(logits, ones)                         # sums each group of `group_size` keys
    targets = torch.arange(group_size, dtype=torch.long, device=q.device).repeat_interleave(group_size)
    return RF.cross_entropy_rows(grouped, targets, 1.0 / temperature)


class _EncoderTrainer(object):
    """What the two encoder trainers share: the reducer cache, the parsing of a ReID batch, the forward, and the epoch of
    `train_iters` draws from an IterLoader on the shell of rg_hip.hostloop."""

    def __init__(self, encoder, memory=None):
        super(_EncoderTrainer, self).__init__()
        self.encoder = encoder
        self.memory = memory
        self.sync_every_step = False
        self._reducers = _ReducerCache()

    def _epoch(self, epoch, data_loader, step, print_freq, train_iters, tail="", wandb_key=None):
        self.encoder.train()
        hostloop.run_epoch(epoch, (data_loader.next() for _ in range(train_iters)), train_iters, len(data_loader), step,
                           print_freq, self.sync_every_step, tail=tail, wandb_key=wandb_key)

    def _reducer(self, optimizer):
        """called BEFORE a step's forward: creating the reducer synchronises the replicas (rank-0 broadcast)"""
        return self._reducers.get(optimizer, self.encoder)

    def _parse_data(self, inputs):
        imgs, _, pids, _, indexes = inputs
        return hostloop.to_device(imgs, pids, indexes)

    def _forward(self, inputs, fuse=True):
        if fuse:
            return self.encoder(inputs)
        return self.encoder(inputs, fuse=fuse)


class ClusterContrastTrainer(_EncoderTrainer):
    def train(self, epoch, data_loader, optimizer, print_freq=10, train_iters=400, acc_iters=0):
        def step(inputs):
            inputs, labels, indexes = self._parse_data(inputs)
            return self.step(inputs, labels, optimizer)
        self._epoch(epoch, data_loader, step, print_freq, train_iters)

    def step(self, inputs, labels, optimizer):
        """One training step (reference loop body :229-244); returns the detached device loss."""
        reducer = self._reducer(optimizer)
        f_out = _first(self._forward(inputs))
        return hostloop.update(RF.weighted_mean(self.memory(f_out, labels)), optimizer, reducer)


class ClusterContrastPartTrainer(ClusterContrastTrainer):
    """The reference's multi-part recipe (trainers.py:79-93) without its GAN term, for the `resnet_mp50` encoder, whose train-mode
    forward returns (f_g, f_p1, f_p2, f_gc):

        loss = memory(f_gc, labels).mean() + intra_cl(f_p1, f_p1.detach()).mean() + intra_cl(f_p2, f_p2.detach()).mean()
               + intra_cl(f_g, f_g.detach()).mean()

    `group_size` (instances per identity in a batch; the batch size is group_size^2 in the reference's sampler) and `temperature`
    (its `opt.cl_temp`) are constructor arguments.

    Data-parallel reduction: the encoder has two branches behind `base` and its `base` is not a whole trunk, so
    rg_hip.parallel.attach_stage_hooks finds no trunk in it and no stage hook is placed; every parameter that received a gradient —
    `base`, `res_g`, `res_p`, the pooling exponent and the three head BatchNorm weights — is reduced exactly once by the
    end-of-backward `reduce()` of `step`."""

    def __init__(self, encoder, memory=None, group_size=16, temperature=0.05):
        super(ClusterContrastPartTrainer, self).__init__(encoder, memory)
        self.group_size = group_size
        self.T = temperature

    def step(self, inputs, labels, optimizer):
        reducer = self._reducer(optimizer)
        f_g, f_p1, f_p2, f_gc = self._forward(inputs)
        terms = [RF.weighted_mean(self.memory(f_gc, labels))]
        for f in (f_p1, f_p2, f_g):
            terms.append(RF.weighted_mean(intra_cl(f, f.detach(), self.T, self.group_size)))
        return hostloop.update(RF._WeightedSum.apply(torch.stack(terms), None, 1.0), optimizer, reducer)


class ClusterContrastWithGANTrainer(_EncoderTrainer):
    def __init__(self, encoder, GAN=None, writer=None, memory=None, opt=None):
        super(ClusterContrastWithGANTrainer, self).__init__(encoder, memory)
        if GAN is None:
            raise TypeError('GAN not implemented!')       # the reference's `raise('...')` is a TypeError too
        self.gan = GAN
        self.memoryb = memory
        self.writer = writer
        self.f_metric = nn.L1Loss()
        if opt is not None:
            self.opt = opt
            self.T = opt.cl_temp

    # ---- ReID-only step with the GAN's inputs staged (trainers.py:129-187) -----------------------
    def train_all(self, epoch, data_loader, optimizer, print_freq=10, train_iters=400, acc_iters=0, conf_weight=None,
                  joint=None):
        """`joint=None` follows trainers.py:129-187 when the GAN has no generator loss API and the joint step of
        trainers_b.py:617-814 when it has (`synthesize_p`, `get_loss_G`, `backward_D`)."""
        print("train both gan and reid")
        if joint is None:
            joint = all(hasattr(self.gan, a) for a in ("synthesize_p", "get_loss_G", "backward_D", "optimizer_G",
                                                       "optimizer_D"))

        def step(inputs):
            reid_inputs, labels, indexes = self._parse_data(inputs[0])
            self.gan.set_input(inputs[1])
            if joint:
                return self.joint_step(reid_inputs, labels, indexes, optimizer, conf_weight)
            return self._reid_only_step(reid_inputs, labels, optimizer)
        self._epoch(epoch, data_loader, step, print_freq, train_iters, tail="\n", wandb_key="total_loss")

    def _reid_only_step(self, reid_inputs, labels, optimizer):
        """the cluster-contrast update of trainers.py:129-187; the encoder's second output, if any, goes to the memory detached"""
        reducer = self._reducer(optimizer)
        out = self._forward(reid_inputs)
        f_gan = out[1] if isinstance(out, (tuple, list)) else None
        loss_ori = self.memory(_first(out), labels, gan_inputs=None if f_gan is None else f_gan.detach())
        return hostloop.update(RF.weighted_mean(loss_ori), optimizer, reducer)

    def joint_step(self, reid_inputs, labels, indexes, optimizer, conf_weight=None):
        """Joint ReID + GAN step, live lines of trainers_b.py:657-774: encode -> synthesize from the detached
        feature -> generator loss (D frozen) + confidence-weighted cluster-contrast loss -> D step -> one backward
        through G and the encoder -> both optimizers step."""
        gan = self.gan
        reducer = self._reducer(optimizer)                # rank-0 broadcast before the first forward, not after its backward
        out = self._forward(reid_inputs)
        f_out = _first(out)
        # train-mode encoders return (bn_x, normalize(feature map)) (CC/clustercontrast/models/resnet.py:107); the
        # committed loop passes that tuple straight to `.detach()`.  The generator's input is the map.
        f_gan = out[1] if isinstance(out, (tuple, list)) and len(out) > 1 and out[1] is not None else f_out
        gan.synthesize_p(f_gan.detach())
        loss_G = gan.get_loss_G(need_cm=False)
        if conf_weight is not None:
            conf_mask = conf_weight[indexes]
        else:
            conf_mask = None
        loss_cl = RF.weighted_mean(self.memory(f_out, labels), conf_mask)
        loss = RF._WeightedSum.apply(torch.stack([loss_cl, loss_G]), None, 1.0)

        gan.optimizer_D.zero_grad()
        gan.backward_D()
        gan.optimizer_D.step()

        gan.optimizer_G.zero_grad()
        optimizer.zero_grad()
        _backward(loss)
        reducer.reduce()
        gan.optimizer_G.step()
        optimizer.step()
        return loss.detach()

    def hard_mix_step(self, reid_inputs, labels, optimizer, group_size=None):
        """The hard-mix step, live lines of trainers.py:65-72, 96-98: encode the batch -> the GAN decodes one hard-mixed image per
        identity from the detached features (`synthesize_fc`) -> `my_transform` -> the encoder embeds those images in eval mode
        -> `memory(f_out, labels, ex_f=f_ex)`, the synthesised images as extra negatives with each row's own identity masked
        -> backward through the encoder's first pass only -> optimizer step.  Returns the detached device loss.

        `group_size` (default `opt.num_instances`): instances per identity; the batch must hold whole groups, checked before
        anything runs.  Under torch.distributed each rank mixes within its local batch.

        Scheduling only: the GAN branch and the second encoder pass take no part in the backward (the reference detaches both
        ends), so they run without a tape and keep no activations.  The GAN's modules stay in the mode the caller left them; the
        encoder's running statistics do not move in the eval pass, and its BatchNorm folds are redone for it on every call."""
        if group_size is None:
            group_size = self.opt.num_instances
        n = reid_inputs.shape[0]
        if group_size <= 0 or n % group_size:
            raise ValueError("hard_mix_step: a batch of %d is not whole identity groups of %d" % (n, group_size))
        reducer = self._reducer(optimizer)
        f_out = _first(self._forward(reid_inputs))
        f_ex = self._embed_hard_mix(f_out.detach(), group_size)
        return hostloop.update(self.memory(f_out, labels, ex_f=f_ex), optimizer, reducer)

    def _embed_hard_mix(self, f_out, group_size):
        """eval-mode embeddings of the GAN's hard-mixed images [identities, D], detached (trainers.py:66-70)"""
        encoder = self.encoder
        with torch.no_grad():
            fc_image = self.gan.synthesize_fc(f_out, group_size)
            x = my_transform(fc_image)
            # the train-mode pass above moved the running statistics behind the fold's key (rg_hip.nn.invalidate_folds)
            invalidate_folds(encoder)
            encoder.eval()
            try:
                return _first(self._forward(x)).detach()
            finally:
                encoder.train()

    def _takes_ex_f(self):
        return "ex_f" in inspect.signature(self.memory.forward).parameters

    def train(self, epoch, data_loader, optimizer, print_freq=10, train_iters=400, acc_iters=0):
        """trainers.py:34-127.  With a memory whose forward takes `ex_f` (ClusterMemory_Gradient, the script's
        `--learnable_memory` mode) this is the reference's loop on `hard_mix_step`.  With a ClusterMemory the reference's
        `memory(f_out, labels, ex_f=...)` is a TypeError; there the well-defined part, the cluster-contrast update with the GAN's
        inputs staged, is what runs (`train_all(joint=False)`)."""
        if not self._takes_ex_f():
            return self.train_all(epoch, data_loader, optimizer, print_freq, train_iters, acc_iters, joint=False)
        if getattr(self.gan, "use_adp", False):
            print("train adaptor and reid")
        group_size = self.opt.num_instances

        def step(inputs):
            reid_inputs, labels, _ = self._parse_data(inputs[0])
            self.gan.set_input(inputs[1])
            return self.hard_mix_step(reid_inputs, labels, optimizer, group_size)
        self._epoch(epoch, data_loader, step, print_freq, train_iters, tail="\n", wandb_key="reid_loss")

    def train_reid(self, epoch, data_loader, optimizer, print_freq=10, train_iters=400, acc_iters=0):
        """The ReID warm-up loop, trainers_b.py:1087-1138: `loss = memory(f_out, labels)` on the ReID half `inputs[0]` of every
        item, the GAN untouched.  A scalar loss (ClusterMemory_Gradient) is used as is; a per-row loss (ClusterMemory,
        reduction='none') is averaged — the reference's `loss.backward()` on that vector is a RuntimeError (grad can be implicitly
        created only for scalar outputs), so its loop only ever ran with the scalar."""
        print("warm up stage for reid")

        def step(inputs):
            reid_inputs, labels, _ = self._parse_data(inputs[0])
            return self._warm_up_step(reid_inputs, labels, optimizer)
        self._epoch(epoch, data_loader, step, print_freq, train_iters)

    def _warm_up_step(self, reid_inputs, labels, optimizer):
        reducer = self._reducer(optimizer)
        loss = self.memory(_first(self._forward(reid_inputs)), labels)
        return hostloop.update(RF.weighted_mean(loss) if loss.dim() else loss, optimizer, reducer)

    def intra_cl(self, q, k, group_size=16):
        """group contrast of trainers.py:200-210 at this trainer's temperature (the module-level `intra_cl`)."""
        return intra_cl(q, k, self.T, group_size)


class GANTrainer(object):
    def __init__(self, GAN=None, encoder=None, writer=None, opt=None):
        super(GANTrainer, self).__init__()
        if GAN is None:
            raise TypeError('GAN not implemented!')
        self.gan = GAN
        self.encoder = encoder
        self.writer = writer
        if opt is not None:
            self.opt = opt
            self.T = opt.cl_temp

    def train_gan(self, epoch, data_loader, print_freq=10, train_iters=400, acc_iters=0):
        print("train gan")
        batch_time = AverageMeter()
        data_time = AverageMeter()
        end = time.time()
        gan_losses = {'G': 0.0, 'D': 0.0}
        for i in range(train_iters):
            inputs = data_loader.next()
            data_time.update(time.time() - end)
            self.gan.set_input(inputs)
            self.gan.optimize_parameters()

            if self.writer is not None or (i + 1) % print_freq == 0:
                gan_losses = self.gan.get_current_errors()
            if self.writer is not None:
                total_steps = acc_iters + i
                self.writer.add_scalar('Loss/G_loss', gan_losses['G'], total_steps)
                self.writer.add_scalar('Loss/D_loss', gan_losses['D'], total_steps)

            batch_time.update(time.time() - end)
            end = time.time()
            if (i + 1) % print_freq == 0:
                hostloop.wandb_log({"GANLoss_G": gan_losses['G'], "GANLoss_D": gan_losses['D']})
                print('Epoch: [{}][{}/{}]\t'
                      'Time {:.3f} ({:.3f})\t'
                      'Data {:.3f} ({:.3f})\t'
                      'GANLoss: G:{:.3f} D:{:.3f}\n'
                      .format(epoch, i + 1, len(data_loader),
                              batch_time.val, batch_time.avg,
                              data_time.val, data_time.avg,
                              gan_losses['G'], gan_losses['D']))
