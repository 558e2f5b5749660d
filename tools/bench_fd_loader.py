"""The input side of an FD-GAN stage-II step (bench configuration 2: 16 pairs of 256x128, 18 joints), measured in ONE process on a
synthetic set (128x64 JPEGs and landmark files written with PIL into a temporary directory from a seed):
    python tools/bench_fd_loader.py [--ids 256] [--per-id 4] [--pairs 16] [--reps 30] [--steps 12] [--workers N] [--out FILE]
    python tools/bench_fd_loader.py --stage1 [...]      the input side of a stage-I step instead (see `stage1` below)

  bank build          DeviceImageBank.from_files(reid_resample='bilinear', pose_root=...): one decode + RectScale per image, the
                      landmark table, the upload
  bank next()         one DevicePairLoader batch: wall clock around a synchronised call (host draws, one copy, two launches), and the
                      two kernels alone with device events on one staged set of draws; the pose kernel a second time with its output
                      offset by one float, which selects its 4-byte stores (the 16-byte path needs a 16-byte aligned output)
  host next()         the pipeline the reference's train.py runs, written here from PIL + oracle.ref_datagen.o_generate_pose_map
                      because torchvision is not installed: decode -> RectScale -> eraser -> flip -> ToTensor / Normalize, the second
                      decode, `_load_landmark`, eighteen scipy Gaussian filters, through a torch DataLoader with 0 and with --workers
                      worker processes, then the copy to the device.  The MEAN over consecutive batches is its throughput
  step                FDGANModel stage-2 optimize_parameters() fed by each: wall clock per step and the part spent waiting for data
Every figure is a MEDIAN of --reps unless it says otherwise; nothing is compared with a threshold."""
import argparse
import os
import random
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "reid-gan_amd"))
import torch  # noqa: E402
from PIL import Image  # noqa: E402

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
H, W, J = 256, 128, 18
LINES = []


def say(text):
    print(text, flush=True)
    LINES.append(text)


def median(v):
    return sorted(v)[len(v) // 2]


def write_set(root, ids, per_id, seed=0):
    """images/ and poses/ under root -> (trainval, pid_imgs)"""
    g = np.random.RandomState(seed)
    os.mkdir(os.path.join(root, "images"))
    os.mkdir(os.path.join(root, "poses"))
    yy, xx = np.mgrid[0:128, 0:64]
    trainval, pid_imgs = [], {}
    for pid in range(ids):
        for k in range(per_id):
            cam = int(g.randint(0, 6))
            name = "%08d_%02d_%04d.jpg" % (pid, cam, k)
            base = np.stack([(yy * 2 + 13 * pid) % 256, (xx * 4 + 40 * cam) % 256, (yy + xx + pid) % 256], axis=2)
            img = np.clip(base + g.randint(-25, 25, size=(128, 64, 3)), 0, 255).astype(np.uint8)
            Image.fromarray(img).save(os.path.join(root, "images", name), quality=90)
            rows, cols = g.uniform(0, 127, size=J), g.uniform(0, 63, size=J)
            rows[g.randint(0, J)] = cols[g.randint(0, J)] = -1.0
            with open(os.path.join(root, "poses", name[:-4] + ".txt"), "w") as f:
                f.write("".join("%.3f %.3f\n" % (r, c) for r, c in zip(rows, cols)))
            trainval.append((name, pid, cam))
            pid_imgs.setdefault(pid, []).append(name)
    return trainval, pid_imgs


class HostPairs(torch.utils.data.Dataset):
    """The reference's Preprocessor(with_pose=True), step by step in PIL + torch + scipy; indexed by a pair, as its DataLoader is"""

    def __init__(self, trainval, pid_imgs, root, pose_aug):
        from reid.utils.data.device_pairs import FDRandomErase
        self.trainval, self.pid_imgs, self.root, self.pose_aug = trainval, pid_imgs, root, pose_aug
        self.erase = FDRandomErase()
        self.mean, self.std = torch.tensor(MEAN).view(3, 1, 1), torch.tensor(STD).view(3, 1, 1)

    def __len__(self):
        return len(self.trainval)

    def tensor(self, img):
        return torch.from_numpy(np.asarray(img).copy()).permute(2, 0, 1).contiguous().float().div(255).sub_(self.mean).div_(self.std)

    def one(self, index):
        from oracle.ref_datagen import o_generate_pose_map
        from reid.utils.data.device_pairs import read_landmarks
        fname, pid, _ = self.trainval[index]
        img = Image.open(os.path.join(self.root, "images", fname)).convert("RGB").resize((W, H), Image.BILINEAR)
        rect = self.erase.draw(H, W)
        if rect is not None and rect[2] > 0:
            r0, c0, eh, ew, rgb = rect
            img.paste(Image.new("RGB", (ew, eh), (rgb & 255, (rgb >> 8) & 255, (rgb >> 16) & 255)), (c0, r0))
        if torch.rand(1) < 0.5:
            img = img.transpose(Image.FLIP_LEFT_RIGHT)
        names = list(self.pid_imgs[pid])
        if fname in names and len(names) > 1:
            names.remove(fname)
        pname = os.path.splitext(random.choice(names))[0]
        gt = Image.open(os.path.join(self.root, "images", pname + ".jpg")).convert("RGB")
        lm = read_landmarks(os.path.join(self.root, "poses", pname + ".txt"), H / gt.size[1], W / gt.size[0])
        maps = o_generate_pose_map(lm, H, W, self.pose_aug)
        if random.choice([True, False]):
            gt, maps = gt.transpose(Image.FLIP_LEFT_RIGHT), np.flip(maps, 2)
        return {"origin": self.tensor(img), "target": self.tensor(gt.resize((W, H), Image.BILINEAR)),
                "posemap": torch.from_numpy(maps.copy()).float(), "pid": torch.LongTensor([pid])}

    def __getitem__(self, pair):
        return [self.one(pair[0]), self.one(pair[1])]


class HostIter(object):
    """an endless iterator over the host DataLoader, with the copy of the batch to the device"""

    def __init__(self, loader, dev):
        self.loader, self.dev, self.it = loader, dev, None

    def next(self):
        if self.it is None:
            self.it = iter(self.loader)
        try:
            b = next(self.it)
        except StopIteration:
            self.it = iter(self.loader)
            b = next(self.it)
        return tuple({k: v.to(self.dev, non_blocking=True) for k, v in d.items()} for d in b)


class BankIter(object):
    def __init__(self, loader):
        self.loader, self.it = loader, None

    def next(self):
        if self.it is None:
            self.it = iter(self.loader)
        try:
            return next(self.it)
        except StopIteration:
            self.it = iter(self.loader)
            return next(self.it)


def wall(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return ts


def events(fn, reps):
    for _ in range(3):
        fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    torch.cuda.synchronize()
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return median([a.elapsed_time(b) for a, b in ev]) * 1e3


def fed_steps(feed, model, steps, warm=2):
    for _ in range(warm):
        model.set_input(feed.next())
        model.optimize_parameters()
    torch.cuda.synchronize()
    data = 0.0
    t0 = time.perf_counter()
    for _ in range(steps):
        t1 = time.perf_counter()
        batch = feed.next()
        data += time.perf_counter() - t1
        model.set_input(batch)
        model.optimize_parameters()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3, data / steps * 1e3


class HostStage1(torch.utils.data.Dataset):
    """baseline.py's Preprocessor with its train transform, step by step in PIL + torch (torchvision is not installed), indexed by a
    pair as its DataLoader is.  Deliberately written from PIL and the stage-II eraser alone, not from the device loader's code:
    it is the host path a run without the raw bank has."""

    def __init__(self, train_set, root):
        from reid.utils.data.device_pairs import FDRandomErase
        self.train_set, self.root = train_set, root
        self.erase = FDRandomErase()
        self.mean, self.std = torch.tensor(MEAN).view(3, 1, 1), torch.tensor(STD).view(3, 1, 1)

    def __len__(self):
        return len(self.train_set)

    def one(self, index):
        fname, pid, camid = self.train_set[index]
        img = Image.open(os.path.join(self.root, "images", fname)).convert("RGB")
        for _ in range(10):                                            # RandomSizedRectCrop
            target = random.uniform(0.64, 1.0) * img.size[0] * img.size[1]
            ratio = random.uniform(2, 3)
            h, w = int(round((target * ratio) ** 0.5)), int(round((target / ratio) ** 0.5))
            if w <= img.size[0] and h <= img.size[1]:
                x1, y1 = random.randint(0, img.size[0] - w), random.randint(0, img.size[1] - h)
                img = img.crop((x1, y1, x1 + w, y1 + h))
                break
        if img.size != (W, H):
            img = img.resize((W, H), Image.BILINEAR)
        rect = self.erase.draw(H, W)
        if rect is not None and rect[2] > 0:
            r0, c0, eh, ew, rgb = rect
            img.paste(Image.new("RGB", (ew, eh), (rgb & 255, (rgb >> 8) & 255, (rgb >> 16) & 255)), (c0, r0))
        if torch.rand(1) < 0.5:
            img = img.transpose(Image.FLIP_LEFT_RIGHT)
        t = torch.from_numpy(np.asarray(img).copy()).permute(2, 0, 1).contiguous().float().div(255).sub_(self.mean).div_(self.std)
        return t, fname, pid, camid

    def __getitem__(self, pair):
        return [self.one(pair[0]), self.one(pair[1])]


def siamese_steps(feed, trainer, opt, steps, warm=2):
    """ms per SiameseTrainer.step fed by feed.next(), and the part spent waiting for the batch"""
    def one():
        t1 = time.perf_counter()
        batch = feed.next()
        waited = time.perf_counter() - t1
        (imgs1, imgs2), targets = trainer._parse_data(batch)
        trainer.step(imgs1, imgs2, targets, opt)
        return waited
    for _ in range(warm):
        one()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    data = sum(one() for _ in range(steps))
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3, data / steps * 1e3


def stage1(args):
    """FD-GAN stage I (baseline.py's defaults: 256 pairs of 256x128 from 128x64 sources, np_ratio 3): the raw bank's kernel and
    loader, the host pipeline on one thread and on --workers processes, and SiameseTrainer.step fed by each"""
    from clustercontrast.utils.data.device_bank import DeviceRawBank, default_workers
    from reid.utils.data.device_pairs import RandomPairSampler
    from reid.utils.data.device_stage1 import DeviceStage1Loader
    from rg_hip import ops
    dev = torch.device("cuda:0")
    workers = default_workers() if args.workers is None else args.workers
    B = args.pairs
    root = tempfile.mkdtemp(prefix="rg_fd1_")
    try:
        train_set, _ = write_set(root, args.ids, args.per_id)
        say("FD-GAN stage I.  synthetic set: %d images of %d identities, 128x64 JPEGs; %d pairs (%d images) of %dx%d per batch, "
            "np_ratio 3, %d host workers of %d CPUs" % (len(train_set), args.ids, B, 2 * B, H, W, workers, len(os.sched_getaffinity(0))))
        t0 = time.perf_counter()
        bank = DeviceRawBank.from_files(train_set, os.path.join(root, "images"), workers, dev, (H, W))
        torch.cuda.synchronize()
        say("raw bank build (once)      %.2f s (%.0f images/s, %d threads); %.1f MB on the device, of which tables %.3f MB"
            % (time.perf_counter() - t0, len(train_set) / (time.perf_counter() - t0), workers, bank.nbytes / 1e6,
               (bank.table_x.numel() + bank.table_y.numel()) * 4 / 1e6))
        random.seed(1), np.random.seed(2), torch.manual_seed(3)
        loader = DeviceStage1Loader(bank, train_set, B, neg_pos_ratio=3)
        feed = BankIter(loader)
        bank_ms = median(wall(feed.next, args.reps)) * 1e3
        say("per batch of %d pairs" % B)
        say("bank next()              %9.3f ms wall (host draws, one copy of the draws, one of the ids, one launch; synchronised)" % bank_ms)
        rows = [loader._item(i % len(train_set)) for i in range(2 * B)]
        d = ops.fd_crop_draws(torch.tensor(rows), device=dev)
        nb = 2 * B * 3 * H * W * 4
        us = events(lambda: ops.bank_fd_crop_batch(bank, d, loader._lut), args.reps)
        say("  %-38s %9.1f us device events   %.2f TB/s of output (%.1f MB written); regime %s, %d crop rows at most"
            % ("rg_bank_fd_crop_batch", us, nb / us / 1e6, nb / 1e6,
               "whole" if ops.fd_crop_regime(max(r[4] for r in rows), W) == ops.FD_CROP_WHOLE else "strips", max(r[4] for r in rows)))
        t0 = time.perf_counter()
        for _ in range(args.reps):
            [loader._item(i % len(train_set)) for i in range(2 * B)]
        say("  %-38s %9.3f ms (Python: crop, eraser and flip of %d items)" % ("host draws alone", (time.perf_counter() - t0) / args.reps * 1e3, 2 * B))
        host = {}
        for nw in (0, workers):
            random.seed(1), np.random.seed(2), torch.manual_seed(3)
            dl = torch.utils.data.DataLoader(HostStage1(train_set, root), batch_size=B, num_workers=nw,
                                             sampler=RandomPairSampler(train_set, 3), pin_memory=True, persistent_workers=nw > 0,
                                             multiprocessing_context="spawn" if nw > 0 else None)
            host[nw] = BankIter(dl)                                 # SiameseTrainer._parse_data copies host tensors itself

            def take(f=host[nw]):
                (a, _, _, _), (b, _, _, _) = f.next()
                a.to(dev, non_blocking=True), b.to(dev, non_blocking=True)
            reps = args.reps if nw else max(3, args.reps // 10)             # one thread: about a second per batch
            ts = wall(take, reps, warm=3 if nw else 1)
            mean = sum(ts) / len(ts) * 1e3
            say("host next() %2d workers    %9.3f ms per batch over %d consecutive batches = %.0f images/s (median wait %.3f ms; copy to "
                "the device included)   host / bank %.1f" % (nw, mean, len(ts), 2 * B / mean * 1e3, median(ts) * 1e3, mean / bank_ms))
        if not args.no_model:
            import reid.models as RM
            from reid.models.embedding import EltwiseSubEmbed
            from reid.models.multi_branch import SiameseNet
            from reid.trainers import SiameseTrainer
            torch.manual_seed(0)
            net = SiameseNet(RM.create("resnet50", pretrained=False, cut_at_pooling=True),
                             EltwiseSubEmbed(use_batch_norm=True, use_classifier=True, num_features=2048, num_classes=2)).to(dev).train()
            opt = torch.optim.SGD([{"params": net.base_model.parameters(), "lr_mult": 1.0}, {"params": net.embed_model.parameters(), "lr_mult": 1.0}],
                                  0.01, momentum=0.9, weight_decay=5e-4)
            trainer = SiameseTrainer(net, torch.nn.CrossEntropyLoss())
            say("SiameseTrainer.step (ResNet-50, torch SGD) at %d pairs, %d consecutive steps: ms per step, of which waiting for the batch"
                % (B, args.steps))
            steps = {}
            for name, f in [("bank", feed), ("host, %d workers" % workers, host[workers])]:
                steps[name], data = siamese_steps(f, trainer, opt, args.steps)
                say("  fed by the %-17s loader   %8.2f ms per step   Data %8.3f ms" % (name, steps[name], data))
            say("device batch below the step it feeds: %s (%.3f ms against %.2f ms)"
                % ("yes" if bank_ms < steps["bank"] else "NO", bank_ms, steps["bank"]))
    finally:
        shutil.rmtree(root, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--stage1", action="store_true", help="stage I (baseline.py) instead of stage II; --pairs defaults to 256")
    ap.add_argument("--ids", type=int, default=256)
    ap.add_argument("--per-id", type=int, default=4)
    ap.add_argument("--pairs", type=int, default=None, help="pairs per batch: 16 (stage II), 256 with --stage1")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--workers", type=int, default=None)
    ap.add_argument("--pose-aug", default="gauss")
    ap.add_argument("--no-model", action="store_true", help="skip the FDGANModel steps")
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_fd_loader.py needs the GPU"
    if args.pairs is None:
        args.pairs = 256 if args.stage1 else 16
    if args.stage1:
        stage1(args)
        if args.out:
            with open(args.out, "w") as f:
                f.write("\n".join(LINES) + "\n")
        return
    from clustercontrast.utils.data.device_bank import DeviceImageBank, default_workers
    from reid.utils.data.device_pairs import DevicePairLoader, RandomPairSampler
    from rg_hip import ops
    from rg_hip.lib import lib
    dev = torch.device("cuda:0")
    workers = default_workers() if args.workers is None else args.workers
    B = args.pairs
    root = tempfile.mkdtemp(prefix="rg_fd_")
    try:
        trainval, pid_imgs = write_set(root, args.ids, args.per_id)
        say("synthetic set: %d images of %d identities, 128x64 JPEGs, %d landmarks each; %d pairs of %dx%d per batch, pose_aug %s, "
            "%d host workers of %d CPUs" % (len(trainval), args.ids, J, B, H, W, args.pose_aug, workers, len(os.sched_getaffinity(0))))
        t0 = time.perf_counter()
        bank = DeviceImageBank.from_files(trainval, os.path.join(root, "images"), (H, W), None, workers=workers, device=dev,
                                          reid_resample="bilinear", pose_root=os.path.join(root, "poses"))
        torch.cuda.synchronize()
        say("bank build (once)          %.2f s (%.0f images/s, %d threads); %.1f MB on the device"
            % (time.perf_counter() - t0, len(trainval) / (time.perf_counter() - t0), workers, bank.nbytes / 1e6))
        random.seed(1), np.random.seed(2), torch.manual_seed(3)
        loader = DevicePairLoader(bank, trainval, pid_imgs, B, neg_pos_ratio=3, pose_aug=args.pose_aug)
        feed = BankIter(loader)
        ts = wall(feed.next, args.reps)
        bank_ms = median(ts) * 1e3
        say("per batch of %d pairs (%d image rows, %d map rows)" % (B, 4 * B, 2 * B))
        say("bank next()              %9.3f ms wall (host draws, one copy, two launches; synchronised)" % bank_ms)
        # the kernels alone: one staged set of draws, launched back to back
        it = [loader._item(i % len(trainval)) for i in range(2 * B)]
        d = ops.fd_draws(torch.tensor([t[0] for t in it] + [t[2] for t in it]),
                         torch.tensor([t[1] for t in it] + [(t[3][0], 0, 0, 0, 0, 0, 0, 0) for t in it]),
                         torch.tensor([t[2] for t in it]), torch.tensor([t[3] for t in it]), device=dev)
        nb_img, nb_map = 4 * B * 3 * H * W * 5, 2 * B * J * H * W * 4
        us = events(lambda: ops.bank_fd_image_batch(bank.reid, d, loader._lut), args.reps)
        say("  %-38s %9.1f us device events   %.2f TB/s (%.1f MB written + read)" % ("rg_bank_fd_image_batch", us, nb_img / us / 1e6, nb_img / 1e6))
        us = events(lambda: ops.bank_fd_pose_batch(bank.landmarks, d, H, W), args.reps)
        say("  %-38s %9.1f us device events   %.2f TB/s (%.1f MB written)" % ("rg_bank_fd_pose_batch, 16-byte stores", us, nb_map / us / 1e6, nb_map / 1e6))
        buf = torch.empty(2 * B * J * H * W + 4, dtype=torch.float32, device=dev)
        stream = torch.cuda.current_stream().cuda_stream
        us = events(lambda: lib.rg_bank_fd_pose_batch(bank.landmarks.data_ptr(), len(trainval), J, d.pose_idx_dev.data_ptr(),
                                                      d.pose_params_dev.data_ptr(), buf.data_ptr() + 4, 2 * B, H, W, stream), args.reps)
        say("  %-38s %9.1f us device events   %.2f TB/s" % ("rg_bank_fd_pose_batch, 4-byte stores", us, nb_map / us / 1e6))
        # the host pipeline
        host = {}
        for nw in (0, workers):
            random.seed(1), np.random.seed(2), torch.manual_seed(3)
            dl = torch.utils.data.DataLoader(HostPairs(trainval, pid_imgs, root, args.pose_aug), batch_size=B, num_workers=nw,
                                             sampler=RandomPairSampler(trainval, 3), pin_memory=True, persistent_workers=nw > 0,
                                             multiprocessing_context="spawn" if nw > 0 else None)
            host[nw] = HostIter(dl, dev)
            reps = args.reps if nw else max(3, args.reps // 10)             # one thread: seconds per batch
            ts = wall(host[nw].next, reps, warm=3 if nw else 1)
            mean = sum(ts) / len(ts) * 1e3
            say("host next() %2d workers    %9.3f ms per batch over %d consecutive batches = %.0f samples/s (median wait %.3f ms; copy to "
                "the device included)   host / bank %.1f" % (nw, mean, len(ts), 2 * B / mean * 1e3, median(ts) * 1e3, mean / bank_ms))
            if nw == 0:
                host.pop(0)
        if not args.no_model:
            from fdgan.model import FDGANModel
            opt = argparse.Namespace(stage=2, checkpoints=os.path.join(root, "ck"), name="bench", norm="batch", drop=0.0, connect_layers=0,
                                     fuse_mode="cat", pose_feature_size=128, noise_feature_size=256, arch="resnet50", lr=0.001,
                                     niter=50, niter_decay=50, lambda_recon=100.0, lambda_veri=10.0, lambda_sp=10.0, smooth_label=False,
                                     random_init=True, quiet=True, batch_size=B)
            torch.manual_seed(0)
            model = FDGANModel(opt)
            model.reset_model_status()
            say("FDGANModel stage-2 step at %d pairs, %d consecutive steps: ms per step, of which waiting for data" % (B, args.steps))
            for name, f in [("bank", feed), ("host", host[workers])]:
                step, data = fed_steps(f, model, args.steps)
                say("  fed by the %-5s loader   %8.2f ms per step   Data %8.3f ms" % (name, step, data))
    finally:
        shutil.rmtree(root, ignore_errors=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
