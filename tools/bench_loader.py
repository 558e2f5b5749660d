"""The input side of a cluster-contrast epoch, measured in ONE process on a synthetic Market-1501-shaped set (12 936 train entries,
751 identities, 6 cameras, 128x64 JPEGs written with PIL into a temporary directory from a seed, with a pose file):
    python tools/bench_loader.py [--images 12936] [--batch 256] [--reps 30] [--steps 12] [--extract 5120] [--workers N]

  bank build            DeviceImageBank.from_files: host staging (one decode + two PIL resizes per image, thread pool) and upload
  bank next()           DeviceTrainLoader.next() at --batch, plain and with_gan (poses included): wall clock around a synchronised
                        call (host draws + launches), and the three kernels alone with device events on one staged set of draws
  bank test pass        a full DeviceTestLoader pass over the set
  host next()           the pipeline the parent commit offers, written here from PIL + torch because torchvision is not installed:
                        a torch.utils.data.DataLoader with up to 16 workers over a dataset that does decode -> bicubic resize ->
                        pad / crop -> ToTensor / Normalize -> erasing -> flip (plus `get_gan_input` with the numpy pose map when
                        with_gan), then the copy of the batch to the device.  Steady state: the wall clock per batch over --reps
                        consecutive batches of a running loader (its workers prefetch), after a warm-up; the MEAN is its
                        throughput (batches arrive in bursts, so the median wait says little)
  step / extract        ClusterContrastTrainer.step (ResNet-50, GeM, 2048 centroids) and extract_features_device at --batch crops
                        fed by each loader: wall clock per step, and the part of it the loop waits for data (the epoch line's
                        "Data" column)
Every figure is a MEDIAN unless it says otherwise.  Without PIL the host baseline is not measured and the bank is built from
seeded arrays."""
import argparse
import json
import os
import random
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "reid-gan_amd"))
import torch  # noqa: E402

try:
    from PIL import Image
except Exception:                       # noqa: BLE001
    Image = None

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def median(v):
    return sorted(v)[len(v) // 2]


def synth_entries(n, ids=751, cams=6, seed=0):
    g = np.random.RandomState(seed)
    pid = np.sort(g.randint(0, ids, size=n))
    pid[:ids] = np.arange(ids)                                   # every identity at least once
    cam = g.randint(0, cams, size=n)
    return [("%04d_c%ds1_%06d_00.jpg" % (pid[i], cam[i] + 1, i), int(pid[i]), int(cam[i])) for i in range(n)]


def write_set(root, entries, seed=0):
    """128x64 JPEGs with some structure (flat noise compresses and decodes unlike a photograph) and the pose file"""
    g = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:128, 0:64]
    with open(os.path.join(root, "pose.csv"), "w") as f:
        f.write("name:keypoints_y:keypoints_x\n")
        for name, pid, cam in entries:
            base = np.stack([(yy * 2 + 13 * pid) % 256, (xx * 4 + 40 * cam) % 256, (yy + xx + pid) % 256], axis=2)
            img = np.clip(base + g.randint(-25, 25, size=(128, 64, 3)), 0, 255).astype(np.uint8)
            Image.fromarray(img).save(os.path.join(root, name), quality=90)
            ys, xs = g.randint(0, 128, size=18), g.randint(0, 64, size=18)
            ys[g.randint(0, 18)] = xs[g.randint(0, 18)] = -1
            f.write("%s: %s: %s\n" % (name, json.dumps([int(v) for v in ys]), json.dumps([int(v) for v in xs])))
    return os.path.join(root, "pose.csv")


class HostPipeline(torch.utils.data.Dataset):
    """The reference's Preprocessor with its train transform, step by step in PIL + torch (see the module docstring)."""

    def __init__(self, entries, root, poses, with_gan, height=256, width=128, pad=10, gan_size=(128, 64)):
        self.entries, self.root, self.poses, self.with_gan = entries, root, poses, with_gan
        self.h, self.w, self.pad, self.gan_size = height, width, pad, gan_size
        from clustercontrast.utils.data.device_transforms import RandomErasing
        self.erasing = RandomErasing(0.5, mean=list(MEAN))
        self.mean, self.std = torch.tensor(MEAN).view(3, 1, 1), torch.tensor(STD).view(3, 1, 1)

    def __len__(self):
        return len(self.entries)

    @staticmethod
    def to_tensor(img):
        return torch.from_numpy(np.asarray(img).copy()).permute(2, 0, 1).contiguous().float().div(255)

    def __getitem__(self, index):
        from PIL import ImageOps
        fname, pid, cam = self.entries[index]
        flip = bool(torch.rand(1) < 0.5)
        img = Image.open(os.path.join(self.root, fname)).convert("RGB")
        x = img.resize((self.w, self.h), Image.BICUBIC)
        x = ImageOps.expand(x, border=self.pad, fill=0)
        top, left = int(torch.randint(0, 2 * self.pad + 1, (1,))), int(torch.randint(0, 2 * self.pad + 1, (1,)))
        x = x.crop((left, top, left + self.w, top + self.h))
        t = self.to_tensor(x).sub_(self.mean).div_(self.std)
        r0, c0, eh, ew = self.erasing.draw(3, self.h, self.w)
        if eh:
            for c in range(3):
                t[c, r0:r0 + eh, c0:c0 + ew] = MEAN[c]
        if flip:
            t = torch.flip(t, [2])
        item = [t, fname, pid, cam, index]
        if not self.with_gan:
            return item
        hg, wg = self.gan_size
        old = (img.size[1], img.size[0])
        xs = self.to_tensor(img.resize((wg, hg), Image.BILINEAR)).sub_(0.5).div_(0.5)
        cords = self.poses[fname].astype(float)
        ps = np.zeros((hg, wg, cords.shape[0]), dtype="float32")
        gx, gy = np.meshgrid(np.arange(wg), np.arange(hg))
        for i, p in enumerate(cords):
            if p[0] == -1 or p[1] == -1:
                continue
            p0, p1 = int(p[0] / old[0] * hg), int(p[1] / old[1] * wg)
            ps[..., i] = np.exp(-((gy - p0) ** 2 + (gx - p1) ** 2) / (2 * 6 ** 2))
        ps = torch.Tensor(np.transpose(ps, (2, 0, 1)))
        if flip:
            xs, ps = torch.flip(xs, [2]), torch.flip(ps, [2])
        return item, {"Xs": xs, "Ps": ps, "Xs_path": fname, "gt_label": int(fname.split("_", 1)[0])}


class TestPipeline(HostPipeline):
    """`get_test_loader`'s transform: decode -> bicubic resize -> ToTensor -> Normalize"""

    def __getitem__(self, index):
        fname, pid, cam = self.entries[index]
        img = Image.open(os.path.join(self.root, fname)).convert("RGB").resize((self.w, self.h), Image.BICUBIC)
        return self.to_tensor(img).sub_(self.mean).div_(self.std), fname, pid, cam, index


def host_loader(dataset, batch, workers, **kw):
    """worker processes are SPAWNED: a forked child of a process that has initialised the GPU would hold the device open too"""
    return torch.utils.data.DataLoader(dataset, batch_size=batch, num_workers=workers, pin_memory=True,
                                       multiprocessing_context="spawn" if workers > 0 else None, **kw)


class HostIter(object):
    """IterLoader over the host DataLoader, with the copy of the image tensors to the device"""

    def __init__(self, loader, dev):
        self.loader, self.dev, self.it = loader, dev, None

    def __len__(self):
        return len(self.loader)

    def next(self):
        if self.it is None:
            self.it = iter(self.loader)
        try:
            b = next(self.it)
        except StopIteration:
            self.it = iter(self.loader)
            b = next(self.it)
        if isinstance(b, (list, tuple)) and isinstance(b[1], dict):
            b[0][0] = b[0][0].to(self.dev, non_blocking=True)
            b[1]["Xs"], b[1]["Ps"] = b[1]["Xs"].to(self.dev, non_blocking=True), b[1]["Ps"].to(self.dev, non_blocking=True)
        else:
            b[0] = b[0].to(self.dev, non_blocking=True)
        return b


def wall_per_call(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return median(ts) * 1e3


def events_per_call(fn, reps):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    torch.cuda.synchronize()
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return median([a.elapsed_time(b) for a, b in ev])


def fed_steps(loader, trainer, opt, steps, warm=3):
    """(ms per step, ms of it waiting in loader.next()) over `steps` consecutive steps"""
    for _ in range(warm):
        imgs, labels, _ = trainer._parse_data(loader.next())
        trainer.step(imgs, labels % 2048, opt)
    torch.cuda.synchronize()
    data = 0.0
    t0 = time.perf_counter()
    for _ in range(steps):
        t1 = time.perf_counter()
        batch = loader.next()
        data += time.perf_counter() - t1
        imgs, labels, _ = trainer._parse_data(batch)
        trainer.step(imgs, labels % 2048, opt)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3, data / steps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=12936)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--extract", type=int, default=5120, help="images of the feature-extraction pass")
    ap.add_argument("--workers", type=int, default=None)
    ap.add_argument("--no-model", action="store_true", help="skip the trainer step and the extraction pass")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_loader.py needs the GPU"
    from clustercontrast.utils.data import device_bank as B
    dev = torch.device("cuda:0")
    workers = B.default_workers() if args.workers is None else args.workers
    entries = synth_entries(args.images)
    N = args.batch
    print("synthetic Market-1501-shaped set: %d entries, %d identities, 6 cameras, 128x64 JPEGs; batch %d, %d host workers of %d CPUs"
          % (len(entries), len({p for _, p, _ in entries}), N, workers, len(os.sched_getaffinity(0))))
    root = None
    try:
        if Image is not None:
            root = tempfile.mkdtemp(prefix="rg_bank_")
            t0 = time.perf_counter()
            pose = write_set(root, entries)
            print("wrote the set in %.1f s" % (time.perf_counter() - t0))
            t0 = time.perf_counter()
            staged = B.stage_files(entries, root, (256, 128), (128, 64), pose, workers)
            t1 = time.perf_counter()
            bank = B.DeviceImageBank.from_arrays(device=dev, **staged)
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            print("bank build (once)          staging %.2f s (%.0f images/s, %d threads), upload %.3f s; %.1f MB on the device"
                  % (t1 - t0, len(entries) / (t1 - t0), workers, t2 - t1, bank.nbytes / 1e6))
            poses = B.read_pose_csv(pose)
        else:
            print("host baseline not measured: PIL is not installed; the bank is built from seeded arrays")
            g = np.random.RandomState(0)
            bank = B.DeviceImageBank.from_arrays(
                g.randint(0, 256, size=(len(entries), 256, 128, 3), dtype=np.uint8), [e[0] for e in entries], [e[1] for e in entries],
                [e[2] for e in entries], gan_u8=g.randint(0, 256, size=(len(entries), 128, 64, 3), dtype=np.uint8),
                cords=g.randint(0, 64, size=(len(entries), 18, 2)), old_sizes=np.tile(np.array([[128, 64]]), (len(entries), 1)),
                device=dev)
        from clustercontrast.utils.data.device_sampler import RandomMultipleGallerySampler
        random.seed(1), np.random.seed(2), torch.manual_seed(3)
        sampler = RandomMultipleGallerySampler(entries, 16)
        loaders = {"plain": B.DeviceTrainLoader(bank, entries, N, sampler=sampler),
                   "with_gan": B.DeviceTrainLoader(bank, entries, N, sampler=sampler, with_gan=True)}
        print("per batch of %d" % N)
        bank_ms = {}
        for k, ld in loaders.items():
            bank_ms[k] = wall_per_call(ld.next, args.reps)
            print("bank next() %-14s %9.3f ms wall (host draws, one copy, the launches; synchronised)" % (k, bank_ms[k]))
        # the kernels alone: one staged set of draws, launched back to back
        from rg_hip import ops
        ld = loaders["with_gan"]
        d = ops.bank_draws([ld._rows[i] for i in range(N)], torch.as_tensor(np.asarray(ld._draw(N), dtype=np.int64)), device=dev)
        for name, fn, nbytes in [
                ("rg_bank_reid_batch", lambda: ops.bank_reid_batch(bank.reid, d, ld._lut, ld._fill, (256, 128), 10), N * 3 * 256 * 128 * 5),
                ("rg_bank_gan_batch", lambda: ops.bank_gan_batch(bank.gan, d, ld._lut_gan), N * 3 * 128 * 64 * 5),
                ("rg_bank_pose_batch", lambda: ops.bank_pose_batch(bank.centres, d, 128, 64, 6.0), N * 18 * 128 * 64 * 4)]:
            for _ in range(3):
                fn()
            us = events_per_call(fn, args.reps) * 1e3
            print("  %-22s %9.1f us device events   %.2f TB/s (%.1f MB written + read)" % (name, us, nbytes / us / 1e6, nbytes / 1e6))
        test = B.DeviceTestLoader(bank, entries, N)
        ts = []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for b in test:
                pass
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        print("bank test pass             %.1f ms for %d images in %d batches (%.3f ms per batch; median of 3 passes)"
              % (median(ts) * 1e3, len(entries), len(test), median(ts) * 1e3 / len(test)))
        host = {}
        if root is not None:
            for k in ("with_gan", "plain"):
                host.pop("with_gan", None)                              # its workers end before the next loader's start
                dl = host_loader(HostPipeline(entries, root, poses, k == "with_gan"), N, workers, sampler=sampler, drop_last=True,
                                 persistent_workers=workers > 0)
                host[k] = HostIter(dl, dev)
                for _ in range(3):
                    host[k].next()
                torch.cuda.synchronize()
                ts = []
                for _ in range(args.reps):
                    t0 = time.perf_counter()
                    host[k].next()
                    torch.cuda.synchronize()
                    ts.append(time.perf_counter() - t0)
                mean = sum(ts) / len(ts) * 1e3
                print("host next() %-14s %9.3f ms per batch over %d consecutive batches = %.0f images/s (median wait %.3f ms: the workers "
                      "deliver in bursts; %d workers, copy to the device included)   host / bank %.1f"
                      % (k, mean, len(ts), N / mean * 1e3, median(ts) * 1e3, workers, mean / bank_ms[k]))
        if not args.no_model:
            from rg_hip import optim as roptim
            import clustercontrast.models as M
            from clustercontrast.evaluators import extract_features_device
            from clustercontrast.models.cm import ClusterMemory
            from clustercontrast.trainers import ClusterContrastTrainer
            torch.manual_seed(0)
            enc = M.create("resnet50", pretrained=False, pooling_type="gem").to(dev).train()
            mem = ClusterMemory(enc.num_features, 2048, temp=0.05, momentum=0.1).to(dev)
            mem.features = torch.nn.functional.normalize(torch.randn(2048, enc.num_features, device=dev), dim=1)
            opt = roptim.Adam([{"params": [p]} for p in enc.parameters() if p.requires_grad], lr=3.5e-4, weight_decay=5e-4)
            trainer = ClusterContrastTrainer(enc, mem)
            print("ClusterContrastTrainer.step at %d crops, %d consecutive steps: ms per step, of which waiting for data" % (N, args.steps))
            for name, ld in [("bank", loaders["plain"])] + ([("host", host["plain"])] if host else []):
                enc.train()
                step, data = fed_steps(ld, trainer, opt, args.steps)
                print("  fed by the %-5s loader   %8.2f ms per step   Data %8.3f ms" % (name, step, data))
            sub = entries[:args.extract]
            feeds = [("bank", B.DeviceTestLoader(bank, sub, N))]
            if root is not None:
                feeds.append(("host", host_loader(TestPipeline(sub, root, None, False), N, workers, shuffle=False,
                                                  persistent_workers=workers > 0)))
            print("extract_features_device over %d images in batches of %d (third of three passes; the host loader's workers persist)"
                  % (len(sub), N))
            for name, ld in feeds:
                for _ in range(3):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    extract_features_device(enc, ld, print_freq=10 ** 9)
                    torch.cuda.synchronize()
                    dt = time.perf_counter() - t0
                print("  fed by the %-5s loader   %8.1f ms   %8.0f images/s" % (name, dt * 1e3, len(sub) / dt))
    finally:
        if root is not None:
            shutil.rmtree(root, ignore_errors=True)


if __name__ == "__main__":
    main()
