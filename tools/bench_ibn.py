"""Timings of the fused IBN layer (rg_ibn_fwd / rg_ibn_bwd) at the five IBN geometries of resnet_ibn50a on 256x128 crops against
the composition the library offered before it — slice_channels x 2 + InstanceNorm2d + BatchNorm2d (ReLU fused into each) +
cat_channels, and the mirror image backward — in ONE process, alternated, with device events:
    python tools/bench_ibn.py [--crops 64] [--reps 30] [--eval]
    python tools/bench_ibn.py --step [--crops 64] [--steps 20]      cluster-contrast step: resnet_ibn50a vs resnet50, GeM, use_hard
GB/s are algorithmic: the fused layer needs 2 tensor passes forward (read x, write y) and 4 backward (x, dy, y, dx)."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "reid-gan_amd"))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402
from rg_hip import nn as rnn  # noqa: E402
from rg_hip import ops  # noqa: E402
from rg_hip.tape import Tape  # noqa: E402

GEOMETRIES = ((64, 64, 32), (128, 64, 32), (128, 32, 16), (256, 32, 16), (256, 16, 8))      # (planes, H, W) of bn1 in layer1..3


def alternate(fns, reps):
    """mean microseconds per call of each function, the functions taken in turn `reps` times after one warm-up round"""
    for fn in fns:
        fn()
    torch.cuda.synchronize()
    ev = [[(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)] for _ in fns]
    for r in range(reps):
        for i, fn in enumerate(fns):
            ev[i][r][0].record()
            fn()
            ev[i][r][1].record()
    torch.cuda.synchronize()
    return [sum(a.elapsed_time(b) for a, b in e) / reps * 1e3 for e in ev]


class Composed(object):
    """the layer as the reference writes it, on the library's own kernels"""

    def __init__(self, ibn):
        self.ibn = ibn

    def fwd(self, tape, x):
        h = self.ibn.half
        a = self.ibn.IN.tf(tape, ops.slice_channels(x, 0, h), act=ops.ACT_RELU)
        b = self.ibn.BN.tf(tape, ops.slice_channels(x, h, x.shape[1]), act=ops.ACT_RELU)
        return ops.cat_channels([a, b])

    def bwd(self, tape, dy):
        h = self.ibn.half
        db = self.ibn.BN.tb(tape, ops.slice_channels(dy, h, dy.shape[1]))
        da = self.ibn.IN.tb(tape, ops.slice_channels(dy, 0, h))
        return ops.cat_channels([da, db])


def layers(args, dev):
    print("IBN layer, %d crops, %s mode, %d alternated repetitions; us per call, algorithmic GB/s" %
          (args.crops, "eval" if args.eval else "train", args.reps))
    print("%-20s | %9s %9s %6s | %9s %9s %6s | GB/s fused fwd bwd | composed fwd bwd" %
          ("(N, C, H, W)", "fused fwd", "comp fwd", "ratio", "fused bwd", "comp bwd", "ratio"))
    for C, H, W in GEOMETRIES:
        x = torch.randn(args.crops, C, H, W, device=dev)
        dy = torch.randn_like(x)
        ibn = rnn.IBN(C).to(dev).train(not args.eval)
        comp = Composed(ibn)

        def f_fwd():
            t = Tape()
            return t, ibn.tf(t, x, act=ops.ACT_RELU)

        def c_fwd():
            t = Tape()
            return t, comp.fwd(t, x)

        # one recorded forward per repetition feeds its backward; the forward of the pair is timed separately
        state = {}

        def f_bwd():
            t, y = state["f"]
            t.stack, t.grads = list(state["fs"]), {}
            ibn.tb(t, dy)

        def c_bwd():
            t, y = state["c"]
            t.stack, t.grads = list(state["cs"]), {}
            comp.bwd(t, dy)

        state["f"], state["c"] = f_fwd(), c_fwd()
        state["fs"], state["cs"] = list(state["f"][0].stack), list(state["c"][0].stack)
        tf, tc, bf, bc = alternate([lambda: f_fwd(), lambda: c_fwd(), f_bwd, c_bwd], args.reps)
        kb = x.numel() * 4 / 1e3
        print("%-20s | %9.1f %9.1f %6.2f | %9.1f %9.1f %6.2f | %14.0f %5.0f | %8.0f %5.0f" %
              ((args.crops, C, H, W), tf, tc, tc / tf, bf, bc, bc / bf, 2 * kb / tf, 4 * kb / bf, 2 * kb / tc, 4 * kb / bc))


def step(args, dev):
    import clustercontrast.models as M
    from clustercontrast.models.cm import ClusterMemory
    from clustercontrast.trainers import ClusterContrastTrainer
    from rg_hip import optim as roptim
    B, K = args.crops, 2048
    runs = []
    for name in ("resnet_ibn50a", "resnet50"):
        torch.manual_seed(0)
        enc = M.create(name, pretrained=False, pooling_type="gem").to(dev).train()
        mem = ClusterMemory(enc.num_features, K, temp=0.05, momentum=0.1, use_hard=True).to(dev)
        g = torch.Generator(device=dev).manual_seed(7)
        mem.features = F.normalize(torch.randn(K, enc.num_features, generator=g, device=dev), dim=1)
        opt = roptim.Adam([{"params": [p]} for p in enc.parameters() if p.requires_grad], lr=3.5e-4, weight_decay=5e-4)
        imgs = torch.randn(B, 3, 256, 128, generator=g, device=dev)
        labels = torch.randint(0, K, (max(B // 16, 1),), generator=g, device=dev).repeat_interleave(min(16, B))[:B]
        trainer = ClusterContrastTrainer(enc, mem)
        runs.append(lambda t=trainer, i=imgs, l=labels, o=opt: t.step(i, l, o))
    for _ in range(args.warmup):
        for fn in runs:
            fn()
    t_ibn, t_plain = alternate(runs, args.steps)
    print("cluster-contrast training step (ClusterContrastTrainer.step, GeM, ClusterMemory(use_hard=True), Adam), %d crops of 256x128, "
          "%d alternated steps after %d warm-up; end-to-end step rates" % (B, args.steps, args.warmup))
    print("resnet_ibn50a  %8.2f ms/step  %8.1f img/s" % (t_ibn / 1e3, B / (t_ibn / 1e6)))
    print("resnet50       %8.2f ms/step  %8.1f img/s" % (t_plain / 1e3, B / (t_plain / 1e6)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--crops", type=int, default=64)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--eval", action="store_true", help="frozen BatchNorm statistics (layer timing)")
    ap.add_argument("--step", action="store_true", help="time the cluster-contrast training step instead of the layer")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_ibn.py needs the GPU"
    dev = torch.device("cuda:0")
    (step if args.step else layers)(args, dev)


if __name__ == "__main__":
    main()
