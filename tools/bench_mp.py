"""Timings of the multi-part encoder's own kernels at the recipe's shapes — the part pooling (rg_part_pool_fwd / rg_part_pool_bwd) on
the [256, 2048, 16, 8] part map and the fused head (rg_mp_head_fwd / rg_mp_head_bwd) on [256, 2048] — against the composition the
library offered before them, in ONE process, alternated, with device events:
    python tools/bench_mp.py [--crops 256] [--reps 30] [--pool gem|avg]
    python tools/bench_mp.py --step [--crops 256] [--steps 20]      ClusterContrastPartTrainer.step with resnet_mp50, GeM, use_hard
Composed part pooling: two slice copies of the map's halves + gem_pool / global_avgpool on each; backward: the two pooling
backwards + one concatenation.  Composed head: BatchNorm1d x 3 + add x 2 + l2norm_rows x 4 and the mirror image backward.
Every figure is the MEDIAN of the timed launches; GB/s are algorithmic (fused pooling: one pass over the map forward, two backward
for GeM — x and dx — one for the average)."""
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


def alternate(fns, reps):
    """median microseconds per call of each function, the functions taken in turn `reps` times after two warm-up rounds"""
    for _ in range(2):
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
    return [sorted(a.elapsed_time(b) for a, b in e)[reps // 2] * 1e3 for e in ev]


def part_pool(args, dev):
    N, C, H, W = args.crops, 2048, 16, 8
    split, HW = H // 2, H * W
    x = torch.randn(N, C, H, W, device=dev).abs_() + 0.01
    dy = torch.randn(2, N, C, device=dev)
    gem = args.pool == "gem"
    p = torch.full((1,), 3.0, device=dev) if gem else None
    halves = x.view(N * C, 2, HW // 2)                  # the two row ranges of a plane as two "channels" of HW / 2 elements

    def f_fwd():
        return ops.part_pool_fwd(x, split, p)

    def c_fwd():
        a, b = ops.slice_channels(halves, 0, 1), ops.slice_channels(halves, 1, 2)
        if gem:
            return a, b, ops.gem_pool_fwd(a, p), ops.gem_pool_fwd(b, p)
        return a, b, ops.global_avgpool_fwd(a), ops.global_avgpool_fwd(b)

    y = f_fwd()
    a, b, ya, yb = c_fwd()

    def f_bwd():
        return ops.part_pool_bwd(x if gem else tuple(x.shape), split, dy, p, y if gem else None)

    def c_bwd():
        if gem:
            da, b_, = ops.gem_pool_bwd(a, p, ya, dy[0].reshape(ya.shape))
            db, c_, = ops.gem_pool_bwd(b, p, yb, dy[1].reshape(yb.shape))
        else:
            da, db = ops.global_avgpool_bwd(dy[0].reshape(ya.shape), a.shape), ops.global_avgpool_bwd(dy[1].reshape(yb.shape), b.shape)
        return ops.cat_channels([da, db])

    assert torch.allclose(y[0].reshape(-1), ya.reshape(-1), rtol=1e-4) and torch.allclose(y[1].reshape(-1), yb.reshape(-1), rtol=1e-4)
    assert torch.allclose(f_bwd()[0].reshape(-1), c_bwd().reshape(-1), rtol=1e-3, atol=1e-7)
    tf, tc, bf, bc = alternate([f_fwd, c_fwd, f_bwd, c_bwd], args.reps)
    kb = x.numel() * 4 / 1e3
    print("part pooling (%s) on %s, split row %d; median of %d alternated launches, us" % (args.pool, (N, C, H, W), split, args.reps))
    print("  forward   fused %8.1f  (%5.0f GB/s)   composed %8.1f   composed / fused %.2f" % (tf, kb / tf, tc, tc / tf))
    print("  backward  fused %8.1f  (%5.0f GB/s)   composed %8.1f   composed / fused %.2f" % (bf, (2 if gem else 1) * kb / bf, bc, bc / bf))
    return tf <= tc and bf <= bc


def head(args, dev):
    B, D = args.crops, 2048
    xs = [torch.randn(B, D, device=dev) for _ in range(3)]
    dys = [torch.randn(B, D, device=dev) for _ in range(4)]
    bns = [rnn.BatchNorm1d(D).to(dev).train() for _ in range(3)]
    for bn in bns:
        bn.bias.requires_grad_(False)

    def f_fwd():
        return ops.mp_head_fwd(xs, [bn.weight for bn in bns], [bn.bias for bn in bns], [bn.running_mean for bn in bns],
                               [bn.running_var for bn in bns], [bn.eps for bn in bns], [bn.momentum for bn in bns], True, 1)

    def c_fwd():
        t = Tape()
        z = [bn.tf(t, x) for bn, x in zip(bns, xs)]
        z.append(ops.add(ops.add(z[0], z[1]), z[2]))
        return t, [ops.l2norm_rows_fwd(v) for v in z]

    out, xhat, _, invstd, norms = f_fwd()
    tape, fs = c_fwd()
    stack = list(tape.stack)

    def f_bwd():
        return ops.mp_head_bwd(dys, xhat, invstd, norms, [bn.weight for bn in bns], [bn.bias for bn in bns], True, 1)

    def c_bwd():
        tape.stack, tape.grads = list(stack), {}
        dz = [ops.l2norm_rows_bwd(f, dy, n) for (f, n), dy in zip(fs, dys)]
        return [bns[j].tb(tape, ops.add(dz[j], dz[3])) for j in (2, 1, 0)]

    assert all(torch.allclose(out[k], fs[k][0], rtol=1e-4, atol=1e-6) for k in range(4))
    assert torch.allclose(f_bwd()[0][0], c_bwd()[2], rtol=1e-3, atol=1e-6)
    tf, tc, bf, bc = alternate([f_fwd, c_fwd, f_bwd, c_bwd], args.reps)
    print("head on three [%d, %d] inputs, train mode, fusion 'sum'; median of %d alternated calls, us (host enqueue included: these "
          "kernels move 6 to 16 MB)" % (B, D, args.reps))
    print("  forward   fused %8.1f  (2 launches)    composed %8.1f  (9 or more launches)   composed / fused %.2f" % (tf, tc, tc / tf))
    print("  backward  fused %8.1f  (2 launches)    composed %8.1f  (10 or more launches)  composed / fused %.2f" % (bf, bc, bc / bf))


def step(args, dev):
    import clustercontrast.models as M
    from clustercontrast.models.cm import ClusterMemory
    from clustercontrast.trainers import ClusterContrastPartTrainer
    from rg_hip import optim as roptim
    group = int(round(args.crops ** 0.5))
    B, K = group * group, 2048
    torch.manual_seed(0)
    enc = M.create("resnet_mp50", pretrained=False, norm=True, pooling_type="gem").to(dev).train()
    mem = ClusterMemory(enc.num_features, K, temp=0.05, momentum=0.1, use_hard=True).to(dev)
    g = torch.Generator(device=dev).manual_seed(7)
    mem.features = F.normalize(torch.randn(K, enc.num_features, generator=g, device=dev), dim=1)
    opt = roptim.Adam([{"params": [p]} for p in enc.parameters() if p.requires_grad], lr=3.5e-4, weight_decay=5e-4)
    imgs = torch.randn(B, 3, 256, 128, generator=g, device=dev)
    labels = torch.randint(0, K, (group,), generator=g, device=dev).repeat_interleave(group)
    trainer = ClusterContrastPartTrainer(enc, mem, group_size=group, temperature=0.05)
    for _ in range(args.warmup):
        trainer.step(imgs, labels, opt)
    t, = alternate([lambda: trainer.step(imgs, labels, opt)], args.steps)
    print("multi-part training step (ClusterContrastPartTrainer.step, resnet_mp50, GeM, ClusterMemory(use_hard=True), Adam), %d crops of "
          "256x128 in groups of %d, median of %d steps after %d warm-up" % (B, group, args.steps, args.warmup))
    print("resnet_mp50    %8.2f ms/step  %8.1f img/s" % (t / 1e3, B / (t / 1e6)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--crops", type=int, default=256)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--pool", choices=("gem", "avg", "both"), default="both")
    ap.add_argument("--step", action="store_true", help="time the multi-part training step instead of the kernels")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    assert args.reps >= 20, "the comparison is a median of at least 20 timed launches"
    assert torch.cuda.is_available(), "bench_mp.py needs the GPU"
    dev = torch.device("cuda:0")
    if args.step:
        return step(args, dev)
    ok = True
    for pool in (("gem", "avg") if args.pool == "both" else (args.pool,)):
        args.pool = pool
        ok = part_pool(args, dev) and ok
    head(args, dev)
    print("part pooling not slower than the composed path in either direction: %s" % ("yes" if ok else "NO"))


if __name__ == "__main__":
    main()
