"""Timings of the domain-specific BatchNorm layer (rg_dsbn_fwd / rg_dsbn_bwd) at the shapes a 128 + 128 batch of 256 x 128 crops
takes through ResNet-50 with layer4 at stride 1, forward and backward, in ONE process, alternated, with device events:
    python tools/bench_dsbn.py [--crops 256] [--reps 30] [--out profiles/dsbn_layer.txt]
    python tools/bench_dsbn.py --step [--dsbn] [--crops 256] [--steps 20]      ClusterContrastTrainer.step of resnet50 (converted)
against
    (a) the composition the reference performs (CC/clustercontrast/models/dsbn.py:17-23): two slice copies of the halves, two
        BatchNorms (rg_hip.nn.norm.BatchNorm2d / 1d as the modules run them), one concatenation; backward: the two BatchNorm backwards on
        the halves of dy (views, as torch's cat backward hands them over) and one concatenation of the two dx (split's backward);
    (b) the existing rg_bn_* entry points called on the two halves by pointer offset (the halves of an NCHW batch are contiguous),
        routed as rg_hip.nn.norm._BatchNorm routes a half: rg_bn_train_*_fused where rg_bn_train_fused_ok says so, else rg_bn_stats +
        rg_bn_apply_fwd / rg_bn_bwd_reduce + rg_bn_bwd_apply — the strongest alternative without new kernels.
The layer carries the ReLU epilogue (as bn1 / bn2 of a Bottleneck do).  Every figure is the MEDIAN of the timed calls, host enqueue
included; GB/s are algorithmic for the fused layer (forward: x read, y written; backward: x, dy, y read, dx written)."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "reid-gan_amd"))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402
from rg_hip import nn as rnn  # noqa: E402
from rg_hip import ops  # noqa: E402
from rg_hip.lib import lib  # noqa: E402
from rg_hip.tape import Tape  # noqa: E402

SHAPES = [(64, 128, 64), (256, 64, 32), (512, 32, 16), (1024, 16, 8), (2048, 16, 8), (2048,)]
ACT = ops.ACT_RELU


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


def _halves(t):
    """the two batch halves of a contiguous tensor as the two 'channels' of [1][2][rest]"""
    return t.view(1, 2, -1)


def layer(N, shape, reps, dev):
    C = shape[0]
    HW = 1
    for d in shape[1:]:
        HW *= d
    h = N // 2
    full = (N,) + tuple(shape)
    half = (h,) + tuple(shape)
    g = torch.Generator(device=dev).manual_seed(C + HW)
    x = torch.randn(full, generator=g, device=dev)
    x[h:] = 3.0 * x[h:] + 4.0
    dy = torch.randn(full, generator=g, device=dev)
    cls = rnn.BatchNorm2d if len(shape) == 3 else rnn.BatchNorm1d
    dsbn = (rnn.DSBN2d if len(shape) == 3 else rnn.DSBN1d)(C).to(dev).train()
    bns = [cls(C).to(dev).train() for _ in range(2)]
    s, t = dsbn.BN_S, dsbn.BN_T
    st = ops._stream

    # ---- the fused layer -------------------------------------------------------------------------------------------------------
    def f_fwd():
        return ops.dsbn_fwd(x, s.weight, s.bias, t.weight, t.bias, (s.running_mean, s.running_var), (t.running_mean, t.running_var),
                            (s.eps, t.eps), (s.momentum, t.momentum), act=ACT)

    y, stats = f_fwd()

    def f_bwd():
        return ops.dsbn_bwd(x, dy, y, stats, s.weight, t.weight, ACT)

    # ---- (a) slice copies + two BatchNorm modules + concatenation ----------------------------------------------------------------
    def a_fwd():
        tp = Tape(param_grad=False)
        xa, xb = ops.slice_channels(_halves(x), 0, 1).view(half), ops.slice_channels(_halves(x), 1, 2).view(half)
        ya, yb = bns[0].tf(tp, xa, act=ACT), bns[1].tf(tp, xb, act=ACT)
        return tp, ops.cat_channels([ya.view(1, 1, -1), yb.view(1, 1, -1)]).view(full)

    tape, ya_ = a_fwd()
    stack = list(tape.stack)

    def a_bwd():
        tape.stack, tape.grads = list(stack), {}
        db = bns[1].tb(tape, dy[h:])
        da = bns[0].tb(tape, dy[:h])
        return ops.cat_channels([da.view(1, 1, -1), db.view(1, 1, -1)]).view(full)

    # ---- (b) rg_bn_* on the halves by pointer offset -----------------------------------------------------------------------------
    fused = bool(lib.rg_bn_train_fused_ok(h, C, HW))
    nb = h * C * HW * 4
    yb_ = torch.empty_like(x)
    dxb = torch.empty_like(x)
    stb = torch.empty(2, 2, C, device=dev)
    sums = torch.empty(2, 2, C, device=dev)
    wsb = ops.workspace(lib.rg_bn_workspace(h, C, HW), dev)

    def b_fwd():
        for d, bn in enumerate((s, t)):
            xp, yp = x.data_ptr() + d * nb, yb_.data_ptr() + d * nb
            if fused:
                lib.rg_bn_train_fwd_fused(xp, bn.weight.data_ptr(), bn.bias.data_ptr(), None, yp, stb[0, d].data_ptr(),
                                          stb[1, d].data_ptr(), bn.running_mean.data_ptr(), bn.running_var.data_ptr(), h, C, HW,
                                          bn.eps, bn.momentum, ACT, 0.0, st())
            else:
                lib.rg_bn_stats(xp, stb[0, d].data_ptr(), stb[1, d].data_ptr(), bn.running_mean.data_ptr(),
                                bn.running_var.data_ptr(), h, C, HW, bn.eps, bn.momentum, wsb.data_ptr(), wsb.numel(), st())
                lib.rg_bn_apply_fwd(xp, stb[0, d].data_ptr(), stb[1, d].data_ptr(), bn.weight.data_ptr(), bn.bias.data_ptr(), None, yp,
                                    h, C, HW, 0, bn.eps, ACT, 0.0, st())
        return yb_

    def b_bwd():
        for d, bn in enumerate((s, t)):
            xp, gp, yp, dp = (v.data_ptr() + d * nb for v in (x, dy, y, dxb))
            m, i, s1, s2 = stats[0, d].data_ptr(), stats[1, d].data_ptr(), sums[0, d].data_ptr(), sums[1, d].data_ptr()
            if fused:
                lib.rg_bn_train_bwd_fused(xp, gp, yp, m, i, bn.weight.data_ptr(), dp, None, s1, s2, h, C, HW, ACT, 0.0, st())
            else:
                lib.rg_bn_bwd_reduce(xp, gp, yp, m, i, s1, s2, h, C, HW, 0, bn.eps, ACT, 0.0, wsb.data_ptr(), wsb.numel(), st())
                lib.rg_bn_bwd_apply(xp, gp, yp, m, i, bn.weight.data_ptr(), s1, s2, dp, None, h, C, HW, 1, 0, bn.eps, ACT, 0.0, st())
        return dxb

    assert torch.allclose(y, ya_, rtol=1e-4, atol=1e-5) and torch.allclose(y, b_fwd(), rtol=1e-4, atol=1e-5)
    dxf = f_bwd()[0]
    assert torch.allclose(dxf, b_bwd(), rtol=1e-3, atol=1e-5)
    tf, ta, tb, bf, ba, bb = alternate([f_fwd, a_fwd, b_fwd, f_bwd, a_bwd, b_bwd], reps)
    mb = x.numel() * 4 / 1e3
    regime = "one launch" if lib.rg_dsbn_one_launch(N, C, HW) else "%d slices per domain" % lib.rg_dsbn_slices(N, C, HW)
    rows = ["%-22s %-22s forward   fused %8.1f (%5.0f GB/s)   (a) %8.1f  x%.2f   (b) %8.1f  x%.2f"
            % (list(full), regime, tf, 2 * mb / tf, ta, ta / tf, tb, tb / tf),
            "%-22s %-22s backward  fused %8.1f (%5.0f GB/s)   (a) %8.1f  x%.2f   (b) %8.1f  x%.2f"
            % ("", "", bf, 4 * mb / bf, ba, ba / bf, bb, bb / bf)]
    return rows, (tf <= tb, bf <= bb)


def step(args, dev):
    import clustercontrast.models as M
    from clustercontrast.models.cm import ClusterMemory
    from clustercontrast.trainers import ClusterContrastTrainer
    from rg_hip import optim as roptim
    group = int(round(args.crops ** 0.5))
    B, K = group * group, 2048
    torch.manual_seed(0)
    enc = M.create("resnet50", pretrained=False, pooling_type="gem")
    if args.dsbn:
        from clustercontrast.models.dsbn import convert_dsbn
        convert_dsbn(enc)
    enc.to(dev).train()
    mem = ClusterMemory(enc.num_features, K, temp=0.05, momentum=0.1).to(dev)
    g = torch.Generator(device=dev).manual_seed(7)
    mem.features = F.normalize(torch.randn(K, enc.num_features, generator=g, device=dev), dim=1)
    opt = roptim.Adam([{"params": [p]} for p in enc.parameters() if p.requires_grad], lr=3.5e-4, weight_decay=5e-4)
    imgs = torch.randn(B, 3, 256, 128, generator=g, device=dev)
    labels = torch.randint(0, K, (group,), generator=g, device=dev).repeat_interleave(group)
    trainer = ClusterContrastTrainer(enc, mem)
    for _ in range(args.warmup):
        trainer.step(imgs, labels, opt)
    t, = alternate([lambda: trainer.step(imgs, labels, opt)], args.steps)
    line = ("ClusterContrastTrainer.step, resnet50%s, GeM, Adam, %d crops of 256x128, median of %d steps after %d warm-up: "
            "%8.2f ms/step  %8.1f img/s" % (" after convert_dsbn" if args.dsbn else " (plain BatchNorm)", B, args.steps, args.warmup,
                                            t / 1e3, B / (t / 1e6)))
    print(line)
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--crops", type=int, default=256)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--step", action="store_true", help="time the training step instead of the layer")
    ap.add_argument("--dsbn", action="store_true", help="--step: convert the encoder with convert_dsbn first")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None, help="also append the table to this file")
    args = ap.parse_args()
    assert args.reps >= 20, "the comparison is a median of at least 20 timed launches"
    assert torch.cuda.is_available() and args.crops % 2 == 0, "bench_dsbn.py needs the GPU and an even batch"
    dev = torch.device("cuda:0")
    if args.step:
        lines = [step(args, dev)]
    else:
        lines = ["DSBN layer, train mode, ReLU epilogue, %d + %d samples; median of %d alternated calls, us; (a) slice copies + two "
                 "BatchNorm modules + cat, (b) rg_bn_* on the halves by pointer offset; xR = time / fused time"
                 % (args.crops // 2, args.crops // 2, args.reps)]
        slower = []
        for shape in SHAPES:
            rows, ok = layer(args.crops, shape, args.reps, dev)
            lines += rows
            slower += ["%s %s" % (shape, d) for d, o in zip(("forward", "backward"), ok) if not o]
        lines.append("fused layer not slower than (b): %s" % ("yes, at every shape and direction" if not slower else "NO at " + ", ".join(slower)))
        print("\n".join(lines))
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
