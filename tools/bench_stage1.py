"""Timings of FD-GAN stage I in ONE process, alternated, with device events:
    python tools/bench_stage1.py [--pairs 256] [--reps 30]           the verification head, forward + backward, at [pairs, 2048], 2 classes
    python tools/bench_stage1.py --step [--pairs 256] [--steps 30]   SiameseTrainer.step at baseline.py's defaults, beside
                                                                     ClusterContrastTrainer.step on 2 x pairs crops
Head: `SiameseNet.forward_loss` + backward (the fused program on csrc/verif_head.hip: 2 launches forward, 1 backward) against the
composed path it replaces — the module call (sub_square, BatchNorm1d, Linear), nn.CrossEntropyLoss(), `accuracy` and their
backward (12 or more launches) — both over an identity base model, so that only the head is timed.  Host enqueue is included:
the problem is latency-bound.  Every figure is the MEDIAN of the timed calls."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "reid-gan_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402
from torch import nn  # noqa: E402
from bench_mp import alternate  # noqa: E402
from rg_hip.tape import RGModule  # noqa: E402
from rg_hip.tape import backward as _backward  # noqa: E402


class _Identity(RGModule):
    """a base model that hands its input on: the head alone is timed"""

    def tf(self, tape, x):
        return x

    def tb(self, tape, dy, need_dx=True):
        return dy


def head(args, dev):
    from reid.evaluation_metrics import accuracy
    from reid.models.embedding import EltwiseSubEmbed
    from reid.models.multi_branch import SiameseNet
    B, D, C = args.pairs, 2048, 2
    torch.manual_seed(0)
    embed = EltwiseSubEmbed(use_batch_norm=True, use_classifier=True, num_features=D, num_classes=C)
    embed.classifier.weight.data.normal_(0, 0.05)
    net = SiameseNet(_Identity(), embed).to(dev).train()
    x1, x2 = torch.randn(B, D, device=dev), torch.randn(B, D, device=dev)
    y = torch.randint(0, C, (B,), device=dev)
    crit = nn.CrossEntropyLoss()

    def zero():
        for p in net.parameters():
            p.grad = None

    def fused():
        zero()
        _, _, _, loss, prec = net.forward_loss(x1, x2, y)
        _backward(loss)
        return loss, prec

    def composed():
        zero()
        _, _, out = net(x1, x2)
        loss = crit(out, y)
        prec, = accuracy(out.data, y.data)
        _backward(loss)
        return loss, prec[0]

    lf, pf = fused()
    gf = [p.grad.clone() for p in net.parameters()]
    lc, pc = composed()
    assert torch.allclose(lf.detach(), lc.detach(), rtol=1e-5) and pf.item() == pc.item()
    assert all(torch.allclose(a, p.grad, rtol=1e-3, atol=1e-7) for a, p in zip(gf, net.parameters()))
    tf, tc = alternate([fused, composed], args.reps)
    print("verification head on two [%d, %d] inputs, %d classes, train mode: forward + loss + precision + backward; median of %d "
          "alternated calls, us (host enqueue included)" % (B, D, C, args.reps))
    print("  fused     %8.1f  (3 launches: column phase, row phase, column phase)" % tf)
    print("  composed  %8.1f  (12 or more launches)   composed / fused %.2f" % (tc, tc / tf))
    print("fused head not slower than the composed path: %s" % ("yes" if tf <= tc else "NO"))


def step(args, dev):
    import clustercontrast.models as M
    import reid.models as RM
    from clustercontrast.models.cm import ClusterMemory
    from clustercontrast.trainers import ClusterContrastTrainer
    from reid.models.embedding import EltwiseSubEmbed
    from reid.models.multi_branch import SiameseNet
    from reid.trainers import SiameseTrainer
    B = args.pairs
    torch.manual_seed(0)
    g = torch.Generator(device=dev).manual_seed(7)
    imgs1, imgs2 = torch.randn(B, 3, 256, 128, generator=g, device=dev), torch.randn(B, 3, 256, 128, generator=g, device=dev)
    targets = torch.randint(0, 2, (B,), generator=g, device=dev)
    res = {}
    for tag, fused in (("fused head", True), ("composed head", False)):
        net = SiameseNet(RM.create('resnet50', pretrained=False, cut_at_pooling=True),
                         EltwiseSubEmbed(use_batch_norm=True, use_classifier=True, num_features=2048, num_classes=2)).to(dev).train()
        opt = torch.optim.SGD([{'params': net.base_model.parameters(), 'lr_mult': 1.0}, {'params': net.embed_model.parameters(), 'lr_mult': 1.0}],
                              0.01, momentum=0.9, weight_decay=5e-4)
        trainer = SiameseTrainer(net, nn.CrossEntropyLoss(), fused_head=fused)
        for _ in range(args.warmup):
            trainer.step(imgs1, imgs2, targets, opt)
        res[tag], = alternate([lambda: trainer.step(imgs1, imgs2, targets, opt)], args.steps)
        del net, opt, trainer
    K = 2048
    enc = M.create("resnet50", pretrained=False).to(dev).train()
    mem = ClusterMemory(enc.num_features, K, temp=0.05, momentum=0.1, use_hard=True).to(dev)
    mem.features = torch.nn.functional.normalize(torch.randn(K, enc.num_features, generator=g, device=dev), dim=1)
    opt = torch.optim.SGD(enc.parameters(), 0.01, momentum=0.9, weight_decay=5e-4)
    crops, labels = torch.cat([imgs1, imgs2], 0), torch.randint(0, K, (2 * B,), generator=g, device=dev)
    cc = ClusterContrastTrainer(enc, mem)
    for _ in range(args.warmup):
        cc.step(crops, labels, opt)
    tcc, = alternate([lambda: cc.step(crops, labels, opt)], args.steps)
    print("stage-I step (SiameseTrainer.step, ResNet-50 cut at pooling, EltwiseSubEmbed(2048 -> 2), torch SGD), %d pairs of 256x128, "
          "median of %d steps after %d warm-up" % (B, args.steps, args.warmup))
    for tag, t in res.items():
        print("  %-14s %8.2f ms/step  %8.1f pairs/s" % (tag, t / 1e3, B / (t / 1e6)))
    print("  yardstick: ClusterContrastTrainer.step on %d crops (one trunk pass of twice the batch) %8.2f ms/step  %8.1f img/s"
          % (2 * B, tcc / 1e3, 2 * B / (tcc / 1e6)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=256)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--step", action="store_true", help="time the training step instead of the head")
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    assert args.reps >= 20, "the comparison is a median of at least 20 timed calls"
    assert torch.cuda.is_available(), "bench_stage1.py needs the GPU"
    dev = torch.device("cuda:0")
    return step(args, dev) if args.step else head(args, dev)


if __name__ == "__main__":
    main()
