"""Timings of the hard-mix ReID step (ClusterContrastWithGANTrainer.hard_mix_step) and of its fused loss, in ONE process, alternated,
with device events, medians of --reps (default 30) timed calls:
    python tools/bench_hardmix.py [--reps 30] [--crops 256] [--out profiles/hardmix_step.txt]
  loss   forward + backward of the cross entropy over the two logit blocks (rg_softmax_ce_ext_fwd / _bwd behind
         rg_hip.functional.cross_entropy_ext) at n = 256, m = 700, t = 16 against the composition it replaced: the ATen mask
         (eye, scale, repeat_interleave), rg_axpby (add), the channel concatenation, rg_softmax_ce_fwd / _bwd and two slice copies
         in backward; and the whole ClusterMemory_Gradient.forward(ex_f=...) + backward at D = 2048 around each (the two
         normalisations and the GEMMs are the same launches on both sides)
  step   hard_mix_step at the recipe's shape — --crops 256x128 crops in identity groups of 16, the AE generator at 128x64 — against
         ClusterContrastTrainer.step on the same encoder (ResNet-50, GeM) with a ClusterMemory: what the GAN branch and the second
         (eval-mode) encoder pass add to a plain cluster-contrast step
Calls include their host enqueue: the loss is a handful of short launches, so its time is launch count, not bandwidth."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "reid-gan_amd"))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402
from rg_hip import functional as RF  # noqa: E402
from rg_hip import ops  # noqa: E402
from rg_hip.tape import backward as _backward  # noqa: E402


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


class _AddConst(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, c):
        return ops.add(x, c)

    @staticmethod
    def backward(ctx, g):
        return g, None


class _Cat2(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b):
        ctx.ca = a.shape[1]
        return ops.cat_channels([a, b])

    @staticmethod
    def backward(ctx, g):
        return ops.slice_channels(g, 0, ctx.ca), ops.slice_channels(g, ctx.ca, g.shape[1])


def composed_loss(la, lb, labels, group, scale):
    """the composition ClusterMemory_Gradient.forward(ex_f=...) ran before the fused kernels"""
    mask = (-10000.0 * torch.eye(lb.shape[1], device=la.device)).repeat_interleave(group, dim=0)
    return RF.cross_entropy(_Cat2.apply(la, _AddConst.apply(lb, mask)), labels, scale)


def loss(args, dev, say):
    from clustercontrast.models.cm import ClusterMemory_Gradient, _MatmulT
    n, m, t, D = 256, 700, 16, 2048
    group = n // t
    g = torch.Generator(device=dev).manual_seed(3)
    la = (torch.rand(n, m, generator=g, device=dev) * 2 - 1).requires_grad_(True)
    lb = (torch.rand(n, t, generator=g, device=dev) * 2 - 1).requires_grad_(True)
    labels = torch.randint(0, m, (n,), generator=g, device=dev)

    def run(fn):
        def go():
            la.grad = lb.grad = None
            _backward(fn())
        return go

    def fused():
        return RF.cross_entropy_ext(la, lb, labels, group, -10000.0, 20.0)

    def composed():
        return composed_loss(la, lb, labels, group, 20.0)

    run(fused)()
    ga, gb, lf = la.grad.clone(), lb.grad.clone(), fused().item()
    run(composed)()
    assert abs(lf - composed().item()) <= 1e-5 * abs(lf) and torch.allclose(ga, la.grad, rtol=1e-4, atol=1e-8) \
        and torch.allclose(gb, lb.grad, rtol=1e-4, atol=1e-8)
    tf, tc = alternate([run(fused), run(composed)], args.reps)
    say("loss over la [%d, %d] | lb [%d, %d], group %d, forward + backward; median of %d alternated calls, us (host enqueue included)"
        % (n, m, n, t, group, args.reps))
    say("  fused     %8.1f  (4 launches: ce_ext fwd, mean, mean bwd, ce_ext bwd)" % tf)
    say("  composed  %8.1f  (mask on ATen, add, cat, ce fwd, mean, mean bwd, ce bwd, 2 slices)   composed / fused %.2f" % (tc, tc / tf))

    mem = ClusterMemory_Gradient(D, m, temp=0.05)
    mem.set_clusters(torch.randn(m, D, generator=g, device=dev), 0.1)
    x = torch.randn(n, D, generator=g, device=dev).requires_grad_(True)
    ex = torch.randn(t, D, generator=g, device=dev)

    def mem_fused():
        x.grad = None
        _backward(mem(x, labels, ex_f=ex))

    def mem_composed():
        x.grad = None
        xi = RF.normalize_rows(x)
        oa = _MatmulT.apply(xi, mem.normed_clusters.detach())
        ob = _MatmulT.apply(xi, RF.normalize_rows(ex))
        _backward(composed_loss(oa, ob, labels, group, 20.0))

    mf, mc = alternate([mem_fused, mem_composed], args.reps)
    say("ClusterMemory_Gradient.forward(ex_f=...) + backward at D = %d (normalisations and GEMMs included), us" % D)
    say("  fused     %8.1f   composed %8.1f   composed / fused %.2f" % (mf, mc, mc / mf))


def gan_opt():
    return argparse.Namespace(
        model="AE", gan_train=True, checkpoints_dir="/tmp/rg_ckpt", name="b", load_pretrain="", model_gen="AE", num_feats=256,
        layers_g=3, image_nc=3, pose_nc=18, norm="instance", use_spect_g=False, use_spect_d=True, use_coord=False, num_blocks=3,
        nhead=2, num_CABs=2, num_TTBs=2, dis_layers=3, init_type="orthogonal", verbose=False, pool_size=0, gan_lr=2e-4,
        gan_mode="lsgan", no_vgg_loss=True, beta1=0.5, ratio_g2d=0.1, lambda_rec=2.0, lambda_g=5.0, gan_lr_policy="lambda",
        iter_start=0, niter=100, niter_decay=100, continue_train=False, which_epoch="latest", bipath_gan=False, use_adp=False,
        lambda_fus=0.8)


def step(args, dev, say):
    import clustercontrast.models as M
    from clustercontrast.models.cm import ClusterMemory, ClusterMemory_Gradient
    from clustercontrast.trainers import ClusterContrastTrainer, ClusterContrastWithGANTrainer
    from dual_gan.models.models import create_model
    from rg_hip import optim as roptim
    B, group, K = args.crops, 16, 700
    assert B % group == 0
    torch.manual_seed(0)
    g = torch.Generator(device=dev).manual_seed(7)
    imgs = torch.randn(B, 3, 256, 128, generator=g, device=dev)
    labels = torch.randperm(K, generator=g, device=dev)[:B // group].repeat_interleave(group)
    xs = (torch.rand(B, 3, 128, 64, generator=g, device=dev) - 0.5) / 0.5

    def encoder():
        enc = M.create("resnet50", pretrained=False, pooling_type="gem").to(dev).train()
        return enc, roptim.Adam([{"params": [p]} for p in enc.parameters() if p.requires_grad], lr=3.5e-4, weight_decay=5e-4)

    enc_a, opt_a = encoder()
    mem_a = ClusterMemory_Gradient(enc_a.num_features, K, temp=0.05)
    mem_a.set_clusters(torch.randn(K, enc_a.num_features, generator=g, device=dev), 0.1)
    gan = create_model(gan_opt())
    gan.set_input({"Xs": xs})
    hard = ClusterContrastWithGANTrainer(enc_a, GAN=gan, memory=mem_a, opt=argparse.Namespace(num_instances=group, cl_temp=0.05))
    enc_b, opt_b = encoder()
    mem_b = ClusterMemory(enc_b.num_features, K, temp=0.05, momentum=0.1).to(dev)
    mem_b.features = F.normalize(torch.randn(K, enc_b.num_features, generator=g, device=dev), dim=1)
    plain = ClusterContrastTrainer(enc_b, mem_b)
    for _ in range(args.warmup):
        hard.hard_mix_step(imgs, labels, opt_a)
        plain.step(imgs, labels, opt_b)
    th, tp = alternate([lambda: hard.hard_mix_step(imgs, labels, opt_a), lambda: plain.step(imgs, labels, opt_b)], args.reps)
    say("training step, ResNet-50 (GeM), %d crops of 256x128 in identity groups of %d, Adam; median of %d alternated steps after %d "
        "warm-up" % (B, group, args.reps, args.warmup))
    say("  hard_mix_step (AE generator at 128x64 -> %d images -> bicubic 256x128 -> eval-mode encoder, ClusterMemory_Gradient with ex_f)"
        % (B // group))
    say("                                   %8.2f ms/step  %8.1f img/s" % (th / 1e3, B / (th / 1e6)))
    say("  ClusterContrastTrainer.step      %8.2f ms/step  %8.1f img/s   hard-mix / plain %.3f" % (tp / 1e3, B / (tp / 1e6), th / tp))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--crops", type=int, default=256)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", choices=("loss", "step", "both"), default="both")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hardmix_step.txt"))
    args = ap.parse_args()
    assert args.reps >= 20, "the comparison is a median of at least 20 timed calls"
    assert torch.cuda.is_available(), "bench_hardmix.py needs the GPU"
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    say("tools/bench_hardmix.py --reps %d --crops %d on %s" % (args.reps, args.crops, torch.cuda.get_device_name(0)))
    if args.only in ("loss", "both"):
        loss(args, dev, say)
    if args.only in ("step", "both"):
        step(args, dev, say)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
