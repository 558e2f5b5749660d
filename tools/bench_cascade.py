"""Timings of the cascade evaluation's second stage in ONE process, alternated, with device events, at Market-1501 size (Q 3 368,
G 15 913, D 2048, 2 classes) on synthetic features, for each k of --topk (default 75 and 100):
    python tools/bench_cascade.py [--reps 30] [--queries 3368] [--gallery 15913] [--topk 75 100]
  pair_score            ops.pair_score on the device top-k of the first-stage matrix, with the rate of its gathered reads
                        (Q k D 4 bytes / time; the probe rows and the coefficients are not counted)
  cascade_merge         ops.cascade_merge, in place on a copy of the first-stage matrix (the copy is timed apart and subtracted)
  second_stage_device   DeviceCascadeEvaluator.second_stage_device end to end: top-k, pair_score, cascade_merge (the top-k, the
                        existing rg_topk_rows on the negated matrix, is also timed alone)
  second_stage          the existing CascadeEvaluator.second_stage on the same inputs as `evaluate` hands them over (features as host
                        rows, the matrix on the host): the yardstick.  Host work is part of it, so it is timed with the wall clock
                        around a synchronised call as well as with events.
Every time is the MEDIAN of the timed calls.  Peak torch.cuda.max_memory_allocated above the resident inputs is measured in one
further call of each path."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "reid-gan_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402
from bench_mp import alternate  # noqa: E402


def peak(fn, dev):
    torch.cuda.synchronize(dev)
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    out = fn()
    torch.cuda.synchronize(dev)
    grown = torch.cuda.max_memory_allocated(dev) - base
    del out
    return grown


def wall(fn, reps, dev):
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize(dev)
        ts.append(time.perf_counter() - t0)
    return sorted(ts)[reps // 2] * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--queries", type=int, default=3368)
    ap.add_argument("--gallery", type=int, default=15913)
    ap.add_argument("--features", type=int, default=2048)
    ap.add_argument("--topk", type=int, nargs="+", default=[75, 100])
    ap.add_argument("--no-existing", action="store_true", help="time the device-resident path alone")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_cascade.py needs the GPU"
    from reid.evaluators import CascadeEvaluator, DeviceCascadeEvaluator, softmax_class0
    from reid.models.embedding import EltwiseSubEmbed
    from rg_hip import ops, search
    dev = torch.device("cuda:0")
    Q, G, D, C = args.queries, args.gallery, args.features, 2
    g = torch.Generator().manual_seed(0)
    host = torch.nn.functional.normalize(torch.randn(Q + G, D, generator=g), dim=1) * 4.0
    probe, gal = host[:Q].to(dev).contiguous(), host[Q:].to(dev).contiguous()
    embed = EltwiseSubEmbed(use_batch_norm=True, use_classifier=True, num_features=D, num_classes=C)
    with torch.no_grad():
        embed.classifier.weight.normal_(0, 0.05 * (64.0 / D) ** 0.5, generator=g)
        embed.bn.running_mean.copy_(torch.rand(D, generator=g) * 0.02)
        embed.bn.running_var.copy_(torch.rand(D, generator=g) * 1e-4 + 1e-4)
    embed = embed.to(dev).eval()
    bn, fc = embed.bn, embed.classifier
    first = search.dist_block(probe, gal, 1.0, True)
    first_host = first.cpu()
    query = [("q%d" % i, i, 0) for i in range(Q)]
    gallery = [("g%d" % j, j, 1) for j in range(G)]
    features = {"q%d" % i: host[i] for i in range(Q)}
    features.update({"g%d" % j: host[Q + j] for j in range(G)})
    new = DeviceCascadeEvaluator(None, embed, softmax_class0)
    old = CascadeEvaluator(None, embed, softmax_class0)
    print("cascade second stage at Q %d, G %d, D %d, %d classes, synthetic features; median of %d calls" % (Q, G, D, C, args.reps))
    print("regime of pair_score: %d (1 16-byte loads, 2 k split)" % ops.pair_score_regime(Q, args.topk[0], D, C))
    for k in args.topk:
        top = search.blocked_topk(Q, k, lambda r0, r1: ops.scale(first[r0:r1], -1.0))
        score = [None]

        def f_pair():
            score[0] = ops.pair_score(probe, gal, top, bn.weight.detach(), bn.bias.detach(), bn.running_mean, bn.running_var,
                                      fc.weight.detach(), fc.bias.detach(), bn.eps)[1]
            return score[0]

        f_pair()
        scratch = first.clone()

        def f_copy():
            scratch.copy_(first)

        def f_merge():
            scratch.copy_(first)
            return ops.cascade_merge(scratch, top, score[0])

        def f_topk():
            return search.blocked_topk(Q, k, lambda r0, r1: ops.scale(first[r0:r1], -1.0))

        def f_new():
            scratch.copy_(first)
            return new.second_stage_device(scratch, probe, gal, rerank_topk=k)

        def f_old():
            return old.second_stage(first_host, features, query, gallery, rerank_topk=k)

        # the two paths agree before anything is timed; the existing path may refuse the size (its [Q k, D] operand is one tensor)
        a, refusal = f_new().cpu().numpy(), None
        try:
            if args.no_existing:
                raise RuntimeError("not asked for (--no-existing)")
            b = f_old()
            err = float(abs(a - b).max() / abs(b).max())
            assert err <= 1e-4, err
            del b
        except RuntimeError as e:
            refusal = str(e)
            torch.cuda.empty_cache()
        t_pair, t_copy, t_merge, t_topk, t_new = alternate([f_pair, f_copy, f_merge, f_topk, f_new], args.reps)
        t_new_wall = wall(f_new, args.reps, dev)
        gathered = 4.0 * Q * k * D
        if refusal is not None:
            print("k = %d   (the existing path does not run at this size: %s)" % (k, refusal))
            print("  pair_score            %10.1f us   gathered reads %.2f GB at %.2f TB/s  (guide, 151 MB table, rows to LDS: 7.4-7.9 TB/s)"
                  % (t_pair, gathered / 1e9, gathered / t_pair / 1e6))
            print("  cascade_merge         %10.1f us   (copy of the matrix %.1f us subtracted from %.1f)" % (t_merge - t_copy, t_copy, t_merge))
            print("  second_stage_device   %10.1f us   events, %.1f us wall  (copy of the matrix %.1f us and the device top-k %.1f us included)"
                  % (t_new, t_new_wall, t_copy, t_topk))
            print("  peak extra device memory   second_stage_device %.1f MB   (one [Q k, D] operand: %.1f MB)"
                  % (peak(lambda: new.second_stage_device(scratch, probe, gal, rerank_topk=k), dev) / 1e6, gathered / 1e6))
            continue
        t_old_ev, = alternate([f_old], args.reps)
        t_old_wall = wall(f_old, max(5, args.reps // 3), dev)
        print("k = %d   (the two paths' merged matrices agree to %.1e of the largest entry)" % (k, err))
        print("  pair_score            %10.1f us   gathered reads %.2f GB at %.2f TB/s  (guide, 151 MB table, rows to LDS: 7.4-7.9 TB/s)"
              % (t_pair, gathered / 1e9, gathered / t_pair / 1e6))
        print("  cascade_merge         %10.1f us   (copy of the matrix %.1f us subtracted from %.1f)" % (t_merge - t_copy, t_copy, t_merge))
        print("  second_stage_device   %10.1f us   events, %.1f us wall  (copy of the matrix %.1f us and the device top-k %.1f us included)"
              % (t_new, t_new_wall, t_copy, t_topk))
        print("  second_stage          %10.1f us   events, %.1f us wall  (existing path, same inputs)   existing / device-resident %.1f"
              % (t_old_ev, t_old_wall, t_old_wall / t_new_wall))
        p_new = peak(lambda: new.second_stage_device(scratch, probe, gal, rerank_topk=k), dev)
        p_old = peak(f_old, dev)
        print("  peak extra device memory   second_stage_device %.1f MB   second_stage %.1f MB   (one [Q k, D] operand: %.1f MB)"
              % (p_new / 1e6, p_old / 1e6, gathered / 1e6))


if __name__ == "__main__":
    main()
