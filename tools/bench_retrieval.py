"""SURVEY §8f ranks 1-2 at the reference's sizes: kNN over 12 936 x 2048 features (k = 15) and the 3 368 x 15 913 x 2048
evaluation distance matrix (Market-1501).  Times exclude the final device->host copies of the results.

`--jaccard N,D,k1,k2 [--noise X]` times compute_jaccard_distance's stages instead (clustered synthetic features, 20 per
identity, noise X relative to the unit centre, default 0.30; larger noise = less separated identities = longer sets):
device events around every stage, one warm-up pass, median of `--reps` passes, the device->host copy of the [N, N]
result separately.  The query expansion reads one integer back (the size of its output), which its time includes.

`--dbscan N,D,k1,k2[,eps] [--noise X]` times the DBSCAN pseudo-labelling that follows on the same kind of input (eps 0.6,
min_samples 4 as the training script): device events around `count` (row counts + their prefix sum, first pass over the
matrix; the read-back of nnz is charged to it), `fill` (second pass), `components`, `labels` (with the read-back of the
cluster count) and `centroids`; a device-to-device copy of the matrix in the same run as the bandwidth yardstick of the two
passes; the wall time of `dbscan_pseudo_labels` end to end (Jaccard + DBSCAN + centroids + the N labels to the host); and
the path it replaces on the same matrix and box: the device->host copy, sklearn.cluster.DBSCAN(n_jobs=-1).fit_predict and
the host-loop generate_cluster_features, on the host clock (skipped with a note when scikit-learn is absent).

`--evaluate [Q,G] [--noise X]` (default 3368,15913: Market-1501's query and gallery sizes; 751 identities, 6 cameras, noise
0.90) times the CMC / mAP scoring of a [Q, G] distance matrix: device events around `rg_rank_eval` on the fp32 matrix and on
its fp64 copy (both kernels and the clearing of the outputs) and around a device-to-device copy of the fp32 matrix as the
bandwidth yardstick, one warm-up pass, median of `--reps`; the wall time of `ops.rank_eval` with its read-back; and, in the
same run, the host path it replaces: the device->host copy plus the numpy model (tests/rank_eval_hostmodel.py: a stable
argsort and one scikit-learn `average_precision_score` call per query, what the reference does twice per evaluation).

`--infomap [N,D,k[,min_sim[,cluster_num]]] [--noise X]` (default 12936,2048,15,0.5,4: Market-1501's training set and the
scripts' --k1 15 --eps 0.5 --k2 4) times the Infomap pseudo-labelling on the kNN table of the same clustered synthetic
features: device events around `links`, `flow`, `search` and `labels` (each with the read-backs its host loop makes), one
warm-up pass, median of `--reps` (default 30); the counts of sweeps, levels and flow iterations; and the wall time of
`infomap_pseudo_labels` end to end (normalise + kNN + Infomap + centroids + the N labels to the host).  There is no host
path to put beside it: the `infomap` package is not part of this environment.

`--kmeans [N,D,K] [--noise X]` (default 12936,2048,500, 30 reps) times one k-means iteration on the same clustered features,
from the state three iterations into a run: device events around `assign`, `tally`, `update` and `split` of csrc/kmeans.hip;
in the same pass and process, the composition the library offered before them — `ops.linear_fwd` (the [N, K] product),
`ops.add_outer_terms`, `ops.topk_rows(k=1)`, then a stable `torch.sort` of the labels with the segment offsets and
`ops.segment_mean` — which writes and re-reads the [N, K] score matrix; one warm-up pass, medians with min / max of the two
per-pass sums; and the wall time of the whole `ops.kmeans` run with its iterations.

`--single-shot [Q,G] [--noise X] [--out FILE]` (default 3368,15913 with the synthetic identities of `--evaluate`, the `cuhk03`
configuration separate_camera_set=True, repeat 10) times the single-gallery-shot CMC: device events around `rg_cmc_shot_order`
and around the `rg_cmc_shot_rank` launches of all chunks (draws already on the device), on the fp32 matrix and on its fp64 copy
(the two gather regimes at this size); the wall time of the copy of `n` and `high` to the host, of the host draws (`randint`
plus the int32 conversion) and of the draw upload; and `cmc_single_shot` end to end; one warm-up pass, medians of `--reps`.
There is no host path to put beside it without a reference tree, so no ratio is printed.  --out appends the JSON line to FILE."""
import os, sys, time, json
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "reid-gan_amd"))
import torch
import torch.nn.functional as F
from rg_hip import ops
from rg_hip.search import dist_block
dev = torch.device("cuda", 0)


def jaccard_mode(spec, reps, noise):
    import numpy as np
    from clustercontrast.utils.faiss_rerank import l2_rank, half_k
    N, D, k1, k2 = (int(v) for v in spec.split(","))
    g = torch.Generator(device=dev).manual_seed(0)
    n_id = (N + 19) // 20
    centres = F.normalize(torch.randn(n_id, D, generator=g, device=dev), dim=1)
    x = centres.repeat_interleave(20, dim=0)[:N] + noise * torch.randn(N, D, generator=g, device=dev) / D ** 0.5
    x = F.normalize(x, dim=1)[torch.randperm(N, generator=g, device=dev)].contiguous()
    kh = min(half_k(k1) + 1, k1)
    names = ["rank", "expand", "weights", "query_expansion", "columns", "jaccard", "d2h"]
    host = torch.empty((N, N), dtype=torch.float32).pin_memory()
    samples = {n: [] for n in names}
    info = {}
    for it in range(reps + 1):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(names) + 1)]
        ev[0].record()
        rank = l2_rank(x, k1); ev[1].record()
        sets, counts = ops.rerank_expand(rank, k1, kh); ev[2].record()
        w = ops.rerank_weights(sets, counts, x=x); ev[3].record()
        csr = ops.rerank_query_expand(sets, w, counts, rank=rank if k2 != 1 else None, k2=k2); ev[4].record()
        csc = ops.rerank_columns(*csr); ev[5].record()
        out = ops.rerank_jaccard(csr, csc, clamp=True); ev[6].record()
        host.copy_(out); ev[7].record()
        torch.cuda.synchronize()
        if it:                                   # pass 0 is the warm-up
            for i, n in enumerate(names):
                samples[n].append(ev[i].elapsed_time(ev[i + 1]))
        info = {"set_mean": round(float(counts.float().mean()), 1), "set_max": int(counts.max()), "nnz": int(csr[1].numel()),
                "support_mean": round(float((out < 1).sum()) / N, 1)}
        del rank, sets, counts, w, csr, csc, out
    med = {n: round(float(np.median(v)), 3) for n, v in samples.items()}
    res = {"jaccard": {"N": N, "D": D, "k1": k1, "k2": k2, "noise": noise, "reps": reps}, "stage_ms_median": med,
           "stage_ms_min_max": {n: [round(min(v), 3), round(max(v), 3)] for n, v in samples.items()},
           "device_total_ms": round(sum(v for n, v in med.items() if n != "d2h"), 3), "d2h_ms": med["d2h"],
           "result_MB": round(N * N * 4 / 1e6, 1)}
    res.update(info)
    print(json.dumps(res))


def _clustered_features(N, D, noise):
    g = torch.Generator(device=dev).manual_seed(0)
    n_id = (N + 19) // 20
    centres = F.normalize(torch.randn(n_id, D, generator=g, device=dev), dim=1)
    x = centres.repeat_interleave(20, dim=0)[:N] + noise * torch.randn(N, D, generator=g, device=dev) / D ** 0.5
    return F.normalize(x, dim=1)[torch.randperm(N, generator=g, device=dev)].contiguous()


def dbscan_mode(spec, reps, noise):
    import numpy as np
    from clustercontrast.utils.faiss_rerank import compute_jaccard_distance
    from clustercontrast.utils.infomap_cluster import generate_cluster_features, generate_cluster_features_device
    from clustercontrast.utils.pseudo_labels import dbscan_pseudo_labels
    parts = spec.split(",")
    N, D, k1, k2 = (int(v) for v in parts[:4])
    eps, min_samples = (float(parts[4]) if len(parts) > 4 else 0.6), 4
    x = _clustered_features(N, D, noise)
    J = compute_jaccard_distance(x, k1=k1, k2=k2, print_flag=False, return_device=True)
    names = ["count", "fill", "components", "labels", "centroids", "d2d_copy"]
    samples = {n: [] for n in names}
    info = {}
    for it in range(reps + 1):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(names) + 1)]
        twin = torch.empty_like(J)
        ev[0].record()
        cnt, rowptr = ops.dbscan_count(J, eps)
        nnz = int(rowptr[N].item()); ev[1].record()
        nbr, core = ops.dbscan_fill(J, eps, min_samples, rowptr, nnz); ev[2].record()
        parent = ops.dbscan_components(rowptr, nbr, core); ev[3].record()
        labels, n_clusters = ops.dbscan_labels(rowptr, nbr, core, parent); ev[4].record()
        cents = generate_cluster_features_device(labels, x) if n_clusters else None; ev[5].record()
        twin.copy_(J); ev[6].record()
        torch.cuda.synchronize()
        if it:                                   # pass 0 is the warm-up
            for i, n in enumerate(names):
                samples[n].append(ev[i].elapsed_time(ev[i + 1]))
        info = {"nnz": nnz, "row_mean": round(nnz / N, 1), "n_clusters": n_clusters, "outliers": int((labels < 0).sum()),
                "core_points": int(core.sum())}
        del cnt, rowptr, nbr, core, parent, cents, twin
    med = {n: round(float(np.median(v)), 3) for n, v in samples.items()}
    new_total = round(sum(v for n, v in med.items() if n != "d2d_copy"), 3)
    mb = N * N * 4 / 1e6
    wall = []
    for it in range(reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got, _, _ = dbscan_pseudo_labels(x, k1=k1, k2=k2, eps=eps, min_samples=min_samples)
        torch.cuda.synchronize()
        if it:
            wall.append((time.perf_counter() - t0) * 1e3)
    res = {"dbscan": {"N": N, "D": D, "k1": k1, "k2": k2, "eps": eps, "min_samples": min_samples, "noise": noise, "reps": reps},
           "stage_ms_median": med, "stage_ms_min_max": {n: [round(min(v), 3), round(max(v), 3)] for n, v in samples.items()},
           "dbscan_device_total_ms": new_total, "matrix_MB": round(mb, 1),
           "count_GBps": round(mb / med["count"], 1), "fill_GBps": round(mb / med["fill"], 1),
           "d2d_copy_read_GBps": round(mb / med["d2d_copy"], 1),
           "pseudo_labels_end_to_end_wall_ms": round(float(np.median(wall)), 3)}
    res.update(info)
    host = torch.empty((N, N), dtype=torch.float32).pin_memory()
    t0 = time.perf_counter()
    host.copy_(J)
    torch.cuda.synchronize()
    t_copy = (time.perf_counter() - t0) * 1e3
    try:
        from sklearn.cluster import DBSCAN as SkDBSCAN
    except ImportError:
        res["host_path"] = {"d2h_ms": round(t_copy, 1), "note": "scikit-learn is not installed here: sklearn DBSCAN not timed"}
    else:
        Jh = host.numpy()
        t0 = time.perf_counter()
        want = SkDBSCAN(eps=eps, min_samples=min_samples, metric="precomputed", n_jobs=-1).fit_predict(Jh)
        t_sk = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        if (want >= 0).any():
            generate_cluster_features(want, x)
        torch.cuda.synchronize()
        t_cf = (time.perf_counter() - t0) * 1e3
        res["host_path"] = {"d2h_ms": round(t_copy, 1), "sklearn_dbscan_ms": round(t_sk, 1), "host_loop_centroids_ms": round(t_cf, 1),
                            "total_ms": round(t_copy + t_sk + t_cf, 1), "labels_equal": bool(np.array_equal(want, got))}
    print(json.dumps(res))


def infomap_mode(spec, reps, noise):
    import numpy as np
    from clustercontrast.utils.infomap_cluster import get_dist_nbr
    from clustercontrast.utils.pseudo_labels import infomap_pseudo_labels
    parts = spec.split(",")
    N, D, k = (int(v) for v in parts[:3])
    min_sim = float(parts[3]) if len(parts) > 3 else 0.5
    cluster_num = int(parts[4]) if len(parts) > 4 else 4
    x = _clustered_features(N, D, noise)
    dists, nbrs = get_dist_nbr(x, k=k, return_device=True)
    names = ["links", "flow", "search", "labels"]
    samples = {n: [] for n in names}
    info = {}
    for it in range(reps + 1):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(names) + 1)]
        ev[0].record()
        g = ops.infomap_links(nbrs, dists, min_sim); ev[1].record()
        g = ops.infomap_flow(g); ev[2].record()
        modules, stats = ops.infomap_search(g); ev[3].record()
        labels, n_clusters = ops.infomap_labels(modules, cluster_num); ev[4].record()
        torch.cuda.synchronize()
        if it:                                   # pass 0 is the warm-up
            for i, n in enumerate(names):
                samples[n].append(ev[i].elapsed_time(ev[i + 1]))
        info = {"links": g["E"], "row_mean": round(g["E"] / N, 1), "singles": int(g["single"].sum()), "flow_iterations": g["flow_iterations"],
                "sweeps": stats["sweeps"], "levels": stats["levels"], "rounds": stats["rounds"], "moves": stats["moves"],
                "rollbacks": stats["rollbacks"], "converged": bool(stats["converged"]), "n_modules": stats["n_modules"],
                "n_clusters": n_clusters, "outliers": int((labels < 0).sum()),
                "codelength_bits": ops.infomap_codelength(g, modules),
                "codelength_one_module_bits": ops.infomap_codelength(g, torch.zeros_like(modules))}
    med = {n: round(float(np.median(v)), 3) for n, v in samples.items()}
    wall = []
    for it in range(min(reps, 5) + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        infomap_pseudo_labels(x, k=k, min_sim=min_sim, cluster_num=cluster_num)
        torch.cuda.synchronize()
        if it:
            wall.append((time.perf_counter() - t0) * 1e3)
    res = {"infomap": {"N": N, "D": D, "k": k, "min_sim": min_sim, "cluster_num": cluster_num, "noise": noise, "reps": reps},
           "stage_ms_median": med, "stage_ms_min_max": {n: [round(min(v), 3), round(max(v), 3)] for n, v in samples.items()},
           "infomap_total_ms": round(sum(med.values()), 3), "pseudo_labels_end_to_end_wall_ms": round(float(np.median(wall)), 3)}
    res.update(info)
    print(json.dumps(res))


def kmeans_mode(spec, reps, noise):
    import numpy as np
    N, D, K = (int(v) for v in spec.split(","))
    x = _clustered_features(N, D, noise)
    # a mid-run state to time one iteration on: the centroids and labels after three iterations
    _, c, _ = ops.kmeans(x, K, niter=3)
    csq, xsq = ops.row_sqsum(c), ops.row_sqsum(x)
    prev = ops.kmeans_assign(x, c, csq)[0]
    nsplit = torch.zeros((1,), dtype=torch.int32, device=dev)
    names = ["assign", "tally", "update", "split"]
    composed = ["gemm", "outer_terms", "top1", "sort", "segment_mean"]
    samples = {n: [] for n in names + composed}
    tally = None
    for it in range(reps + 1):
        c1, q1 = c.clone(), csq.clone()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(names) + 1)]
        ev[0].record()
        label, score = ops.kmeans_assign(x, c1, q1); ev[1].record()
        tally = ops.kmeans_tally(label, prev, xsq, score, K, out=tally); ev[2].record()
        ops.kmeans_update(x, tally["order"], tally["rowptr"], c1, q1); ev[3].record()
        ops.kmeans_split(c1, q1, tally["cnt"], nsplit); ev[4].record()
        # the composition the library offered before: GEMM, score matrix, row top-1, then a stable sort and segment_mean
        cv = [torch.cuda.Event(enable_timing=True) for _ in range(len(composed) + 1)]
        cv[0].record()
        s = ops.linear_fwd(x, c); cv[1].record()
        ops.add_outer_terms(s, None, csq, alpha=2.0, b=-1.0); cv[2].record()          # 2 x.c - |c|^2: its maximum is the nearest centroid
        lab2 = ops.topk_rows(s, 1)[0].flatten(); cv[3].record()
        sl, order = torch.sort(lab2.long(), stable=True)
        _, sizes = torch.unique_consecutive(sl, return_counts=True)
        offsets = torch.zeros(sizes.numel() + 1, dtype=torch.int64, device=dev)
        offsets[1:] = torch.cumsum(sizes, dim=0); cv[4].record()
        means = ops.segment_mean(x, order, offsets); cv[5].record()
        torch.cuda.synchronize()
        if it:                                   # pass 0 is the warm-up
            for i, n in enumerate(names):
                samples[n].append(ev[i].elapsed_time(ev[i + 1]))
            for i, n in enumerate(composed):
                samples[n].append(cv[i].elapsed_time(cv[i + 1]))
        agree = float((lab2 == label).float().mean())
        del s, lab2, sl, order, offsets, means
    med = {n: round(float(np.median(v)), 3) for n, v in samples.items()}
    fused = np.sum([samples[n] for n in names], axis=0)
    comp = np.sum([samples[n] for n in composed], axis=0)
    wall, info = [], {}
    for it in range(min(reps, 5) + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        _, _, info = ops.kmeans(x, K)
        torch.cuda.synchronize()
        if it:
            wall.append((time.perf_counter() - t0) * 1e3)
    res = {"kmeans": {"N": N, "D": D, "K": K, "noise": noise, "reps": reps},
           "stage_ms_median": {n: med[n] for n in names}, "stage_ms_min_max": {n: [round(min(samples[n]), 3), round(max(samples[n]), 3)] for n in names},
           "fused_iteration_ms": {"median": round(float(np.median(fused)), 3), "min": round(float(fused.min()), 3), "max": round(float(fused.max()), 3)},
           "assign_TFLOPS": round(2.0 * N * K * D / med["assign"] / 1e9, 1),
           "composed_stage_ms_median": {n: med[n] for n in composed},
           "composed_iteration_ms": {"median": round(float(np.median(comp)), 3), "min": round(float(comp.min()), 3), "max": round(float(comp.max()), 3)},
           "score_matrix_MB": round(N * K * 4 / 1e6, 1), "labels_agree": round(agree, 6),
           "kmeans_wall_ms": round(float(np.median(wall)), 3), "iterations": info["iterations"], "converged": info["converged"],
           "n_split": info["n_split"], "objective_first_last": [info["obj"][0], info["obj"][-1]]}
    print(json.dumps(res))


def evaluate_mode(spec, reps, noise):
    import numpy as np
    from rg_hip.lib import lib
    from clustercontrast.evaluation_metrics import cmc, mean_ap
    sys.path.insert(0, REPO)
    from tests import rank_eval_hostmodel as M
    Q, G = (int(v) for v in spec.split(","))
    D, n_id, n_cam, topk = 128, 751, 6, 100
    g = torch.Generator(device=dev).manual_seed(0)
    centres = F.normalize(torch.randn(n_id, D, generator=g, device=dev), dim=1)
    ids = torch.randint(0, n_id, (Q + G,), generator=g, device=dev)
    cams = torch.randint(0, n_cam, (Q + G,), generator=g, device=dev).int()
    x = F.normalize(centres[ids] + noise * torch.randn(Q + G, D, generator=g, device=dev) / D ** 0.5, dim=1)
    ids = ids.int()
    qid, gid, qcam, gcam = ids[:Q].contiguous(), ids[Q:].contiguous(), cams[:Q].contiguous(), cams[Q:].contiguous()
    dist = dist_block(x[:Q].contiguous(), x[Q:].contiguous(), 1.0, True)
    out = dict(npos=torch.empty(Q, dtype=torch.int32, device=dev), ap=torch.empty(Q, dtype=torch.float64, device=dev),
               first=torch.empty(Q, dtype=torch.int32, device=dev), hits=torch.empty((Q, topk), dtype=torch.int32, device=dev),
               counts=torch.empty(topk + 2, dtype=torch.int32, device=dev), sums=torch.empty(topk + 1, dtype=torch.float64, device=dev))
    twin = torch.empty_like(dist)
    dist64 = dist.double()
    names = ["rank_eval_fp32", "rank_eval_fp64", "d2d_copy"]
    samples = {n: [] for n in names}
    p = ops._p
    for it in range(reps + 1):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(names) + 1)]
        ev[0].record()
        for k, d in enumerate((dist, dist64)):
            lib.rg_rank_eval(p(d), k, Q, G, G, p(qid), p(gid), p(qcam), p(gcam), 0, topk, 0, p(out["npos"]), p(out["ap"]), p(out["first"]),
                             p(out["hits"]), p(out["counts"]), p(out["sums"]), ops._stream())
            ev[k + 1].record()
        twin.copy_(dist); ev[3].record()
        torch.cuda.synchronize()
        if it:                                   # pass 0 is the warm-up
            for i, n in enumerate(names):
                samples[n].append(ev[i].elapsed_time(ev[i + 1]))
    med = {n: round(float(np.median(v)), 3) for n, v in samples.items()}
    wall = []
    for it in range(reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = ops.rank_eval(dist, qid, gid, qcam, gcam, topk=topk)
        if it:
            wall.append((time.perf_counter() - t0) * 1e3)
    mAP = res["ap_sum"] / res["num_valid"]
    top1 = float(res["first_hist"][0]) / res["num_valid"]
    mb = Q * G * 4 / 1e6
    npos = out["npos"]
    res = {"evaluate": {"Q": Q, "G": G, "D": D, "identities": n_id, "cameras": n_cam, "topk": topk, "noise": noise, "reps": reps},
           "stage_ms_median": med, "stage_ms_min_max": {n: [round(min(v), 3), round(max(v), 3)] for n, v in samples.items()},
           "matrix_MB": round(mb, 1), "rank_eval_fp32_GBps": round(mb / med["rank_eval_fp32"], 1),
           "rank_eval_fp64_GBps": round(2 * mb / med["rank_eval_fp64"], 1), "d2d_copy_read_GBps": round(mb / med["d2d_copy"], 1),
           "rank_eval_with_readback_wall_ms": round(float(np.median(wall)), 3), "readback_numbers": 2 * topk + 3,
           "positives_mean": round(float(npos.float().mean()), 1), "positives_max": int(npos.max()),
           "valid_queries": int((npos > 0).sum()), "mAP": round(mAP, 6), "top1": round(top1, 6)}
    # the path it replaces on the same matrix and box: the copy to the host, then a stable argsort and one scikit-learn call per query
    host = torch.empty((Q, G), dtype=torch.float32).pin_memory()
    t0 = time.perf_counter()
    host.copy_(dist)
    torch.cuda.synchronize()
    t_copy = (time.perf_counter() - t0) * 1e3
    hid = [v.cpu().numpy() for v in (qid, gid, qcam, gcam)]
    t0 = time.perf_counter()
    want = M.summarize(*M.per_query(host.numpy(), *hid, topk=topk))
    t_model = (time.perf_counter() - t0) * 1e3
    res["host_path"] = {"d2h_ms": round(t_copy, 1), "argsort_and_sklearn_loop_ms": round(t_model, 1), "total_ms": round(t_copy + t_model, 1),
                        "mAP_abs_diff": float(abs(want[0] - mAP)), "top1_equal": bool(want[1][0] == top1),
                        "cmc_equal": bool(np.array_equal(want[1], cmc(dist, qid, gid, qcam, gcam, topk=topk, first_match_break=True))),
                        "mean_ap_abs_diff": float(abs(want[0] - mean_ap(dist, qid, gid, qcam, gcam)))}
    print(json.dumps(res))


def single_shot_mode(spec, reps, noise, out_path=None):
    import numpy as np
    from rg_hip.lib import lib
    from clustercontrast.evaluation_metrics import cmc_single_shot
    Q, G = (int(v) for v in spec.split(","))
    D, n_id, n_cam, topk, repeat = 128, 751, 6, 100, 10
    g = torch.Generator(device=dev).manual_seed(0)
    centres = F.normalize(torch.randn(n_id, D, generator=g, device=dev), dim=1)
    ids = torch.randint(0, n_id, (Q + G,), generator=g, device=dev)
    cams = torch.randint(0, n_cam, (Q + G,), generator=g, device=dev).int()
    x = F.normalize(centres[ids] + noise * torch.randn(Q + G, D, generator=g, device=dev) / D ** 0.5, dim=1)
    ids = ids.int()
    qid, gid, qcam, gcam = ids[:Q].contiguous(), ids[Q:].contiguous(), cams[:Q].contiguous(), cams[Q:].contiguous()
    dist = dist_block(x[:Q].contiguous(), x[Q:].contiguous(), 1.0, True)
    mats = {"fp32": dist, "fp64": dist.double()}
    p = ops._p
    med, spread, regimes = {}, {}, {}
    plan = None
    for tag, d in mats.items():
        plan = ops.cmc_shot_order(d, qid, gid, qcam, gcam, True)
        regimes[tag] = ops.cmc_shot_regime(G, plan["nid"], tag == "fp64")
        n_h, high_h = plan["n_host"], plan["high_host"]
        # the chunks `ops.cmc_shot` takes, their draws made and uploaded ahead of the timed launches
        per_query, bounds, q0 = n_h.astype(np.int64) * repeat * 4, [], 0
        while q0 < Q:
            q1 = q0 + max(1, int(np.searchsorted(np.cumsum(per_query[q0:]), ops.CMC_SHOT_DRAW_BYTES, side="right")))
            bounds.append((q0, q1))
            q0 = q1
        rs = np.random.RandomState(0)
        chunks = []
        for q0, q1 in bounds:
            highs = np.concatenate([np.tile(high_h[q, :n_h[q]], repeat) for q in range(q0, q1) if n_h[q] > 0])
            off = np.zeros(q1 - q0, dtype=np.int64)
            off[1:] = np.cumsum(n_h[q0:q1 - 1].astype(np.int64) * repeat)
            chunks.append((q0, q1, torch.from_numpy(rs.randint(0, highs).astype(np.int32)).to(dev), torch.from_numpy(off).to(dev)))
        rank = torch.empty((Q, repeat), dtype=torch.int32, device=dev)
        hist = torch.zeros(topk, dtype=torch.int32, device=dev)
        status = torch.empty(1, dtype=torch.int32, device=dev)
        samples = {"order": [], "rank": []}
        for it in range(reps + 1):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            ev[0].record()
            lib.rg_cmc_shot_order(p(d), int(tag == "fp64"), Q, G, G, plan["nid"], p(plan["seg_ptr"]), p(plan["seg_perm"]), p(gcam),
                                  p(plan["query_seg"]), p(qcam), 1, p(plan["n"]), p(plan["slot"]), p(plan["high"]), p(status), ops._stream())
            ev[1].record()
            for q0, q1, draws_d, off_d in chunks:
                lib.rg_cmc_shot_rank(p(d), int(tag == "fp64"), Q, q0, q1 - q0, G, G, plan["nid"], p(plan["seg_ptr"]), p(plan["seg_perm"]),
                                     p(gcam), p(plan["query_seg"]), p(qcam), 1, p(plan["n"]), p(plan["slot"]), p(draws_d), p(off_d),
                                     repeat, topk, p(rank), p(hist), ops._stream())
            ev[2].record()
            torch.cuda.synchronize()
            if it:                                   # pass 0 is the warm-up
                samples["order"].append(ev[0].elapsed_time(ev[1]))
                samples["rank"].append(ev[1].elapsed_time(ev[2]))
        for k, v in samples.items():
            med["%s_%s" % (k, tag)] = round(float(np.median(v)), 3)
            spread["%s_%s" % (k, tag)] = [round(min(v), 3), round(max(v), 3)]
        del chunks
    # host steps on the fp32 plan: the copy of n and high, the draws of all chunks, their upload
    n_h, high_h = plan["n_host"], plan["high_host"]
    host = {"highs_copy": [], "draws": [], "upload": []}
    highs_all = np.concatenate([np.tile(high_h[q, :n_h[q]], repeat) for q in range(Q) if n_h[q] > 0])
    for it in range(reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        plan["n"].cpu().numpy(); plan["high"].cpu().numpy()
        t1 = time.perf_counter()
        draws = np.random.RandomState(it).randint(0, highs_all).astype(np.int32)
        t2 = time.perf_counter()
        torch.from_numpy(draws).to(dev)
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        if it:
            for k, v in zip(("highs_copy", "draws", "upload"), (t1 - t0, t2 - t1, t3 - t2)):
                host[k].append(v * 1e3)
    wall = {}
    for tag, d in mats.items():
        w = []
        for it in range(reps + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            curve = cmc_single_shot(d, qid, gid, qcam, gcam, topk=topk, separate_camera_set=True, random_state=np.random.RandomState(0))
            if it:
                w.append((time.perf_counter() - t0) * 1e3)
        wall[tag] = round(float(np.median(w)), 1)
    res = {"single_shot": {"Q": Q, "G": G, "D": D, "identities": int(plan["nid"]), "cameras": n_cam, "topk": topk, "repeat": repeat,
                           "separate_camera_set": True, "noise": noise, "reps": reps},
           "regime": regimes, "kernel_ms_median": med, "kernel_ms_min_max": spread, "matrix_MB_fp32": round(Q * G * 4 / 1e6, 1),
           "draws": int(highs_all.size), "draw_MB": round(highs_all.size * 4 / 1e6, 1), "valid_queries": int((n_h > 0).sum()),
           "host_ms_median": {k: round(float(np.median(v)), 2) for k, v in host.items()},
           "cmc_single_shot_wall_ms_median": wall, "top1": round(float(curve[0]), 6)}
    line = json.dumps(res)
    print(line)
    if out_path:
        with open(out_path, "a") as f:
            f.write(line + "\n")


if "--single-shot" in sys.argv:
    _i = sys.argv.index("--single-shot") + 1
    _spec = sys.argv[_i] if _i < len(sys.argv) and not sys.argv[_i].startswith("--") else "3368,15913"
    _reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 5
    _noise = float(sys.argv[sys.argv.index("--noise") + 1]) if "--noise" in sys.argv else 0.90
    _out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    single_shot_mode(_spec, _reps, _noise, _out)
    sys.exit(0)

if "--evaluate" in sys.argv:
    _i = sys.argv.index("--evaluate") + 1
    _spec = sys.argv[_i] if _i < len(sys.argv) and not sys.argv[_i].startswith("--") else "3368,15913"
    _reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 5
    _noise = float(sys.argv[sys.argv.index("--noise") + 1]) if "--noise" in sys.argv else 0.90
    evaluate_mode(_spec, _reps, _noise)
    sys.exit(0)

if "--kmeans" in sys.argv:
    _i = sys.argv.index("--kmeans") + 1
    _spec = sys.argv[_i] if _i < len(sys.argv) and not sys.argv[_i].startswith("--") else "12936,2048,500"
    _reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 30
    _noise = float(sys.argv[sys.argv.index("--noise") + 1]) if "--noise" in sys.argv else 0.30
    kmeans_mode(_spec, _reps, _noise)
    sys.exit(0)

if "--infomap" in sys.argv:
    _i = sys.argv.index("--infomap") + 1
    _spec = sys.argv[_i] if _i < len(sys.argv) and not sys.argv[_i].startswith("--") else "12936,2048,15,0.5,4"
    _reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 30
    _noise = float(sys.argv[sys.argv.index("--noise") + 1]) if "--noise" in sys.argv else 0.30
    infomap_mode(_spec, _reps, _noise)
    sys.exit(0)

if "--dbscan" in sys.argv:
    _reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 5
    _noise = float(sys.argv[sys.argv.index("--noise") + 1]) if "--noise" in sys.argv else 0.30
    dbscan_mode(sys.argv[sys.argv.index("--dbscan") + 1], _reps, _noise)
    sys.exit(0)

if "--jaccard" in sys.argv:
    _reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 5
    _noise = float(sys.argv[sys.argv.index("--noise") + 1]) if "--noise" in sys.argv else 0.30
    jaccard_mode(sys.argv[sys.argv.index("--jaccard") + 1], _reps, _noise)
    sys.exit(0)

g = torch.Generator(device=dev).manual_seed(0)
x = F.normalize(torch.randn(12936, 2048, generator=g, device=dev), dim=1)

def knn(k=15, block=2048):
    n = x.shape[0]
    for r0 in range(0, n, block):
        r1 = min(n, r0 + block)
        ops.topk_rows(ops.linear_fwd(x[r0:r1], x), k)

def timeit(fn, reps=3):
    fn(); torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps): fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps

t_knn = timeit(knn)
q = F.normalize(torch.randn(3368, 2048, generator=g, device=dev), dim=1)
gal = F.normalize(torch.randn(15913, 2048, generator=g, device=dev), dim=1)
t_dist = timeit(lambda: dist_block(q, gal, 1.0, True))
print(json.dumps({"knn_12936x2048_k15_ms": round(t_knn * 1e3, 2), "knn_gemm_tflops": round(2 * 12936 ** 2 * 2048 / t_knn / 1e12, 1),
                  "pairwise_3368x15913x2048_ms": round(t_dist * 1e3, 2),
                  "pairwise_tflops": round(2 * 3368 * 15913 * 2048 / t_dist / 1e12, 1)}))
