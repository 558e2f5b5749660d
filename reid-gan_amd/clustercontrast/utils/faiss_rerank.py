"""k-reciprocal Jaccard distance for the DBSCAN pseudo-labelling step on the MI355X, without faiss.

Mirror of CC/clustercontrast/utils/faiss_rerank.py (Zhong et al., "Re-ranking Person Re-identification with k-reciprocal
Encoding", CVPR 2017): `compute_jaccard_distance` (:31-127) and `k_reciprocal_neigh` (:24-28), same names, arguments and
return types, so `rerank_dist = compute_jaccard_distance(features, k1=args.k1, k2=args.k2)`
(examples/cluster_contrast_train_usl.py:154) runs unchanged.  Every stage runs on the device and only the final
[N, N] matrix leaves it:

  1. initial ranking: the k1 nearest rows by squared L2 distance |x_j|^2 - 2 x_i . x_j (faiss IndexFlatL2), row blocks of
     the MFMA GEMM + `rg_row_sqsum` + `rg_topk_rows` — distance ascending, ties by lower index (faiss leaves ties unspecified);
  2. k-reciprocal sets and their expansion, 3. softmax weights, 4. local query expansion, 5. column lists,
  6. Jaccard rows: `ops.rerank_from_rank` (csrc/rerank.hip).  The reference's dense V [N, N] is never built.

`search_option` selects between four faiss code paths in the reference; here there is one path and the argument is
accepted and ignored.  `use_float16=True` makes the reference hold V and the result in float16; here the computation stays
fp32 and the fp32 result is cast to float16 on return (same dtype as the reference's, closer to the exact values).
The input is the CPU tensor `extract_features` yields or a device tensor; there is no CPU path.
`return_device=True` (not in the reference) keeps the result on the device for clustercontrast.utils.dbscan /
clustercontrast.utils.pseudo_labels, which removes the 669 MB copy per epoch at Market-1501 size.
"""
from __future__ import absolute_import, print_function

import time

import numpy as np

from rg_hip import ops, search


def k_reciprocal_neigh(initial_rank, i, k1):
    """members j of initial_rank[i, :k1+1] that have i in initial_rank[j, :k1+1] (host helper, numpy arrays)"""
    forward = initial_rank[i, :k1 + 1]
    return forward[(initial_rank[forward, :k1 + 1] == i).any(axis=1)]


def half_k(k1):
    """int(np.around(k1 / 2)): half to even, as the reference (k1 = 5 -> 2, k1 = 30 -> 15)"""
    return int(np.around(k1 / 2.))


def l2_rank(x, k):
    """int32 [N, k]: the k nearest rows of x [N, D] (device, fp32) by squared L2 distance, ascending, ties by lower index"""
    sq = ops.row_sqsum(x)

    def score_block(r0, r1):
        block = ops.linear_fwd(x[r0:r1], x)                                      # [rows, n] inner products
        return ops.add_outer_terms(block, None, sq, alpha=2.0, b=-1.0)           # 2 x_i . x_j - |x_j|^2 = |x_i|^2 - d^2
    return search.blocked_topk(x.shape[0], k, score_block)


def compute_jaccard_distance(target_features, k1=20, k2=6, print_flag=True, search_option=0, use_float16=False, chunk=0,
                             debug=False, return_device=False):
    """numpy [N, N] float32 (float16 with use_float16: the fp32 result, cast) k-reciprocal Jaccard distance of the rows of
    `target_features` [N, D].  As in the reference the weights treat the rows as L2-normalised (2 - 2 x.y) whatever the
    input is, while the ranking uses the true L2 distance.  `chunk` (columns per workgroup of the Jaccard kernel, 0 =
    automatic) and `debug` (also return the device-side ranks, sets and encodings) are for tests.  `return_device=True`
    returns the fp32 [N, N] device tensor instead (whatever `use_float16` says) and copies nothing to the host: the input
    of clustercontrast.utils.dbscan.DBSCAN."""
    end = time.time()
    if print_flag:
        print('Computing jaccard distance...')
    target_features = search.as_matrix(target_features, "compute_jaccard_distance: target_features")
    N = target_features.size(0)
    k1, k2 = int(k1), int(k2)
    if not 1 <= k1 < N:
        raise ValueError("compute_jaccard_distance: need 1 <= k1 < N, got k1=%d, N=%d" % (k1, N))
    if not 1 <= k2 <= k1:
        raise ValueError("compute_jaccard_distance: need 1 <= k2 <= k1, got k2=%d, k1=%d" % (k2, k1))
    x = target_features.to(search.device()).contiguous()
    rank = l2_rank(x, k1)              # the reference searches k1 neighbours: its slice [:k1+1] has k1 entries
    res = ops.rerank_from_rank(rank, k1, min(half_k(k1) + 1, k1), k2, x=x, clamp=True, chunk=chunk, debug=debug)
    out = res[0] if debug else res
    if return_device:
        jaccard_dist = out
    else:
        jaccard_dist = out.cpu().numpy()
        if use_float16:
            jaccard_dist = jaccard_dist.astype(np.float16)
    if print_flag:
        print("Jaccard distance computing time cost: {}".format(time.time() - end))
    return (jaccard_dist, res[1]) if debug else jaccard_dist
