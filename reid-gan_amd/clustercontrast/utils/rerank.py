"""k-reciprocal re-ranking of a query / gallery distance matrix on the MI355X.

Mirror of CC/clustercontrast/utils/rerank.py `re_ranking` (:32-99; Zhong et al., CVPR 2017), same name, arguments and
return type, so `Evaluator.evaluate(..., rerank=True)` (CC/clustercontrast/evaluators.py:138-142, inherited from the
reference tree) picks it up through `from .utils.rerank import re_ranking`.  The reference builds dense [Q+G, Q+G]
matrices and loops over them in numpy; here

  1. `rg_rerank_orig_dist` assembles transpose(d^2 / max(d^2, axis=0)) from the three inputs in fp32 with the
     reference's operation order (:40-46), and `rg_topk_rows` on its negated row blocks yields the first
     max(k1 + 1, k2) columns of the argsort (ties by lower index; numpy's quicksort leaves them unspecified);
  2. - 6. `ops.rerank_from_rank` (csrc/rerank.hip): k-reciprocal sets, weights exp(-d) / sum, local query expansion,
     column lists, Jaccard rows of the Q queries blended with the normalised distance, columns Q: only.

Inputs are numpy arrays or tensors (any float type; computed in fp32 like the reference's `.astype(np.float32)`).
"""
from __future__ import absolute_import, division, print_function

from rg_hip import ops, search

from .faiss_rerank import half_k

__all__ = ['re_ranking']


def re_ranking(q_g_dist, q_q_dist, g_g_dist, k1=20, k2=6, lambda_value=0.3, chunk=0, debug=False, return_device=False):
    """numpy [Q, G] float32: (1 - lambda) * Jaccard distance + lambda * normalised original distance
    (return_device=True: the same matrix as a device tensor, not copied to the host)"""
    q_g, q_q, g_g = (search.as_matrix(a, "re_ranking: " + name)
                     for a, name in ((q_g_dist, "q_g_dist"), (q_q_dist, "q_q_dist"), (g_g_dist, "g_g_dist")))
    Q, G = q_g.shape
    if tuple(q_q.shape) != (Q, Q) or tuple(g_g.shape) != (G, G):
        raise ValueError("re_ranking: q_g_dist %s needs q_q_dist [%d, %d] and g_g_dist [%d, %d], got %s and %s"
                         % (tuple(q_g.shape), Q, Q, G, G, tuple(q_q.shape), tuple(g_g.shape)))
    N = Q + G
    k1, k2 = int(k1), int(k2)
    if not 1 <= k1 < N:
        raise ValueError("re_ranking: need 1 <= k1 < Q + G, got k1=%d, Q + G=%d" % (k1, N))
    if not 1 <= k2 <= k1:
        raise ValueError("re_ranking: need 1 <= k2 <= k1, got k2=%d, k1=%d" % (k2, k1))
    dev = search.device()
    orig = ops.rerank_orig_dist(q_g.to(dev).contiguous(), q_q.to(dev).contiguous(), g_g.to(dev).contiguous())
    R = k1 + 1                                      # the only columns of the argsort that are read (k2 <= k1)
    # top-k of -d = the k smallest d
    rank = search.blocked_topk(N, R, lambda r0, r1: ops.add_outer_terms(orig[r0:r1].clone(), alpha=-1.0))
    res = ops.rerank_from_rank(rank, k1 + 1, half_k(k1) + 1, k2, orig=orig, rows=Q, col_off=Q, lambda_value=lambda_value,
                               clamp=False, chunk=chunk, debug=debug)
    out = res[0] if debug else res
    final_dist = out if return_device else out.cpu().numpy()
    return (final_dist, res[1]) if debug else final_dist
