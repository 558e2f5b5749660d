"""CPU: the stage model of the re-ranking kernels (tests/rerank_hostmodel.py) is one a correct implementation meets and a subtly
wrong one does not.

  * the references on the kernels' own objects agree with the dense model (expand_sets, dense_weights, query_expand,
    jaccard_rows) on the three golden inputs and on the case lists: integers exactly, floats within a written budget;
  * plain float32 torch, on every weights case of the device tests, stays inside the per-element budget — and its ratio is the
    source of C_KIND["softmax"] = max(8, 4 x ratio);
  * the case lists reach every regime of the mirrored dispatch arithmetic (asserted from the mirrors);
  * fourteen one-defect variants of the references are each told apart from the true model by some case of the lists.

Run as a script (python -m tests.test_rerank_hostmodel_cpu) it prints the ratio table of the host model's docstring."""
import functools
import os

import numpy as np
import pytest
import torch

from tests import rerank_hostmodel as H
from tests.golden import cases_rerank as C

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(REPO, "tests", "golden", "reference_rerank.npz"))
F32 = np.float32


def _scatter(rowptr, cols, vals, N):
    V = np.zeros((N, N), dtype=F32)
    row = np.repeat(np.arange(N), np.diff(rowptr))
    V[row, cols] = vals
    return V


def _jaccard_tol(rowptr):
    """|J_f32 - J_f64|: the sequential float32 sum of n non-negative terms is within (n - 1) 2^-24 of m <= 1 (relative), |dJ/dm|
    = 2 / (2 - m)^2 <= 2 on [0, 1]; the float32 subtraction, division and subtraction of values <= 2 add three roundings of at
    most 2^-24 * 2 each, the dense model's final cast one more"""
    return 2.0 * int(np.diff(rowptr).max()) * H.U24 + 8.0 * H.U24


# ---- the stage model against the dense model ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(C.CASES))
def test_stage_model_equals_dense_model_on_the_golden_inputs(name):
    cs, x = C.CASES[name], GOLD[name + "_x"]
    k1, k2, n = cs["k1"], cs["k2"], len(x)
    kh = min(C.half_k(k1) + 1, k1)
    rank = C.rank_of(C.sq_l2(x), k1)
    dense_sets = H.expand_sets(rank, k1, kh)
    sets, counts = H.expand(rank, k1, kh)
    assert all(np.array_equal(a, b) for a, b in zip(sets, dense_sets)) and counts.tolist() == [len(s) for s in dense_sets]
    cap = H.default_cap(n, k1, kh)
    assert counts.max() <= cap
    padded = H.pad_sets(sets, cap)
    V = H.dense_weights(dense_sets, x=x)
    ref = H.weights_feat(x, padded, counts)
    got = np.full((n, cap), H.FILL, dtype=F32)
    for i, s in enumerate(sets):
        got[i, :len(s)] = V[i, s]
    assert H.compare(got, ref).ok                        # the dense model is the fp64 value rounded once
    w = ref.value.astype(F32)
    for form in ("feat", "dist"):
        if form == "dist":
            orig = C.normalised_dist64(*C.euclid_inputs(x)).astype(F32)
            V = H.dense_weights(dense_sets, orig=orig)
            ref = H.weights_dist(orig, padded, counts)
            for i, s in enumerate(sets):
                got[i, :len(s)] = V[i, s]
            assert H.compare(got, ref).ok
        for i, s in enumerate(sets):                     # the same float32 weights on both sides from here on
            w[i, :len(s)] = V[i, s]
        rowcnt, rowptr, cols, vals = H.query_expand_csr(padded, w, counts, rank if k2 != 1 else None, k2)
        Vq = H.query_expand(V, rank, k2)
        assert np.array_equal(_scatter(rowptr, cols, vals, n), Vq) and int(rowptr[-1]) == int((Vq != 0).sum())
        rows = n // 4
        J = H.jaccard_rows_csr(rowptr, cols, vals, n, rows, clamp=False)
        assert np.abs(J.astype(np.float64) - H.jaccard_rows(Vq, range(rows))).max() <= _jaccard_tol(rowptr)
    q_g, q_q, g_g = C.euclid_inputs(x)
    o = H.orig_dist(q_g, q_q, g_g)
    assert np.abs(o - C.normalised_dist64(q_g, q_q, g_g)).max() <= 4.0 * H.U24      # values <= 1: a square, a division, a cast


def test_stage_model_equals_dense_model_on_the_case_lists():
    seen = 0
    for case in H.expand_cases():
        tag, N, R, kf, kh, opts, capmode = case
        if opts.get("invalid") or capmode != "default":
            continue                                     # the dense model indexes with every entry and never truncates
        rank, cap = H.expand_input(case)
        sets, counts = H.expand(rank, kf, kh, cap)
        dense = H.expand_sets(rank.astype(np.int64), kf, kh)
        assert all(np.array_equal(a, b) for a, b in zip(sets, dense)), tag
        assert counts.tolist() == [len(s) for s in dense] and counts.max() <= cap
        seen += 1
    assert seen >= 5
    rank, kf, kh, row, want = H.two_thirds_graph()
    assert H.expand(rank, kf, kh)[0][row].tolist() == want == H.expand_sets(rank.astype(np.int64), kf, kh)[row].tolist()
    # query expansion and Jaccard rows of the device cases against the dense operations on the scattered matrices
    for case in H.QE_CASES[:5]:
        sets, counts, w, rank = H.qe_input(case)
        N, k2 = case[1], case[3]
        V = np.zeros((N, N), dtype=F32)
        for i in range(N):
            n = min(int(counts[i]), sets.shape[1])
            ok = (sets[i, :n] >= 0) & (sets[i, :n] < N)
            V[i, sets[i, :n][ok]] = w[i, :n][ok]
        acc = np.zeros_like(V)
        for l in range(k2):
            r = np.arange(N) if rank is None else rank[:, l].astype(np.int64)
            ok = (r >= 0) & (r < N)
            acc[ok] += V[r[ok]]
        rowcnt, rowptr, cols, vals = H.query_expand_csr(sets, w, counts, rank, k2)
        assert np.array_equal(_scatter(rowptr, cols, vals, N), acc / F32(k2)), case[0]
        assert np.array_equal(np.diff(rowptr), rowcnt) and all(
            (np.diff(cols[rowptr[i]:rowptr[i + 1]]) > 0).all() for i in range(N))
    rowptr, cols, vals, N = H.jaccard_input()
    Vq = _scatter(rowptr, cols, vals, N)
    J = H.jaccard_rows_csr(rowptr, cols, vals, N, N, clamp=False)
    with np.errstate(divide="ignore"):
        assert np.abs(J.astype(np.float64) - H.jaccard_rows(Vq, range(N))).max() <= _jaccard_tol(rowptr) * 4.0   # m up to 1.25: |dJ/dm| <= 8 / 2.25
    assert (J == 0).any() and (J == 1).any() and (J < 0).any()          # m exactly 1, no common column, and work for the clamp
    assert np.array_equal(J[:8, :8] == 0, np.kron(np.eye(4), np.ones((2, 2))) == 1)
    for name in ("n1", "n5", "n257"):
        rowptr, cols, vals, N = H.columns_input(name)
        colptr, crow, cval = H.columns(rowptr, cols, vals, N)
        V = _scatter(rowptr, cols, vals, N)
        assert np.array_equal(np.diff(colptr), (V != 0).sum(axis=0))
        for c in range(N):
            assert np.array_equal(crow[colptr[c]:colptr[c + 1]], np.nonzero(V[:, c])[0])
            assert np.array_equal(cval[colptr[c]:colptr[c + 1]], V[crow[colptr[c]:colptr[c + 1]], c])


# ---- float32 torch of every weights case: the source of C_KIND["softmax"] -------------------------------------------------------------
def _torch_weights(src, sets, counts, cap, feat):
    N = src.shape[0]
    out = np.full((N, cap), H.FILL, dtype=F32)
    t = torch.from_numpy(src)
    for i in range(N):
        n = min(int(counts[i]), cap)
        s = torch.from_numpy(sets[i, :n].astype(np.int64))
        ok = (s >= 0) & (s < N)
        row = torch.zeros(n)
        if n and not bool(ok.any()):
            row[:] = float("nan")
        elif n:
            if feat:
                row[ok] = torch.softmax(-(2.0 - 2.0 * (t[s[ok]] @ t[i])), 0)
            else:
                e = torch.exp(-t[i, s[ok]])
                row[ok] = e / e.sum()
        out[i, :n] = row.numpy()
    return out


def _weights_outputs():
    sets, counts = H.weights_sets()
    for D in H.WEIGHTS_D:
        for fam in H.FEAT_FAMILIES:
            x = H.feat_input(D, fam)
            yield "feat D %d %s" % (D, fam), _torch_weights(x, sets, counts, H.WEIGHTS_CAP, True), H.weights_feat(x, sets, counts)
    for fam in H.DIST_FAMILIES:
        o = H.dist_input(fam)
        yield "dist %s" % fam, _torch_weights(o, sets, counts, H.WEIGHTS_CAP, False), H.weights_dist(o, sets, counts)


@functools.lru_cache(maxsize=None)
def _ratios():
    worst, bad = 0.0, []
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        for name, got, ref in _weights_outputs():
            w = H.compare(got, ref)
            worst = max(worst, w.ratio)
            if not w.ok:
                bad.append("%s: worst %s err %.3e budget %.3e ratio %.2f" % (name, w.index, w.err, w.budget, w.ratio))
    finally:
        torch.set_num_threads(threads)
    return worst, bad


def test_float32_torch_meets_the_budget_on_every_weights_case():
    worst, bad = _ratios()
    print("softmax: float32 torch ratio %.2f" % worst)
    assert not bad, "\n".join(bad)
    assert np.isfinite(worst) and worst > 0


def test_constant_follows_the_rule():
    """C_KIND = max(8, 4 x float32-torch ratio) as measured where the table was made; torch's summation order differs between
    hosts (threads, vector width), hence a quarter of slack instead of equality, as in the other host models"""
    worst, _ = _ratios()
    assert H.C_KIND["softmax"] >= 8.0 and 4.0 * worst <= 1.25 * H.C_KIND["softmax"], worst
    assert abs(H.C_KIND["softmax"] - max(8.0, 4.0 * worst)) <= 0.25 * H.C_KIND["softmax"]
    assert H.C_KIND["exact"] == 0.0 and set(H.C_KIND) == {"softmax", "exact"}


def test_weights_references_pin_the_edges():
    sets, counts = H.weights_sets()
    x = H.feat_input(64, "scaled8")
    ref = H.weights_feat(x, sets, counts)
    for r in (ref, H.weights_dist(H.dist_input("to80"), sets, counts)):
        v, M = r.value, r.M
        assert np.isnan(v[16, :2]).all() and np.isnan(v[17, :5]).all() and (M[16:18] == 0).all()     # only invalid entries
        assert v[10, 2] == 0 and v[10, 3] == 0 and M[10, 2] == 0 and v[11, 128] == 0 and v[11, 129] == 0
        assert (v[0] == H.FILL).all() and (v[1, 1:] == H.FILL).all() and (v[6] != H.FILL).all() and counts[6] > H.WEIGHTS_CAP
        rows = [i for i in range(H.WEIGHTS_N) if i not in (16, 17) and counts[i]]
        assert np.abs(np.array([v[i, :min(counts[i], H.WEIGHTS_CAP)].sum() for i in rows]) - 1).max() < 1e-12
    d = -(2.0 - 2.0 * (x.astype(np.float64) * x.astype(np.float64)).sum(axis=1))
    with np.errstate(over="ignore"):
        assert 125.0 < d.max() < 127.0 and np.exp(F32(d.max())) == np.inf                                # only the subtraction saves expf
    o = H.dist_input("to80")
    assert o.max() > 79.0 and np.exp(-o.max()) > 2.0 ** -126


# ---- reach: asserted from the mirrors --------------------------------------------------------------------------------------------------
def test_case_lists_reach_every_regime():
    ec = H.expand_cases()
    assert set(c[1] for c in ec) >= set(H.EXPAND_N) | {H.EXPAND_WIDE_N} and set((c[3], c[4]) for c in ec) >= set(H.EXPAND_K)
    assert set(H.emit_per(c[1]) for c in ec) == {1, 2} and H.emit_per(8192) == 1 and H.emit_per(8200) == 2
    assert H.emit_last_thread_words(8200) == 1 and H.words(8200) == 257
    assert set(H.words(n) for n in (1, 31, 32, 33)) == {1, 2}
    assert set(H.strided_trips(c[3]) for c in ec) == {1, 2}                                  # the p += 256 loops
    assert set(min(H.strided_trips(c[3] * c[4]), 3) for c in ec) == {1, 2, 3}                # the idx += 256 loops
    assert any(c[2] == c[3] for c in ec) and any(c[2] > c[3] for c in ec)                    # R == kf, R > kf
    kf, kh = H.largest_expand(H.EXPAND_WIDE_N, H.EXPAND_WIDE_N)
    assert any((c[1], c[3], c[4]) == (H.EXPAND_WIDE_N, kf, kh) for c in ec)
    assert H.expand_lds(H.EXPAND_WIDE_N, kf, kh) <= H.LDS_LIMIT < H.expand_lds(H.EXPAND_WIDE_N, kf, kh + 1)
    assert all(a * b <= kf * kh for a in range(1, 321) for b in range(1, a + 1) if H.expand_lds(320, a, b) <= H.LDS_LIMIT)
    assert all(H.expand_lds(c[1], c[3], c[4]) <= H.LDS_LIMIT for c in ec)
    caps = [(c, H.default_cap(c[1], c[3], c[4])) for c in ec]
    assert any(cap == c[1] < c[3] * (c[4] + 1) for c, cap in caps) and any(cap == c[3] * (c[4] + 1) < c[1] for c, cap in caps)
    assert set(c[6] for c in ec) == {"default", "below", "one"}
    assert any(c[5].get("swap_first") for c in ec) and any(c[5].get("invalid") for c in ec)
    for c in ec:
        rank, cap = H.expand_input(c)
        cnt = H.expand(rank, c[3], c[4], cap)[1]
        if c[6] == "below":
            assert cnt.max() == cap + 1
        if c[6] == "one":
            assert cnt.max() > 1 == cap
        if c[5].get("invalid"):
            assert (rank[:, :c[3]] == -1).any() and (rank[:, :c[3]] == c[1]).any()
        if c[5].get("swap_first"):
            assert (rank[:, 0] != np.arange(c[1])).any()
    # weights
    Ds = H.WEIGHTS_D
    assert set(d % 4 for d in Ds) >= {0, 1, 3} and min(Ds) == 1 and any(d < 64 for d in Ds) and 64 in Ds
    assert set(H.strided_trips(d) for d in Ds) == {1, 2, 3}                                  # the x_i staging loop
    assert set(min(H.cdiv(d // 4, 64), 3) for d in Ds if d % 4 == 0) == {1, 2, 3}            # the float4 dot product
    assert any(d % 4 and d > 256 for d in Ds)
    sets, counts = H.weights_sets()
    n_eff = np.minimum(counts, H.WEIGHTS_CAP)
    assert set(n_eff.tolist()) == set(H.WEIGHTS_SIZES) and set(H.strided_trips(int(n)) for n in n_eff if n) == {1, 2}
    assert set(int(n) % 4 for n in n_eff) >= {0, 1, 2} and (counts > H.WEIGHTS_CAP).any()
    D, cap_bad, cap_ok = H.weights_refusal()
    assert H.weights_lds(D, cap_ok) <= H.LDS_LIMIT < H.weights_lds(D, cap_bad) and cap_bad == cap_ok + 1
    assert H.weights_lds(0, H.LDS_LIMIT // 4) <= H.LDS_LIMIT < H.weights_lds(0, H.LDS_LIMIT // 4 + 1)
    # query expansion
    assert set(c[1] for c in H.QE_CASES) == {33, 257, 8200} and set(c[3] for c in H.QE_CASES) == {1, 6, 64}
    assert any(c[2] is None for c in H.QE_CASES) and any(c[2] is not None and c[3] == 1 for c in H.QE_CASES)
    assert any(c[2] == c[3] for c in H.QE_CASES) and any(c[2] is not None and c[2] > c[3] for c in H.QE_CASES)
    assert set(H.emit_per(c[1]) for c in H.QE_CASES) == {1, 2}
    for case in H.QE_CASES:
        sets, counts, w, rank = H.qe_input(case)
        assert (counts > H.QE_CAP).any() and (counts == 0).any() and (sets == case[1]).any()
        if rank is not None:
            k2 = case[3]
            head = rank[:, :k2]
            assert ((head < 0) | (head >= case[1])).any()
            if k2 > 1:
                assert any(len(set(r.tolist())) < k2 for r in head)
    # column lists
    trips = {}
    for name in ("n1", "n5", "n257", "big"):
        rowptr, cols, vals, N = H.columns_input(name)
        trips[name] = H.col_count_trips(len(cols))
        if name in ("n5", "n257"):
            assert (np.diff(rowptr) == 0).any() and (np.bincount(cols, minlength=N) == 0).any()
        if name == "n257":
            assert np.diff(rowptr).max() == 200
        if name == "big":
            assert len(cols) == 256 * H.COL_COUNT_GRID + 1 and N <= H.MAX_N and len(set(np.diff(rowptr).tolist())) == 1
    assert trips == {"n1": 1, "n5": 1, "n257": 1, "big": 2} and H.col_count_trips(256 * H.COL_COUNT_GRID) == 1
    # Jaccard rows
    N, Q = H.JACCARD_N, H.JACCARD_Q
    assert H.jaccard_blocks() == [(N, 0), (Q, Q), (1, N - 1)]
    got = set()
    for rows, off in H.jaccard_blocks():
        for chunk in H.jaccard_chunk_values(N - off):
            got.add(H.jaccard_chunks(N, off, chunk))
    assert (1, 1) in got and (1, N) in got and (63, 3) in got and (64, 3) in got and (N, 1) in got and (N - Q, 1) in got
    assert H.jaccard_chunks(N, 0, N + 5) == (N, 1) and H.jaccard_chunks(N, Q, 0) == (N - Q, 1)
    B = H.JACCARD_BIG_N
    assert B == 16448 and H.jaccard_chunks(B, 0, 0) == (8256, 2) and H.jaccard_chunks(B, 0, 16384) == (16384, 2)
    assert 4 * H.jaccard_chunks(B, 0, H.JACCARD_MAX_CHUNK)[0] == 64 * 1024
    # normalised distances
    assert [H.colmax_segments(q + g) for q, g in H.ORIG_QG] == [(1, 2), (1, 41), (1, 64), (1, 64), (2, 300)]
    assert any((q + g) % 32 == 0 for q, g in H.ORIG_QG) and any(q % 32 and g % 32 and (q + g) % 32 == 0 for q, g in H.ORIG_QG)
    assert any((q + g) % 32 for q, g in H.ORIG_QG) and (100 + 500) % 256 and (100 + 500) > 512


# ---- one-defect variants: the case lists must tell each from the true model -----------------------------------------------------------------
def _expand_differs(variant):
    hits = []
    for case in H.expand_cases():
        rank, cap = H.expand_input(case)
        true, mut = H.expand(rank, case[3], case[4], cap), H.expand(rank, case[3], case[4], cap, variant)
        if not (all(np.array_equal(a, b) for a, b in zip(true[0], mut[0])) and np.array_equal(true[1], mut[1])):
            hits.append(case[0])
    return hits


def _weights_differs(variant):
    sets, counts = H.weights_sets()
    hits = []
    for D in (4, 64):
        for fam in H.FEAT_FAMILIES:
            x = H.feat_input(D, fam)
            ref = H.weights_feat(x, sets, counts)
            assert H.compare(ref.value.astype(F32), ref).ok
            if not H.compare(H.weights_feat(x, sets, counts, variant=variant).value.astype(F32), ref).ok:
                hits.append("feat D %d %s" % (D, fam))
    if variant == "invalid_exp0":
        for fam in H.DIST_FAMILIES:
            o = H.dist_input(fam)
            ref = H.weights_dist(o, sets, counts)
            if not H.compare(H.weights_dist(o, sets, counts, variant=variant).value.astype(F32), ref).ok:
                hits.append("dist " + fam)
    return hits


def _qe_differs(variant):
    hits = []
    for case in H.QE_CASES[:5]:
        sets, counts, w, rank = H.qe_input(case)
        true, mut = H.query_expand_csr(sets, w, counts, rank, case[3]), H.query_expand_csr(sets, w, counts, rank, case[3], variant)
        if not (np.array_equal(true[2], mut[2]) and H.same_bits(true[3], mut[3])):
            hits.append(case[0])
    return hits


def _jaccard_differs(variant):
    rowptr, cols, vals, N = H.jaccard_input()
    hits = []
    for rows, off in H.jaccard_blocks():
        for orig in (None, H.jaccard_orig(N, rows)):
            for clamp in (False, True):
                a = H.jaccard_rows_csr(rowptr, cols, vals, N, rows, off, orig, H.JACCARD_LAMBDA, clamp)
                b = H.jaccard_rows_csr(rowptr, cols, vals, N, rows, off, orig, H.JACCARD_LAMBDA, clamp, variant)
                if not H.same_bits(a, b):
                    hits.append((rows, off, orig is not None, clamp))
    return hits


def _orig_differs(variant):
    hits = []
    for Q, G in H.ORIG_QG:
        blocks = H.orig_input(Q, G)
        if not H.same_bits(H.orig_dist(*blocks), H.orig_dist(*blocks, variant=variant)):
            hits.append((Q, G))
    return hits


DEFECTS = [("two_thirds_ge", _expand_differs, "ge"), ("half_sets_tested_with_kf", _expand_differs, "kf_half"),
           ("truncation_keeps_the_last", _expand_differs, "keep_last"), ("counts_clipped_to_cap", _expand_differs, "clip_counts"),
           ("invalid_entry_weighs_exp0", _weights_differs, "invalid_exp0"), ("softmax_without_max", _weights_differs, "no_max"),
           ("qe_divides_by_valid_rows", _qe_differs, "div_valid"), ("qe_sums_in_row_order", _qe_differs, "row_order"),
           ("jaccard_descending_columns", _jaccard_differs, "desc"), ("jaccard_orig_not_offset", _jaccard_differs, "orig_shift"),
           ("clamp_before_blend", _jaccard_differs, "clamp_first"), ("orig_dist_row_maximum", _orig_differs, "rowmax"),
           ("orig_dist_not_transposed", _orig_differs, "no_transpose"), ("assembled_lower_left_untransposed", _orig_differs, "lower_left")]


@pytest.mark.parametrize("name,differs,variant", DEFECTS, ids=[d[0] for d in DEFECTS])
def test_the_case_lists_expose_every_defect(name, differs, variant):
    hits = differs(variant)
    print(name, "exposed by", hits)
    assert hits, "no case tells the %s variant from the true model" % name


def test_defects_are_exposed_where_they_should_be():
    """the two-thirds rule at equality is decided by the hand-made graph alone; the softmax without its maximum fails on the
    scaled rows and only there; the wrong orig offset shows only where col_off > 0; the clamp order only with a blend"""
    rank, kf, kh, row, want = H.two_thirds_graph()
    assert H.expand(rank, kf, kh, variant="ge")[0][row].tolist() == sorted(want + [10, 11, 12])
    assert all("scaled8" in h for h in _weights_differs("no_max"))
    assert all(off > 0 and has_orig for _, off, has_orig, _ in _jaccard_differs("orig_shift"))
    assert all(has_orig and clamp for _, _, has_orig, clamp in _jaccard_differs("clamp_first"))
    assert set(_orig_differs("lower_left")) >= {(31, 33), (100, 500)}


def test_comparator():
    ref = H.Ref(np.array([1.0, 0.0, np.nan, H.FILL]), np.array([1.0, 0.0, 0.0, 0.0]), "softmax")
    k = H.C_KIND["softmax"]
    assert H.compare(np.array([1.0 + 0.9 * k * H.U24, 0.0, np.nan, H.FILL]), ref).ok
    assert not H.compare(np.array([1.0 + 1.1 * k * H.U24, 0.0, np.nan, H.FILL]), ref).ok
    assert not H.compare(np.array([1.0, 1e-30, np.nan, H.FILL]), ref).ok                 # M == 0: equality
    assert not H.compare(np.array([1.0, 0.0, 0.0, H.FILL]), ref).ok                      # NaN only matches NaN
    assert not H.compare(np.array([np.inf, 0.0, np.nan, H.FILL]), ref).ok
    assert not H.compare(np.array([1.0, 0.0, np.nan, 0.5]), ref).ok                      # an element that must keep the fill value
    assert H.same_bits(np.array([0.5, np.nan], F32), np.array([0.5, np.nan], F32))
    assert not H.same_bits(np.array([0.0], F32), np.array([-0.0], F32))


if __name__ == "__main__":
    worst, bad = _ratios()
    print("\n".join(bad))
    print("    kind       float32 torch ratio    C_KIND")
    print("    %-10s %-22s %g" % ("softmax", "%.2f" % worst, max(8.0, round(4.0 * worst, 2))))
