"""Host model of the staged re-ranking pipeline (csrc/rerank.hip), for the tests.  No tests and no GPU here.

Two layers:

  the dense model    expand_sets, dense_weights, query_expand, jaccard_rows: the same stages on the same intermediate objects
                     (ranking -> expanded sets -> weights -> query expansion -> Jaccard rows), dense and slow; the yardstick of
                     tests/test_rerank_gpu.py and tests/test_rerank_fixture_cpu.py for whole-pipeline results.
  the stage model    the comparison partner of tests/test_rerank_stages_gpu.py, tied to the dense model and to float32 torch by
                     tests/test_rerank_hostmodel_cpu.py.  Three parts, as in the other host models:

      dispatch mirrors   words, emit_per, expand_lds / weights_lds against the 60 KB refusals, default_cap, jaccard_chunks,
                         colmax_segments, col_count_trips, strided_trips: the host arithmetic that shapes a launch, so that the
                         case lists below are BUILT from the launch regimes.
      references         on the kernels' own objects (padded [N, cap] sets with counts, CSR arrays, column lists), never dense
                         in N x N, so that N = 16 448 stays cheap.
      error budgets      every reference is Ref(value, M, kind); an element passes when
                             |got - value| <= C_KIND[kind] * 2^-24 * M        (M == 0: equality; NaN only matches NaN)
                         exact     M = 0.  Every stage but the two weights kernels: integer outputs; fp32 results whose every
                                   operation is one correctly rounded IEEE operation in one documented order (the build has no
                                   fast-math flag, an fp32 division is the v_div_scale / v_div_fixup sequence, the blend uses
                                   __fmul_rn / __fadd_rn), modelled in float32 numpy; elements an entry point must not write.
                         softmax   w = exp(d_e - mx) / sum: M = w (1 + A_e + sum_e' w_e' A_e'), A the absolute error carried
                                   into exp's argument: 2 sum_t |x_i[t] x_e[t]| + |d_e| + |mx| for the feature form (the dot
                                   product, the affine step, the subtraction), |orig| for the distance form; the third term is
                                   the same quantity through the normaliser.  An entry outside [0, N) has weight 0, M = 0.

C_KIND["softmax"] is NOT taken from the kernels: tests/test_rerank_hostmodel_cpu.py evaluates every weights case below with
plain float32 torch on the CPU (torch.softmax of float32 dot products; torch.exp(-orig) / sum), records max err / (2^-24 M), and
C_KIND = max(8, 4 x that ratio).  Measured (torch 2.10, CPU, one thread):

    kind       float32 torch ratio    C_KIND
    softmax    2.49                   9.94
    exact      0                      0

The ratio is torch's float32 sum of the normaliser in the distance form with orig in [0, 1] (300 terms of nearly equal size, whose
rounding the budget does not count); the feature cases stay at or below 1.24, the distance form up to 80 at 1.75.
"""
import collections

import numpy as np


def expand_sets(rank, kf, kh):
    """list of sorted unique int arrays: R(i, kf) united with every R(c, kh), c in R(i, kf), that lies to more than two
    thirds inside R(i, kf);  R(i, k) = { j in rank[i, :k] : i in rank[j, :k] }"""
    n = rank.shape[0]

    def recip(i, k):
        fwd = rank[i, :k]
        return fwd[(rank[fwd, :k] == i).any(axis=1)]

    full = [recip(i, kf) for i in range(n)]
    half = [recip(i, kh) for i in range(n)]
    out = []
    for i in range(n):
        members = set(full[i].tolist())
        grown = set(members)
        for c in full[i]:
            h = half[c]
            if len(members.intersection(h.tolist())) > 2. / 3 * len(h):
                grown.update(h.tolist())
        out.append(np.array(sorted(grown), dtype=np.int64))
    return out


def dense_weights(sets, x=None, orig=None):
    """fp32 [N, N]: row i holds softmax(-(2 - 2 x_i . x_e)) (features) or exp(-orig[i, e]) / sum (distances) on its set"""
    n = len(sets)
    V = np.zeros((n, n), dtype=np.float32)
    for i, s in enumerate(sets):
        if x is not None:
            d = -(2.0 - 2.0 * (x[s].astype(np.float64) @ x[i].astype(np.float64)))
            e = np.exp(d - d.max())
        else:
            e = np.exp(-orig[i, s].astype(np.float64))
        V[i, s] = (e / e.sum()).astype(np.float32)
    return V


def query_expand(V, rank, k2):
    if k2 == 1:
        return V
    acc = np.zeros_like(V)
    for l in range(k2):
        acc += V[rank[:, l]]
    return acc / np.float32(k2)


def jaccard_rows(V, rows):
    """fp32 [len(rows), N]: 1 - m / (2 - m), m[j] = sum_c min(V[i, c], V[j, c]) over the non-zero columns of row i"""
    out = np.empty((len(rows), V.shape[0]), dtype=np.float32)
    for t, i in enumerate(rows):
        nz = np.nonzero(V[i])[0]
        m = np.minimum(V[i, nz][None, :], V[:, nz]).astype(np.float64).sum(axis=1)
        out[t] = (1.0 - m / (2.0 - m)).astype(np.float32)
    return out


# ==== the stage model ==============================================================================================================
U24 = 2.0 ** -24
FILL = -7777.0                      # guard / untouched-output fill value of the device tests (float and int32 buffers alike)
TINY_M = 2.0 ** -102                # 2^-24 * TINY_M = 2^-126, the smallest normal float32
C_KIND = {"softmax": 9.94, "exact": 0.0}
F32 = np.float32

Ref = collections.namedtuple("Ref", "value M kind")
Worst = collections.namedtuple("Worst", "ok index err budget ratio")


def exact(v):
    v = np.asarray(v)
    return Ref(v, np.zeros(v.shape), "exact")


def compare(got, ref):
    """per-element check of `got` against ref = Ref(value, M, kind); every element takes part.  M == 0 asks for equality; a NaN
    or infinite reference passes only with the same NaN / infinity; a non-finite `got` anywhere else fails"""
    g = np.asarray(got, dtype=np.float64).reshape(-1)
    v, M = np.asarray(ref.value, dtype=np.float64).reshape(-1), np.asarray(ref.M, dtype=np.float64).reshape(-1)
    assert g.size == v.size, ("shape", np.shape(got), np.shape(ref.value))
    if g.size == 0:
        return Worst(True, (), 0.0, 0.0, 0.0)
    with np.errstate(invalid="ignore"):
        same = (g == v) | (np.isnan(g) & np.isnan(v))
        err = np.where(same, 0.0, np.abs(g - v))
    err = np.where(np.isfinite(err), err, np.inf)
    bud = C_KIND[ref.kind] * U24 * np.where(M > 0, M + TINY_M, 0.0)
    with np.errstate(invalid="ignore"):
        over = np.where(err <= bud, -1.0, np.where(np.isfinite(err), err - bud, np.inf))
    i = int(np.argmax(over))
    ratio = np.where((err > 0) & (M > 0), err / (U24 * (M + TINY_M)), np.where(err > 0, np.inf, 0.0))
    idx = tuple(int(k) for k in np.unravel_index(i, np.shape(ref.value))) if np.ndim(ref.value) else ()
    return Worst(bool((err <= bud).all()), idx, float(err[i]), float(bud[i]), float(ratio.max()))


def check(got, ref, what):
    w = compare(got, ref)
    assert w.ok, "%s: worst element %s err %.3e > budget %.3e (%s, max err/(2^-24 M) = %.2f)" % (
        what, w.index, w.err, w.budget, ref.kind, w.ratio)
    return w.ratio


def same_bits(got, want):
    """float32 arrays equal bit for bit, a NaN matching any NaN"""
    got, want = np.ascontiguousarray(got, dtype=F32), np.ascontiguousarray(want, dtype=F32)
    if got.shape != want.shape:
        return False
    nan = np.isnan(got) & np.isnan(want)
    return bool(((got.view(np.int32) == want.view(np.int32)) | nan).all())


# ---- dispatch mirrors ---------------------------------------------------------------------------------------------------------------
MAX_N = 65536                       # kMaxN
JACCARD_MAX_CHUNK = 16384           # kJaccardMaxChunk
LDS_LIMIT = 60 * 1024               # the refusals of rg_rerank_expand / rg_rerank_weights_*
MAX_KF = 1024
THREADS = 256
COL_COUNT_GRID = 4096


def cdiv(a, b):
    return -(-a // b)


def words(N):
    """32-column words of one LDS bitmap"""
    return (N + 31) // 32


def emit_per(N):
    """emit_bitmap: words every thread counts and prefixes"""
    return cdiv(words(N), THREADS)


def emit_last_thread_words(N):
    """words the last thread of emit_bitmap that owns any has"""
    per = emit_per(N)
    return words(N) - (cdiv(words(N), per) - 1) * per


def strided_trips(n):
    """most trips a thread makes through a `for (t = tid; t < n; t += 256)` loop"""
    return cdiv(n, THREADS)


def expand_lds(N, kf, kh):
    """bytes of dynamic LDS rg_rerank_expand asks for: three bitmaps, four kf-arrays, the kf * kh member table"""
    return 4 * (3 * words(N) + 4 * kf + kf * kh)


def weights_lds(D, cap):
    """bytes of dynamic LDS of the weights kernels (D = 0: the distance form)"""
    return 4 * (cap + D)


def default_cap(N, kf, kh):
    """rg_hip.ops.rerank_expand: the worst case kf * (kh + 1), capped at N"""
    return min(N, kf * (kh + 1))


def largest_expand(N, R):
    """(kf, kh) with the largest kf * kh that rg_rerank_expand admits at N: 1 <= kh <= kf <= min(R, 1024) inside LDS_LIMIT"""
    best = (1, 1)
    for kf in range(1, min(R, MAX_KF) + 1):
        kh = min(kf, (LDS_LIMIT // 4 - 3 * words(N) - 4 * kf) // kf)
        if kh >= 1 and kf * kh > best[0] * best[1]:
            best = (kf, kh)
    return best


def jaccard_chunks(N, col_off, chunk):
    """rg_rerank_jaccard: (W, parts) = columns per workgroup and workgroups per row"""
    width = N - col_off
    W = chunk
    if W == 0:
        parts = cdiv(width, JACCARD_MAX_CHUNK)
        W = cdiv(cdiv(width, parts), 64) * 64
    W = min(W, width)
    return W, cdiv(width, W)


def colmax_segments(N):
    """rg_rerank_orig_dist: (row segments of the column maximum, rows per segment)"""
    segs = cdiv(N, 512)
    return segs, cdiv(N, segs)


def col_count_trips(nnz):
    """most trips a thread of rerank_col_count_kernel makes"""
    return cdiv(nnz, min(cdiv(nnz, 256), COL_COUNT_GRID) * 256)


# ---- rg_rerank_expand ---------------------------------------------------------------------------------------------------------------
def _valid(v, N):
    return (v >= 0) & (v < N)


def _recip_lists(rank, N, k, k_back=None):
    """per row c the list (in rank order, one entry per position) of the valid m = rank[c, q], q < k, with c in rank[m, :k_back]"""
    k_back = k if k_back is None else k_back
    out = []
    for c in range(N):
        fwd = rank[c, :k]
        ok = _valid(fwd, N)
        keep = np.zeros(k, dtype=bool)
        keep[ok] = (rank[fwd[ok], :k_back] == c).any(axis=1)
        out.append(fwd[keep])
    return out


def expand(rank, kf, kh, cap=None, variant=None):
    """(sets, counts): per row the sorted unique list of the expanded k-reciprocal set, cut to its first `cap` members, and the
    UNtruncated count.  Indices outside [0, N) never match.  variant: the defects 'ge' (>= in the two-thirds rule), 'kf_half'
    (the half sets' reciprocity looked up in kf columns), 'keep_last' (truncation keeps the last cap), 'clip_counts'"""
    rank = np.asarray(rank, dtype=np.int64)
    N = rank.shape[0]
    cap = default_cap(N, kf, kh) if cap is None else cap
    full = _recip_lists(rank, N, kf)
    half = _recip_lists(rank, N, kh, kf if variant == "kf_half" else None)
    sets, counts = [], np.zeros(N, dtype=np.int64)
    for i in range(N):
        members = set(full[i].tolist())
        grown = set(members)
        for c in full[i].tolist():                       # one candidate per reciprocal POSITION of rank[i, :kf]
            h = half[c]
            inter = sum(1 for m in h.tolist() if m in members)
            if (inter >= 2.0 / 3.0 * len(h) and len(h)) if variant == "ge" else (inter > 2.0 / 3.0 * len(h)):
                grown.update(h.tolist())
        s = np.array(sorted(grown), dtype=np.int64)
        counts[i] = min(len(s), cap) if variant == "clip_counts" else len(s)
        sets.append(s[len(s) - cap:] if variant == "keep_last" and len(s) > cap else s[:cap])
    return sets, counts


def pad_sets(sets, cap, fill=int(FILL)):
    """[N, cap] int32 with the lists in front and `fill` behind, as the device buffer looks after the call"""
    out = np.full((len(sets), cap), fill, dtype=np.int32)
    for i, s in enumerate(sets):
        out[i, :len(s)] = s
    return out


# ---- rg_rerank_weights_feat / rg_rerank_weights_dist ----------------------------------------------------------------------------------
def _softmax_rows(N, sets, counts, cap, arg, use_max, variant):
    """arg(i, members) -> (d, A) in fp64 for the valid members of row i"""
    value = np.full((N, cap), FILL, dtype=np.float64)
    M = np.zeros((N, cap), dtype=np.float64)
    for i in range(N):
        n = int(min(counts[i], cap))
        if n == 0:
            continue
        s = np.asarray(sets[i, :n], dtype=np.int64)
        ok = _valid(s, N)
        d, A = np.full(n, 0.0 if variant == "invalid_exp0" else -np.inf), np.zeros(n)
        if ok.any():
            d[ok], A[ok] = arg(i, s[ok])
        if variant == "no_max":                          # float32 arithmetic without the subtraction: exp overflows
            with np.errstate(over="ignore", invalid="ignore"):
                e = np.exp(d.astype(F32))
                value[i, :n] = e / e.sum(dtype=F32)
            continue
        mx = d.max() if use_max else 0.0
        with np.errstate(invalid="ignore"):
            e = np.exp(d - mx)                           # all entries invalid: exp(-inf + inf) or 0 / 0 = NaN, as the kernels
            w = e / e.sum()
        value[i, :n] = w
        fin = np.isfinite(d)
        Ae = np.where(fin, A + np.abs(np.where(fin, d, 0.0)) + (abs(mx) if np.isfinite(mx) else 0.0), 0.0)
        with np.errstate(invalid="ignore"):
            M[i, :n] = np.where(w > 0, w * (1.0 + Ae + np.nansum(w * Ae)), 0.0)
    return Ref(value, M, "softmax")


def weights_feat(x, sets, counts, cap=None, variant=None):
    """w[i][e] = softmax over the first min(counts[i], cap) entries of row i of d_e = -(2 - 2 x_i . x_e); an entry outside
    [0, N) has weight exactly 0; a set of ONLY such entries is NaN throughout (exp(-inf - -inf)); w[i][min(count, cap):] keeps
    FILL.  variant: the defects 'invalid_exp0' and 'no_max'"""
    x64 = np.asarray(x, dtype=np.float64)
    N = x64.shape[0]
    cap = sets.shape[1] if cap is None else cap

    def arg(i, s):
        t = x64[s] * x64[i][None, :]
        return -(2.0 - 2.0 * t.sum(axis=1)), 2.0 * np.abs(t).sum(axis=1)
    return _softmax_rows(N, sets, counts, cap, arg, True, variant)


def weights_dist(orig, sets, counts, cap=None, variant=None):
    """w[i][e] = exp(-orig[i][e]) / sum, NO maximum subtracted: the domain is exp(-orig) normal in float32"""
    o64 = np.asarray(orig, dtype=np.float64)
    N = o64.shape[0]
    cap = sets.shape[1] if cap is None else cap

    def arg(i, s):
        return -o64[i, s], np.zeros(len(s))
    return _softmax_rows(N, sets, counts, cap, arg, False, variant)


# ---- rg_rerank_qe_count / rg_rerank_qe_fill -------------------------------------------------------------------------------------------
def query_expand_csr(sets, w, counts, rank, k2, variant=None):
    """float32 model: (rowcnt [N], rowptr [N + 1], cols, vals).  Row i = the union of the valid columns of the valid rows among
    rank[i, :k2] (rank None: row i itself), ascending; every value adds its terms in rank order in float32 from 0.0f and is
    divided once by float32(k2) — rows that were skipped still count in k2.  variant: the defects 'div_valid' and 'row_order'"""
    sets, w, counts = np.asarray(sets), np.asarray(w, dtype=F32), np.asarray(counts)
    N, cap = sets.shape
    rowcnt = np.zeros(N, dtype=np.int64)
    cols, vals = [], []
    for i in range(N):
        src = [i] if rank is None else [int(r) for r in rank[i, :k2]]
        src = [r for r in src if 0 <= r < N]
        if variant == "row_order":
            src = sorted(src)
        parts = []
        for r in src:
            n = int(min(counts[r], cap))
            s = sets[r, :n].astype(np.int64)
            ok = _valid(s, N)
            parts.append((s[ok], w[r, :n][ok]))
        u = np.unique(np.concatenate([p[0] for p in parts])) if parts else np.zeros(0, dtype=np.int64)
        acc = np.zeros(len(u), dtype=F32)
        for s, ww in parts:
            acc[np.searchsorted(u, s)] += ww             # the columns of one set are distinct: one float32 add per element
        div = F32(len(src) if variant == "div_valid" else k2)
        rowcnt[i] = len(u)
        cols.append(u)
        vals.append(acc / div)
    rowptr = np.concatenate([[0], np.cumsum(rowcnt)])
    return (rowcnt, rowptr, np.concatenate(cols).astype(np.int64) if cols else np.zeros(0, np.int64),
            np.concatenate(vals).astype(F32) if vals else np.zeros(0, F32))


# ---- rg_rerank_columns ----------------------------------------------------------------------------------------------------------------
def canon_columns(colptr, crow, cval):
    """(crow, cval) with every column's entries sorted by (row, value bits): the column as a SET of pairs"""
    colptr = np.asarray(colptr, dtype=np.int64)
    col = np.repeat(np.arange(len(colptr) - 1), np.diff(colptr))
    cval = np.ascontiguousarray(cval, dtype=F32)
    order = np.lexsort((cval.view(np.int32), np.asarray(crow), col))
    return np.asarray(crow)[order], cval[order]


def columns(rowptr, cols, vals, N):
    """(colptr [N + 1], crow, cval): the column lists of a CSR matrix, every column in canonical (row-ascending) order"""
    rowptr, cols = np.asarray(rowptr, dtype=np.int64), np.asarray(cols, dtype=np.int64)
    row = np.repeat(np.arange(N), np.diff(rowptr))
    colptr = np.concatenate([[0], np.cumsum(np.bincount(cols, minlength=N))])
    vals = np.ascontiguousarray(vals, dtype=F32)
    order = np.lexsort((vals.view(np.int32), row, cols))
    return colptr, row[order], vals[order]


# ---- rg_rerank_jaccard ----------------------------------------------------------------------------------------------------------------
def jaccard_rows_csr(rowptr, cols, vals, N, rows, col_off=0, orig=None, lambda_value=0.0, clamp=True, variant=None):
    """float32 model, [rows, N - col_off]: m[j] accumulated from 0.0f over the columns of row i in ascending order, one
    fminf(V[i][c], V[j][c]) per column; 1 - m / (2 - m); with orig fl(fl(v (1 - lambda)) + fl(orig[i][j] lambda)), 1 - lambda
    rounded from the double difference; then the clamp.  variant: the defects 'desc', 'orig_shift', 'clamp_first'"""
    rowptr = np.asarray(rowptr, dtype=np.int64)
    vals = np.asarray(vals, dtype=F32)
    colptr, crow, cval = columns(rowptr, cols, vals, N)
    lam = F32(lambda_value)
    oml = F32(1.0 - float(lam))
    out = np.empty((rows, N - col_off), dtype=F32)
    for i in range(rows):
        acc = np.zeros(N, dtype=F32)
        ps = range(rowptr[i], rowptr[i + 1])
        for p in (reversed(ps) if variant == "desc" else ps):
            c = int(cols[p])
            b, e = colptr[c], colptr[c + 1]
            acc[crow[b:e]] += np.minimum(vals[p], cval[b:e])          # the rows of one column are distinct
        m = acc[col_off:]
        v = F32(1.0) - m / (F32(2.0) - m)
        if clamp and variant == "clamp_first":
            v = np.where(v < 0, F32(0.0), v)
        if orig is not None:
            o = np.asarray(orig, dtype=F32)[i, :N - col_off] if variant == "orig_shift" else np.asarray(orig, dtype=F32)[i, col_off:]
            v = (v * oml).astype(F32) + (o * lam).astype(F32)
        if clamp and variant != "clamp_first":
            v = np.where(v < 0, F32(0.0), v)
        out[i] = v
    return out


# ---- rg_rerank_orig_dist --------------------------------------------------------------------------------------------------------------
def orig_dist(q_g, q_q, g_g, variant=None):
    """float32 model: orig[c][r] = fl(fl(A[r][c]^2) / colmax[c]), colmax[c] the exact maximum of the float32 squares of column c
    of A = [[q_q, q_g], [q_g^T, g_g]]; an all-zero column gives 0 / 0 = NaN along its row of orig, as the reference's numpy
    expression does.  variant: the defects 'rowmax', 'no_transpose', 'lower_left' (the lower-left block read untransposed)"""
    q_g, q_q, g_g = (np.asarray(t, dtype=F32) for t in (q_g, q_q, g_g))
    Q, G = q_g.shape
    ll = q_g.T
    if variant == "lower_left":
        ll = q_g.reshape(-1)[(np.arange(G)[:, None] * G + np.arange(Q)[None, :]) % (Q * G)]
    A = np.block([[q_q, q_g], [ll, g_g]]).astype(F32)
    sq = A * A
    with np.errstate(invalid="ignore", divide="ignore"):
        if variant == "rowmax":
            return np.ascontiguousarray((sq / sq.max(axis=1)[:, None]).T)
        r = sq / sq.max(axis=0)[None, :]
    return np.ascontiguousarray(r if variant == "no_transpose" else r.T)


# ==== case lists, built from the launch regimes =======================================================================================
def rng(seed):
    return np.random.RandomState(seed)


def make_rank(N, R, seed, swap_first=False, invalid=False):
    """hand-built int32 ranking [N, R] without repeated entries in a row.  N <= 512: the stable order of a random SYMMETRIC
    integer distance with the row itself first.  Larger N: the row itself, then R - 1 distinct pseudo-random offsets from
    [-R, R] around it on the ring.  swap_first: every third row has its first two entries exchanged (the row is not its own
    nearest).  invalid: rows with i % 5 == 1 carry -1 at position 2, rows with i % 5 == 3 carry N at position 1"""
    g = rng(seed)
    if N <= 512:
        d = g.randint(0, 1 << 20, size=(N, N))
        d = d + d.T
        d[np.arange(N), np.arange(N)] = -1
        full = np.argsort(d, axis=1, kind="stable")
        rank = np.full((N, R), -1, dtype=np.int64)           # R > N: the row is padded with -1
        rank[:, :min(R, N)] = full[:, :R]
    else:
        assert N > 2 * R + 1
        offs = np.concatenate([np.arange(1, R + 1), -np.arange(1, R + 1)])
        rank = np.empty((N, R), dtype=np.int64)
        rank[:, 0] = np.arange(N)
        for i in range(N):
            rank[i, 1:] = (i + g.permutation(offs)[:R - 1]) % N
    if swap_first and R > 1:
        rank[::3, [0, 1]] = rank[::3, [1, 0]]
    if invalid and R > 2:
        rank[1::5, 2] = -1
        rank[3::5, 1] = N
    return rank.astype(np.int32)


def two_thirds_graph():
    """(rank [24, 8], kf, kh, row, wanted set): row 0 has R(0, 8) = {0 .. 5}; its candidates' half sets (kh = 6) are
        R(1, 6) = {1, 4, 10}              2 of 3 inside: excluded (10 stays out)
        R(2, 6) = {2, 3, 4, 5, 11, 12}    4 of 6 inside: excluded (11, 12 stay out)
        R(3, 6) = {3, 2, 5, 13}           3 of 4 inside: included (13 comes in)
    and R(0, 6) = {0}, R(4, 6) = {4, 1, 2}, R(5, 6) = {5, 2, 3} bring nothing new.  Rows 16 .. 23 list only each other and fill
    the other rows without ever listing them back"""
    N, R = 24, 8
    half = {0: [], 1: [4, 10], 2: [3, 4, 5, 11, 12], 3: [2, 5, 13], 4: [1, 2], 5: [2, 3], 10: [1], 11: [2], 12: [2], 13: [3]}
    rank = np.zeros((N, R), dtype=np.int32)
    for i in range(16):
        row = [i] + half.get(i, [])
        sinks = iter(range(16, 24))
        while len(row) < 6:                              # the kh columns: the row, its half set, rows that never list it back
            row.append(next(sinks))
        rank[i] = row + ([0] if 1 <= i <= 5 else [next(sinks)]) + [next(sinks)]      # rows 1 .. 5 list row 0 beyond kh only
    rank[0] = [0, 1, 2, 3, 4, 5, 6, 7]                   # rows 6 and 7 do not list row 0
    for s in range(16, 24):
        rank[s] = [s] + [t for t in range(16, 24) if t != s]
    return rank, 8, 6, 0, [0, 1, 2, 3, 4, 5, 13]


EXPAND_N = [1, 31, 32, 33, 257, 8200]
EXPAND_K = [(1, 1), (8, 4), (40, 7), (300, 2)]
EXPAND_WIDE_N = 320


def expand_cases():
    """[(tag, N, R, kf, kh, rank options, cap mode)]; cap mode 'default', 'below' (largest count - 1) or 'one'"""
    big = largest_expand(EXPAND_WIDE_N, EXPAND_WIDE_N)
    out = [("n1", 1, 1, 1, 1, {}, "default"),
           ("n31", 31, 8, 8, 4, dict(invalid=True), "default"),                        # R == kf
           ("n32", 32, 12, 8, 4, dict(swap_first=True), "default"),                    # R > kf
           ("n33", 33, 3, 1, 1, {}, "default"),
           ("n33_k8", 33, 9, 8, 4, dict(swap_first=True, invalid=True), "default"),
           ("n33_below", 33, 9, 8, 4, dict(swap_first=True, invalid=True), "below"),
           ("n33_one", 33, 9, 8, 4, dict(swap_first=True, invalid=True), "one"),
           ("n257", 257, 48, 40, 7, dict(invalid=True), "default"),                    # kf * kh > 256
           ("n257_below", 257, 48, 40, 7, dict(invalid=True), "below"),
           ("n8200", 8200, 10, 8, 4, dict(invalid=True), "default"),                   # emit_per == 2
           ("n320_kf300", EXPAND_WIDE_N, 320, 300, 2, {}, "default"),                  # kf > 256
           ("n320_largest", EXPAND_WIDE_N, 320, big[0], big[1], {}, "default")]
    return out


def expand_input(case):
    tag, N, R, kf, kh, opts, capmode = case
    rank = make_rank(N, R, seed=N * 7 + kf, **opts)
    if capmode == "default":
        cap = default_cap(N, kf, kh)
    elif capmode == "one":
        cap = 1
    else:
        cap = int(expand(rank, kf, kh)[1].max()) - 1
    return rank, cap


WEIGHTS_N = 320
WEIGHTS_D = [1, 3, 4, 63, 64, 68, 257, 260, 516]
WEIGHTS_SIZES = [0, 1, 2, 5, 256, 257, 300]
WEIGHTS_CAP = 300
FEAT_FAMILIES = ("unit", "scaled8")
DIST_FAMILIES = ("unit_range", "to80")


def weights_sets(seed=0, cap=WEIGHTS_CAP, N=WEIGHTS_N):
    """(sets [N, cap] int32, counts [N] int32): row i has WEIGHTS_SIZES[i % 7] members, row i first where there is one, the rest
    a sorted random choice; the rows of 300 report a count of 307 (> cap); rows 10 and 11 (sizes 5 and 256) carry -1 and N in
    the middle; rows 16 and 17 (sizes 2 and 5) hold only invalid entries.  The tail of every row is -1 (never read)"""
    g = rng(seed)
    sets = np.full((N, cap), -1, dtype=np.int32)
    counts = np.zeros(N, dtype=np.int32)
    for i in range(N):
        n = min(WEIGHTS_SIZES[i % len(WEIGHTS_SIZES)], cap)
        if n:
            others = np.setdiff1d(np.arange(N), [i])
            sets[i, :n] = np.sort(np.concatenate([[i], g.choice(others, n - 1, replace=False)]))
        counts[i] = n + 7 if n == cap else n
    for i in (10, 11):
        sets[i, counts[i] // 2] = -1
        sets[i, counts[i] // 2 + 1] = N
    for i in (16, 17):
        sets[i, :counts[i]] = [-1, N, -5, N + 3, 1 << 30][:counts[i]]
    return sets, counts


def feat_input(D, fam, seed=0, N=WEIGHTS_N):
    """float32 [N, D]: noisy copies of 8 unit centres, normalised ('unit'); the same times 8 ('scaled8': x_i . x_i = 64, d up to
    +126, where only the subtraction of the maximum keeps expf finite)"""
    g = rng(1000 * seed + D)
    c = g.randn(8, D)
    x = c[np.arange(N) % 8] + 0.3 * g.randn(N, D) / np.sqrt(D)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    return np.ascontiguousarray(x * (8.0 if fam == "scaled8" else 1.0), dtype=F32)


def dist_input(fam, seed=0, N=WEIGHTS_N):
    """float32 [N, N]: uniform in [0, 1] with a zero diagonal, as rg_rerank_orig_dist produces it ('unit_range'); uniform in
    [0, 80] ('to80': exp(-80) = 1.8e-35 is still a normal float32)"""
    g = rng(77 + seed)
    o = g.rand(N, N) * (80.0 if fam == "to80" else 1.0)
    o[np.arange(N), np.arange(N)] = 0.0
    return np.ascontiguousarray(o, dtype=F32)


def weights_refusal():
    """(D, cap) just past the LDS limit, and the largest admitted cap at that D"""
    D = WEIGHTS_D[-1]
    cap = LDS_LIMIT // 4 - D
    return D, cap + 1, cap


QE_CASES = [("n33_null", 33, None, 1, 0), ("n33_k1", 33, 5, 1, 1), ("n33_k6", 33, 6, 6, 2), ("n257_k64", 257, 64, 64, 3),
            ("n257_k6", 257, 9, 6, 4), ("n8200_k6", 8200, 7, 6, 5), ("n8200_null", 8200, None, 1, 6)]
QE_CAP = 12


def qe_input(case):
    """(sets, counts, w, rank): sorted random sets of 0 .. 14 reported members in cap = 12 (a count above cap, empty rows, an
    entry N at the end of some sets), positive float32 weights over three decades, and a ranking [N, R] whose rows with
    i % 4 == 1 carry an invalid entry (-1 or N) and whose rows with i % 4 == 2 carry the same row twice among the first k2"""
    tag, N, R, k2, seed = case
    g = rng(100 + seed)
    cap = QE_CAP
    sets = np.full((N, cap), int(FILL), dtype=np.int32)
    counts = g.randint(0, cap + 3, size=N).astype(np.int32)
    counts[0] = cap
    for i in range(N):
        n = min(int(counts[i]), cap, N)
        lo = max(0, min(i - 20, N - 40))
        sets[i, :n] = lo + np.sort(g.choice(min(N, 40), n, replace=False))
        if n and i % 6 == 5:
            sets[i, n - 1] = N
    w = (10.0 ** (g.rand(N, cap) * 3.0 - 3.0)).astype(F32)
    rank = None
    if R is not None:
        rank = np.empty((N, R), dtype=np.int32)
        win = min(N, max(60, R + 8))
        for i in range(N):
            rank[i] = (i + g.choice(win, R, replace=False) - win // 2) % N
        rank[:, 0] = np.arange(N)
        rank[1::4, k2 - 1] = np.where(np.arange(len(rank[1::4])) % 2 == 0, -1, N)
        if k2 > 1:
            rank[2::4, k2 - 1] = rank[2::4, 0]
    return sets, counts, w, rank


COLUMNS_BIG = (61681, 17)                               # 61681 * 17 = 256 * 4096 + 1: the smallest nnz of the second trip


def columns_input(name):
    """(rowptr, cols, vals, N) of 'n1', 'n5' (rows 1 and 4 and columns 2 and 4 empty), 'n257' (a row of 200 entries, every
    seventh row empty, the columns divisible by 5 empty) and 'big' (COLUMNS_BIG equal rows)"""
    if name == "n1":
        rows = [[0]]
    elif name == "n5":
        rows = [[0, 3], [], [3], [0, 1, 3], []]
    elif name == "n257":
        g = rng(5)
        allowed = np.array([c for c in range(257) if c % 5])
        rows = [[] if i % 7 == 0 else np.sort(g.choice(allowed, 200 if i == 3 else g.randint(1, 70), replace=False)).tolist()
                for i in range(257)]
    else:
        N, per = COLUMNS_BIG
        cols = (np.arange(N)[:, None] + np.arange(per)[None, :] * 3631) % N
        cols = np.sort(cols, axis=1)
        vals = ((np.arange(N * per) % 8191 + 1) / 8192.0).astype(F32)
        return np.arange(N + 1, dtype=np.int64) * per, cols.reshape(-1).astype(np.int64), vals, N
    N = len(rows)
    rowptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    cols = np.array([c for r in rows for c in r], dtype=np.int64)
    vals = ((np.arange(len(cols)) * 37 % 1021 + 1) / 1024.0).astype(F32)
    return rowptr, cols, vals, N


JACCARD_N, JACCARD_Q = 150, 37
JACCARD_BIG_N, JACCARD_BIG_ROWS = JACCARD_MAX_CHUNK + 64, 4
JACCARD_LAMBDA = 0.3


def jaccard_blocks(N=JACCARD_N, Q=JACCARD_Q):
    return [(N, 0), (Q, Q), (1, N - 1)]


def jaccard_chunk_values(width):
    return [0, 1, 63, 64, width, width + 5]


def jaccard_input():
    """CSR (rowptr, cols, vals, N) of the query-expansion model (k2 = 3) on hand-built sets of N = 150 rows: rows 0 .. 7 are
    four pairs of identical rows with four weights of 0.25 (m exactly 1 within a pair and on their diagonal), rows 8 .. 11 hold
    weights 0.5, 0.5, 0.25 (m = 1.25: a negative distance that only the clamp removes), rows 140 .. 149 use columns no other row
    has, the rest are random; the first 12 rows expand over themselves only"""
    N, cap = JACCARD_N, 8
    g = rng(11)
    sets = np.full((N, cap), int(FILL), dtype=np.int32)
    counts = np.zeros(N, dtype=np.int32)
    w = np.zeros((N, cap), dtype=F32)
    rank = np.empty((N, 3), dtype=np.int32)
    for i in range(N):
        if i < 8:
            s, ww = [100 + 4 * (i // 2) + t for t in range(4)], [0.25] * 4
        elif i < 12:
            s, ww = [120, 121, 122], [0.5, 0.5, 0.25]
        elif i >= 140:
            s, ww = [130 + (i - 140)], [1.0]
        else:
            n = g.randint(1, cap + 1)
            s = np.sort(g.choice(100, n, replace=False)).tolist()
            ww = g.rand(n) + 0.05
            ww = (ww / ww.sum()).tolist()
        counts[i] = len(s)
        sets[i, :len(s)] = s
        w[i, :len(s)] = ww
        rank[i] = [i, i, i] if (i < 12 or i >= 140) else [i, 12 + (i * 7) % 128, 12 + (i * 13 + 5) % 128]
    _, rowptr, cols, vals = query_expand_csr(sets, w, counts, rank, 3)
    return rowptr, cols, vals, N


def jaccard_big_input():
    """CSR at N = 16 448: row j holds the columns {0, j, (7 j + 3) % N}, so every row meets every other in column 0 and the
    first four rows reach both chunks of the automatic split and the 64 columns past 16 384"""
    N = JACCARD_BIG_N
    j = np.arange(N)
    cols = np.stack([np.zeros(N, dtype=np.int64), j, (7 * j + 3) % N], axis=1)
    vals = np.stack([(j % 509 + 1) / 1024.0, (j % 251 + 1) / 512.0, (j % 127 + 1) / 256.0], axis=1).astype(F32)
    rows_c, rows_v, lens = [], [], []
    for r in range(N):
        u, idx = np.unique(cols[r], return_index=True)
        rows_c.append(u)
        rows_v.append(vals[r][idx])
        lens.append(len(u))
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64), np.concatenate(rows_c), np.concatenate(rows_v).astype(F32), N


def jaccard_orig(N, rows, seed=3):
    """float32 [rows, N] in [0, 1] whose value tells its (i, j)"""
    g = rng(seed)
    return np.ascontiguousarray(g.rand(rows, N), dtype=F32)


ORIG_QG = [(1, 1), (1, 40), (31, 33), (32, 32), (100, 500)]


def orig_input(Q, G, zero_col=None):
    """asymmetric float32 blocks whose values tell block, row and column, signs alternating; zero_col: that column of A (a
    gallery column) is zero in q_g and g_g"""
    def blk(r, c, base):
        v = base + np.arange(r)[:, None] / 64.0 + np.arange(c)[None, :] / 65536.0
        return (v * np.where((np.arange(r)[:, None] + np.arange(c)[None, :]) % 2 == 0, 1.0, -1.0)).astype(F32)
    q_g, q_q, g_g = blk(Q, G, 1.0), blk(Q, Q, 2.0), blk(G, G, 3.0)
    if zero_col is not None:
        q_g[:, zero_col - Q] = 0.0
        g_g[:, zero_col - Q] = 0.0
    return q_g, q_q, g_g
