"""GPU: the eight entry points of csrc/rerank.hip one at a time, against the stage model of tests/rerank_hostmodel.py, at cases
built from the launch arithmetic (asserted to reach every regime by tests/test_rerank_hostmodel_cpu.py): the strided loops of
the set kernels on their second and later trips, emit_bitmap with two words per thread, truncated sets, rank entries outside
[0, N), the two-thirds rule at equality; both dot-product paths of the weights at every staging regime, sets of 0 .. 300
members, invalid members, rows that need the maximum subtracted, the LDS refusal; the query expansion with and without a ranking
up to k2 = 64; column lists with empty rows and columns and on the second trip of the counting loop; Jaccard row blocks at every
chunk width including W == 1, the automatic two-way split and exactly 64 KB of accumulators; the normalised distances at ragged
tiles and two column-maximum segments.

Inputs are hand-built rankings and lists, so no ranking tie can matter.  The C ABI is called on test-owned buffers between two
rows of guard values; the elements an entry point must not write keep the fill value.  Every stage is compared bit for bit with
its float32 model except the two weights kernels, which are checked per element against fp64 with the `softmax` budget and
print `RATIO <entry point> <output> <family> <max err / (2^-24 M)>` (pytest -s shows them).  Each entry point also runs once
through its rg_hip.ops wrapper.

_Out is a copy of the one in tests/test_body_elementwise_gpu.py."""
import numpy as np
import pytest
import torch

from tests import rerank_hostmodel as H

pytestmark = pytest.mark.gpu

GUARD = 64
F32 = np.float32


def _ops():
    from rg_hip import ops
    return ops


def _lib():
    from rg_hip.lib import lib
    return lib


def _st():
    return _ops()._stream()


class _Out(object):
    """an output tensor between two rows of 64 guard elements; unwritten elements keep the fill value"""

    def __init__(self, shape, dev, dtype=torch.float32, fill=H.FILL):
        n = 1
        for d in shape:
            n *= d
        self.n, self.fill = n, fill if dtype == torch.float32 else int(fill)
        self.buf = torch.full((n + 2 * GUARD,), self.fill, dtype=dtype, device=dev)
        self.t = self.buf[GUARD:GUARD + n].view(shape)
        assert self.buf.data_ptr() % 16 == 0

    @property
    def ptr(self):
        return self.t.data_ptr()

    def np(self, what):
        """the output as numpy, after checking the guards"""
        b = self.buf.cpu()
        assert bool((b[:GUARD] == self.fill).all()) and bool((b[GUARD + self.n:] == self.fill).all()), "%s: guard elements written" % what
        return b[GUARD:GUARD + self.n].view(self.t.shape).numpy()


def _int(shape, dev):
    return _Out(shape, dev, dtype=torch.int32)


def _dev(dev, a, dtype=None):
    if a is None:
        return None
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(dev)


def _p(t):
    return None if t is None else (t.ptr if isinstance(t, _Out) else t.data_ptr())


# ---- rg_rerank_expand ---------------------------------------------------------------------------------------------------------------
def _expand(dev, rank, kf, kh, cap, tag):
    N, R = rank.shape
    rd = _dev(dev, rank)
    sets, counts = _int((N, cap), dev), _int((N,), dev)
    _lib().rg_rerank_expand(rd.data_ptr(), N, R, kf, kh, sets.ptr, counts.ptr, cap, _st())
    want_sets, want_counts = H.expand(rank, kf, kh, cap)
    got_counts = counts.np("rg_rerank_expand counts | " + tag)
    assert np.array_equal(got_counts, want_counts), "rg_rerank_expand counts | %s: rows %s" % (tag, np.nonzero(got_counts != want_counts)[0][:8])
    got = sets.np("rg_rerank_expand sets | " + tag)
    want = H.pad_sets(want_sets, cap)                     # sets[i][min(count, cap):] keeps the fill value
    assert np.array_equal(got, want), "rg_rerank_expand sets | %s: rows %s" % (tag, np.nonzero((got != want).any(axis=1))[0][:8])
    return rd, want_sets, want_counts


def test_expand(dev):
    for case in H.expand_cases():
        tag, N, R, kf, kh, opts, capmode = case
        rank, cap = H.expand_input(case)
        _expand(dev, rank, kf, kh, cap, "%s N %d R %d kf %d kh %d cap %d" % (tag, N, R, kf, kh, cap))
    rank, kf, kh, row, want = H.two_thirds_graph()
    _, sets, _ = _expand(dev, rank, kf, kh, H.default_cap(len(rank), kf, kh), "two-thirds graph")
    assert sets[row].tolist() == want
    # the wrapper: default cap and a given one
    case = H.expand_cases()[4]
    rank, _ = H.expand_input(case)
    rd = _dev(dev, rank)
    for cap in (None, 3):
        s, c = _ops().rerank_expand(rd, case[3], case[4], cap=cap)
        ws, wc = H.expand(rank, case[3], case[4], cap)
        assert tuple(s.shape) == (case[1], H.default_cap(case[1], case[3], case[4]) if cap is None else cap)
        assert np.array_equal(c.cpu().numpy(), wc)
        s = s.cpu().numpy()
        assert all(np.array_equal(s[i, :len(w)], w) for i, w in enumerate(ws))


# ---- rg_rerank_weights_feat / rg_rerank_weights_dist ----------------------------------------------------------------------------------
def _weights(dev, entry, src, sets, counts, cap, sd, cd, fam, tag):
    N = src.shape[0]
    xd = _dev(dev, src)
    w = _Out((N, cap), dev)
    if entry == "rg_rerank_weights_feat":
        _lib().rg_rerank_weights_feat(xd.data_ptr(), N, src.shape[1], sd.data_ptr(), cd.data_ptr(), cap, w.ptr, _st())
        ref = H.weights_feat(src, sets, counts, cap)
    else:
        _lib().rg_rerank_weights_dist(xd.data_ptr(), N, sd.data_ptr(), cd.data_ptr(), cap, w.ptr, _st())
        ref = H.weights_dist(src, sets, counts, cap)
    what = "%s w | %s" % (entry, tag)
    r = H.check(w.np(what), ref, what)                    # w[i][min(count, cap):] is FILL in the reference, with M = 0
    print("RATIO %s w %s %.3f" % (entry, fam, r))
    return ref


def test_weights_feat(dev):
    sets, counts = H.weights_sets()
    sd, cd = _dev(dev, sets), _dev(dev, counts)
    for D in H.WEIGHTS_D:
        for fam in H.FEAT_FAMILIES:
            _weights(dev, "rg_rerank_weights_feat", H.feat_input(D, fam), sets, counts, H.WEIGHTS_CAP, sd, cd, "%s_D%d" % (fam, D), "D %d %s" % (D, fam))
    # the LDS limit: the largest admitted cap runs, one more is refused with a status and a message, nothing written
    D, cap_bad, cap_ok = H.weights_refusal()
    x = H.feat_input(D, "unit")
    wide = np.full((H.WEIGHTS_N, cap_ok), -1, dtype=np.int32)
    wide[:, :H.WEIGHTS_CAP] = sets
    wd = _dev(dev, wide)
    _weights(dev, "rg_rerank_weights_feat", x, wide, counts, cap_ok, wd, cd, "unit_D%d_cap%d" % (D, cap_ok), "D %d cap %d (LDS limit)" % (D, cap_ok))
    w = _Out((8,), dev)
    xd = _dev(dev, x)
    with pytest.raises(RuntimeError, match="LDS"):
        _lib().rg_rerank_weights_feat(xd.data_ptr(), H.WEIGHTS_N, D, wd.data_ptr(), cd.data_ptr(), cap_bad, w.ptr, _st())
    assert bool((w.np("refusal") == H.FILL).all())
    # the wrapper, with an x whose address is not a multiple of 16 bytes (it clones it)
    x = H.feat_input(68, "unit")
    buf = torch.zeros(x.size + 8, device=dev)
    xm = buf[1:1 + x.size].view(x.shape)
    xm.copy_(torch.from_numpy(x))
    assert xm.data_ptr() % 16 == 4
    got = _ops().rerank_weights(sd, cd, x=xm).cpu().numpy()
    ref = H.weights_feat(x, sets, counts)
    live = ref.value != H.FILL
    H.check(got[live], H.Ref(ref.value[live], ref.M[live], ref.kind), "ops.rerank_weights x")


def test_weights_dist(dev):
    sets, counts = H.weights_sets()
    sd, cd = _dev(dev, sets), _dev(dev, counts)
    for fam in H.DIST_FAMILIES:
        o = H.dist_input(fam)
        ref = _weights(dev, "rg_rerank_weights_dist", o, sets, counts, H.WEIGHTS_CAP, sd, cd, fam, fam)
    cap_ok = H.LDS_LIMIT // 4
    w = _Out((8,), dev)
    od = _dev(dev, o)
    with pytest.raises(RuntimeError, match="LDS"):
        _lib().rg_rerank_weights_dist(od.data_ptr(), H.WEIGHTS_N, sd.data_ptr(), cd.data_ptr(), cap_ok + 1, w.ptr, _st())
    assert bool((w.np("refusal") == H.FILL).all())
    got = _ops().rerank_weights(sd, cd, orig=od).cpu().numpy()
    live = ref.value != H.FILL
    H.check(got[live], H.Ref(ref.value[live], ref.M[live], ref.kind), "ops.rerank_weights orig")


# ---- rg_rerank_qe_count / rg_rerank_qe_fill -------------------------------------------------------------------------------------------
def _qe(dev, case):
    tag, N, R, k2, _ = case
    sets, counts, w, rank = H.qe_input(case)
    cap = sets.shape[1]
    sd, cd, wd, rd = _dev(dev, sets), _dev(dev, counts), _dev(dev, w), _dev(dev, rank)
    rowcnt, rowptr, cols, vals = H.query_expand_csr(sets, w, counts, rank, k2)
    g_cnt, g_ptr = _int((N,), dev), _int((N + 1,), dev)
    _lib().rg_rerank_qe_count(_p(rd), R or 0, k2, N, sd.data_ptr(), cd.data_ptr(), cap, g_cnt.ptr, g_ptr.ptr, _st())
    assert np.array_equal(g_cnt.np("rg_rerank_qe_count rowcnt | " + tag), rowcnt), "rg_rerank_qe_count rowcnt | " + tag
    assert np.array_equal(g_ptr.np("rg_rerank_qe_count rowptr | " + tag), rowptr), "rg_rerank_qe_count rowptr | " + tag
    nnz = int(rowptr[-1])
    g_cols, g_vals = _int((nnz,), dev), _Out((nnz,), dev)
    _lib().rg_rerank_qe_fill(_p(rd), R or 0, k2, N, sd.data_ptr(), wd.data_ptr(), cd.data_ptr(), cap, g_ptr.ptr, g_cols.ptr, g_vals.ptr, _st())
    got_cols, got_vals = g_cols.np("rg_rerank_qe_fill cols | " + tag), g_vals.np("rg_rerank_qe_fill vals | " + tag)
    assert np.array_equal(got_cols, cols), "rg_rerank_qe_fill cols | " + tag
    assert H.same_bits(got_vals, vals), "rg_rerank_qe_fill vals | %s: %d elements differ, first %s" % (
        tag, int((got_vals != vals).sum()), np.nonzero(got_vals != vals)[0][:4])
    if rank is None:                                     # the identity: cols are the sets, vals are w, bit for bit
        for i in range(0, N, max(1, N // 64)):
            n = min(int(counts[i]), cap)
            ok = (sets[i, :n] >= 0) & (sets[i, :n] < N)
            assert np.array_equal(got_cols[rowptr[i]:rowptr[i + 1]], sets[i, :n][ok])
            assert H.same_bits(got_vals[rowptr[i]:rowptr[i + 1]], w[i, :n][ok])
    return (sd, wd, cd, rd, k2), (rowptr, cols, vals)


def test_query_expand(dev):
    for case in H.QE_CASES:
        dev_in, want = _qe(dev, case)
        if case[0] in ("n33_null", "n257_k6"):
            sd, wd, cd, rd, k2 = dev_in
            rowptr, cols, vals = _ops().rerank_query_expand(sd, wd, cd, rank=rd, k2=k2)
            assert np.array_equal(rowptr.cpu().numpy(), want[0]) and np.array_equal(cols.cpu().numpy(), want[1])
            assert H.same_bits(vals.cpu().numpy(), want[2])


# ---- rg_rerank_columns ----------------------------------------------------------------------------------------------------------------
def test_columns(dev):
    for name in ("n1", "n5", "n257", "big"):
        rowptr, cols, vals, N = H.columns_input(name)
        nnz = len(cols)
        pd, cd, vd = _dev(dev, rowptr, torch.int32), _dev(dev, cols, torch.int32), _dev(dev, vals)
        w_ptr, w_row, w_val = H.columns(rowptr, cols, vals, N)
        runs = []
        for _ in range(2):
            colptr, cursor, crow, cval = _int((N + 1,), dev), _int((N,), dev), _int((nnz,), dev), _Out((nnz,), dev)
            _lib().rg_rerank_columns(pd.data_ptr(), cd.data_ptr(), vd.data_ptr(), N, nnz, colptr.ptr, cursor.ptr, crow.ptr, cval.ptr, _st())
            what = "rg_rerank_columns | " + name
            cursor.np(what)
            g_ptr = colptr.np(what)
            assert np.array_equal(g_ptr, w_ptr), what + ": colptr"
            g_row, g_val = H.canon_columns(g_ptr, crow.np(what), cval.np(what))
            assert np.array_equal(g_row, w_row) and H.same_bits(g_val, w_val), what + ": a column's (row, value) pairs differ"
            runs.append((g_ptr, g_row, g_val))
        assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1]) and H.same_bits(runs[0][2], runs[1][2])
        if name == "n257":
            colptr, crow, cval = _ops().rerank_columns(pd, cd, vd)
            g_ptr = colptr.cpu().numpy()
            g_row, g_val = H.canon_columns(g_ptr, crow.cpu().numpy(), cval.cpu().numpy())
            assert np.array_equal(g_ptr, w_ptr) and np.array_equal(g_row, w_row) and H.same_bits(g_val, w_val)


# ---- rg_rerank_jaccard ----------------------------------------------------------------------------------------------------------------
def _jaccard_dev(dev, rowptr, cols, vals, N):
    colptr, crow, cval = H.columns(rowptr, cols, vals, N)
    i32 = torch.int32
    return [_dev(dev, rowptr, i32), _dev(dev, cols, i32), _dev(dev, vals), _dev(dev, colptr, i32), _dev(dev, crow, i32), _dev(dev, cval)]


def _jaccard(dev, arrays, host, rows, off, orig, clamp, chunks):
    rowptr, cols, vals, N = host
    lam = H.JACCARD_LAMBDA if orig is not None else 0.0
    want = H.jaccard_rows_csr(rowptr, cols, vals, N, rows, off, orig, lam, clamp)
    od = _dev(dev, orig)
    for chunk in chunks:
        out = _Out((rows, N - off), dev)
        _lib().rg_rerank_jaccard(*([a.data_ptr() for a in arrays] + [N, rows, off, _p(od), lam, int(clamp), out.ptr, chunk, _st()]))
        what = "rg_rerank_jaccard | N %d rows %d col_off %d orig %s clamp %d chunk %d (W, parts) %s" % (
            N, rows, off, orig is not None, clamp, chunk, H.jaccard_chunks(N, off, chunk))
        got = out.np(what)
        assert H.same_bits(got, want), "%s: %d elements differ, first %s" % (what, int((got != want).sum()), np.argwhere(got != want)[:4].tolist())
    return want


def test_jaccard(dev):
    host = H.jaccard_input()
    N = host[3]
    arrays = _jaccard_dev(dev, *host)
    changed = 0
    for rows, off in H.jaccard_blocks():
        for orig in (None, H.jaccard_orig(N, rows)):
            free = _jaccard(dev, arrays, host, rows, off, orig, False, H.jaccard_chunk_values(N - off))
            clamped = _jaccard(dev, arrays, host, rows, off, orig, True, H.jaccard_chunk_values(N - off))
            changed += int((free != clamped).sum())
    assert changed > 0                                   # the clamp had work to do
    big = H.jaccard_big_input()
    arrays_big = _jaccard_dev(dev, *big)
    for orig, clamp in ((None, True), (H.jaccard_orig(big[3], H.JACCARD_BIG_ROWS), False)):
        _jaccard(dev, arrays_big, big, H.JACCARD_BIG_ROWS, 0, orig, clamp, [0, H.JACCARD_MAX_CHUNK])
    # the wrapper
    Q = H.JACCARD_Q
    orig = H.jaccard_orig(N, Q)
    got = _ops().rerank_jaccard(tuple(arrays[:3]), tuple(arrays[3:]), rows=Q, col_off=Q, orig=_dev(dev, orig),
                                lambda_value=H.JACCARD_LAMBDA, clamp=True, chunk=63)
    assert H.same_bits(got.cpu().numpy(), H.jaccard_rows_csr(host[0], host[1], host[2], N, Q, Q, orig, H.JACCARD_LAMBDA, True))


# ---- rg_rerank_orig_dist --------------------------------------------------------------------------------------------------------------
def test_orig_dist(dev):
    for Q, G in H.ORIG_QG:
        for zero_col in ((None, Q + G // 2) if G > 1 and Q > 1 else (None,)):
            blocks = H.orig_input(Q, G, zero_col)
            N = Q + G
            want = H.orig_dist(*blocks)
            assert (zero_col is None and not np.isnan(want).any()) or np.isnan(want[zero_col]).all()      # 0 / 0 along that row
            qg, qq, gg = (_dev(dev, b) for b in blocks)
            colmax, orig = _Out((N,), dev), _Out((N, N), dev)
            _lib().rg_rerank_orig_dist(qg.data_ptr(), qq.data_ptr(), gg.data_ptr(), Q, G, colmax.ptr, orig.ptr, _st())
            what = "rg_rerank_orig_dist | Q %d G %d zero column %s" % (Q, G, zero_col)
            A = np.block([[blocks[1], blocks[0]], [blocks[0].T, blocks[2]]]).astype(F32)
            assert H.same_bits(colmax.np(what), (A * A).max(axis=0)), what + ": colmax"
            got = orig.np(what)
            assert H.same_bits(got, want), "%s: %d elements differ, first %s" % (what, int((got != want).sum()), np.argwhere(got != want)[:4].tolist())
    blocks = H.orig_input(31, 33)
    got = _ops().rerank_orig_dist(*(_dev(dev, b) for b in blocks))
    assert H.same_bits(got.cpu().numpy(), H.orig_dist(*blocks))
