"""tests/golden/reference_rerank.npz (the reference's compute_jaccard_distance / re_ranking outputs, made by
tests/golden/make_golden_rerank.py) is a fair yardstick: the gap condition holds on the stored inputs, the staged
algorithm the kernels implement (tests/rerank_hostmodel.py) reproduces the stored outputs, and the public modules import,
resolve through the overlay and refuse bad arguments — all without a GPU and without the reference tree or faiss."""
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

from tests import rerank_hostmodel as H
from tests.golden import cases_rerank as C

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATH = os.path.join(REPO, "tests", "golden", "reference_rerank.npz")
GOLD = np.load(PATH)


def test_fixture_is_small_and_complete():
    assert os.path.getsize(PATH) < 300 * 1024
    for name, cs in C.CASES.items():
        n = cs["n_id"] * cs["per"]
        x = GOLD[name + "_x"]
        assert x.shape == (n, cs["D"]) and x.dtype == np.float32
        assert np.abs(np.linalg.norm(x.astype(np.float64), axis=1) - 1).max() < 1e-6
        assert np.array_equal(x, C.make_features(cs["n_id"], cs["per"], cs["D"], cs["noise"], seed=int(GOLD[name + "_seed"])))
        assert GOLD[name + "_jaccard_upper"].shape == (n * (n + 1) // 2,) and GOLD[name + "_jaccard_upper"].dtype == np.float32
        assert GOLD[name + "_final"].shape == (n // 4, n - n // 4) and GOLD[name + "_final"].dtype == np.float32


@pytest.mark.parametrize("name", sorted(C.CASES))
def test_gap_condition_on_the_stored_inputs(name):
    cs, x = C.CASES[name], GOLD[name + "_x"]
    g_l2 = C.cut_gap(C.sq_l2(x), cs["k1"], cs["k2"])
    g_rr = C.cut_gap(C.normalised_dist64(*C.euclid_inputs(x)), cs["k1"], cs["k2"])
    print(name, "gap l2 %.3e rerank %.3e" % (g_l2, g_rr))
    assert g_l2 >= C.GAP and g_rr >= C.GAP
    assert np.allclose([g_l2, g_rr], GOLD[name + "_gaps"], rtol=1e-6)


@pytest.mark.parametrize("name", sorted(C.CASES))
def test_staged_algorithm_reproduces_the_reference(name):
    """ranking -> expanded sets -> weights -> query expansion -> Jaccard rows with the column counts the public modules
    use (k1 / k1 + 1 forward columns, round-half-even(k1 / 2) + 1 for the half sets) gives the reference's matrices"""
    cs, x = C.CASES[name], GOLD[name + "_x"]
    k1, k2, n = cs["k1"], cs["k2"], len(x)
    ref = C.unpack_upper(GOLD[name + "_jaccard_upper"], n)
    rank = C.rank_of(C.sq_l2(x), k1)
    sets = H.expand_sets(rank, k1, min(C.half_k(k1) + 1, k1))
    V = H.query_expand(H.dense_weights(sets, x=x), rank, k2)
    jac = np.maximum(H.jaccard_rows(V, range(n)), 0)
    assert np.array_equal(jac < 1, ref < 1)
    assert np.abs(jac - ref).max() <= 2e-6
    q_g, q_q, g_g = C.euclid_inputs(x)
    q = len(q_g)
    o64 = C.normalised_dist64(q_g, q_q, g_g)
    rank = C.rank_of(o64, k1 + 1)
    sets = H.expand_sets(rank, k1 + 1, C.half_k(k1) + 1)
    orig = o64.astype(np.float32)
    V = H.query_expand(H.dense_weights(sets, orig=orig), rank, k2)
    fin = (H.jaccard_rows(V, range(q)) * np.float32(1 - C.LAMBDA) + orig[:q] * np.float32(C.LAMBDA))[:, q:]
    assert np.abs(fin - GOLD[name + "_final"]).max() <= 2e-6


def test_half_to_even():
    from clustercontrast.utils.faiss_rerank import half_k
    assert [half_k(k) for k in (1, 5, 6, 7, 20, 30)] == [0, 2, 3, 4, 10, 15]


def test_k_reciprocal_neigh_host_helper():
    from clustercontrast.utils.faiss_rerank import k_reciprocal_neigh
    rank = np.array([[0, 1, 2], [1, 0, 3], [2, 3, 0], [3, 2, 1]])
    assert k_reciprocal_neigh(rank, 0, 1).tolist() == [0, 1]
    assert k_reciprocal_neigh(rank, 0, 2).tolist() == [0, 1, 2]
    assert k_reciprocal_neigh(rank, 1, 2).tolist() == [1, 0, 3]


def test_modules_import_without_reference_tree_or_faiss():
    code = textwrap.dedent("""
        import sys
        from clustercontrast.utils.faiss_rerank import compute_jaccard_distance, k_reciprocal_neigh
        from clustercontrast.utils.rerank import re_ranking
        import inspect
        assert 'faiss' not in sys.modules
        assert list(inspect.signature(compute_jaccard_distance).parameters)[:6] == ['target_features', 'k1', 'k2', 'print_flag', 'search_option', 'use_float16']
        assert [p.default for p in inspect.signature(compute_jaccard_distance).parameters.values()][1:6] == [20, 6, True, 0, False]
        assert list(inspect.signature(re_ranking).parameters)[:6] == ['q_g_dist', 'q_q_dist', 'g_g_dist', 'k1', 'k2', 'lambda_value']
        assert [p.default for p in inspect.signature(re_ranking).parameters.values()][3:6] == [20, 6, 0.3]
        print('RERANK-IMPORT-OK')
        """)
    env = dict(os.environ)
    env["PYTHONPATH"] = os.path.join(REPO, "reid-gan_amd")
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "RERANK-IMPORT-OK" in out.stdout, out.stdout + out.stderr


def test_overlay_resolves_to_this_build(tmp_path):
    """a reference-like tree behind this one holds its own utils/rerank.py and a faiss-importing utils/faiss_rerank.py:
    both names resolve to this build, and an inherited Evaluator's `from .utils.rerank import re_ranking` gets ours"""
    ref = tmp_path / "ref" / "clustercontrast"
    (ref / "utils").mkdir(parents=True)
    (ref / "__init__.py").write_text("")
    (ref / "utils" / "__init__.py").write_text("")
    (ref / "utils" / "rerank.py").write_text("def re_ranking(*a, **k):\n    return 'reference re_ranking'\n")
    (ref / "utils" / "faiss_rerank.py").write_text("import faiss\n")
    (ref / "evaluators.py").write_text(textwrap.dedent("""
        def pairwise_distance(features, query=None, gallery=None):
            return 'reference pairwise_distance'
        class Evaluator(object):
            def rerank_function(self):
                from .utils.rerank import re_ranking
                return re_ranking
        """))
    code = textwrap.dedent("""
        import sys
        REPO = %r
        import clustercontrast.utils.faiss_rerank as F
        import clustercontrast.utils.rerank as R
        from clustercontrast.evaluators import Evaluator
        assert F.__file__.startswith(REPO) and R.__file__.startswith(REPO), (F.__file__, R.__file__)
        assert Evaluator.__module__ == 'clustercontrast._ref_evaluators'
        assert Evaluator().rerank_function() is R.re_ranking
        assert 'faiss' not in sys.modules
        print('RERANK-OVERLAY-OK')
        """ % os.path.join(REPO, "reid-gan_amd"))
    env = dict(os.environ)
    env["PYTHONPATH"] = os.pathsep.join([os.path.join(REPO, "reid-gan_amd"), str(tmp_path / "ref")])
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "RERANK-OVERLAY-OK" in out.stdout, out.stdout + out.stderr


def test_bad_arguments_are_refused_before_the_device_is_touched():
    import torch
    from clustercontrast.utils.faiss_rerank import compute_jaccard_distance
    from clustercontrast.utils.rerank import re_ranking
    from rg_hip import ops
    x = torch.randn(12, 8)
    with pytest.raises(ValueError, match="k1"):
        compute_jaccard_distance(x, k1=12, k2=2, print_flag=False)
    with pytest.raises(ValueError, match="k2"):
        compute_jaccard_distance(x, k1=4, k2=5, print_flag=False)
    with pytest.raises(ValueError, match=r"\[N, D\]"):
        compute_jaccard_distance(x[0], k1=4, k2=2, print_flag=False)
    qg, qq, gg = np.ones((3, 9), np.float32), np.ones((3, 3), np.float32), np.ones((9, 9), np.float32)
    with pytest.raises(ValueError, match="q_q_dist"):
        re_ranking(qg, np.ones((4, 4), np.float32), gg)
    with pytest.raises(ValueError, match="g_g_dist"):
        re_ranking(qg, qq, np.ones((9, 8), np.float32))
    with pytest.raises(ValueError, match="k1"):
        re_ranking(qg, qq, gg, k1=12)
    with pytest.raises(ValueError, match="k2"):
        re_ranking(qg, qq, gg, k1=4, k2=6)
    rank = torch.zeros((12, 5), dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.rerank_expand(rank, 5, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.rerank_orig_dist(torch.from_numpy(qg), torch.from_numpy(qq), torch.from_numpy(gg))
