"""CPU: the numpy model of the CMC / mAP scoring (tests/rank_eval_hostmodel.py) against the reference's recorded results
(tests/golden/reference_eval.npz), the closed formula for average precision against scikit-learn's on tied inputs, and the
host side of the new evaluation_metrics packages (imports, argument checks that need no GPU)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import rank_eval_hostmodel as M
from tests.golden import cases_eval as C

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(REPO, "tests", "golden", "reference_eval.npz"))


def test_fixture_holds_what_the_cases_describe():
    for name, cs in C.CASES.items():
        d, qid, gid, qcam, gcam = C.load(GOLD, name)
        assert d.dtype == np.float32 and d.shape == (cs["Q"], cs["G"]) and d.shape[0] <= 40 and d.shape[1] <= 1000
        assert all(v.dtype == np.int32 for v in (qid, gid, qcam, gcam))
        want = C.make_inputs(name)
        assert all(np.array_equal(a, b) for a, b in zip((d, qid, gid, qcam, gcam), want)), name
    assert os.path.getsize(os.path.join(REPO, "tests", "golden", "reference_eval.npz")) < 200 * 1024
    for name in C.TIE_FREE:
        assert C.rows_tie_free(GOLD[name + "_dist"]), name
    d = GOLD["tied_dist"]
    assert 4 <= len(np.unique(d)) <= 8 and not C.rows_tie_free(d)
    gid = GOLD["edge_ids_gid"]
    assert (gid == -1).any() and (gid == 0).any() and len(gid) == 257
    # `wide`: query 0's only matches share its camera
    d, qid, gid, qcam, gcam = C.load(GOLD, "wide")
    same = gid == qid[0]
    assert same.any() and (gcam[same] == qcam[0]).all()


@pytest.mark.parametrize("name", C.TIE_FREE)
def test_model_equals_reference_on_tie_free_cases(name):
    d, qid, gid, qcam, gcam = C.load(GOLD, name)
    for dt in (np.float32, np.float64):
        plain = M.summarize(*M.per_query(d.astype(dt), qid, gid, qcam, gcam, topk=C.TOPK))
        sep = M.summarize(*M.per_query(d.astype(dt), qid, gid, qcam, gcam, topk=C.TOPK, separate_camera_set=True))
        assert abs(plain[0] - float(GOLD[name + "_map"])) <= 1e-12
        assert np.array_equal(plain[1], GOLD[name + "_cmc_market1501"])
        assert np.array_equal(sep[1], GOLD[name + "_cmc_sepcam_first"])
        assert np.abs(plain[2] - GOLD[name + "_cmc_allshots"]).max() <= 1e-12
        assert np.abs(sep[2] - GOLD[name + "_cmc_sepcam"]).max() <= 1e-12
    if name == "wide":
        assert M.per_query(d, qid, gid, qcam, gcam)[0][0] == 0          # the skipped query


def test_model_map_equals_reference_on_tied_case():
    d, qid, gid, qcam, gcam = C.load(GOLD, "tied")
    got = M.summarize(*M.per_query(d, qid, gid, qcam, gcam))[0]
    assert abs(got - float(GOLD["tied_map"])) <= 1e-12


def test_closed_formula_equals_sklearn_on_tied_inputs():
    g = np.random.RandomState(0)
    worst = 0.0
    for trial in range(60):
        n = int(g.randint(1, 400))
        levels = int(g.choice([1, 2, 4, 8, 1000000]))
        d = (g.randint(0, levels, size=n) / 8.0).astype(np.float32 if trial % 2 else np.float64)
        match = g.rand(n) < g.choice([0.02, 0.3, 0.9])
        if not match.any():
            match[g.randint(n)] = True
        worst = max(worst, abs(M.ap_formula(match, d) - M.ap_sklearn(match, d)))
    print("closed formula vs scikit-learn: worst difference %.2e" % worst)
    assert worst <= 1e-12
    # -0.0 and 0.0 are one value
    d = np.array([0.0, -0.0, 1.0, -0.0])
    match = np.array([False, True, True, False])
    assert abs(M.ap_formula(match, d) - M.ap_sklearn(match, d)) <= 1e-12 and abs(M.ap_formula(match, d) - (1 / 3 + 2 / 4) / 2) <= 1e-15


def test_model_first_and_hits_follow_the_stable_order():
    # one query, id 7 / camera 0; columns: junk (same id, same camera), non-match, match (tie with the next), non-match, match
    d = np.array([[0.0, 0.1, 0.2, 0.2, 0.3]])
    gid, gcam = np.array([7, 1, 7, 2, 7]), np.array([0, 0, 1, 1, 1])
    npos, ap, first, hits = M.per_query(d, [7], gid, [0], gcam, topk=3)
    assert npos[0] == 2 and first[0] == 1 and hits[0].tolist() == [0, 1, 1]
    assert abs(ap[0] - (1 / 3 + 2 / 4) / 2) <= 1e-15                    # the tie counts its non-matching partner against the match
    # separate cameras: the camera-0 non-match leaves
    npos, ap, first, hits = M.per_query(d, [7], gid, [0], gcam, topk=3, separate_camera_set=True)
    assert npos[0] == 2 and first[0] == 0 and hits[0].tolist() == [1, 1, 0]
    with pytest.raises(RuntimeError, match="No valid query"):
        M.summarize(*M.per_query(d, [9], gid, [0], gcam))


def test_new_packages_import_without_a_gpu_or_a_reference_tree():
    code = ("from clustercontrast.evaluation_metrics import cmc, mean_ap\n"
            "from clustercontrast.evaluation_metrics.ranking import cmc as c2\n"
            "import reid.evaluation_metrics as RE, clustercontrast.evaluation_metrics as CE\n"
            "from clustercontrast.evaluators import DeviceEvaluator, evaluate_all_device, extract_features_device, pairwise_distance\n"
            "from clustercontrast.utils.rerank import re_ranking\n"
            "import inspect\n"
            "assert RE.cmc is cmc is c2 and RE.mean_ap is mean_ap and not hasattr(CE, 'accuracy')\n"
            "assert str(inspect.signature(cmc)) == '(distmat, query_ids=None, gallery_ids=None, query_cams=None, gallery_cams=None, "
            "topk=100, separate_camera_set=False, single_gallery_shot=False, first_match_break=False)'\n"
            "assert str(inspect.signature(mean_ap)) == '(distmat, query_ids=None, gallery_ids=None, query_cams=None, gallery_cams=None)'\n"
            "assert inspect.signature(pairwise_distance).parameters['return_device'].default is False\n"
            "assert inspect.signature(re_ranking).parameters['return_device'].default is False\n"
            "assert str(inspect.signature(DeviceEvaluator.evaluate)) == '(self, data_loader, query, gallery, cmc_flag=False, rerank=False)'\n"
            "import clustercontrast.evaluators as E\n"
            "assert not any(hasattr(E, n) for n in ('Evaluator', 'evaluate_all', 'extract_features'))\n"
            "print('IMPORT-OK')\n")
    env = dict(os.environ)
    env["PYTHONPATH"] = os.path.join(REPO, "reid-gan_amd")
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "IMPORT-OK" in out.stdout, out.stdout + out.stderr


def test_single_gallery_shot_needs_the_reference_tree():
    from clustercontrast.evaluation_metrics import cmc
    with pytest.raises(NotImplementedError, match="single_gallery_shot"):
        cmc(np.zeros((2, 3), dtype=np.float32), single_gallery_shot=True)


def test_single_gallery_shot_is_handed_to_a_reference_tree_behind(tmp_path):
    ref = tmp_path / "ref" / "clustercontrast" / "evaluation_metrics"
    ref.mkdir(parents=True)
    (ref / "__init__.py").write_text("from .classification import accuracy\nfrom .ranking import cmc, mean_ap\n")
    (ref / "classification.py").write_text("def accuracy(*a, **k):\n    return 'ref accuracy'\n")
    (ref / "ranking.py").write_text("def cmc(distmat, *a, **k):\n    return ('ref cmc', type(distmat).__name__, k['single_gallery_shot'])\n"
                                    "def mean_ap(*a, **k):\n    return 'ref mean_ap'\n")
    (tmp_path / "ref" / "clustercontrast" / "__init__.py").write_text("")
    code = ("import numpy as np, torch\n"
            "import clustercontrast.evaluation_metrics as CE\n"
            "assert CE.accuracy() == 'ref accuracy' and CE.cmc.__module__ == 'clustercontrast.evaluation_metrics.ranking'\n"
            "assert CE.__file__.startswith(%r)\n"
            "assert CE.cmc(np.zeros((2, 3)), single_gallery_shot=True) == ('ref cmc', 'ndarray', True)\n"
            "assert CE.cmc(torch.zeros(2, 3), single_gallery_shot=True) == ('ref cmc', 'Tensor', True)\n"
            "print('HANDOVER-OK')\n" % os.path.join(REPO, "reid-gan_amd"))
    env = dict(os.environ)
    env["PYTHONPATH"] = os.pathsep.join([os.path.join(REPO, "reid-gan_amd"), str(tmp_path / "ref")])
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "HANDOVER-OK" in out.stdout, out.stdout + out.stderr


def test_id_range_and_type_checks_need_no_gpu():
    from clustercontrast.evaluation_metrics import ranking as R
    import torch
    cpu = torch.device("cpu")
    assert R._ids_on_device([3, -1, 0], "ids", 3, cpu).dtype == torch.int32
    assert R._ids_on_device(np.array([2 ** 31 - 1], dtype=np.int64), "ids", 1, cpu).tolist() == [2 ** 31 - 1]
    with pytest.raises(ValueError, match="int32"):
        R._ids_on_device(np.array([2 ** 31], dtype=np.int64), "ids", 1, cpu)
    with pytest.raises(ValueError, match="int32"):
        R._ids_on_device(torch.tensor([-2 ** 31 - 1]), "ids", 1, cpu)
    with pytest.raises(ValueError, match="integers"):
        R._ids_on_device(np.array([1.5]), "ids", 1, cpu)
    with pytest.raises(ValueError, match="entries"):
        R._ids_on_device([1, 2], "ids", 3, cpu)
