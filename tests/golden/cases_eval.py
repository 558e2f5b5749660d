"""Cases shared by make_golden_eval.py (reference side) and the CMC / mAP tests (fixture / device side).

CMC ranks are discrete and the reference sorts with numpy's unstable quicksort, so the fixture is a fair yardstick for CMC
only where no row holds two equal distances: the three tie-free cases draw fp32 distances and the maker asserts that every
row's values are distinct (re-asserted from the stored inputs by tests/test_rank_eval_cpu.py).  The values are exactly
representable in fp32, so the same fixture serves the fp32 and the fp64 runs.  Average precision groups tied scores and is
independent of their order: the quantised case stores mAP only.
"""
import numpy as np

TOPK = 100
# name -> queries, gallery entries, identities, cameras, seed; `levels`: distances quantised to that many values (mAP only)
CASES = {
    "edge_ids": dict(Q=24, G=257, n_id=12, n_cam=3, seed=3),         # gallery ids -1 (junk) and 0, G one past a multiple of 64
    "wide": dict(Q=12, G=1000, n_id=9, n_cam=6, seed=4),            # many positives per query; one query is skipped
    "narrow": dict(Q=40, G=120, n_id=30, n_cam=2, seed=5),           # few gallery entries per identity, two cameras
    "tied": dict(Q=20, G=300, n_id=10, n_cam=4, seed=7, levels=6),
}
TIE_FREE = ("edge_ids", "wide", "narrow")
# the reference's CMC configurations without sampling (single_gallery_shot=False)
CMC_CONFIGS = {
    "market1501": dict(separate_camera_set=False, first_match_break=True),
    "allshots": dict(separate_camera_set=False, first_match_break=False),
    "sepcam": dict(separate_camera_set=True, first_match_break=False),
    "sepcam_first": dict(separate_camera_set=True, first_match_break=True),
}


def make_inputs(name):
    """(dist fp32 [Q, G], query_ids, gallery_ids, query_cams, gallery_cams int32): matching entries tend to be closer"""
    cs = CASES[name]
    g = np.random.RandomState(cs["seed"])
    Q, G = cs["Q"], cs["G"]
    lo = -1 if name == "edge_ids" else 1
    gid = g.randint(lo, lo + cs["n_id"], size=G).astype(np.int32)
    qid = g.randint(max(lo, 0), lo + cs["n_id"], size=Q).astype(np.int32)
    gcam = g.randint(0, cs["n_cam"], size=G).astype(np.int32)
    qcam = g.randint(0, cs["n_cam"], size=Q).astype(np.int32)
    if name == "wide":
        # query 0: every gallery entry of its identity shares its camera, so it has no valid match and is skipped
        gcam[gid == qid[0]] = qcam[0]
    d = g.rand(Q, G) + 0.15 * (gid[None, :] != qid[:, None])
    if "levels" in cs:
        d = np.floor(d / d.max() * cs["levels"]).clip(0, cs["levels"] - 1) / 4.0
    return np.ascontiguousarray(d, dtype=np.float32), qid, gid, qcam, gcam


def rows_tie_free(d):
    return all(len(np.unique(r)) == len(r) for r in np.asarray(d))


def load(gold, name):
    return tuple(gold["%s_%s" % (name, k)] for k in ("dist", "qid", "gid", "qcam", "gcam"))
