"""Cases shared by make_golden_sgs.py (reference side) and the single-gallery-shot CMC tests (model / device side).

The reference's `cmc(single_gallery_shot=True)` sorts with numpy's unstable quicksort, so only tie-free rows are a fair
yardstick: the inputs are the three tie-free cases of cases_eval.py (read from reference_eval.npz, not stored twice) and one
case of its own, `bigseg`: 65 gallery identities of which one owns 712 of the 1 000 entries (a segment that takes a wave
many sweeps, beside segments of a handful), 16 queries of which half ask for the big identity.  The maker asserts that every
row is tie-free; the values are exactly representable in fp32, so the fixture serves the fp32 and the fp64 runs.
For every case: both `separate_camera_set`, both `first_match_break`, seeds 0 and 11 of numpy's global generator; stored are
the reference's curve at topk = 20 and the generator state after the call (np.random.get_state()[1:3]).
"""
import numpy as np

from tests.golden import cases_eval as CE

TOPK = 20
REPEAT = 10            # the reference's constant
SEEDS = (0, 11)
OWN = ("bigseg",)      # inputs stored in reference_sgs.npz; the others come from reference_eval.npz
CASES = tuple(CE.TIE_FREE) + OWN
BIGSEG = dict(Q=16, G=1000, n_id=65, big=712, n_cam=3, seed=6)
CONFIGS = {
    "plain": dict(separate_camera_set=False, first_match_break=False),
    "first": dict(separate_camera_set=False, first_match_break=True),
    "sepcam": dict(separate_camera_set=True, first_match_break=False),       # the reference's `cuhk03` configuration
    "sepcam_first": dict(separate_camera_set=True, first_match_break=True),
}


def make_inputs(name):
    """(dist fp32 [Q, G], query_ids, gallery_ids, query_cams, gallery_cams int32)"""
    if name in CE.TIE_FREE:
        return CE.make_inputs(name)
    cs = BIGSEG
    g = np.random.RandomState(cs["seed"])
    Q, G = cs["Q"], cs["G"]
    gid = np.concatenate([np.zeros(cs["big"], dtype=np.int64), np.arange(1, cs["n_id"]),
                          g.randint(1, cs["n_id"], size=G - cs["big"] - (cs["n_id"] - 1))])
    gid = gid[g.permutation(G)].astype(np.int32)
    qid = np.where(np.arange(Q) % 2 == 0, 0, g.randint(1, cs["n_id"], size=Q)).astype(np.int32)
    gcam = g.randint(0, cs["n_cam"], size=G).astype(np.int32)
    qcam = g.randint(0, cs["n_cam"], size=Q).astype(np.int32)
    d = g.rand(Q, G) + 0.15 * (gid[None, :] != qid[:, None])
    return np.ascontiguousarray(d, dtype=np.float32), qid, gid, qcam, gcam


def key(name, cfg, seed, what):
    return "%s_%s_s%d_%s" % (name, cfg, seed, what)


def load(gold_sgs, gold_eval, name):
    gold = gold_sgs if name in OWN else gold_eval
    return tuple(gold["%s_%s" % (name, k)] for k in ("dist", "qid", "gid", "qcam", "gcam"))
