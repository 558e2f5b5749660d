"""CPU: profiles/conv_choices_mi355x.txt — the measured conv choices the bench pins (RG_CONV_TUNE_CACHE) — stays consistent with
the candidate lists of the conv library (plans: csrc/conv_igemm.hip; kernel implementations and paths: csrc/conv_fwd.hip,
conv_dgrad.hip, conv_wgrad.hip).  A line is the 16-field choice key and the index of the candidate that won; an index
the library cannot have produced would be clamped or re-measured silently, and the bench would no longer time fixed kernels."""
import os

CHOICES = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "conv_choices_mi355x.txt")

IMPL_KINDS = (1, 2, 4)          # kernel implementation: round-3, four-wave plane, eight-wave plane (fwd / dgrad / wgrad)
PATH_KINDS = (16, 32)           # tap-reuse 3x3 kernel vs generic implicit GEMM (fwd / dgrad)
PLAN_KINDS = (64, 128, 256)     # tile / split-K plan (fwd / dgrad / wgrad); field 13 is the candidate count


def _lines():
    with open(CHOICES) as f:
        return [ln.split() for ln in f if ln.strip()]


def _impl_count(key):
    """candidates of an implementation choice: the eight-wave form exists on the forward 128x128 / 64x128 tiles, the data-gradient
    128x128 tile and 64x128 tile without fused row sums, and the weight-gradient 128x128 tile"""
    kind, tile, epi = key[0], key[13], key[15]
    if kind == 1:
        return 3 if tile <= 1 else 2
    if kind == 2:
        return 3 if (tile == 0 or (tile == 1 and not epi & 4)) else 2
    return 3 if tile == 0 else 2


def test_choice_file_lines_are_valid():
    lines = _lines()
    assert len(lines) > 1000, "the bench's choice file is (nearly) empty"
    bad = [ln for ln in lines if len(ln) != 17]
    assert not bad, "lines without 17 integers: %s" % bad[:5]
    rows = [[int(v) for v in ln] for ln in lines]
    keys = {}
    dups = []
    for r in rows:
        k = tuple(r[:16])
        if k in keys:
            dups.append(k)
        keys[k] = r[16]
    assert not dups, "keys recorded twice: %s" % dups[:5]
    wrong = []
    for r in rows:
        kind, idx = r[0], r[16]
        if kind in IMPL_KINDS:
            ok = 0 <= idx < _impl_count(r)
        elif kind in PATH_KINDS:
            ok = 0 <= idx <= 1
        elif kind in PLAN_KINDS:
            ok = 0 <= idx < r[13]
        else:
            ok = False
        if not ok:
            wrong.append(r)
    assert not wrong, "%d lines name a candidate the library does not have: %s" % (len(wrong), wrong[:5])


def test_pick_knob_is_host_state():
    """rg_conv_set_pick / rg_conv_pick_log (the candidate sweep's knob) answer without a GPU: previous index back, unknown kinds
    refused, the log empty while nothing ran"""
    from rg_hip.lib import lib
    assert lib.rg_conv_pick_log(None, 0) == 0
    assert lib.rg_conv_set_pick(64, 3) == -1
    assert lib.rg_conv_set_pick(64, 1) == 3
    assert lib.rg_conv_set_pick(64, -1) == 1
    for kind, index in ((8, 0), (3, 0), (512, 0), (0, 0), (1, -2)):
        assert lib.rg_conv_set_pick(kind, index) < -1, (kind, index)
    assert "rg_conv_set_pick" in lib.rg_last_error().decode()
    assert lib.rg_conv_pick_log(None, 0) == 0
