"""CPU: the multi-part encoder's public interface (registry, state_dict layout, refused arguments), the host model of
tests/mp_hostmodel.py against the values tests/golden/make_golden_mp.py recorded from the reference's own modules, the calibration
of the fused head's error budgets on float32 torch, and the argument checks of the new entry points.  No reference and no GPU
needed."""
import os

import numpy as np
import pytest
import torch

from tests import head_hostmodel as HH
from tests import mp_hostmodel as H
from tests.golden import cases_mp as C
from tests.golden.cases import recording_threads, sub

GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "reference_mp.npz"))


@pytest.fixture(autouse=True, scope="module")
def _threads_of_the_recording():
    with recording_threads():
        yield


def _cmp(got, key, tol):
    ref = GOLD[key]
    got = np.asarray(got.detach().numpy() if torch.is_tensor(got) else got, dtype=np.float64).reshape(ref.shape)
    scale = max(np.abs(ref).max(), 1e-12)
    err = np.abs(got - ref).max()
    assert err <= tol * scale + 1e-12, "%s: %.3e vs scale %.3e (rel %.2e > %.1e)" % (key, err, scale, err / scale, tol)


def vs_fixture(rec, name, mode, cmp=_cmp):
    """every recorded quantity of one (case, mode) at max(2e-5, 4 x the reference's own recorded distance from fp64)"""
    for k, v in rec.items():
        key = "%s_%s_%s" % (name, mode, k)
        tol = max(2e-5, 4.0 * float(GOLD[key + "_ref_vs_fp64"]))
        if k.startswith("stat:"):
            cmp(v.double(), key, tol)
            continue
        s, stats = sub(v, C.SUB)
        cmp(s, key, tol)
        cmp(stats, key + "_stats", tol)


# ---- the host model reproduces the reference ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_encoders():
    made = {}

    def get(name):
        if name not in made:
            m = H.HResNetMP(50, **C.CASES[name][0])
            made[name] = (m, C.fill(m.state_dict(), "mp_" + name))
        return made[name]
    return get


@pytest.mark.parametrize("mode", ["train"] + list(C.EVAL_CALLS))
@pytest.mark.parametrize("name", list(C.CASES))
def test_hostmodel_encoder(host_encoders, name, mode):
    m, sd = host_encoders(name)
    m.load_state_dict(sd)
    rec = C.record(m, name, mode)
    if mode == "train":
        assert rec.pop("_gradless") == [str(k) for k in GOLD[name + "_gradless"]]
    vs_fixture(rec, name, mode)


def test_fixture_facts():
    """what the recording established about the reference: 410 entries with the predictor, the frozen / never-called parameters
    without gradient, the part map of an 80 x 32 crop split 2 + 3"""
    assert len(GOLD["keys_predictor"]) == 410 and len(GOLD["keys_plain"]) == 410 - 7
    gl = [str(k) for k in GOLD["gem64_gradless"]]
    assert "feat_bn_gan.weight" in gl and "proj_gan.weight" in gl and "predictor.0.weight" in gl and "fc_id_p2.weight" in gl
    assert "gpool2d.p" not in gl and "feat_bn_p2.weight" not in gl
    assert all(k.endswith(".bias") or k.split(".")[0] in ("feat_bn_gan", "predictor", "fc_id_g", "fc_id_p1", "fc_id_p2", "proj_gan")
               for k in gl)


# ---- public interface ---------------------------------------------------------------------------------------------------------
def test_registry_lists_the_multi_part_encoder():
    import clustercontrast.models as M
    assert "resnet_mp50" in M.names()
    m = M.create("resnet_mp50", pretrained=False, norm=True, num_proj=256, pooling_type="gem", need_predictor=True)
    assert type(m).__name__ == "ResNet_MP" and m.num_features == 2048
    assert m.res_g[0].conv2.stride == (2, 2) and m.res_p[0].conv2.stride == (1, 1) and m.res_p[0].downsample[0].stride == (1, 1)
    assert len(m.base) == 7
    assert not m.feat_bn_g.bias.requires_grad and not m.feat_bn_gan.bias.requires_grad and m.feat_bn_p2.weight.requires_grad
    with pytest.raises(KeyError):
        M.create("resnet_mp101")            # the reference's factory registers resnet_mp50 only
    with pytest.raises(KeyError):
        M.create("resnet_bip50")


@pytest.mark.parametrize("tag,kw", [("plain", {}), ("predictor", dict(need_predictor=True))])
def test_state_dict_layout_is_the_reference_s(tag, kw):
    import clustercontrast.models as M
    sd = M.create("resnet_mp50", pretrained=False, norm=True, pooling_type="gem", **kw).state_dict()
    assert list(sd.keys()) == [str(k) for k in GOLD["keys_" + tag]]
    assert [";".join(map(str, v.shape)) for v in sd.values()] == [str(s) for s in GOLD["shapes_" + tag]]


def test_unbuildable_variants_are_refused():
    from clustercontrast.models import resnet_mp as R
    assert R.__all__ == ['ResNet_MP', 'resnet_mp50', 'resnet_mp101', 'resnet_mp152']
    for depth in (18, 34):
        with pytest.raises(KeyError, match="Unsupported depth"):
            R.ResNet_MP(depth, pretrained=False, norm=True)
    with pytest.raises(ValueError, match="UnboundLocalError"):
        R.resnet_mp50(pretrained=False, norm=False)
    with pytest.raises(KeyError, match="Unknown pooling"):
        R.resnet_mp50(pretrained=False, norm=True, pooling_type="gemFpn")


def test_res_p_starts_from_layer4_of_a_local_checkpoint(tmp_path, monkeypatch):
    import clustercontrast.models as M
    from rg_hip.resnet_trunk import TVResNet
    sd = C.fill(TVResNet(50).state_dict(), "ckpt")
    path = str(tmp_path / "resnet50.pth")
    torch.save(sd, path)
    monkeypatch.setenv("RG_RESNET50_WEIGHTS", path)
    got = M.create("resnet_mp50", pretrained=True, norm=True).state_dict()
    for src, dst in (("conv1.weight", "base.0.weight"), ("layer3.5.bn3.running_var", "base.6.5.bn3.running_var"),
                     ("layer4.0.conv2.weight", "res_g.0.conv2.weight"), ("layer4.0.conv2.weight", "res_p.0.conv2.weight"),
                     ("layer4.2.bn3.bias", "res_p.2.bn3.bias"), ("layer4.0.downsample.0.weight", "res_p.0.downsample.0.weight")):
        assert torch.equal(got[dst], sd[src]), dst


# ---- the head's error budgets are calibrated on float32 torch ------------------------------------------------------------------
def test_head_budgets_hold_for_float32_torch():
    """C_KIND >= max(8, 4 x the worst ratio float32 torch reaches over HEAD_CASES), per kind; prints the ratios"""
    worst = {}

    def note(got, ref):
        if ref is None:
            return
        w = HH.compare(got, H.Ref(ref.value, ref.M, ref.kind), table={k: float("inf") for k in H.C_KIND})
        if ref.kind != "exact":
            worst[ref.kind] = max(worst.get(ref.kind, 0.0), w.ratio)
    torch.set_num_threads(1)
    for B, D, fam, train, fusion, pat, zero in H.head_cases():
        args = H.head_input(B, D, fam, zero_branch=zero)
        ref, got = H.head_fwd(*args, train, fusion), H.head_fwd_f32(*args, train, fusion)
        for k in ref:
            note(got[k], ref[k])
        xhat, invstd, norms = ref["xhat"].value.float(), ref["invstd"].value.float(), ref["norms"].value.float()
        dys = H.head_dys(B, D, pat)
        rb = H.head_bwd(dys, xhat, invstd, norms, args[1], args[2], train, fusion)
        dx, dga, dbe, _ = H.head_bwd_terms(dys, xhat, invstd, norms, args[1], args[2], train, fusion, dtype=torch.float32)
        for j in range(3):
            assert (rb["dx"][j] is None) == (dx[j] is None)
            if dx[j] is not None:
                note(dx[j], rb["dx"][j]), note(dga[j], rb["dgamma"][j]), note(dbe[j], rb["dbeta"][j])
    for kind, r in sorted(worst.items()):
        print("float32 torch ratio %-13s %.2f   C_KIND %.2f" % (kind, r, H.C_KIND[kind]))
        assert H.C_KIND[kind] >= max(8.0, 4.0 * r) - 0.01, (kind, r, H.C_KIND[kind])
        assert H.C_KIND[kind] <= max(8.0, 4.0 * r) * 1.25 + 0.01, ("budget wider than its derivation", kind, r, H.C_KIND[kind])


def test_head_cases_cover_the_launch_arithmetic():
    cases = H.head_cases()
    assert {c[0] for c in cases} == set(H.HEAD_B) and {c[1] for c in cases} == set(H.HEAD_D)
    assert 100 % H.KCG and 65 > 64 and min(H.HEAD_B) == 2
    for mode in (0, 1):
        assert {c[5] for c in cases if c[3] == mode} == set(H.GRAD_PATTERNS) and {c[4] for c in cases if c[3] == mode} == {0, 1}
        assert any(c[6] is not None for c in cases if c[3] == mode)
    assert H.head_workspace(65, 100) == 4 * 7 * 65 * 4


# ---- C ABI: argument checks answer before any launch, so they run without a GPU ------------------------------------------------
def test_entry_points_reject_bad_arguments_before_launching():
    from rg_hip.lib import lib
    p = 4096                                            # stands for a device address; never dereferenced: every call below is refused

    def fwd(x=p, y=p, N=2, C=3, H=4, W=2, split=2):
        return lib.rg_part_pool_fwd(x, p, y, N, C, H, W, split, 1e-6, None)

    def bwd(dy=p, dx=p, dp=p, H=4, split=2, ws=p, nbytes=2 * 3 * 4, pp=p, x=p, y=p):
        return lib.rg_part_pool_bwd(x, pp, y, dy, dx, dp, 2, 3, H, 2, split, 1e-6, ws, nbytes, None)
    for kw, msg in ((dict(split=0), "part of the 4 rows empty"), (dict(split=4), "part of the 4 rows empty"),
                    (dict(H=1, split=0), "empty"), (dict(H=1, split=1), "empty"), (dict(y=None), "bad arguments"),
                    (dict(x=None), "bad arguments"), (dict(N=0), "bad arguments"), (dict(W=0), "bad arguments")):
        with pytest.raises(RuntimeError, match=msg):
            fwd(**kw)
    for kw, msg in ((dict(split=0), "empty"), (dict(split=4), "empty"), (dict(H=1, split=1), "empty"), (dict(dx=None), "bad arguments"),
                    (dict(dy=None), "bad arguments"), (dict(y=None), "GeM needs x and y"), (dict(x=None), "GeM needs x and y"),
                    (dict(pp=None), "no exponent gradient"), (dict(nbytes=2 * 3 * 4 - 1), "workspace too small"),
                    (dict(ws=None), "workspace too small")):
        with pytest.raises(RuntimeError, match=msg):
            bwd(**kw)
    B, D = 3, 100
    need = lib.rg_mp_head_workspace(B, D)
    assert need == H.head_workspace(B, D)

    def head(x=p, out=p, B=B, train=1, fusion=1, ws=p, nbytes=need):
        return lib.rg_mp_head_fwd(x, p, p, p, p, p, p, p, p, p, p, p, p, p, p, out, p, p, p, p, B, D, train, fusion, 1e-5, 1e-5, 1e-5,
                                  0.1, 0.1, 0.1, ws, nbytes, None)
    for kw, msg in ((dict(x=None), "bad arguments"), (dict(out=None), "bad arguments"), (dict(fusion=2), "fusion is 0"),
                    (dict(B=1), "more than 1 row"), (dict(nbytes=need - 1), "workspace too small"), (dict(ws=None), "workspace too small")):
        with pytest.raises(RuntimeError, match=msg):
            head(**kw)

    def hbwd(dys=(p, p, p, p), dzs=(None, None, None), dxs=(p, p, p), dgs=(p, p, p), fusion=1, xhat=p):
        return lib.rg_mp_head_bwd(*dys, *dzs, xhat, p, p, p, p, p, p, p, p, *dxs, *dgs, None, None, None, B, D, 1, fusion, None)
    for kw, msg in ((dict(xhat=None), "bad arguments"), (dict(dys=(None,) * 4), "no upstream gradient"), (dict(fusion=3), "fusion is 0"),
                    (dict(dxs=(None, p, p)), "dx_g is needed"), (dict(dys=(None, None, None, p), dxs=(p, None, p)), "dx_p1 is needed"),
                    (dict(dys=(p, None, None, None), dxs=(p, None, None)), "affine gradients of a branch without dx"),
                    (dict(dzs=(None, None, p), dys=(p, None, None, None), dxs=(p, None, None), dgs=(p, None, None)), "dx_p2 is needed")):
        with pytest.raises(RuntimeError, match=msg):
            hbwd(**kw)
