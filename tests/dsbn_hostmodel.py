"""Host model of the domain-specific BatchNorm layer (rg_dsbn_fwd / rg_dsbn_bwd, rg_hip.nn.DSBN2d / DSBN1d) — the comparison
partner of tests/test_dsbn_ops_gpu.py and tests/test_dsbn_models_gpu.py, tied to the values recorded from the reference's own
modules (tests/golden/reference_dsbn.npz) by tests/test_dsbn_cpu.py.  No tests and no GPU here.

A domain is a BatchNorm over h = N / 2 samples, so everything comes from tests/norm_hostmodel.py UNCHANGED: the fp64 closed forms
`forward('bn', ...)` / `backward('bn', ...)` on each half, value and M concatenated per domain, and the per-element budget
C_KIND * 2^-24 * M with the same constants (no new ones).

  dispatch mirrors   dsbn_one_launch, dsbn_slices, dsbn_regime: the host arithmetic of rg_dsbn_* that picks a kernel
  fp64 references    forward / backward -> dict of Ref; statistics are [2][C] (S row, T row)
  input family       `two_domains`: source half around 0 with unit scale, target half around 4 with scale 3, and gamma, beta and the
                     running statistics of the T set far from the S set (see tests/test_dsbn_ops_gpu.py for the margins)
  plain torch        HDSBN: the layer as F.batch_norm on the two halves, for the converted trees
"""
import collections

import torch
import torch.nn as nn
import torch.nn.functional as F

from tests import norm_hostmodel as H

Ref = H.Ref
Set = collections.namedtuple("Set", "gamma beta running_mean running_var")
NOSET = Set(None, None, None, None)


# ---- dispatch mirrors ----------------------------------------------------------------------------------------------------------
def dsbn_one_launch(N, C, HW):
    """rg_dsbn_one_launch(): the per-domain extent fits one workgroup per virtual channel; no channel threshold (rg_bn_train_fused_ok
    wants C >= 128)"""
    return N % 2 == 0 and (N // 2) * HW <= 16384


def dsbn_slices(N, C, HW):
    """(S, L) of the slice regime: S slices of L elements over ONE domain's (N/2)*HW values (pick_slices over 2C virtual channels)"""
    return H.pick_slices(N // 2, 2 * C, HW)


def dsbn_regime(N, C, HW):
    """('reg', U) | ('loop', float4 rows?) | ('slice', S, L)"""
    if dsbn_one_launch(N, C, HW):
        U = H.bn_reg_units(N // 2, C, HW)
        return ("reg", U) if U else ("loop", HW % 4 == 0)
    return ("slice",) + dsbn_slices(N, C, HW)


def workspace_bytes(N, C, HW):
    """rg_dsbn_workspace()"""
    return 2 * C * dsbn_slices(N, C, HW)[0] * 3 * 4


# ---- fp64 references -----------------------------------------------------------------------------------------------------------
def _cat(a, b, dim=0):
    return Ref(torch.cat((a.value, b.value), dim), torch.cat((a.M, b.M), dim), a.kind)


def forward(x, s, t, residual=None, eps=(1e-5, 1e-5), act=H.ACT_NONE, slope=0.0, momentum=(0.1, 0.1)):
    """x [N][C][HW], s / t: Set.  -> {'y' [N][C][HW], 'mean' / 'invstd' [2C], 'running_mean_s', 'running_var_s', 'running_mean_t',
    'running_var_t' (where the set has them)}"""
    h = x.shape[0] // 2
    assert 2 * h == x.shape[0]
    halves = []
    for d, p in enumerate((s, t)):
        sl = slice(d * h, (d + 1) * h)
        halves.append(H.forward("bn", x[sl], p.gamma, p.beta, None if residual is None else residual[sl], eps[d], act, slope,
                                p.running_mean, p.running_var, momentum[d]))
    out = {k: _cat(halves[0][k], halves[1][k]) for k in ("y", "mean", "invstd")}
    for d, tag in enumerate("st"):
        for k in ("running_mean", "running_var"):
            if k in halves[d]:
                out[k + "_" + tag] = halves[d][k]
    return out


def backward(x, dy, y_act, mean, invstd, gamma_s=None, gamma_t=None, act=H.ACT_NONE, slope=0.0):
    """mean / invstd [2C] (or [2][C]) -> {'dx', 'dres' [N][C][HW], 'd_beta_s', 'd_gamma_s', 'd_beta_t', 'd_gamma_t' [C]}"""
    h, C = x.shape[0] // 2, x.shape[1]
    mean, invstd = mean.reshape(2, C), invstd.reshape(2, C)
    halves = []
    for d, gamma in enumerate((gamma_s, gamma_t)):
        sl = slice(d * h, (d + 1) * h)
        halves.append(H.backward("bn", x[sl], dy[sl], None if y_act is None else y_act[sl], mean[d], invstd[d], gamma, act, slope))
    out = {k: _cat(halves[0][k], halves[1][k]) for k in ("dx", "dres")}
    for d, tag in enumerate("st"):
        out["d_beta_" + tag] = halves[d]["sum_g"]
        out["d_gamma_" + tag] = halves[d]["sum_g_xhat"]
    return out


# ---- input family ---------------------------------------------------------------------------------------------------------------
Inputs = collections.namedtuple("Inputs", "x residual dy s t")


def two_domains(N, C, HW, family="plain", seed=0):
    """H.make_inputs' families in the source half and the S set; the target half of x is 3 x + 4 of its own draw (per channel scale of
    the `scales` family kept), and the T set is drawn apart from the S set: |gamma_t| in 2..3 with the opposite signs, beta_t around
    +5, running_mean_t around 4, running_var_t in 8.5..9.5"""
    inp = H.make_inputs("bn", N, C, HW, family, seed)
    h = N // 2
    g = torch.Generator().manual_seed(77000 + 1000 * seed + 7 * N + 131 * C + HW)
    cs = (10.0 ** torch.linspace(-3, 3, C)) if family == "scales" else torch.ones(C)
    x = inp.x.clone()
    x[h:] = 3.0 * x[h:] + 4.0 * cs.reshape(1, C, 1)
    gamma_t = -torch.sign(inp.gamma) * (torch.rand(C, generator=g) + 2.0) / cs
    beta_t = torch.randn(C, generator=g) + 5.0
    rm_t = torch.randn(C, generator=g) * 0.1 + 4.0
    rv_t = torch.rand(C, generator=g) + 8.5
    return Inputs(x.contiguous(), inp.residual, inp.dy, Set(inp.gamma, inp.beta, inp.running_mean, inp.running_var),
                  Set(gamma_t, beta_t, rm_t, rv_t))


# ---- case lists, built from the dispatch mirrors ---------------------------------------------------------------------------------
# one launch, (N, C, HW): per = ceil(N/2 * HW / 4 / 256) float4 units per thread of ONE domain, rounded up to U.  C from 3 (far below
# the 128 channels rg_bn_train_fused_ok asks of a BatchNorm) to 130, most of them no multiple of 64
ONE_LAUNCH = [
    (4, 3, 64), (8, 65, 256),          # U = 1 ragged (32 units), full (256)
    (6, 5, 344), (4, 64, 1024),        # U = 2 ragged (258), full
    (6, 67, 1028), (8, 4, 1024),       # U = 4 ragged (771), full
    (10, 7, 820), (16, 6, 1024),       # U = 8 ragged (1025), full
    (6, 64, 2732), (32, 3, 1024),      # U = 16 ragged (2049), full = the largest one-launch extent (16384 per domain)
    (10, 66, 21), (2, 5, 35),          # scalar rows: the loop kernels; h = 1
    (6, 130, 1), (2, 63, 1),           # HW = 1, the 1d layer: h = 3; h = 1 (one value per virtual channel)
]
ONE_LAUNCH_EXPECT = [("reg", 1)] * 2 + [("reg", 2)] * 2 + [("reg", 4)] * 2 + [("reg", 8)] * 2 + [("reg", 16)] * 2 + \
    [("loop", False)] * 4

# slice regime, (N, C, HW): a per-domain extent above 16384, S = min(ceil(2048 / 2C), ceil(h HW / 4096)) slices per domain.  In every
# case the per-domain extent is NOT a multiple of the slice length L, so the same slices laid over the whole batch would straddle
# sample h (checked in slice_cases()).  (Fewer than 4 slices need 2C > 512 channels at such an extent, tensors of 70 MB and more;
# S is a loop bound of the finalize kernels and a grid size, not another code path.)
SLICE = [
    (2, 3, 16388),                     # extent just above the one-launch limit, h = 1: S = 5, float4 rows, L = 3280
    (6, 5, 5463),                      # S = 5, scalar rows (HW odd), L = 3280: boundaries mid-row, ragged last slice
    (10, 3, 4100),                     # S = 6, float4 rows, L = 3420: boundaries mid-row
    (2, 260, 16388),                   # S = 4 by the channel count (2C = 520), L = 4100, C no multiple of 64
    (4, 66, 8193),                     # S = 5, scalar rows, h = 2, L = 3280
]


def one_launch_cases():
    out = []
    for i, (shape, want) in enumerate(zip(ONE_LAUNCH, ONE_LAUNCH_EXPECT)):
        assert dsbn_regime(*shape) == want, (shape, dsbn_regime(*shape), want)
        out.append(shape + (H.FAMILIES[(i // 2 + (i % 2) * 2) % 5],))
    return out


def slice_cases():
    out = []
    for i, (N, C, HW) in enumerate(SLICE):
        reg = dsbn_regime(N, C, HW)
        assert reg[0] == "slice", (N, C, HW, reg)
        assert ((N // 2) * HW) % reg[2] != 0, "slices of %d would not straddle sample %d of %s" % (reg[2], N // 2, (N, C, HW))
        out.append((N, C, HW, H.FAMILIES[(i + 1) % 5]))
    assert sorted(set(dsbn_slices(N, C, HW)[0] for N, C, HW, _ in out)) == [4, 5, 6]
    assert set(HW % 4 == 0 for _, _, HW, _ in out) == {True, False}
    return out


# ---- the layer in plain torch ------------------------------------------------------------------------------------------------------
class HDSBN(nn.Module):
    """DSBN2d / DSBN1d as F.batch_norm on the two halves (views, one concatenation); eval mode: BN_T on the whole batch"""

    def __init__(self, planes, dims=2):
        super(HDSBN, self).__init__()
        self.num_features = planes
        cls = nn.BatchNorm2d if dims == 2 else nn.BatchNorm1d
        self.BN_S, self.BN_T = cls(planes), cls(planes)

    def forward(self, x):
        if not self.training:
            t = self.BN_T
            return F.batch_norm(x, t.running_mean, t.running_var, t.weight, t.bias, False, t.momentum, t.eps)
        h = x.shape[0] // 2
        if 2 * h != x.shape[0]:
            raise AssertionError("odd batch")
        ys = []
        for bn, part in ((self.BN_S, x[:h]), (self.BN_T, x[h:])):
            bn.num_batches_tracked += 1
            ys.append(F.batch_norm(part, bn.running_mean, bn.running_var, bn.weight, bn.bias, True, bn.momentum, bn.eps))
        return torch.cat(ys, 0)


def convert_h(model):
    """the host model's convert_dsbn on a torch.nn tree"""
    for name, child in list(model.named_children()):
        if isinstance(child, (nn.BatchNorm2d, nn.BatchNorm1d)):
            m = HDSBN(child.num_features, 2 if isinstance(child, nn.BatchNorm2d) else 1)
            m.BN_S.load_state_dict(child.state_dict())
            m.BN_T.load_state_dict(child.state_dict())
            setattr(model, name, m)
        else:
            convert_h(child)
    return model


def rtree():
    """tests/golden/cases_dsbn.Tree on THIS build's modules (same attribute names, so the same state_dict keys): the stem and the
    block run through rg_hip.resnet_trunk's trunk program, i.e. through conv_bn_tf / conv_bn_tb with their epilogues"""
    from clustercontrast.models.pooling import build_pooling_layer
    from rg_hip import nn as rnn
    from rg_hip.resnet_trunk import Bottleneck, trunk_tb, trunk_tf
    from rg_hip.tape import RGModule
    from tests.golden.cases_dsbn import TREE

    class RTree(RGModule):
        def __init__(self):
            super(RTree, self).__init__()
            s, w, f = TREE["stem"], TREE["width"], TREE["feat"]
            ds = rnn.Sequential(rnn.Conv2d(s, 4 * w, 1, bias=False), rnn.BatchNorm2d(4 * w))
            self.base = rnn.Sequential(rnn.Conv2d(3, s, 3, stride=1, padding=1, bias=False), rnn.BatchNorm2d(s), rnn.ReLU(inplace=True),
                                       rnn.MaxPool2d(3, 2, 1), rnn.Sequential(Bottleneck(s, w, 1, ds)))
            self.gap = build_pooling_layer("avg")
            self.feat_bn = rnn.BatchNorm1d(f)

        def tf(self, tape, x):
            fmap = trunk_tf(tape, list(self.base), x)
            return self.feat_bn.tf(tape, self.gap.tf(tape, fmap).reshape(fmap.shape[0], -1))

        def tb(self, tape, dy, need_dx=True):
            dy = self.feat_bn.tb(tape, dy)
            return trunk_tb(tape, list(self.base), self.gap.tb(tape, dy.reshape(dy.shape[0], -1, 1, 1)), need_dx)

    return RTree()
