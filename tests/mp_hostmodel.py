"""Host model of the multi-part encoder — the comparison partner of tests/test_mp_ops_gpu.py and tests/test_mp_models_gpu.py,
tied to the values recorded from the reference's own modules (tests/golden/reference_mp.npz) and to float32 torch by
tests/test_mp_cpu.py.  No tests and no GPU here.

Two parts:

  HResNetMP          plain torch, usable in fp64: oracle.ref_torch's OTVResNet / OBottleneck / OGeM put together as
                     CC/clustercontrast/models/resnet_mp.py:39-158 does, with the reference's attribute names (state_dict keys),
                     and `part_step`, the multi-part training step of CC/clustercontrast/trainers.py:79-93 without its GAN term.

  the fused head     fp64 closed forms of rg_mp_head_fwd / rg_mp_head_bwd (csrc/part_head.hip) with per-element error budgets in
                     the Ref(value, M, kind) scheme of tests/head_hostmodel.py: an element passes when
                         |got - value| <= C_KIND[kind] * 2^-24 * (M + 2^-102).

Budgets of the forward.  Per branch j and channel, K = 1 + |mean| invstd is the condition of the channel (the figure of
tests/norm_hostmodel.py: an error of u |mean| in x - mean is u (K - 1) in xhat):
    mean          mean_b |x|
    invstd        invstd                                                   (relative)
    running_mean  (1 - m) |old| + m M_mean;   running_var  (1 - m) old + m var_unbiased      (relative)
    xhat          K + |xhat|
    z_j           M_z = (K + |xhat|) |gamma| + |beta|                      (the `y` budget of norm_hostmodel)
    z_gc          sum_j M_z + sum_j |z_j|                                  (fusion 1: each addition rounds at most the sum of |z_j|)
    norm_k        n = sqrt(sum_c z^2):  sum_c |z| M_z / n + n              (the derivative z / n times each element's budget, plus
                                                                            the rounding of the sum and the root, relative to n);
                                                                            n = 0: sqrt(sum_c M_z^2)
    f_k           z / nn, nn = max(n, 1e-12):  M_z / nn + |f| M_n / nn [n >= 1e-12] + |f|
Budgets of the backward.  It is handed the float32 xhat, invstd and norms of the forward reference and recomputes z and f from
them, so E_z = |gamma xhat| + |beta| (one fused multiply-add), E_zgc = sum_j E_z + sum_j |z_j|, E_f = E_z / nn + |f|, and with
t = <dy, f> over the row (dropped for n < 1e-12):
    E_t           sum_c (|dy| E_f + |dy f|)
    dz_k          (dy - f t) / nn:  E_dz = (|dy| + 2 |f t| + E_f |t| + |f| E_t) / nn + |dz|
    dzt_j         the sum of the dz that reach branch j:  E_dzt = sum E_dz + sum |dz|
    dbeta  = s1   sum_b (E_dzt + |dzt|);     dgamma = s2   sum_b (E_dzt |xhat| + |dzt xhat|)
    dx            k (dzt - s1 / B - xhat s2 / B), k = gamma invstd (train; eval: k dzt):
                  |k| (E_dzt + |dzt| + (E_s1 + |s1|) / B + |xhat| (E_s2 + 2 |s2|) / B) + |dx|
Every M is built from the magnitudes that enter that element's own sums, never from a tensor-wide maximum.

The constants C_KIND are NOT taken from the kernels.  tests/test_mp_cpu.py evaluates every case of head_cases() with float32 torch on
the CPU (F.batch_norm, F.normalize, and for the backward the formulas above in float32 tensors), records max err / (2^-24 M) per
kind, and C_KIND = max(8, 4 x that ratio): 4 for another summation order and the hardware rsqrt / reciprocal, the floor of 8 so that
a lucky CPU run cannot make a budget tighter than two roundings per term.  Measured (torch 2.10, CPU, one thread):

    kind           float32 torch ratio    C_KIND
    mean           3.88                   15.6
    invstd         2.18                   8.8
    running_mean   2.57                   10.4
    running_var    2.57                   10.4
    xhat           7.72                   31.0
    norm           2.65                   10.7
    f              7.81                   31.3
    dsum           1.39                   8
    dx             0.80                   8

The larger ratios are torch's own summation order, not the formulas: `xhat` and `f` are driven by the `offset` family at B = 65 (a
serial float32 sum of 65 values near 300 carries several roundings of 300 into the batch mean, and invstd multiplies them).
"""
import collections

import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle import ref_torch as O
from tests.head_hostmodel import FILL, TINY_M, U24, Ref, family, gen  # noqa: F401  (one scheme, one comparator)

NORM_EPS = 1e-12


# ---- the encoder ---------------------------------------------------------------------------------------------------------------
class HResNetMP(nn.Module):
    def __init__(self, depth=50, norm=True, dropout=0, num_proj=256, pooling_type='avg', need_predictor=False):
        super(HResNetMP, self).__init__()
        r = O.OTVResNet(depth)
        self.base = nn.Sequential(r.conv1, r.bn1, r.relu, r.maxpool, r.layer1, r.layer2, r.layer3)
        self.res_g = r.layer4
        self.res_p = nn.Sequential(
            O.OBottleneck(1024, 512, 1, nn.Sequential(nn.Conv2d(1024, 2048, 1, bias=False), nn.BatchNorm2d(2048))),
            O.OBottleneck(2048, 512), O.OBottleneck(2048, 512))
        self.res_p.load_state_dict(r.layer4.state_dict())
        self.gpool2d = O.OGeM() if pooling_type == 'gem' else nn.AdaptiveAvgPool2d(1)
        self.norm, self.dropout = norm, dropout
        self.num_features = D = r.fc.in_features
        for name in ("feat_bn_g", "feat_bn_p1", "feat_bn_p2"):
            bn = nn.BatchNorm1d(D)
            bn.bias.requires_grad_(False)
            setattr(self, name, bn)
        self.feat_bn_gan = nn.BatchNorm2d(D)
        self.feat_bn_gan.bias.requires_grad_(False)
        if dropout > 0:
            self.drop = nn.Dropout(dropout)
        if need_predictor:
            self.predictor = nn.Sequential(nn.Linear(D, 2 * D, bias=False), nn.BatchNorm1d(2 * D), nn.ReLU(inplace=True),
                                           nn.Linear(2 * D, D, bias=False))
        self.fc_id_g = nn.Linear(D, D // 2, bias=False)
        self.fc_id_p1 = nn.Linear(D, D // 4, bias=False)
        self.fc_id_p2 = nn.Linear(D, D // 4, bias=False)
        self.proj_gan = nn.Conv2d(D, num_proj, 1, bias=False)

    def forward(self, x, clustering=False, fusion='sum'):
        bs = x.size(0)
        x = self.base(x)
        x_g, x_p = self.res_g(x), self.res_p(x)
        div = x_p.shape[2] // 2
        x_p1 = self.gpool2d(x_p[:, :, :div, :]).view(bs, -1)
        x_p2 = self.gpool2d(x_p[:, :, div:, :]).view(bs, -1)
        x_g = self.gpool2d(x_g).view(bs, -1)
        x_g, x_p1, x_p2 = self.feat_bn_g(x_g), self.feat_bn_p1(x_p1), self.feat_bn_p2(x_p2)
        self.feat_bn_gan(x_p)                                   # only its running statistics matter: the output is discarded
        if fusion == "cat":
            x_gc = torch.cat([self.fc_id_g(x_g), self.fc_id_p1(x_p1), self.fc_id_p2(x_p2)], dim=1)
        elif fusion == "sum":
            x_gc = x_g + x_p1 + x_p2
        else:
            x_gc = x_g
        f_g, f_p1, f_p2, f_gc = F.normalize(x_g), F.normalize(x_p1), F.normalize(x_p2), F.normalize(x_gc)
        if not self.training:
            return (f_gc, f_g) if clustering else f_gc
        if self.dropout > 0:
            f_g, f_gc = self.drop(f_g), self.drop(f_gc)
        return f_g, f_p1, f_p2, f_gc


def intra_cl(q, k, temperature, group_size):
    """group contrast of CC/clustercontrast/trainers.py:200-210"""
    q, k = F.normalize(q, dim=1), F.normalize(k, dim=1)
    logits = q @ k.t()
    qs, ks = logits.shape
    logits = logits.reshape(qs, ks // group_size, group_size).sum(2)
    targets = torch.arange(group_size, dtype=torch.long).repeat_interleave(group_size)
    return F.cross_entropy(logits / temperature, targets, reduction="none")


def part_step(encoder, memory, optimizer, imgs, labels, temperature, group_size):
    """the multi-part step of CC/clustercontrast/trainers.py:79-93 without the GAN term"""
    f_g, f_p1, f_p2, f_gc = encoder(imgs)
    loss = memory(f_gc, labels).mean()
    for f in (f_p1, f_p2, f_g):
        loss = loss + intra_cl(f, f.detach(), temperature, group_size).mean()
    optimizer.zero_grad()
    loss.backward()
    optimizer.step()
    return loss.item()


# ---- the fused head ------------------------------------------------------------------------------------------------------------
C_KIND = {"mean": 15.6, "invstd": 8.8, "running_mean": 10.4, "running_var": 10.4, "xhat": 31.0, "norm": 10.7, "f": 31.3, "dsum": 8.0,
          "dx": 8.0, "exact": 0.0}

KCG = 16                            # kCG, part_head.hip: channels per workgroup of the column phase (16 row slices each)
HEAD_B = [2, 3, 16, 65]             # 2: the smallest batch BatchNorm1d takes; 3, 16: fewer rows than slices and one each; 65 crosses 64
HEAD_D = [8, 100, 2048]             # 100 is no multiple of the channel group
GRAD_PATTERNS = {"all": (1, 1, 1, 1), "gc": (0, 0, 0, 1), "g": (1, 0, 0, 0)}        # which of (f_g, f_p1, f_p2, f_gc) has a gradient


def head_workspace(B, D):
    return 4 * (-(-D // KCG)) * B * 4


def _d(t):
    return None if t is None else t.detach().double()


def head_input(B, D, fam, seed=0, zero_branch=None):
    """(xs, gammas, betas, running_means, running_vars, epss, momenta) in float32; zero_branch: gamma = beta = 0 there, so every
    row of that branch's z is exactly zero (the norm clamp at 1e-12)"""
    g = gen(1000 * seed + 7 * B + D)
    xs = [family((B, D), fam, g) for _ in range(3)]
    gammas = [(torch.rand(D, generator=g) * 0.6 + 0.2).float() * (1.0 if j else -1.0) for j in range(3)]
    betas = [(torch.randn(D, generator=g) * 0.1).float() for _ in range(3)]
    rms = [(torch.randn(D, generator=g) * 0.1 + float(xs[j].mean())).float() for j in range(3)]
    rvs = [((torch.rand(D, generator=g) * 0.4 + 0.8) * max(float(xs[j].var()), 1e-3)).float() for j in range(3)]
    if zero_branch is not None:
        gammas[zero_branch], betas[zero_branch] = torch.zeros(D), torch.zeros(D)
    return xs, gammas, betas, rms, rvs, [1e-5, 1e-5, 1e-3], [0.1, 0.1, 0.25]


def _f32(v):
    return float(torch.tensor(float(v), dtype=torch.float32))


def head_fwd(xs, gammas, betas, rms, rvs, epss, moms, train, fusion):
    """-> dict of Ref: out [4, B, D], xhat [3, B, D], mean / invstd [3, D], norms [4, B], running_mean / running_var [3, D]"""
    B, D = xs[0].shape
    val, Mv = collections.defaultdict(list), collections.defaultdict(list)
    zs, Mz = [], []
    for j in range(3):
        x, ga, be, eps, m = _d(xs[j]), _d(gammas[j]), _d(betas[j]), _f32(epss[j]), _f32(moms[j])
        if train:
            mean, Mmean = x.mean(0), x.abs().mean(0)
            var = ((x - mean) ** 2).mean(0)
            unb = var * (B / (B - 1.0))
            val["running_mean"].append((1 - m) * _d(rms[j]) + m * mean)
            Mv["running_mean"].append((1 - m) * _d(rms[j]).abs() + m * Mmean)
            val["running_var"].append((1 - m) * _d(rvs[j]) + m * unb)
            Mv["running_var"].append((1 - m) * _d(rvs[j]) + m * unb)
        else:
            mean, Mmean, var = _d(rms[j]), torch.zeros(D, dtype=torch.float64), _d(rvs[j])
            val["running_mean"].append(_d(rms[j])), Mv["running_mean"].append(torch.zeros(D, dtype=torch.float64))
            val["running_var"].append(_d(rvs[j])), Mv["running_var"].append(torch.zeros(D, dtype=torch.float64))
        invstd = (var + eps).rsqrt()
        K = 1.0 + mean.abs() * invstd
        xhat = (x - mean) * invstd
        val["mean"].append(mean), Mv["mean"].append(Mmean)
        val["invstd"].append(invstd), Mv["invstd"].append(invstd)
        val["xhat"].append(xhat), Mv["xhat"].append(K + xhat.abs())
        zs.append(xhat * ga + be)
        Mz.append((K + xhat.abs()) * ga.abs() + be.abs())
    if fusion:
        zs.append(zs[0] + zs[1] + zs[2])
        Mz.append(Mz[0] + Mz[1] + Mz[2] + zs[0].abs() + zs[1].abs() + zs[2].abs())
    else:
        zs.append(zs[0]), Mz.append(Mz[0])
    for z, M in zip(zs, Mz):
        n = z.pow(2).sum(1)
        n = n.sqrt()
        Mn = torch.where(n > 0, (z.abs() * M).sum(1) / n.clamp_min(1e-300) + n, M.pow(2).sum(1).sqrt())
        nn_ = n.clamp_min(NORM_EPS).reshape(B, 1)
        f = z / nn_
        Mf = M / nn_ + f.abs() * torch.where(n >= NORM_EPS, Mn, torch.zeros_like(Mn)).reshape(B, 1) / nn_ + f.abs()
        val["norms"].append(n), Mv["norms"].append(Mn)
        val["out"].append(f), Mv["out"].append(Mf)
    kinds = {"out": "f", "norms": "norm", "xhat": "xhat", "mean": "mean" if train else "exact", "invstd": "invstd",
             "running_mean": "running_mean" if train else "exact", "running_var": "running_var" if train else "exact"}
    return {k: Ref(torch.stack(val[k]), torch.stack(Mv[k]), kinds[k]) for k in kinds}


def head_fwd_f32(xs, gammas, betas, rms, rvs, epss, moms, train, fusion):
    """the same quantities from float32 torch (F.batch_norm, F.normalize): what C_KIND is calibrated on"""
    rms, rvs, train = [t.clone() for t in rms], [t.clone() for t in rvs], bool(train)
    out = collections.defaultdict(list)
    zs = []
    for j in range(3):
        x = xs[j]
        if train:
            mean = x.mean(0)
            var = x.var(0, unbiased=False)
        else:
            mean, var = rms[j].clone(), rvs[j].clone()
        invstd = (var + epss[j]).rsqrt()
        zs.append(F.batch_norm(x, rms[j], rvs[j], gammas[j], betas[j], train, moms[j], epss[j]))
        out["xhat"].append(F.batch_norm(x, None if train else rms[j], None if train else rvs[j], None, None, train, 0.0, epss[j]))
        out["mean"].append(mean), out["invstd"].append(invstd)
        out["running_mean"].append(rms[j]), out["running_var"].append(rvs[j])
    zs.append(zs[0] + zs[1] + zs[2] if fusion else zs[0])
    for z in zs:
        out["out"].append(F.normalize(z)), out["norms"].append(z.norm(dim=1))
    return {k: torch.stack(v) for k, v in out.items()}


def head_bwd_terms(dys, xhat, invstd, norms, gammas, betas, train, fusion, dtype=torch.float64):
    """the backward formulas in tensors of `dtype` from the handed forward tensors -> (dx [3, B, D], dgamma [3, D], dbeta [3, D],
    budgets or None); float64 gives the reference and its budgets, float32 the calibration partner"""
    _, B, D = xhat.shape
    c = lambda t: None if t is None else t.detach().to(dtype)      # noqa: E731
    xh, iv, nr = c(xhat), c(invstd), c(norms)
    budget = dtype == torch.float64
    zs = [xh[j] * c(gammas[j]) + c(betas[j]) for j in range(3)]
    Ez = [(xh[j] * c(gammas[j])).abs() + c(betas[j]).abs() for j in range(3)]
    if fusion:
        zs.append(zs[0] + zs[1] + zs[2])
        Ez.append(Ez[0] + Ez[1] + Ez[2] + zs[0].abs() + zs[1].abs() + zs[2].abs())
    else:
        zs.append(zs[0]), Ez.append(Ez[0])
    dz, Edz = [], []
    for k in range(4):
        if dys[k] is None:
            dz.append(None), Edz.append(None)
            continue
        g = c(dys[k])
        nn_ = nr[k].clamp_min(NORM_EPS).reshape(B, 1)
        f = zs[k] / nn_
        live = (nr[k] >= NORM_EPS).to(dtype).reshape(B, 1)
        t = (g * f).sum(1, keepdim=True) * live
        v = (g - f * t) / nn_
        dz.append(v)
        if budget:
            Ef = Ez[k] / nn_ + f.abs()
            Et = (g.abs() * Ef + (g * f).abs()).sum(1, keepdim=True) * live
            Edz.append((g.abs() + 2.0 * (f * t).abs() + Ef * t.abs() + f.abs() * Et) / nn_ + v.abs())
    dx, dga, dbe, M = [], [], [], {"dx": [], "dgamma": [], "dbeta": []}
    for j in range(3):
        parts = [k for k in ((j, 3) if (fusion or j == 0) else (j,)) if dz[k] is not None]
        if not parts:
            dx.append(None), dga.append(None), dbe.append(None)
            for m in M.values():
                m.append(None)
            continue
        dzt = dz[parts[0]] if len(parts) == 1 else dz[parts[0]] + dz[parts[1]]
        s1, s2 = dzt.sum(0), (dzt * xh[j]).sum(0)
        k_ = c(gammas[j]) * iv[j]
        v = k_ * (dzt - s1 / B - xh[j] * s2 / B) if train else k_ * dzt
        dx.append(v), dga.append(s2), dbe.append(s1)
        if budget:
            Edzt = sum(Edz[k] for k in parts) + (sum(dz[k].abs() for k in parts) if len(parts) > 1 else 0.0)
            Es1, Es2 = (Edzt + dzt.abs()).sum(0), (Edzt * xh[j].abs() + (dzt * xh[j]).abs()).sum(0)
            if train:
                Mdx = k_.abs() * (Edzt + dzt.abs() + (Es1 + s1.abs()) / B + xh[j].abs() * (Es2 + 2.0 * s2.abs()) / B) + v.abs()
            else:
                Mdx = k_.abs() * (Edzt + dzt.abs()) + v.abs()
            M["dx"].append(Mdx), M["dgamma"].append(Es2), M["dbeta"].append(Es1)
    return dx, dga, dbe, (M if budget else None)


def head_bwd(dys, xhat, invstd, norms, gammas, betas, train, fusion):
    """-> {'dx': [Ref or None] * 3, 'dgamma': ..., 'dbeta': ...}; None: no gradient reaches the branch (nothing is written)"""
    dx, dga, dbe, M = head_bwd_terms(dys, xhat, invstd, norms, gammas, betas, train, fusion)
    ref = lambda v, m, kind: None if v is None else Ref(v, m, kind)      # noqa: E731
    return {"dx": [ref(v, m, "dx") for v, m in zip(dx, M["dx"])], "dgamma": [ref(v, m, "dsum") for v, m in zip(dga, M["dgamma"])],
            "dbeta": [ref(v, m, "dsum") for v, m in zip(dbe, M["dbeta"])]}


def head_cases():
    """[(B, D, family, train, fusion, gradient pattern, zero branch)]: every B with every D; families, mode, fusion and the pattern of
    NULL upstream gradients go round so that each B and each D meets each of them; one case per mode with an all-zero branch"""
    fams = ("plain", "scales", "offset", "constant")
    pats = list(GRAD_PATTERNS)
    out, i = [], 0
    for B in HEAD_B:
        for D in HEAD_D:
            for train in (1, 0):
                out.append((B, D, fams[i % 4], train, (i // 2) % 2, pats[i % 3], None))
                i += 1
    out += [(3, 100, "plain", 1, 1, "all", 1), (3, 100, "plain", 0, 1, "all", 1), (16, 100, "plain", 1, 0, "gc", None),
            (16, 100, "plain", 1, 1, "g", None), (16, 8, "plain", 0, 0, "all", None)]
    return out


def head_dys(B, D, pattern, seed=0):
    g = gen(31 * seed + B + D)
    return [torch.randn(B, D, generator=g).float() if on else None for on in GRAD_PATTERNS[pattern]]
