"""Host model of the cross entropy over two logit blocks with a group-diagonal mask — rg_softmax_ce_ext_fwd / _bwd, csrc/loss.hip —
in the conventions of tests/head_hostmodel.py: fp64 references taking the float32 tensors the C ABI takes, every reference a
Ref(value, M, kind) judged by head_hostmodel.compare.  The comparison partner of tests/test_ce_ext_gpu.py, tied to torch's own
F.cross_entropy and autograd in fp64 by tests/test_ce_ext_cpu.py.  No tests and no GPU here.

Definition.  Row i of la [n, m] | lb [n, t], n == t * group, is the cross entropy of the m + t values

    z[i][j]     = scale * la[i][j]                                          j < m
    z[i][m + j] = scale * fl32(lb[i][j] + (j == i // group ? mask : 0))     j < t

The addition is ONE float32 operation before the multiply (the reference's `outputs_ex += -10000 * eye(t).repeat_interleave(group,
0)`, then `/= temp`), so the model rounds it to float32 and works in fp64 from there; `scale` and `mask` are the float32 values the
C ABI receives.  A label outside [0, m + t) gives loss 0 and two zero gradient rows.

Error budgets.  The kinds and constants are head_hostmodel's `ce` and `ce_bwd` (C = 8 each, derived there from the operation
count and tied to float32 torch; nothing here is tuned), with the same per-element M read on the m + t values above:

    ce        lse: |lse| + max |z_j| + 1 over the LIVE columns j (p_j >= 2^-160); loss: that + |z_y|.  The argument of exp carries
              |z| + |lse|, but a column whose exp is exactly 0 adds exactly 0 to the sum whatever its argument's rounding, and it
              cannot be the maximum: counting the masked column's |z| ~ 2e5 would widen every row's budget 100-fold for nothing
    ce_bwd    |g| (p (1 + |z| + |lse|) + onehot), p = exp(z - lse)
    exact     M = 0: the rows of a label out of range, and every element whose fp64 p is below 2^-160 — its float32 exp argument
              is below -110 even after the budgeted error of the argument (|z| + |lse| <= 2^23 here, so that error stays under 1),
              and expf is exactly 0 below -103.98: a masked column at mask = -10000, scale = 20 has z - lse ~ -2e5

The rounded sum `lb + mask` is part of the definition, not of the budget: both sides form it with one float32 addition.
"""
import torch

from tests import head_hostmodel as HH

Ref = HH.Ref
P_ZERO = 2.0 ** -160                 # below this fp64 probability the float32 kernel's expf returns exactly 0 (see above)


def mask_matrix(n, t, group, mask):
    """the [n, t] float32 tensor the reference adds to the second block: mask * eye(t).repeat_interleave(group, 0)"""
    assert n == t * group
    return (HH.f32(mask) * torch.eye(t, dtype=torch.float64)).repeat_interleave(group, 0).float()


def values(la, lb, group, mask, scale):
    """z [n, m + t] in fp64: the float32 sum lb + mask matrix, then the multiply by the float32 scale"""
    n, t = lb.shape
    lbm = lb.float() + mask_matrix(n, t, group, mask)              # ONE float32 addition per element, as the kernel's
    return torch.cat([la.double(), lbm.double()], 1) * HH.f32(scale)


def fwd(la, lb, labels, group, mask, scale):
    """loss[i] = lse(z_i) - z_i[y_i], 0 for a label outside [0, m + t); lse[i] for every row"""
    z = values(la, lb, group, mask, scale)
    n, K = z.shape
    lse = torch.logsumexp(z, 1)
    ok = HH.in_range(labels, K)
    zy = z.gather(1, labels.clamp(0, K - 1).reshape(n, 1)).reshape(n)
    live = torch.exp(z - lse.reshape(n, 1)) >= P_ZERO
    Ml = lse.abs() + torch.where(live, z.abs(), torch.zeros_like(z)).max(1).values + 1.0
    loss =torch.where(ok, lse - zy, torch.zeros_like(lse))
    return {"loss": Ref(loss, torch.where(ok, Ml + zy.abs(), torch.zeros_like(Ml)), "ce"), "lse": Ref(lse, Ml, "ce")}


def bwd(la, lb, labels, lse, grow, gscale, group, mask, scale):
    """(dla, dlb) = grow[i] gscale scale (softmax - onehot) from the lse it is handed; an ignored row and an element whose
    probability underflows float32's exp are exactly zero"""
    z = values(la, lb, group, mask, scale)
    n, K = z.shape
    m = la.shape[1]
    l = lse.detach().double().reshape(n, 1)
    g = (torch.ones(n, dtype=torch.float64) if grow is None else grow.detach().double()).reshape(n, 1) * HH.f32(gscale) * HH.f32(scale)
    p = torch.exp(z - l)
    ok = HH.in_range(labels, K).reshape(n, 1)
    onehot = torch.zeros(n, K, dtype=torch.float64).scatter_(1, labels.clamp(0, K - 1).reshape(n, 1), 1.0)
    dead = (p < P_ZERO) & (onehot == 0)
    v = torch.where(ok & ~dead, g * (p - onehot), torch.zeros_like(p))
    M = torch.where(ok & ~dead, g.abs() * (p * (1.0 + z.abs() + l.abs()) + onehot), torch.zeros_like(p))
    return Ref(v[:, :m], M[:, :m], "ce_bwd"), Ref(v[:, m:], M[:, m:], "ce_bwd")


# ---- the cases of tests/test_ce_ext_gpu.py ----------------------------------------------------------------------------------------
TG = [(1, 1), (2, 2), (4, 4), (3, 5), (16, 16)]          # (t, group); n = t * group
MS = [1, 7, 64, 257, 1500]                                # m: block boundary inside a wave, at a wave edge, past the 256-thread trip
MASK, SCALE = -10000.0, 20.0                              # the reference's mask and 1 / temp at temp = 0.05


def case(t, group, m, seed=0):
    """cosine-like logits (|x| <= 1, as the normalised GEMMs give) with the planted rows, each planted once where n allows:

        row 0        logits of +-80 before the scale (max subtraction)
        row 1        all logits equal
        row 2        a label in block B (not the masked column when t > 1)
        row 3        a label out of range (m + t); row 4: a negative label
        row 5        the masked column holds the row's largest raw logit (n <= 5: row min(2, n - 1) instead)
    rows beyond n are not planted, and n == 1 keeps its only row random apart from the masked maximum.  Labels otherwise uniform
    in block A.  -> (la, lb, labels, grow)"""
    n = t * group
    g = HH.gen(1000 * t + 10 * group + m + seed)
    la = (torch.rand(n, m, generator=g) * 2 - 1).float()
    lb = (torch.rand(n, t, generator=g) * 2 - 1).float()
    labels = torch.randint(0, m, (n,), generator=g)
    grow = torch.randn(n, generator=g).float()

    def planted(r):
        return r < n
    if planted(0) and n > 1:
        la[0] = torch.where(torch.arange(m) % 2 == 0, torch.tensor(80.0), torch.tensor(-80.0))
        lb[0] = -80.0
    if planted(1):
        la[1] = 0.37
        lb[1] = 0.37
    if planted(2):
        col = (2 // group + 1) % t                       # another identity's column when there is one
        labels[2] = m + col
    if planted(3):
        labels[3] = m + t
    if planted(4):
        labels[4] = -1
    r = 5 if planted(5) else min(2, n - 1)               # n = 4: row 2, whose label sits in the OTHER column of block B
    lb[r, r // group] = 3.0                              # above every |x| <= 1 of the row
    assert float(lb[r, r // group]) > float(la[r].max()) and float(lb[r].max()) == 3.0
    return la.contiguous(), lb.contiguous(), labels, grow
