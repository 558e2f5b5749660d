"""The seeded inputs of tests/golden/reference_siamese.npz: features for an identity base model, the verification head's parameters
and running statistics, and the pair labels.  Shared by make_golden_siamese.py (which runs the reference's own modules on them) and
tests/test_verif_hostmodel_cpu.py (which runs the host model on the same tensors).  Plain data, no reference code."""
import torch

CASES = {"b8": (8, 48, 2), "b33": (33, 100, 2)}          # (B, D, C)
QUANTITIES = ("logits", "loss", "prec", "df1", "df2", "dW", "dbias", "dgamma", "dbeta", "running_mean", "running_var")


def inputs(name):
    """float32: f1, f2 [B, D]; W [C, D], bias [C], gamma, beta [D]; rm, rv [D]; targets int64 [B].  The classifier weights are
    normal(0, 0.05): with the reference's own 0.001 every logit is a rounding away from its neighbour and the argmax of a row
    could differ between float32 and float64"""
    B, D, C = CASES[name]
    g = torch.Generator().manual_seed(20260000 + 1000 * B + D)
    f1, f2 = torch.randn(B, D, generator=g), torch.randn(B, D, generator=g)
    return {"f1": f1, "f2": f2, "W": torch.randn(C, D, generator=g) * 0.05, "bias": torch.randn(C, generator=g) * 0.1,
            "gamma": torch.rand(D, generator=g) * 0.6 + 0.7, "beta": torch.randn(D, generator=g) * 0.1,
            "rm": torch.rand(D, generator=g) * 2.0, "rv": torch.rand(D, generator=g) * 4.0 + 2.0,
            "targets": torch.randint(0, C, (B,), generator=g)}
