"""Optimizer steps (csrc/optim.hip)."""
from __future__ import absolute_import

from ._base import _p, _stream, lib


# ------------------------------------------------------------------------------------------------
# optimizers
# ------------------------------------------------------------------------------------------------
def adam_advance(state, beta1, beta2):
    lib.rg_adam_advance(_p(state), beta1, beta2, _stream())


def adam_step_dev(p, g, m, v, lr, beta1, beta2, eps, weight_decay, state, grad_scale=1.0):
    lib.rg_adam_step_dev(_p(p), _p(g), _p(m), _p(v), p.numel(), lr, beta1, beta2, eps, weight_decay, _p(state), grad_scale,
                         _stream())


def adam_step(p, g, m, v, lr, beta1, beta2, eps, weight_decay, step, grad_scale=1.0):
    lib.rg_adam_step(_p(p), _p(g), _p(m), _p(v), p.numel(), lr, beta1, beta2, eps, weight_decay, step, grad_scale,
                     _stream())


def sgd_step(p, g, buf, lr, momentum, weight_decay, first_step, grad_scale=1.0):
    lib.rg_sgd_step(_p(p), _p(g), _p(buf), p.numel(), lr, momentum, weight_decay, int(first_step), grad_scale, _stream())
