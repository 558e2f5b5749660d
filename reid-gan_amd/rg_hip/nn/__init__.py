"""Layer set of the hot path as RGModules (same constructor arguments, parameter names, default
initialisation and state_dict layout as the torch.nn layers the reference composes).

Fusion available to the network programs (all exact, no re-association beyond fp32 rounding):
  Conv2d / ConvTranspose2d : + bias, + activation in the MFMA epilogue
  BatchNorm               : normalise + affine (+ residual add) (+ activation) in one pass

This file is the namespace and nothing else: `rg_hip.nn.<name>` for every layer, defined in one submodule.

    _base    _pair, the convolution initialisation and geometry, the bias gradient
    conv     Conv2d, ConvTranspose2d, Linear, their fp8 branch; the (r,s)-major filter cache, KrscGroup, group_krsc
    norm     BatchNorm1d / 2d, DSBN1d / 2d, InstanceNorm1d / 2d, IBN; the deferred num_batches_tracked counter
    fold     convolution + eval-mode BatchNorm as one layer: FoldGroup, conv_bn_tf / conv_bn_tb, invalidate_folds
    sn       SNConv2d, sn_prepare
    layers   activations, Dropout, MaxPool2d, AvgPool2d, ReflectionPad2d, Sequential

Imports between them: conv, layers <- _base; sn <- _base, conv; fold <- conv, norm; norm stands alone.  No cycle.  From the rest
of rg_hip they import ops, tape, wcache and (conv, sn) lowp; rg_hip.tape and rg_hip.lowp therefore import this package inside the
functions that need it, not at their top.

Callers outside the package go through `rg_hip.nn.<name>` at call time, never through a submodule: tests replace conv_bn_tb on
THIS module, and that reaches the network programs only because they look it up here and nothing inside the package calls it.

Importing this package neither loads libreidgan_hip.so nor needs a GPU.
"""
from ..ops import ACT_NONE, ACT_RELU, ACT_LEAKY, ACT_TANH
from .conv import KrscGroup, group_krsc, Conv2d, ConvTranspose2d, Linear
from .norm import BatchNorm1d, BatchNorm2d, DSBN1d, DSBN2d, InstanceNorm1d, InstanceNorm2d, IBN, nbt_pending, nbt_add
from .fold import FoldGroup, invalidate_folds, lib_fold_chunk, conv_bn_tf, conv_bn_tb
from .sn import SNConv2d, sn_prepare
from .layers import ReLU, LeakyReLU, Tanh, Dropout, MaxPool2d, AvgPool2d, ReflectionPad2d, Sequential

# ---- underscore names that code outside the package reads (resnet_trunk, netgraph, fdgan/networks.py, the tests, tools/) ----------
from .norm import _BatchNorm, _DSBN
from .layers import _Act
from .fold import _fold_bn, _fold_of
from .conv import _KrscCache

# ---- the other module-level underscore names of the former single file: nothing outside reads them today, they stay reachable ----
from ._base import _pair, _geom_gflop, _bias_grad
from .conv import _f8_backward_operands
from .fold import _Fold, _foldable, _fold_key, _FOLD_IN_CAPTURE
