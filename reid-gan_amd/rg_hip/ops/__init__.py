"""Tensor-level wrappers over the C ABI: shape logic, output allocation (torch caching allocator),
stream hand-off.  No autograd here and no arithmetic in torch — every number is produced by a HIP
kernel of libreidgan_hip.so.  All functions require contiguous fp32 CUDA(HIP) tensors and raise
otherwise (there is deliberately no CPU path).

This file is the namespace and nothing else: `ops.<name>` for every wrapper, defined in the submodule of the kernel-library
unit(s) it calls.

    _base      library handle, ACT_* codes, device binding, the validators (_chk, _dense, _chk_rr), the two-pass list total,
               workspace, split-K counters
    streams    concurrent_stream and its hardware-queue probe, the weight-gradient side-stream session (side_*)
    conv       csrc/conv_*.hip: conv2d_fwd / dgrad / wgrad, linear_*
    norm       csrc/norm_*.hip: bn_*, instnorm_*, ibn_*, dsbn_*, the folded-BatchNorm helpers, channel_sum
    eltwise    csrc/eltwise.hip, bgemm.hip, resize.hip: act, axpby, fills, dropout, l2norm, channel copies, softmax, bgemm, bicubic
    gan        csrc/gan_extra.hip: avgpool2d, reflection padding, spectral normalisation
    pool       csrc/pool.hip, part_head.hip: maxpool, global average, GeM, part pooling, the multi-part head
    loss       csrc/loss.hip, verif_head.hip: the losses, the fused verification head
    retrieval  csrc/cm.hip, retrieval.hip, rerank.hip, rank_eval.hip, cmc_shot.hip, cascade.hip: cluster memory, kNN helpers, sort
               segments and label compaction (torch), re-ranking, CMC / mAP, the single-gallery-shot CMC, the cascade's pair
               scores and merge
    dbscan     csrc/dbscan.hip
    infomap    csrc/infomap.hip: the wrappers and the host-driven search
    kmeans     csrc/kmeans.hip: assign / tally / update / split and the host loop over them
    optimizer  csrc/optim.hip
    profile    the launch profiler
    datagen    csrc/datagen.hip: on-device input synthesis
    databank   csrc/databank.hip: batches gathered from the device-resident uint8 image bank, the host-checked draws

The names are re-exported BY VALUE, which is safe because shared state (_DEV, CAPTURE_GEN, CAPTURING, _SIDE, _ws_sizes, _HANDED,
_INLINE_SIDE, _CONST_FILL, _CLOCK, _PROFILING) is created in exactly one submodule and only ever mutated in place, and the RG_*
environment switches are read once at import and never assigned afterwards.

Callers outside this package go through `ops.<name>`, never through a submodule: tests replace bn_fold, fold_filters_multi,
linear_fwd, linear_dgrad and cm_update on THIS module (to count calls, or with CPU stand-ins), and that reaches every caller only
because all of them look the name up here and no wrapper inside the package calls these five.

`ops.dbscan`, `ops.infomap` and `ops.kmeans` are the functions; they replace the attributes the import system set for the submodules of the
same name (importlib.import_module("rg_hip.ops.dbscan") still returns the submodule).

Importing this package neither loads libreidgan_hip.so nor needs a GPU.
"""
from __future__ import absolute_import

from ._base import lib, ACT_NONE, ACT_RELU, ACT_LEAKY, ACT_TANH, CAPTURE_GEN, CAPTURING, splitk_inkernel, workspace
from .streams import concurrent_stream, side_inline, side_enable, side_begin, side_sync, side_join, side_worth, side_call
from .conv import conv_out_size, weights_to_krsc, conv2d_fwd, conv2d_dgrad, conv2d_wgrad, linear_fwd, linear_dgrad, linear_wgrad
from .norm import (bn_stats, bn_apply_fwd, bn_bwd_reduce, bn_train_fused_ok, bn_train_fwd_fused, bn_train_bwd_fused,
                   instnorm_fwd, instnorm_bwd, rows_sum_pair, ibn_fwd, ibn_bwd, dsbn_fwd, dsbn_bwd, bn_bwd_apply, bn_eval_bwd,
                   bn_fold, act_bwd_sum, bn_fold_wgrad, act_bwd_partial, fold_filters_multi, scale_rows, channel_sum)
from .eltwise import (act_fwd, act_bwd, axpby, add, scale, pair_cat, fill_, zeros, const_fill, sub_square_fwd, sub_square_bwd,
                      step_clock, advance_step_clock, dropout, l2norm_rows_fwd, l2norm_rows_bwd, l2norm_channels_fwd,
                      l2norm_channels_bwd, copy_channels, bicubic_normalize_fwd, bicubic_normalize_bwd, bgemm, softmax_rows_fwd,
                      softmax_rows_bwd, mix_rows_fwd, mix_rows_bwd, cat_channels, slice_channels)
from .gan import (avgpool2d_fwd, avgpool2d_bwd, reflection_pad_fusable, reflection_pad2d_fwd, reflection_pad2d_bwd,
                  spectral_norm_fwd, spectral_norm_fwd_multi, spectral_norm_bwd)
from .pool import (maxpool2d_fwd, maxpool2d_bwd, global_avgpool_fwd, global_avgpool_bwd, gem_pool_fwd, gem_pool_bwd,
                   part_pool_fwd, part_pool_bwd, mp_head_fwd, mp_head_bwd)
from .loss import (sigmoid_bce_fwd, sigmoid_bce_bwd, mse_const_fwd, mse_const_bwd, affine_relu_mean_fwd, affine_relu_mean_bwd,
                   grad_penalty_rows, l1_fwd, l1_bwd, l1_rows_fwd, l1_rows_bwd, mse_const_rows_fwd, mse_const_rows_bwd,
                   softmax_ce_fwd, softmax_ce_bwd, softmax_ce_ext_fwd, softmax_ce_ext_bwd, weighted_sum_fwd, weighted_sum_bwd,
                   verif_head_fwd, verif_head_bwd)
from .retrieval import (cm_update, normalize_listed_rows, topk_rows, row_sqsum, add_outer_terms, segment_mean, sorted_segments,
                        compact_labels, rerank_expand, rerank_weights, rerank_query_expand, rerank_columns, rerank_jaccard,
                        rerank_orig_dist, rerank_from_rank, rank_eval, CMC_SHOT_MAX_IDS, CMC_SHOT_MAX_REPEAT,
                        CMC_SHOT_DRAW_BYTES, CMC_SHOT_GLOBAL, CMC_SHOT_LDS_ROW, cmc_shot_regime, cmc_shot_order, cmc_shot_rank,
                        cmc_shot, PAIR_SCORE_MAX_C, PAIR_SCORE_MAX_D, PAIR_SCORE_MAX_Q,
                        CASCADE_MERGE_MAX_G, PAIR_VEC4, PAIR_SPLIT_K, pair_score_regime, pair_score, cascade_merge)
from .dbscan import dbscan_count, dbscan_fill, dbscan_neighbors, dbscan_components, dbscan_labels, dbscan_asymmetry, dbscan
from .infomap import (INFOMAP_MAX_N, INFOMAP_MAX_K, INFOMAP_FLOW_MAX_ITERS, INFOMAP_FLOW_BATCH, INFOMAP_SWEEP_CAP,
                      INFOMAP_LEVEL_CAP, INFOMAP_ROUND_CAP, infomap_links, infomap_flow, infomap_codelength, infomap_search,
                      infomap_labels, infomap)
from .kmeans import (KMEANS_MAX_N, KMEANS_MAX_K, KMEANS_MAX_D, kmeans_rand_perm, kmeans_assign, kmeans_tally, kmeans_update,
                     kmeans_split, kmeans)
from .optimizer import adam_advance, adam_step_dev, adam_step, sgd_step
from .profile import profile_enable, check_not_profiling, profile_reset, profile_collect
from .datagen import pose_maps, flip_pad_crop, erase_rects_
from .databank import (bank_lut, BankDraws, bank_draws, bank_reid_batch, bank_gan_batch, bank_pose_batch, FDDraws, fd_draws,
                       bank_fd_image_batch, bank_fd_pose_batch, FD_CROP_WHOLE, FD_CROP_STRIPS, FD_CROP_INTS, fd_crop_strip_width, fd_crop_regime,
                       FDCropDraws, fd_crop_draws, bank_fd_crop_batch)

# ---- underscore names that code outside the package reads (rg_hip.nn / netgraph / parallel / lowp, the tests, tools/) ------------
from ._base import _stream, _p, _chk, _pair, _ws_query, _ws_sizes
from .streams import _side_session, _SIDE
from .gan import _SNDesc
from .profile import _PROFILING
from .infomap import _infomap_leaf_units, _infomap_totals, _infomap_codelength_of

# ---- the other module-level underscore names of the former single file: nothing outside reads them today, they stay reachable ------
from ._base import _DEV, _bind_device, _dense, _chk_rr, _nchw, _same_size, _eps32, _list_total, _SPLITK_INKERNEL, _Workspace, _ws
from .streams import _HANDED, _PROBE_US, _share_a_queue, _INLINE_SIDE, _SideSession, _SIDE_MIN_US
from .eltwise import _CONST_FILL, _CLOCK
from .loss import _loss_ws, _verif_vec
from .retrieval import _pair_vec
from .dbscan import _chk_dbscan_matrix, _chk_dbscan_lists, _nbr_ptr
from .infomap import _chk_infomap_table, _chk_infomap_graph, _infomap_level, _infomap_aggregate
from .kmeans import _chk_kmeans_shape, _row_sqsum
from .databank import _chk_bank, _chk_draws, _chk_lut, _chk_fd_draws
