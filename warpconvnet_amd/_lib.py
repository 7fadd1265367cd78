"""ctypes binding of the C-ABI library ``libwcn_hip.so`` (declared in ``include/wcn.h``).

The library is built in-tree by ``make -C warpconvnet_amd/csrc`` (``__graft_entry__.build()``); this
module never falls back to another implementation: if the shared object is missing or a symbol is
absent, ``lib()`` raises.  Tensors cross the boundary as raw device pointers + sizes, the stream as
``torch.cuda.current_stream().cuda_stream`` (a ``hipStream_t``).
"""
import ctypes
import os
import subprocess
import threading
from ctypes import c_char_p, c_int, c_int32, c_int64, c_size_t, c_void_p
from typing import Optional

import torch

_CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc")
# WARPCONVNET_AMD_LIB: alternative build of the same library (e.g. the phase-stamp build `make prof`)
LIB_PATH = os.environ.get("WARPCONVNET_AMD_LIB") or os.path.join(_CSRC, "libwcn_hip.so")

WCN_F32, WCN_F16, WCN_BF16 = 0, 1, 2
WCN_ALGO_AUTO, WCN_ALGO_REF, WCN_ALGO_MFMA = 0, 1, 2
WCN_FLAG_TABLE_FULL, WCN_FLAG_COORD_RANGE, WCN_FLAG_PAIR_OVERFLOW, WCN_FLAG_DUPLICATE_COORD = 1, 2, 4, 8
WCN_FLAG_NEED_STRICT = 16
WCN_FLAG_ROW_OVERFLOW = 32
WCN_SLOT_X_FASTEST, WCN_SLOT_Z_FASTEST = 0, 1  # column order of a child table (csrc/resample.hip)
WCN_MASK_U8 = 3  # mask_dtype of wcn_resample_expand: a bool / uint8 mask
WCN_GRID_KEY_CELL, WCN_GRID_KEY_CORNER = 0, 1  # mode of wcn_grid_point_keys (csrc/grid.hip)
WCN_SEG_MOMENTS, WCN_SEG_RANGE, WCN_SEG_DOT = 0, 1, 2  # mode of wcn_seg_stats (csrc/segmented.hip)
WCN_SEG_ADD, WCN_SEG_SUB, WCN_SEG_MUL, WCN_SEG_DIV, WCN_SEG_NORM, WCN_SEG_NORM_BWD = 0, 1, 2, 3, 4, 5  # op of wcn_seg_apply
WCN_FPS_AUTO, WCN_FPS_RESIDENT, WCN_FPS_STREAMED = 0, 1, 2  # tier of wcn_fps (csrc/fps.hip)
WCN_ATTN_AUTO, WCN_ATTN_ONE_WAVE, WCN_ATTN_SHARED = 0, 1, 2  # variant of wcn_attn_varlen_kv_*_v (csrc/attn_varlen.hip)

_I32P = c_void_p  # all pointers travel as void*
_3I = c_int32 * 3
_EC_LISTS = [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_int32, c_int64, c_int64, c_int64, c_int32]

# name -> (restype, argtypes); one line per declaration in include/wcn.h
SIGNATURES = {
    "wcn_abi_version": (c_int, []),
    "wcn_status_string": (c_char_p, [c_int]),
    "wcn_hash_prepare": (c_int, [c_void_p, c_int64, c_void_p]),
    "wcn_hash_insert": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p]),
    "wcn_hash_search": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p]),
    "wcn_kmap_row_pitch": (c_int32, [c_int32]),
    "wcn_kmap_mask_words": (c_int32, [c_int32]),
    "wcn_kmap_num_blocks": (c_int64, [c_int64]),
    "wcn_kmap_probe": (
        c_int,
        [c_void_p, c_int64, c_void_p, c_int64, _3I, _3I, _3I, c_void_p, c_void_p, c_void_p],
    ),
    "wcn_batch_indexed_coords": (c_int, [c_void_p, c_int64, c_int32, c_void_p, c_int32, c_void_p, c_void_p]),
    "wcn_bn_workspace": (c_size_t, [c_int32]),
    "wcn_bn_max_channels": (c_int32, []),
    "wcn_bn_stats": (c_int, [c_void_p, c_int64, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "wcn_bn_stats_fold": (c_int, [c_void_p, c_int64, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, ctypes.c_float,
                                  ctypes.c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t,
                                  c_void_p]),
    "wcn_bn_fold": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, ctypes.c_float, c_int32, c_void_p, c_void_p, c_void_p,
                            c_void_p, c_void_p]),
    "wcn_bn_apply": (c_int, [c_void_p, c_int64, c_int32, c_int32, c_void_p, c_void_p, c_int32, c_void_p, c_void_p]),
    "wcn_bn_backward_reduce": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int32, c_int32, c_void_p, c_void_p,
                                       c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "wcn_bn_backward_apply": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int32, c_int32, c_void_p, c_void_p,
                                      c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "wcn_bn_apply_residual": (c_int, [c_void_p, c_void_p, c_int64, c_int32, c_int32, c_void_p, c_void_p, c_int32, c_void_p,
                                      c_void_p]),
    "wcn_bn_backward_reduce_masked": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int32, c_int32, c_void_p, c_void_p,
                                              c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "wcn_bn_backward_apply_masked": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int32, c_int32, c_void_p, c_void_p,
                                             c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "wcn_bn_train_forward": (c_int, [c_void_p, c_void_p, c_int64, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p,
                                     ctypes.c_float, ctypes.c_float, c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_size_t,
                                     c_void_p]),
    "wcn_bn_train_backward": (c_int, [c_void_p, c_void_p, c_void_p, c_int32, c_int64, c_int32, c_int32, c_void_p, c_void_p,
                                      c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "wcn_bn_train_backward_ld": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_int32, c_int64, c_int32, c_int32, c_void_p, c_void_p,
                                         c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "wcn_conv_bn_backward_ld": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_int32, c_void_p, c_void_p, c_int32, c_void_p,
                                        c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_void_p, c_void_p, c_void_p,
                                        c_void_p, c_void_p, c_void_p, c_size_t, c_int64, c_int64, c_int32, c_int32, c_int32, c_int32,
                                        c_void_p, c_size_t, c_void_p]),
    "wcn_conv_bn_backward_teams": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_int32, c_void_p, c_void_p, c_int32, c_void_p,
                                           c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_void_p, c_void_p, c_void_p,
                                           c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_int64, c_int64, c_int32, c_int32, c_int32,
                                           c_int32, c_void_p, c_size_t, c_void_p]),
    "wcn_conv_bn_backward": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_void_p, c_void_p, c_int32, c_void_p, c_void_p,
                                     c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_void_p,
                                     c_void_p, c_void_p, c_size_t, c_int64, c_int64, c_int32, c_int32, c_int32, c_int32, c_void_p,
                                     c_size_t, c_void_p]),
    "wcn_pool_gather": (c_int, [c_void_p, c_void_p, c_int64, c_int64, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p,
                                c_void_p, c_void_p]),
    "wcn_pool_gather_scaled": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int32, c_int32, c_int32, c_int32, c_void_p,
                                       c_void_p, c_void_p, c_void_p]),
    "wcn_pool_row_vec": (c_int, [c_void_p, c_void_p, c_int32, c_int32]),
    "wcn_pool_select": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int32, c_int32, c_int32, c_void_p, c_void_p]),
    "wcn_morton_code": (c_int, [c_void_p, c_int64, c_int32, c_void_p, c_void_p, c_void_p, c_void_p]),
    "wcn_kmap_counts_bytes": (c_size_t, [c_int64, c_int32]),
    "wcn_kmap_slab_bounds_offset": (c_int64, [c_int64, c_int32]),
    "wcn_kmap_binned_workspace": (c_size_t, [c_int64, c_int64]),
    "wcn_kmap_binned_supported": (c_int, [_3I, _3I]),
    "wcn_kmap_build_binned": (
        c_int,
        [c_void_p, c_int64, _3I, _3I, c_int64, c_int32, c_int32, c_void_p, c_size_t, c_void_p, c_void_p, c_void_p, c_void_p],
    ),
    "wcn_kmap_compact_supported": (c_int, [c_int32]),
    "wcn_kmap_densify": (c_int, [c_void_p, c_int64, c_int32, c_void_p, c_void_p]),
    "wcn_kmap_tally_sort_workspace": (c_size_t, [c_int64]),
    "wcn_kmap_tally_sort": (
        c_int,
        [c_void_p, c_void_p, c_int64, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t,
         c_void_p, c_void_p, c_int64, c_int64, c_int32, c_void_p, c_void_p, c_int64, c_void_p],
    ),
    "wcn_kmap_count": (c_int, [c_void_p, c_int64, c_int32, c_void_p, c_void_p]),
    "wcn_kmap_scan": (c_int, [c_void_p, c_int64, c_int32, c_void_p, c_void_p]),
    "wcn_kmap_scan_to_host": (c_int, [c_void_p, c_int64, c_int32, c_void_p, c_void_p, c_void_p, c_void_p]),
    "wcn_kmap_scatter": (
        c_int,
        [c_void_p, c_void_p, c_int64, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_int32, c_void_p],
    ),
    "wcn_kmap_cells_build": (c_int, [c_void_p, c_int64, c_int64, c_void_p, c_size_t, c_void_p, c_void_p, c_void_p]),
    "wcn_cells_stride_supported": (c_int, [_3I]),
    "wcn_cells_stride_tiles": (c_int64, [c_int64]),
    "wcn_cells_stride_count": (c_int, [c_void_p, c_int64, c_int64, c_void_p, _3I, c_void_p, c_void_p, c_int32, c_void_p,
                                       c_void_p]),
    "wcn_cells_stride_emit": (c_int, [c_void_p, c_int64, c_int64, c_void_p, _3I, c_void_p, c_void_p, c_void_p, c_void_p,
                                      c_void_p, c_void_p, c_void_p]),
    "wcn_kmap_probe_cells": (c_int, [c_void_p, c_int64, c_int64, c_void_p, c_int64, _3I, _3I, _3I, c_void_p, c_void_p,
                                     c_void_p]),
    "wcn_kmap_transpose": (c_int, [c_void_p, c_int64, c_int32, c_void_p, c_void_p]),
    "wcn_kmap_reverse": (
        c_int,
        [c_void_p, c_void_p, c_void_p, c_int32, c_int64, c_int64, c_void_p, c_void_p, c_void_p],
    ),
    "wcn_kmap_from_csr": (
        c_int,
        [c_void_p, c_void_p, c_void_p, c_int32, c_int64, c_int64, c_void_p, c_void_p, c_void_p],
    ),
    "wcn_mask_argsort_workspace": (c_size_t, [c_int64]),
    "wcn_mask_argsort": (c_int, [c_void_p, c_int32, c_int32, c_int64, c_void_p, c_void_p, c_size_t, c_void_p]),
    "wcn_mask_tile_order": (c_int, [c_void_p, c_int32, c_int32, c_int64, c_void_p, c_void_p, c_size_t, c_void_p]),
    "wcn_mfma_gather_supported": (c_int, [c_int32, c_int32, c_int32, c_int32]),
    "wcn_mfma_wgrad_supported": (c_int, [c_int32, c_int32, c_int32]),
    "wcn_conv_identity_supported": (c_int, [c_int32, c_int32, c_int32]),
    "wcn_dense_rows_supported": (c_int, [c_int32, c_int32, c_int32]),
    "wcn_dense_rows": (
        c_int,
        [c_void_p, c_int32, c_void_p, c_int32, c_int32, c_void_p, c_void_p, c_int64, c_int32, c_int32, c_int32, c_void_p],
    ),
    "wcn_packed_weight_bytes": (c_size_t, [c_int32, c_int32, c_int32, c_int32, c_int32]),
    "wcn_pack_weight": (
        c_int,
        [c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p, c_size_t, c_void_p],
    ),
    "wcn_pack_weight_f32": (
        c_int,
        [c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p, c_size_t, c_void_p],
    ),
    "wcn_pack_weight_pair_supported": (c_int, [c_int32, c_int32, c_int32, c_int32]),
    "wcn_conv_compact_table_supported": (c_int, [c_int32, c_int32, c_int32, c_int32]),
    "wcn_pack_weight_f32_pair": (c_int, [c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p, c_size_t, c_void_p, c_size_t,
                                         c_void_p]),
    "wcn_conv_gather_gemm": (
        c_int,
        [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int32, c_int32,
         c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p],
    ),
    "wcn_mfma_grouped_supported": (c_int, [c_int32, c_int32, c_int32, c_int32]),
    "wcn_pack_weight_grouped": (
        c_int,
        [c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p],
    ),
    "wcn_conv_gather_gemm_grouped": (
        c_int,
        [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int32, c_int32,
         c_int32, c_int32, c_int32, c_void_p],
    ),
    "wcn_conv_gather_gemm_f32out": (
        c_int,
        [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int32, c_int32,
         c_int32, c_int32, c_void_p],
    ),
    "wcn_conv_gather_gemm_fused": (
        c_int,
        [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int32,
         c_int64, c_int64, c_int32, c_int32, c_int32, c_int32, c_void_p],
    ),
    "wcn_colsum_workspace": (c_size_t, [c_int32]),
    "wcn_colsum": (c_int, [c_void_p, c_int64, c_int32, c_int32, c_void_p, c_void_p, c_size_t, c_void_p]),
    "wcn_conv_wgrad_workspace": (c_size_t, [c_int32, c_int32, c_int32, c_int32]),
    "wcn_conv_wgrad": (
        c_int,
        [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int32, c_int32, c_int32,
         c_int32, c_int32, c_void_p, c_size_t, c_void_p],
    ),
    "wcn_dwconv_gather": (
        c_int,
        [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int32, c_int32, c_int32, c_int32, c_void_p],
    ),
    "wcn_dwconv_wgrad_workspace": (c_size_t, [c_int32, c_int32]),
    "wcn_dwconv_wgrad": (
        c_int,
        [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int32, c_int32, c_int32,
         c_void_p, c_size_t, c_void_p],
    ),
    "wcn_radius_grid_count": (
        c_int,
        [c_void_p, c_void_p, c_void_p, ctypes.c_float * 3, ctypes.c_float, c_int32 * 3, c_void_p, c_int64, ctypes.c_float,
         c_void_p, c_void_p],
    ),
    "wcn_radius_grid_write": (
        c_int,
        [c_void_p, c_void_p, c_void_p, ctypes.c_float * 3, ctypes.c_float, c_int32 * 3, c_void_p, c_int64, ctypes.c_float,
         c_void_p, c_void_p, c_void_p, c_void_p],
    ),
    "wcn_knn_grid": (
        c_int,
        [c_void_p, c_void_p, c_void_p, ctypes.c_float * 3, ctypes.c_float, c_int32 * 3, c_void_p, c_int64, c_int32, c_void_p,
         c_void_p, c_void_p],
    ),
    "wcn_segment_reduce": (c_int, [c_void_p, c_void_p, c_int64, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p]),
    "wcn_pointconv_supported": (c_int, [c_int32] * 7),
    "wcn_pointconv_packed_floats": (c_int64, [c_int32] * 3),
    "wcn_pointconv_grad_floats": (c_int64, [c_int32] * 4),
    "wcn_pointconv_backward_workspace": (c_size_t, [c_int64, c_int32, c_int32, c_int32, c_int32, c_int32]),
    "wcn_pointconv_pack": (c_int, [c_void_p] * 10 + [c_int32] * 3 + [c_void_p, c_void_p]),
    "wcn_pointconv_edge_forward": (
        c_int,
        [c_void_p] * 5 + [c_int64] + [c_int32] * 4 + [c_void_p, c_int32, c_int32, ctypes.c_float, ctypes.c_float, c_int32,
                                                      c_int32, c_void_p, c_void_p],
    ),
    "wcn_pointconv_edge_backward": (
        c_int,
        [c_void_p] * 5 + [c_int64] + [c_int32] * 4 + [c_void_p, c_int32, c_int32, ctypes.c_float, ctypes.c_float, c_int32,
                                                      c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t,
                                                      c_void_p],
    ),
    "wcn_pointconv_edge_backward_peredge": (
        c_int,
        [c_void_p] * 5 + [c_int64] + [c_int32] * 4 + [c_void_p, c_int32, c_int32, ctypes.c_float, ctypes.c_float, c_int32,
                                                      c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t,
                                                      c_void_p],
    ),
    "wcn_pointconv_edge_forward_ragged": (
        c_int,
        [c_void_p] * 7 + [c_int64, c_int64] + [c_int32] * 3 + [c_void_p, c_int32, c_int32, ctypes.c_float, ctypes.c_float,
                                                               c_int32, c_void_p, c_void_p],
    ),
    "wcn_pointconv_edge_backward_ragged": (
        c_int,
        [c_void_p] * 7 + [c_int64, c_int64] + [c_int32] * 3 + [c_void_p, c_int32, c_int32, ctypes.c_float, ctypes.c_float,
                                                               c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                                               c_size_t, c_void_p],
    ),
    "wcn_attn_varlen_supported": (c_int, [c_int32, c_int32]),
    "wcn_attn_varlen_workspace_bytes": (c_size_t, [c_int64, c_int32]),
    "wcn_attn_varlen_fwd": (
        c_int,
        [c_void_p, c_void_p, c_int64, c_int64, c_int32, c_int32, c_int32, ctypes.c_float, c_int32, c_void_p, c_void_p,
         c_void_p],
    ),
    "wcn_attn_varlen_bwd": (
        c_int,
        [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int32, c_int32, c_int32, ctypes.c_float,
         c_int32, c_void_p, c_void_p, c_size_t, c_void_p],
    ),
    "wcn_attn_varlen_kv_splits": (c_int32, [c_int64, c_int32, c_int32, c_int32]),
    "wcn_attn_varlen_kv_workspace_bytes": (c_size_t, [c_int64, c_int64, c_int32, c_int32, c_int32]),
    "wcn_attn_varlen_kv_fwd": (
        c_int,
        [c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_int64, c_int64, c_int32, c_int32,
         c_int32, c_int32, ctypes.c_float, c_int32, c_void_p, c_void_p, c_void_p],
    ),
    "wcn_attn_varlen_kv_bwd": (
        c_int,
        [c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64,
         c_int64, c_int32, c_int32, c_int32, c_int32, ctypes.c_float, c_int32, c_void_p, c_int64, c_void_p, c_void_p, c_int64,
         c_int32, c_void_p, c_size_t, c_void_p],
    ),
    "wcn_attn_varlen_variant": (c_int32, [c_int64, c_int32, c_int32, c_int32, c_int32]),
    "wcn_attn_varlen_kv_fwd_v": (
        c_int,
        [c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_int64, c_int64, c_int32, c_int32,
         c_int32, c_int32, ctypes.c_float, c_int32, c_void_p, c_void_p, c_int32, c_void_p],
    ),
    "wcn_attn_varlen_kv_bwd_v": (
        c_int,
        [c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64,
         c_int64, c_int32, c_int32, c_int32, c_int32, ctypes.c_float, c_int32, c_void_p, c_int64, c_void_p, c_void_p, c_int64,
         c_int32, c_void_p, c_size_t, c_int32, c_void_p],
    ),
    "wcn_attn_varlen_k_splits": (c_int32, [c_int64, c_int32, c_int32, c_int32, c_int32]),
    "wcn_attn_varlen_ksplit_workspace_bytes": (c_size_t, [c_int64, c_int64, c_int32, c_int32, c_int32, c_int32, c_int32]),
    "wcn_attn_varlen_kv_fwd_s": (
        c_int,
        [c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_int64, c_int64, c_int32, c_int32,
         c_int32, c_int32, ctypes.c_float, c_int32, c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_size_t, c_void_p],
    ),
    "wcn_attn_varlen_kv_bwd_s": (
        c_int,
        [c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64,
         c_int64, c_int32, c_int32, c_int32, c_int32, ctypes.c_float, c_int32, c_void_p, c_int64, c_void_p, c_void_p, c_int64,
         c_int32, c_int32, c_void_p, c_size_t, c_int32, c_void_p],
    ),
    "wcn_rope_table": (c_int, [c_void_p, c_int32, c_int64, c_void_p, ctypes.c_float, c_void_p, c_int32, c_void_p, c_void_p]),
    "wcn_rope_table_axes": (c_int, [c_void_p, c_int32, c_int64, c_void_p, ctypes.c_float, c_void_p, _3I, c_void_p, c_void_p]),
    "wcn_qk_prologue_supported": (c_int, [c_int32, c_int32, c_int32]),
    "wcn_qk_prologue_workspace_bytes": (c_size_t, [c_int64, c_int32, c_int32]),
    "wcn_qk_prologue_fwd": (
        c_int,
        [c_void_p, c_int32, c_int64, c_int32, c_int32, c_void_p, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_int32,
         c_void_p, c_void_p],
    ),
    "wcn_qk_prologue_bwd": (
        c_int,
        [c_void_p, c_int32, c_void_p, c_int32, c_int64, c_int32, c_int32, c_void_p, c_int32, c_void_p, c_void_p, c_void_p,
         c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p],
    ),
    "wcn_adaln_supported": (c_int, [c_int32, c_int32]),
    "wcn_adaln_workspace_bytes": (c_size_t, [c_int64, c_int64, c_int32]),
    "wcn_adaln_fwd": (
        c_int,
        [c_void_p] * 5 + [c_int64, c_void_p, c_int64, c_int64, c_int32, ctypes.c_float, c_int32, c_void_p, c_void_p, c_void_p,
                          c_void_p],
    ),
    "wcn_adaln_bwd": (
        c_int,
        [c_void_p] * 6 + [c_int64, c_void_p, c_void_p, c_int64, c_int64, c_int32, c_int32] + [c_void_p] * 5 +
        [c_int64, c_void_p, c_size_t, c_void_p],
    ),
    "wcn_ln_act_supported": (c_int, [c_int32, c_int32]),
    "wcn_ln_act_workspace_bytes": (c_size_t, [c_int64, c_int32]),
    "wcn_ln_act_fwd": (c_int, [c_void_p] * 3 + [c_int64, c_int32, ctypes.c_float, c_int32, c_int32, c_void_p, c_void_p,
                                                 c_void_p]),
    "wcn_ln_act_bwd": (c_int, [c_void_p] * 5 + [c_int64, c_int32, c_int32, c_int32] + [c_void_p] * 4 + [c_size_t, c_void_p]),
    "wcn_ln_permute_fwd": (c_int, [c_void_p] * 4 + [c_int64, c_int32, ctypes.c_float, c_int32, c_void_p, c_void_p, c_void_p]),
    "wcn_ln_permute_bwd": (c_int, [c_void_p] * 5 + [c_int64, c_int32, c_int32] + [c_void_p] * 4 + [c_size_t, c_void_p]),
    "wcn_permute_add": (c_int, [c_void_p] * 4 + [c_int32, c_int64, c_int32, c_int32, c_void_p, c_void_p]),
    "wcn_channel_spread": (c_int, [c_void_p, c_void_p, c_int64, c_int32, c_int32, ctypes.c_float, c_int32, c_void_p,
                                   c_void_p]),
    "wcn_channel_fold": (c_int, [c_void_p, c_void_p, c_int64, c_int32, c_int32, ctypes.c_float, c_int32, c_void_p, c_void_p]),
    "wcn_window_group_max_segment": (c_int32, []),
    "wcn_window_group_workspace_bytes": (c_size_t, [c_int64, c_int64]),
    "wcn_window_group": (c_int, [c_void_p, c_int64, c_void_p, c_int32, _3I, _3I, _3I, _3I] + [c_void_p] * 7 +
                         [c_size_t, c_void_p]),
    "wcn_csr_chunk_rows": (c_int32, []),
    "wcn_voxel_keys": (c_int, [c_void_p, c_int64, c_void_p, c_int32, ctypes.c_float, c_void_p, c_void_p, c_void_p]),
    "wcn_voxel_map_workspace_bytes": (c_size_t, [c_int64]),
    "wcn_voxel_map": (c_int, [c_void_p, c_void_p, c_int64, c_int32] + [c_void_p] * 7 + [c_void_p, c_size_t, c_void_p]),
    "wcn_csr_gather_reduce_workspace_bytes": (c_size_t, [c_int64, c_int32, c_int32]),
    "wcn_csr_gather_reduce": (
        c_int,
        [c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_int64, c_int64, c_int32, c_int32, c_int32, c_int64, c_void_p,
         c_void_p, c_void_p, c_size_t, c_void_p],
    ),
    "wcn_row_spread": (c_int, [c_void_p, c_void_p, c_int64, c_int64, c_int32, c_void_p, c_int32, c_int64, c_int32, c_void_p,
                               c_void_p, c_int32, c_void_p, c_void_p]),
    "wcn_resample_pack": (c_int, [c_void_p, c_void_p, c_int64, c_int64, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32,
                                  c_void_p, c_void_p]),
    "wcn_resample_unpack": (c_int, [c_void_p, c_void_p, c_int64, c_int64, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32,
                                    c_int32, c_void_p, c_void_p]),
    "wcn_resample_expand_workspace": (c_size_t, [c_int64]),
    "wcn_resample_expand": (c_int, [c_void_p, c_void_p, c_int32, c_int64, c_int32, c_int32, c_int32, c_int32, c_void_p, c_size_t,
                                    c_void_p, c_int64, c_void_p, c_void_p, c_int32, c_void_p]),
    "wcn_mfma_wgrad_bias_supported": (c_int, [c_int32, c_int32, c_int32]),
    "wcn_conv_wgrad_bias": (
        c_int,
        [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int32, c_int32, c_int32,
         c_int32, c_int32, c_void_p, c_void_p, c_size_t, c_void_p],
    ),
    "wcn_conv_wgrad_teams": (
        c_int,
        [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int32, c_int32, c_int32,
         c_int32, c_int32, c_void_p, c_void_p, c_size_t, c_void_p],
    ),
    "wcn_wgrad_plan_host": (c_int, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p]),
    "wcn_lattice_chunk_rows": (c_int32, []),
    "wcn_hash128_insert": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_int32, c_void_p, c_void_p]),
    "wcn_hash128_search": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_int32, c_int32, c_void_p,
                                   c_void_p]),
    "wcn_permuto_simplex": (c_int, [c_void_p, c_int64, c_int32, ctypes.c_float * 6] + [c_void_p] * 6),
    "wcn_grid_corners": (c_int, [c_void_p, c_int64, c_int32] + [c_void_p] * 7),
    "wcn_lattice_map_workspace_bytes": (c_size_t, [c_int64]),
    "wcn_lattice_map": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int32] + [c_void_p] * 5 + [c_size_t, c_void_p]),
    "wcn_lattice_plan_items": (c_int64, [c_int64]),
    "wcn_lattice_plan_ints": (c_int64, [c_int64]),
    "wcn_lattice_plan": (c_int, [c_void_p, c_int64, c_int64, c_void_p, c_void_p]),
    "wcn_lattice_splat": (c_int, [c_void_p] * 4 + [c_int64, c_int64, c_int32, c_int32, ctypes.c_float] + [c_void_p] * 4),
    "wcn_lattice_blur": (c_int, [c_void_p] * 3 + [ctypes.c_float] * 3 + [c_int64, c_int32, c_void_p, c_void_p]),
    "wcn_lattice_slice": (c_int, [c_void_p] * 3 + [c_int64, c_int32, c_int64, c_int32, ctypes.c_float, c_void_p, c_void_p]),
    "wcn_lattice_max_grid": (c_int32, []),
    "wcn_lattice_row_grid": (c_int32, [c_int64, c_int32]),
    "wcn_bilateral_matvec": (c_int, [c_void_p, c_int32, c_int64, c_int32] + [ctypes.c_float] * 3 + [c_void_p, c_void_p,
                                                                                                   ctypes.c_float] + [c_void_p] * 5),
    "wcn_bilateral_pcg": (c_int, [c_void_p, c_int32, c_int64, c_int32] + [ctypes.c_float] * 3 + [c_void_p] * 3 + [ctypes.c_float] +
                          [c_void_p] * 5 + [c_int32, ctypes.c_double, c_void_p]),
    "wcn_bilateral_knn_weights": (c_int, [c_void_p] * 5 + [c_int64, c_int64, c_int32, c_int32, c_int32, ctypes.c_float,
                                                           ctypes.c_float, c_void_p, c_void_p]),
    "wcn_grid_max_grid": (c_int32, []),
    "wcn_grid_chunk_points": (c_int32, []),
    "wcn_grid_point_keys": (c_int, [c_void_p, c_int64, c_void_p, c_int32, _3I, ctypes.c_float * 3, ctypes.c_float * 3, c_int32,
                                    c_void_p, c_void_p, c_void_p]),
    "wcn_grid_sample": (c_int, [c_void_p, c_int64 * 5, _3I, c_int32, c_int32, c_int64, c_void_p, c_void_p, c_void_p, c_int64,
                                c_void_p, c_int64, c_int64, c_void_p]),
    "wcn_grid_sample_backward_workspace_bytes": (c_size_t, [c_int64, c_int32]),
    "wcn_grid_sample_backward": (c_int, [c_void_p, c_int64, c_int64, c_int64 * 5, _3I, c_int32, c_int32, c_int64, c_void_p,
                                         c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_size_t,
                                         c_void_p]),
    "wcn_seg_chunk_rows": (c_int32, []),
    "wcn_seg_max_grid": (c_int32, []),
    "wcn_seg_stats_workspace_bytes": (c_size_t, [c_int64, c_int64, c_int32, c_int32]),
    "wcn_seg_stats": (c_int, [c_int32] + [c_void_p] * 4 + [c_int64, c_int64, c_int32, c_int32] + [c_void_p] * 5 +
                      [c_size_t, c_void_p]),
    "wcn_seg_apply": (c_int, [c_int32] + [c_void_p] * 3 + [c_int32] + [c_void_p] * 7 + [c_int64, c_int64, c_int32, c_int32,
                                                                                       c_void_p, c_void_p]),
    "wcn_fps_resident_max_points": (c_int64, []),
    "wcn_fps_block_threads": (c_int32, []),
    "wcn_fps_blocks_per_segment": (c_int32, []),
    "wcn_fps_max_grid": (c_int32, []),
    "wcn_fps_workspace_bytes": (c_size_t, [c_int64, c_int64, c_int32]),
    "wcn_fps": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_int64, c_int32, c_int64, c_void_p, c_int32, c_void_p,
                        c_size_t, c_void_p, c_void_p]),
    "wcn_fdg_supported": (c_int, [c_int32, c_int32]),
    "wcn_fdg_workspace": (c_size_t, [c_int64]),
    "wcn_fdg_count": (c_int, [c_void_p, c_int32, c_void_p, c_int64, c_void_p, c_int32, c_void_p, c_size_t, c_void_p, c_void_p]),
    "wcn_fdg_emit": (c_int, [c_void_p, c_int32, c_void_p, c_void_p, c_int64, c_void_p, c_int32, c_void_p, c_int32, c_void_p,
                             c_int32, ctypes.c_float, ctypes.c_float * 3, c_void_p, c_size_t, c_int64, c_void_p, c_void_p,
                             c_void_p, c_void_p]),
    "wcn_pad_max_grid": (c_int32, []),
    "wcn_pad_block_threads": (c_int32, []),
    "wcn_pad_repack": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_int64, c_void_p, c_int64, c_int64,
                               c_int64, c_int32, ctypes.c_uint64, c_void_p]),
    "wcn_seg_bmm_max_channels": (c_int32, []),
    "wcn_seg_bmm_tile_rows": (c_int32, []),
    "wcn_seg_bmm_chunk_rows": (c_int32, []),
    "wcn_seg_bmm_workspace_bytes": (c_size_t, [c_int64, c_int64, c_int32, c_int32, c_int32]),
    "wcn_seg_bmm": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int32, c_int32, c_int32, c_int32, c_void_p,
                            c_void_p, c_size_t, c_void_p]),
    "wcn_seg_bmm_wgrad": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int32, c_int32, c_int32, c_void_p,
                                  c_void_p, c_size_t, c_void_p]),
    "wcn_edgeconv_max_channels": (c_int32, []),
    "wcn_edgeconv_sum_blocks": (c_int32, []),
    "wcn_edgeconv_arg_bytes": (c_int32, [c_int64]),
    "wcn_edgeconv_sums_workspace_bytes": (c_size_t, [c_int32]),
    "wcn_edgeconv_backward_input_workspace_bytes": (c_size_t, [c_int64, c_int32]),
    # every entry starts with the lists: P, ld_p, Q, ld_q, nbr, row_splits, k, num_edges, num_queries, num_inputs, channels
    "wcn_edgeconv_stats": (c_int, _EC_LISTS + [c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "wcn_edgeconv_forward": (c_int, _EC_LISTS + [c_void_p, c_void_p, ctypes.c_float, c_void_p, c_void_p, c_int32, c_void_p]),
    "wcn_edgeconv_backward_sums": (c_int, _EC_LISTS + [c_void_p] * 4 + [ctypes.c_float, c_void_p, c_void_p, c_int32, c_void_p,
                                                                        c_void_p, c_void_p, c_size_t, c_void_p]),
    "wcn_edgeconv_backward_query": (c_int, _EC_LISTS + [c_void_p] * 6 + [ctypes.c_float, c_void_p, c_void_p, c_int32, c_void_p,
                                                                         c_void_p]),
    "wcn_edgeconv_backward_input": (c_int, _EC_LISTS + [c_void_p] * 3 + [c_void_p] * 6 +
                                    [ctypes.c_float, c_void_p, c_void_p, c_int32, c_void_p, c_void_p, c_size_t, c_void_p]),
}

_LIB = None  # _GuardedLib


class _GuardedLib:
    """The loaded library with the reference bindings' device guard (`c10::cuda::CUDAGuard` in every pybind entry point):
    the C-ABI takes raw pointers and a stream, launches go to the CURRENT device, so a call whose tensors live on another
    GPU (model on cuda:1 while cuda:0 is current, several GPUs driven from one process) switches the device for the call.
    The device of a call is the one its stream handle was asked for (`stream_handle(device)`, evaluated as the last
    argument of every launching call); pure host entry points never pass through the switch."""

    def __init__(self, handle: ctypes.CDLL):
        self._h = handle

    def __getattr__(self, name):
        fn = getattr(self._h, name)
        argtypes = fn.argtypes or []
        if not argtypes or argtypes[-1] is not c_void_p or name in _HOST_ONLY or _single_gpu():
            setattr(self, name, fn)  # (one visible GPU: there is no other device to be current)
            return fn

        def guarded(*args, _fn=fn):
            dev = getattr(_CALL_DEVICE, "dev", None)
            if dev is None or dev == torch.cuda.current_device():
                return _fn(*args)
            with torch.cuda.device(dev):
                return _fn(*args)

        guarded.__name__ = name
        setattr(self, name, guarded)
        return guarded


def _single_gpu() -> bool:
    try:
        return torch.cuda.is_available() and torch.cuda.device_count() == 1
    except Exception:
        return False


_HOST_ONLY = {"wcn_status_string", "wcn_wgrad_plan_host"}
_CALL_DEVICE = threading.local()  # .dev = device index of the stream this THREAD asked for last (evaluated per call)


def build(verbose: bool = False) -> str:
    """Compile the HIP sources for gfx950 (cross-compiles without a GPU). Returns the .so path."""
    cmd = ["make", "-C", _CSRC, "-j", str(min(8, os.cpu_count() or 1))]
    res = subprocess.run(cmd, capture_output=True, text=True)
    if res.returncode != 0:
        raise RuntimeError(f"building libwcn_hip.so failed:\n{res.stdout[-4000:]}\n{res.stderr[-4000:]}")
    if verbose:
        print(res.stdout[-2000:])
    return LIB_PATH


def lib() -> ctypes.CDLL:
    """Load (once) and return the C-ABI library; raise loudly if it is not there."""
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} not found: the HIP extension is not built. Run "
                "`python -c 'import __graft_entry__ as g; g.build()'` (or `make -C warpconvnet_amd/csrc`). "
                "There is no CPU fallback for the HIP paths."
            )
        handle = ctypes.CDLL(LIB_PATH)
        for name, (restype, argtypes) in SIGNATURES.items():
            fn = getattr(handle, name)  # AttributeError if the symbol is missing
            fn.restype = restype
            fn.argtypes = argtypes
        _LIB = _GuardedLib(handle)
    return _LIB


def status_string(code: int) -> str:
    return lib().wcn_status_string(int(code)).decode()


def check(code: int, what: str) -> None:
    """Non-zero C status -> RuntimeError (reference convention: `backends.py:489-510`)."""
    if code != 0:
        raise RuntimeError(f"{what} error: {status_string(code)} ({code})")


def ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    if t is None:
        return None
    return t.data_ptr()


_RAW_STREAM = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def stream_handle(device: torch.device) -> int:
    """hipStream_t of the current PyTorch stream on ``device``.  Every C-ABI call needs it (~900 per MinkUNet iteration):
    the raw accessor skips building a ``torch.cuda.Stream`` object (≈ 6 us -> 0.3 us per call)."""
    idx = device.index
    if idx is None:
        idx = torch.cuda.current_device()
    _CALL_DEVICE.dev = idx
    if _RAW_STREAM is not None:
        return _RAW_STREAM(idx)
    return torch.cuda.current_stream(device).cuda_stream


def dtype_code(dtype: torch.dtype) -> int:
    if dtype == torch.float32:
        return WCN_F32
    if dtype == torch.float16:
        return WCN_F16
    if dtype == torch.bfloat16:
        return WCN_BF16
    raise TypeError(f"unsupported feature dtype {dtype} (supported: float32, float16, bfloat16)")


def torch_dtype(code: int) -> torch.dtype:
    return {WCN_F32: torch.float32, WCN_F16: torch.float16, WCN_BF16: torch.bfloat16}[code]


def i3(v) -> "ctypes.Array":
    return _3I(int(v[0]), int(v[1]), int(v[2]))


def require_gpu_tensor(t: torch.Tensor, name: str) -> None:
    if not t.is_cuda:
        raise RuntimeError(f"{name} must live on a GPU for the HIP path (got {t.device}); there is no CPU fallback")
    if not t.is_contiguous():
        raise RuntimeError(f"{name} must be contiguous")
