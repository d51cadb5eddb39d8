"""ctypes binding of libgnx.so (include/gnx.h) -- the only way the package reaches the GPU.

There is deliberately NO fallback: if the library is missing or a call fails, an Exception
is raised.  Nothing here imports the CPU oracle.
"""
from __future__ import annotations

import ctypes
import os
from ctypes import POINTER, c_char_p, c_double, c_float, c_int, c_int64, c_uint64, c_void_p

_HERE = os.path.dirname(os.path.abspath(__file__))
ABI_VERSION = 900         # include/gnx.h GNX_ABI_VERSION: the header this binding was written against
# GNX_LIBRARY: another build of the same library (the tuning build of tools/, `make TUNING=1` -> lib/tune/libgnx.so)
LIB_PATH = os.environ.get("GNX_LIBRARY") or os.path.join(os.path.dirname(_HERE), "lib", "libgnx.so")

NORM = {"none": 0, "symmetric": 1, "bipartite": 2}
EYE = {"none": 0, "before": 1, "after": 2}
ACT_NONE, ACT_RELU, ACT_SKIP_EMPTY = 0, 1, 256
ACT_LEAKY = 2             # tf.nn.leaky_relu at slope 0.2: gnx_ngcf_step and gnx_ngcf_back_gate only
HALO_ALL, HALO_PULL, HALO_PUSH = 0, 1, 2
RESERVE_TRANSPOSED, RESERVE_K_LOOP, RESERVE_TRAIN_GATHER, RESERVE_GATHER_HINTS = 1, 2, 4, 8
ORD_X, ORD_OUT = 1, 2     # `order` of the _ord training entries: X stored in the handle's gather order / the result written in it

# name -> (restype, argtypes); must list every symbol include/gnx.h declares
SIGNATURES = {
    "gnx_last_error": (c_char_p, []),
    "gnx_version": (c_int, []),
    "gnx_graph_create_coo": (c_int, [c_int64, c_int64, c_int64, c_void_p, c_void_p, c_void_p, POINTER(c_void_p)]),
    "gnx_graph_create_csr": (c_int, [c_int64, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, POINTER(c_void_p)]),
    "gnx_graph_destroy": (c_int, [c_void_p]),
    "gnx_graph_info": (c_int, [c_void_p, POINTER(c_int64), POINTER(c_int64), POINTER(c_int64), POINTER(c_int64)]),
    "gnx_graph_hub_rows": (c_int, [c_void_p, POINTER(c_int64), POINTER(c_int64)]),
    "gnx_graph_csr": (c_int, [c_void_p, POINTER(c_void_p), POINTER(c_void_p), POINTER(c_void_p)]),
    "gnx_graph_export": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "gnx_graph_normalize": (c_int, [c_void_p, c_int, c_int, c_float, c_uint64, c_uint64, c_void_p, c_void_p, c_void_p]),
    "gnx_graph_normalize_t": (c_int, [c_void_p, c_int, c_int, c_float, c_uint64, c_uint64, c_void_p, c_void_p, c_void_p]),
    "gnx_graph_reserve": (c_int, [c_void_p, c_int64, c_int, c_void_p]),
    "gnx_graph_enable_entry_dropout": (c_int, [c_void_p, c_void_p]),
    "gnx_graph_set_row_window": (c_int, [c_void_p, c_int64, c_void_p]),
    "gnx_graph_set_gather_hints": (c_int, [c_void_p, c_int64, c_void_p]),
    "gnx_graph_gather_hints": (c_int, [c_void_p, POINTER(c_void_p), POINTER(c_int64), POINTER(c_int64)]),
    "gnx_graph_set_pendant_elision": (c_int, [c_void_p, c_int, c_void_p]),
    "gnx_graph_pendant_elision": (c_int, [c_void_p, POINTER(c_int64), POINTER(c_void_p), POINTER(c_int)]),
    "gnx_graph_set_dropout_counter": (c_int, [c_void_p, c_void_p]),
    "gnx_graph_set_block": (c_int, [c_void_p, c_int64, c_int64, c_void_p, c_void_p]),
    "gnx_graph_colsum": (c_int, [c_void_p, c_float, c_uint64, c_uint64, c_void_p, c_void_p]),
    "gnx_graph_colsum_streams": (c_int, [c_void_p, c_float, c_uint64, c_uint64, c_int, c_void_p, c_void_p]),
    "gnx_degree_scale": (c_int, [c_void_p, c_int64, c_int, c_int, c_void_p]),
    "gnx_graph_scale_values": (c_int, [c_void_p, c_float, c_uint64, c_uint64, c_void_p, c_void_p, c_void_p, c_void_p]),
    "gnx_spmm": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_int64, c_float, c_float,
                         c_int, c_void_p, c_int64, c_void_p]),
    "gnx_spmm_t": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_int64, c_float, c_float,
                           c_int, c_void_p, c_int64, c_void_p]),
    "gnx_spmm_scatter": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_int64, c_float, c_float,
                                 c_int, c_void_p, c_void_p, c_int64, c_void_p]),
    "gnx_spmm_dropped": (c_int, [c_void_p, c_void_p, c_float, c_uint64, c_uint64, c_int, c_void_p, c_int64, c_int64, c_void_p, c_int64,
                                 c_float, c_float, c_int, c_void_p, c_int64, c_void_p]),
    "gnx_spmm_dropped_chained": (c_int, [c_void_p, c_void_p, c_float, c_uint64, c_uint64, c_int, c_void_p, c_void_p, c_int64, c_int64, c_void_p,
                                         c_int64, c_float, c_float, c_int, c_void_p, c_int64, c_void_p]),
    "gnx_spmm_dropped_back": (c_int, [c_void_p, c_void_p, c_float, c_uint64, c_uint64, c_int, c_void_p, c_void_p, c_int64, c_int64, c_void_p,
                                      c_int64, c_float, c_float, c_void_p, c_int64, c_float, c_void_p, c_int64, c_int, c_void_p]),
    "gnx_graph_gather_order": (c_int, [c_void_p, POINTER(c_void_p), POINTER(c_void_p)]),
    "gnx_spmm_dropped_chained_ord": (c_int, [c_void_p, c_void_p, c_float, c_uint64, c_uint64, c_int, c_void_p, c_void_p, c_int64, c_int64,
                                             c_void_p, c_int64, c_float, c_float, c_int, c_void_p, c_int64, c_int, c_void_p]),
    "gnx_spmm_dropped_back_ord": (c_int, [c_void_p, c_void_p, c_float, c_uint64, c_uint64, c_int, c_void_p, c_void_p, c_int64, c_int64,
                                          c_void_p, c_int64, c_float, c_float, c_void_p, c_int64, c_float, c_void_p, c_int64, c_int, c_int,
                                          c_void_p]),
    "gnx_spmm_rows": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_int64, c_float, c_float, c_int,
                              c_void_p, c_void_p, c_int64, c_void_p]),
    "gnx_spmm_tv": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_int64, c_float, c_float,
                            c_int, c_void_p, c_int64, c_void_p]),
    "gnx_graph_permute_values_t": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p]),
    "gnx_ppr_step": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_int64, c_int, c_void_p, c_void_p]),
    "gnx_appnp_propagate": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_int, c_int64, c_void_p, c_void_p,
                                    c_void_p]),
    "gnx_appnp_propagate_act": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_int, c_int64, c_int, c_void_p, c_void_p,
                                        c_void_p]),
    "gnx_cast_bf16": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_void_p, c_int64, c_void_p]),
    "gnx_spmm_bf16": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_int64, c_float, c_float,
                              c_int, c_void_p, c_int, c_int64, c_void_p]),
    "gnx_spmm_rows_bf16": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_int64, c_float, c_float, c_int,
                                   c_void_p, c_void_p, c_int, c_int64, c_void_p]),
    "gnx_halo_pack_bf16": (c_int, [c_void_p, c_int, c_void_p, c_int64, c_int64, c_void_p, c_int64, c_void_p]),
    "gnx_halo_exchange_bf16": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int64, c_void_p]),
    "gnx_appnp_propagate_bf16": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_int, c_int64, c_int, c_void_p, c_void_p,
                                         c_void_p]),
    "gnx_spmm_dropped_chained_bf16": (c_int, [c_void_p, c_void_p, c_float, c_uint64, c_uint64, c_int, c_void_p, c_void_p, c_int64, c_int64,
                                              c_void_p, c_int64, c_float, c_float, c_int, c_void_p, c_int, c_int64, c_void_p]),
    "gnx_spmm_dropped_back_bf16": (c_int, [c_void_p, c_void_p, c_float, c_uint64, c_uint64, c_int, c_void_p, c_void_p, c_int64, c_int64,
                                           c_void_p, c_int64, c_float, c_float, c_void_p, c_int64, c_float, c_void_p, c_int64, c_int,
                                           c_void_p]),
    "gnx_halo_plan_create": (c_int, [c_int, c_int, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, POINTER(c_void_p)]),
    "gnx_halo_plan_destroy": (c_int, [c_void_p]),
    "gnx_halo_plan_layout": (c_int, [c_void_p, POINTER(c_int64), POINTER(c_int64), POINTER(c_int64), POINTER(c_int64), c_void_p, c_void_p,
                                     c_void_p]),
    "gnx_halo_pack": (c_int, [c_void_p, c_int, c_void_p, c_int64, c_int64, c_void_p, c_int64, c_void_p]),
    "gnx_halo_exchange": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int64, c_void_p]),
    "gnx_halo_bind_rccl": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p]),
    "gnx_gather_rows32": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_int64, c_void_p, c_int64, c_void_p]),
    "gnx_gather_rows": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_int64, c_void_p, c_int64, c_void_p]),
    "gnx_gcnii_step": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_int64, c_void_p, c_int64, c_int, c_void_p,
                               c_void_p, c_void_p]),
    "gnx_gcnii_step_bf16": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_int64, c_void_p, c_int64, c_int, c_void_p,
                                    c_int, c_void_p, c_void_p]),
    "gnx_gcnii_step_back": (c_int, [c_void_p, c_void_p, c_void_p, c_float, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_float,
                                    c_void_p, c_void_p, c_void_p]),
    "gnx_gcnii_step_drop": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_int64, c_void_p, c_int64, c_int, c_double, c_uint64,
                                    c_uint64, c_void_p, c_void_p, c_void_p]),
    "gnx_feature_dropout": (c_int, [c_void_p, c_void_p, c_int64, c_int64, c_int64, c_void_p, c_double, c_uint64, c_uint64, c_void_p, c_int64,
                                    c_void_p]),
    "gnx_feature_dropout_back": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_int64, c_int64, c_double, c_uint64, c_uint64,
                                         c_int, c_void_p, c_int64, c_void_p]),
    "gnx_gcnii_step_train_bf16": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_int64, c_void_p, c_int64, c_int, c_double,
                                          c_uint64, c_uint64, c_void_p, c_int, c_void_p, c_void_p, c_void_p]),
    "gnx_feature_dropout_back_bf16": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_int64, c_int64, c_double, c_uint64, c_uint64,
                                              c_int, c_void_p, c_int64, c_void_p, c_int64, c_void_p]),
    "gnx_gcnii_step_back_bf16": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_int64, c_void_p, c_int64, c_void_p, c_void_p,
                                         c_float, c_void_p, c_void_p, c_void_p]),
    "gnx_gcnii_wgrad": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_int64,
                                c_void_p]),
    "gnx_gcnii_wgrad_bf16": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_int64,
                                     c_void_p]),
    "gnx_gcnii_step_drop_bf16": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_int64, c_void_p, c_int64, c_int, c_double,
                                         c_uint64, c_uint64, c_void_p, c_int, c_void_p, c_void_p]),
    "gnx_gcnii_step_spectral": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_int64, c_void_p, c_int64, c_void_p, c_int, c_double,
                                        c_uint64, c_uint64, c_void_p, c_void_p, c_void_p, c_void_p]),
    "gnx_gcnii_spectral_back": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_int64, c_int, c_double, c_uint64, c_uint64, c_void_p,
                                        c_int64, c_void_p, c_void_p, c_int64, c_void_p]),
    "gnx_gcnii_step_dropped": (c_int, [c_void_p, c_void_p, c_float, c_uint64, c_uint64, c_void_p, c_void_p, c_float, c_int64, c_void_p, c_int64,
                                       c_int, c_double, c_uint64, c_uint64, c_void_p, c_void_p, c_void_p]),
    "gnx_gcnii_step_back_dropped": (c_int, [c_void_p, c_void_p, c_float, c_uint64, c_uint64, c_void_p, c_float, c_int64, c_void_p, c_int64,
                                            c_void_p, c_void_p, c_float, c_void_p, c_void_p, c_void_p]),
    "gnx_gcn_step": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_int64, c_int64, c_void_p, c_int, c_double, c_uint64,
                             c_uint64, c_void_p, c_int64, c_void_p, c_void_p, c_void_p]),
    "gnx_gcn_step_dropped": (c_int, [c_void_p, c_void_p, c_float, c_uint64, c_uint64, c_void_p, c_int64, c_int64, c_void_p, c_int64, c_int64,
                                     c_void_p, c_int, c_double, c_uint64, c_uint64, c_void_p, c_int64, c_void_p, c_void_p, c_void_p]),
    "gnx_gcn_step_back": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_int64, c_int64, c_void_p, c_int64, c_void_p,
                                  c_int64, c_void_p]),
    "gnx_gcn_step_back_dropped": (c_int, [c_void_p, c_void_p, c_float, c_uint64, c_uint64, c_void_p, c_int64, c_int64, c_void_p, c_int64,
                                          c_int64, c_void_p, c_int64, c_void_p, c_int64, c_void_p]),
    "gnx_step_spectral_gcn": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_int64, c_int64, c_void_p, c_int, c_double,
                                      c_uint64, c_uint64, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p]),
    "gnx_step_spectral_gcn_dropped": (c_int, [c_void_p, c_void_p, c_float, c_uint64, c_uint64, c_void_p, c_int64, c_int64, c_void_p, c_int64,
                                              c_int64, c_void_p, c_int, c_double, c_uint64, c_uint64, c_void_p, c_int64, c_void_p, c_void_p,
                                              c_void_p, c_void_p]),
    "gnx_ngcf_step": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_int64, c_void_p, c_void_p,
                              c_int, c_double, c_uint64, c_uint64, c_int, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_int64,
                              c_void_p]),
    "gnx_ngcf_back_gate": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_int64, c_int, c_double,
                                   c_uint64, c_uint64, c_void_p, c_void_p, c_int64, c_void_p]),
    "gnx_step_back_ngcf": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_int, c_double,
                                   c_uint64, c_uint64, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_void_p,
                                   c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_int64,
                                   c_void_p]),
    "gnx_step_back_wide_ngcf": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_int, c_double,
                                        c_uint64, c_uint64, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_void_p,
                                        c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_int64,
                                        c_void_p]),
    "gnx_step_wide_ngcf": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_int64, c_void_p,
                                   c_void_p, c_int, c_double, c_uint64, c_uint64, c_int, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p,
                                   c_int64, c_void_p]),
    "gnx_dense": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_void_p, c_int64, c_int64, c_void_p, c_int, c_void_p, c_int64,
                          c_void_p]),
    "gnx_dense_wgrad": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_int64, c_void_p]),
    "gnx_dense_drop": (c_int, [c_void_p, c_void_p, c_int64, c_int64, c_int64, c_void_p, c_int64, c_int64, c_void_p, c_int, c_double, c_uint64,
                               c_uint64, c_double, c_uint64, c_uint64, c_void_p, c_int64, c_void_p]),
    "gnx_dense_wgrad_drop": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_int64, c_int64, c_int64, c_double, c_uint64, c_uint64,
                                     c_void_p, c_void_p, c_int64, c_void_p]),
    "gnx_node_ce": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p]),
    "gnx_node_ce_backward": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_int64,
                                     c_void_p]),
    "gnx_node_argmax": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_void_p, c_int64, c_void_p, c_void_p]),
    "gnx_edge_scores": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_void_p]),
    "gnx_edge_scores_backward": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_int64,
                                         c_void_p]),
    "gnx_sample_negatives": (c_int, [c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_int64, c_int64, c_uint64, c_uint64, c_void_p, c_void_p,
                                     c_void_p]),
    "gnx_edge_plan_bytes": (c_int64, [c_int64]),
    "gnx_edge_plan": (c_int, [c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p]),
    "gnx_edge_sorted_work_floats": (c_int64, [c_int64, c_int64]),
    "gnx_edge_scores_backward_sorted": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_int64,
                                                c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p]),
    "gnx_rank_candidates_bytes": (c_int64, [c_int64, c_int64, c_int64, c_int64, c_int64]),
    "gnx_rank_candidates": (c_int, [c_void_p, c_void_p, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_int64,
                                    c_void_p, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                    c_void_p, c_void_p, c_void_p, c_int64, c_void_p]),
    "gnx_signal_project": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_void_p, c_int, c_void_p, c_void_p]),
    "gnx_signal_spmv": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_float, c_float, c_void_p, c_void_p]),
    "gnx_signal_ppr": (c_int, [c_void_p, c_void_p, c_void_p, c_float, c_int, c_void_p, c_void_p, c_void_p]),
    "gnx_signal_smoothness": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "gnx_signal_smoothness_back": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "gnx_signal_uniform": (c_int, [c_void_p, c_int64, c_float, c_uint64, c_uint64, c_void_p, c_void_p]),
    "gnx_linear_combination": (c_int, [c_int, c_void_p, c_void_p, c_int64, c_void_p, c_void_p]),
    "gnx_stream_read": (c_int, [c_void_p, c_int64, c_void_p, c_void_p]),
    "gnx_stream_copy": (c_int, [c_void_p, c_void_p, c_int64, c_void_p]),
    "gnx_probe_block_xcd": (c_int, [c_int64, c_void_p, c_void_p]),
    "gnx_graph_last_kernel": (c_char_p, [c_void_p]),
}

# entries added within ABI 0.9 that a library of the same minor version may lack: found by probing (has_symbol); their callers raise
PROBED = ("gnx_step_wide_ngcf", "gnx_step_back_wide_ngcf", "gnx_step_spectral_gcn", "gnx_step_spectral_gcn_dropped", "gnx_dense_drop",
          "gnx_dense_wgrad_drop", "gnx_signal_project", "gnx_signal_spmv", "gnx_signal_ppr", "gnx_signal_smoothness",
          "gnx_signal_smoothness_back", "gnx_signal_uniform")

_lib = None


def has_symbol(name: str) -> bool:
    """Whether the loaded library exports ``name`` (the entries of PROBED)."""
    return hasattr(lib(), name)


def lib():
    """Loads libgnx.so once; raises if it has not been built (no CPU fallback exists)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise Exception(f"gnntf: the HIP library {LIB_PATH} is missing -- build it with "
                            f"`make -C gnn-tf_amd/csrc` (or __graft_entry__.build()); there is no CPU fallback")
        handle = ctypes.CDLL(LIB_PATH)
        for name, (restype, argtypes) in SIGNATURES.items():
            if name in PROBED and not hasattr(handle, name):
                continue
            fn = getattr(handle, name)  # AttributeError if a declared symbol is not exported
            fn.restype = restype
            fn.argtypes = argtypes
        # the argument lists of several entries changed under the same names at 0.3 (include/gnx.h, GNX_ABI_VERSION): a library
        # of another minor version would be called with shifted arguments -- refused, not tried
        version = int(handle.gnx_version())
        if version // 100 != ABI_VERSION // 100:
            raise Exception(f"gnntf: {LIB_PATH} implements ABI {version}, this package binds ABI {ABI_VERSION}: rebuild the library "
                            f"(make -C gnn-tf_amd/csrc)")
        _lib = handle
    return _lib


def check(rc: int):
    if rc != 0:
        msg = lib().gnx_last_error()
        raise Exception((msg.decode() if msg else "") or f"libgnx error {rc}")


def ptr(t):
    """Device pointer of a torch tensor (None -> NULL)."""
    return None if t is None else c_void_p(t.data_ptr())


def current_stream():
    """The raw hipStream_t of torch's current stream on the current device (the cheap accessor: this sits on every launch)."""
    import torch
    return c_void_p(torch._C._cuda_getCurrentRawStream(torch.cuda.current_device()))


class on_device:
    """``with on_device(t.device):`` -- makes the tensor's device current for the launch; free when it already is
    (the usual case: one process per GPU)."""

    __slots__ = ("index", "prev")

    def __init__(self, device):
        self.index = device.index

    def __enter__(self):
        import torch
        self.prev = torch.cuda.current_device()
        if self.index is None:
            self.index = self.prev
        if self.prev != self.index:
            torch.cuda.set_device(self.index)

    def __exit__(self, *exc):
        if self.prev != self.index:
            import torch
            torch.cuda.set_device(self.prev)


def require_cuda(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise Exception("gnntf: the propagation path runs on the GPU only (tensor on %s); there is no CPU "
                            "fallback" % t.device)
