"""ctypes binding of libvad_amd.so (include/vad_amd.h).

torch is imported first so that libamdhip64.so.7 resolves to the copy torch
already loaded: the library and PyTorch then share one HIP runtime, one
device context and the same streams.  There is no fallback: if the library
is missing or a call fails, an exception is raised.
"""
from __future__ import annotations

import ctypes
import os

import torch  # noqa: F401  (load torch's HIP runtime before ours)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("VAD_AMD_LIB", os.path.join(_HERE, "lib", "libvad_amd.so"))

VAD_OK = 0
VAD_EINVAL = -1
VAD_EUNSUPPORTED = -2
VAD_ENOMEM = -3
VAD_ERCCL = -4
FEAT_ANALYSER = 0
FEAT_OFFLINE = 1
FFN_EXACT_F32 = 0
FFN_SPLIT_F16 = 1
TREE_WALK_AUTO = 0
TREE_WALK_GLOBAL = 1
LABEL_NO_HOP = 254
LABEL_INIT = 253
CSV_TILE = 4096
CSV_CARRY_PASS = 256
CSV_MAX_LINE = 4096
CSV_MAX_COLS = 2048
CSV_MAX_USED = 1024
CSV_ROW_HOST = 1
CSV_ROW_MALFORMED = 2
CSV_ROW_LABEL = 4
SIMPLE_MAX_NOISE = 64
SCORE_MAX_CLASSES = 8
SCORE_MAX_BINS = 4096

c_i32, c_i64, c_vp, c_sz = ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p, ctypes.c_size_t
c_int, c_f32 = ctypes.c_int, ctypes.c_float

# name -> (restype, argtypes); every symbol include/vad_amd.h declares
SIGNATURES = {
    "vad_version": (ctypes.c_char_p, []),
    "vad_n_frames": (c_i64, [c_i64, c_i32, c_i32]),
    "vad_mfcc_plan_create": (c_int, [c_vp, c_i32, c_i32, c_i32, c_i32, c_vp]),
    "vad_mfcc_plan_destroy": (c_int, [c_vp]),
    "vad_mfcc_plan_variant": (c_i32, [c_vp]),
    "vad_mfcc_plan_set_variant": (c_int, [c_vp, c_i32]),
    "vad_mfcc_plan_set_window": (c_int, [c_vp, c_vp, c_i32]),
    "vad_preemphasis_f32": (c_int, [c_vp, c_vp, c_i64, c_i64, c_i64, ctypes.c_float, c_vp]),
    "vad_spec_f32": (c_int, [c_vp, c_vp, c_i64, c_i32, c_i64, c_vp, c_vp]),
    "vad_mfcc_f32": (c_int, [c_vp, c_vp, c_i64, c_i32, c_i64, c_vp, c_vp]),
    "vad_spec_i16": (c_int, [c_vp, c_vp, c_i64, c_i32, c_i64, c_vp, c_vp]),
    "vad_mfcc_i16": (c_int, [c_vp, c_vp, c_i64, c_i32, c_i64, c_vp, c_vp]),
    "vad_mfcc_from_spec_f32": (c_int, [c_vp, c_vp, c_i64, c_vp, c_vp]),
    "vad_ffn_plan_create": (c_int, [c_i32, c_vp, c_vp, c_vp, c_vp]),
    "vad_ffn_plan_destroy": (c_int, [c_vp]),
    "vad_ffn_plan_arith": (c_i32, [c_vp]),
    "vad_ffn_plan_set_arith": (c_int, [c_vp, c_i32]),
    "vad_features_f32": (c_int, [c_vp, c_i64, c_i32, c_i32, c_vp, c_vp]),
    "vad_features_ffn": (c_int, [c_vp, c_vp, c_i64, c_i32, c_i32, c_vp, c_vp]),
    "vad_features_ffn_logits": (c_int, [c_vp, c_vp, c_i64, c_i32, c_i32, c_vp, c_vp, c_vp]),
    "vad_ffn_predict": (c_int, [c_vp, c_vp, c_i64, c_vp, c_vp]),
    "vad_ffn_train_param_count": (c_i64, [c_i32, c_vp]),
    "vad_ffn_train_steps": (c_int, [c_i32, c_vp, c_vp, c_i64, c_vp, c_vp, c_i64, c_vp, c_i64, c_i32, c_i64, c_vp,
                                    c_vp, c_vp]),
    "vad_ffn_train_eval_chunks": (c_i64, [c_i64]),
    "vad_ffn_train_eval": (c_int, [c_i32, c_vp, c_vp, c_i64, c_vp, c_vp, c_i64, c_vp, c_vp, c_vp]),
    "vad_tree_plan_create": (c_int, [c_i32, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_i32, c_vp]),
    "vad_tree_plan_destroy": (c_int, [c_vp]),
    "vad_tree_predict": (c_int, [c_vp, c_vp, c_i64, c_vp, c_vp]),
    "vad_features_tree": (c_int, [c_vp, c_vp, c_i64, c_i32, c_i32, c_vp, c_vp]),
    "vad_tree_train_node_capacity": (c_i64, [c_i64, c_i32]),
    "vad_tree_train_workspace_bytes": (c_sz, [c_i64, c_i32, c_i32, c_i32, c_vp]),
    "vad_tree_train": (c_int, [c_vp, c_vp, c_i64, c_i32, c_i32, c_vp, c_vp, c_i32, c_vp, c_vp, c_vp, c_sz, c_vp,
                               c_vp]),
    "vad_simple_features": (c_int, [c_vp, c_i64, c_i32, c_i64, c_i32, c_i32, c_i32, c_i32, c_vp,
                                    c_vp]),
    "vad_simple_stream_state_bytes": (c_sz, [c_i32]),
    "vad_simple_stream_init": (c_int, [c_vp, c_i64, c_i32, c_vp, c_vp]),
    "vad_simple_stream_block_f32": (c_int, [c_vp, c_i64, c_i64, c_i32, c_i32, c_i32, c_i32, c_i64, c_i32, c_i32, c_vp,
                                            c_vp, c_i64, c_vp, c_vp, c_i64, c_vp, c_vp]),
    "vad_simple_stream_block_i16": (c_int, [c_vp, c_i64, c_i64, c_i32, c_i32, c_i32, c_i32, c_i64, c_i32, c_i32, c_vp,
                                            c_vp, c_i64, c_vp, c_vp, c_i64, c_vp, c_vp]),
    "vad_simple_stream_state": (c_int, [c_vp, c_i64, c_i32, c_i32, c_vp, c_vp, c_i64, c_vp]),
    # sessions: the sibling's arguments, then frame_counts, restart, init_left, stream
    **{"vad_simple_stream_block_sessions_" + t: (c_int, [c_vp, c_i64, c_i64, c_i32, c_i32, c_i32, c_i32, c_i64, c_i32,
                                                         c_i32, c_vp, c_vp, c_i64, c_vp, c_vp, c_i64, c_vp, c_vp, c_vp,
                                                         c_vp, c_vp])
       for t in ("f32", "i16")},
    "vad_simple_stream_state_sessions": (c_int, [c_vp, c_i64, c_i32, c_i32, c_vp, c_vp, c_i64, c_vp, c_vp, c_vp,
                                                 c_vp]),
    "vad_scale_workspace_bytes": (c_sz, []),
    "vad_scale_features": (c_int, [c_vp, c_i64, c_i32, c_vp, c_sz, c_vp]),
    "vad_format_csv_rows": (c_i64, [c_vp, c_i64, c_i32, ctypes.c_double, c_vp, c_i64]),
    "vad_csv_workspace_bytes": (c_sz, [c_i64]),
    "vad_csv_count_lines": (c_int, [c_vp, c_i64, c_vp, c_vp, c_sz, c_vp]),
    "vad_csv_index": (c_int, [c_vp, c_i64, c_i64, c_i64, c_vp, c_i64, c_vp, c_sz, c_vp]),
    "vad_csv_parse": (c_int, [c_vp, c_i64, c_vp, c_i64, c_i64, c_i32, c_vp, c_i32, c_i32, c_vp, c_vp, c_vp, c_vp]),
    "vad_mfcc_ffn_workspace_bytes": (c_sz, [c_vp, c_vp, c_i64, c_i32, c_i32]),
    "vad_mfcc_ffn": (c_int, [c_vp, c_vp, c_vp, c_i64, c_i32, c_i32, c_i32, c_vp, c_vp, c_sz,
                             c_vp]),
    "vad_mfcc_ffn_i16": (c_int, [c_vp, c_vp, c_vp, c_i64, c_i32, c_i32, c_i32, c_vp, c_vp, c_sz,
                                 c_vp]),
    "vad_mfcc_ffn_fusable": (c_i32, [c_vp, c_vp, c_i32, c_i32]),
    "vad_stream_ring_floats": (c_i64, [c_i64, c_i32]),
    "vad_stream_push_hop": (c_int, [c_vp, c_i64, c_i32, c_vp, c_i64, c_i32, c_i64, c_vp]),
    "vad_stream_hop": (c_int, [c_vp, c_vp, c_vp, c_i64, c_i32, c_vp, c_i64, c_i32, c_i64, c_vp, c_vp, c_vp,
                               c_vp]),
    "vad_stream_hops": (c_int, [c_vp, c_vp, c_vp, c_i64, c_i32, c_vp, c_i64, c_i32, c_i64, c_i32, c_i64, c_vp,
                                c_vp, c_vp, c_i64, c_vp]),
    "vad_stream_push_hop_i16": (c_int, [c_vp, c_i64, c_i32, c_vp, c_i64, c_i32, c_i64, c_vp]),
    "vad_stream_hop_i16": (c_int, [c_vp, c_vp, c_vp, c_i64, c_i32, c_vp, c_i64, c_i32, c_i64, c_vp, c_vp, c_vp,
                                   c_vp]),
    "vad_stream_hops_i16": (c_int, [c_vp, c_vp, c_vp, c_i64, c_i32, c_vp, c_i64, c_i32, c_i64, c_i32, c_i64, c_vp,
                                    c_vp, c_vp, c_i64, c_vp]),
    "vad_stream_step": (c_int, [c_vp, c_vp, c_vp, c_i64, c_i32, c_i64, c_vp, c_vp, c_vp, c_vp,
                                c_vp]),
    "vad_stream_hops_tree": (c_int, [c_vp, c_vp, c_vp, c_i64, c_i32, c_vp, c_i64, c_i32, c_i64, c_i32, c_i64, c_vp,
                                     c_vp, c_vp, c_i64, c_i32, c_vp]),
    "vad_stream_hops_tree_i16": (c_int, [c_vp, c_vp, c_vp, c_i64, c_i32, c_vp, c_i64, c_i32, c_i64, c_i32, c_i64,
                                         c_vp, c_vp, c_vp, c_i64, c_i32, c_vp]),
    "vad_stream_step_tree": (c_int, [c_vp, c_vp, c_vp, c_i64, c_i32, c_i64, c_vp, c_vp, c_vp, c_vp,
                                     c_vp]),
    "vad_stream_tree_max_lds_nodes": (c_i64, [c_vp]),
    "vad_stream_hop_table_bytes": (c_i64, [c_vp, c_vp]),
    "vad_stream_hop_tree_table_bytes": (c_i64, [c_vp, c_vp, c_i32]),
    "vad_stream_hop_block_waves": (c_i32, [c_i64, c_i64, c_i32]),
    "vad_tree_plan_set_scores": (c_int, [c_vp, c_vp, c_i32]),
    "vad_tree_plan_score_classes": (c_i32, [c_vp]),
    **{"vad_stream_hops_scores" + t: (c_int, [c_vp, c_vp, c_vp, c_i64, c_i32, c_vp, c_i64, c_i32, c_i64, c_i32, c_i64,
                                              c_vp, c_vp, c_vp, c_i64, c_i32, c_vp, c_i64, c_vp])
       for t in ("", "_i16")},
    **{"vad_stream_hops_tree_scores" + t: (c_int, [c_vp, c_vp, c_vp, c_i64, c_i32, c_vp, c_i64, c_i32, c_i64, c_i32,
                                                   c_i64, c_vp, c_vp, c_vp, c_i64, c_i32, c_i32, c_vp, c_i64, c_vp])
       for t in ("", "_i16")},
    **{"vad_stream_" + n + "_floats": (c_i64, [c_i64]) for n in ("spec_ring", "noise_rows", "noise_est")},
    # the scored entries' arguments, then spec_ring, noise_rows, noise_count, noise_est, alpha, noise_class, update
    **{"vad_stream_hops_denoise" + t: (c_int, [c_vp, c_vp, c_vp, c_i64, c_i32, c_vp, c_i64, c_i32, c_i64, c_i32, c_i64,
                                               c_vp, c_vp, c_vp, c_i64, c_i32, c_vp, c_i64, c_vp, c_vp, c_vp, c_vp,
                                               c_f32, c_i32, c_i32, c_vp])
       for t in ("", "_i16")},
    **{"vad_stream_hops_tree_denoise" + t: (c_int, [c_vp, c_vp, c_vp, c_i64, c_i32, c_vp, c_i64, c_i32, c_i64, c_i32,
                                                    c_i64, c_vp, c_vp, c_vp, c_i64, c_i32, c_i32, c_vp, c_i64, c_vp,
                                                    c_vp, c_vp, c_vp, c_f32, c_i32, c_i32, c_vp])
       for t in ("", "_i16")},
    # the denoising entries' arguments (the state all null: no denoising), then hop_counts, restart
    **{"vad_stream_hops_sessions" + t: (c_int, [c_vp, c_vp, c_vp, c_i64, c_i32, c_vp, c_i64, c_i32, c_i64, c_i32,
                                                c_i64, c_vp, c_vp, c_vp, c_i64, c_i32, c_vp, c_i64, c_vp, c_vp, c_vp,
                                                c_vp, c_f32, c_i32, c_i32, c_vp, c_vp, c_vp])
       for t in ("", "_i16")},
    **{"vad_stream_hops_tree_sessions" + t: (c_int, [c_vp, c_vp, c_vp, c_i64, c_i32, c_vp, c_i64, c_i32, c_i64, c_i32,
                                                     c_i64, c_vp, c_vp, c_vp, c_i64, c_i32, c_i32, c_vp, c_i64, c_vp,
                                                     c_vp, c_vp, c_vp, c_f32, c_i32, c_i32, c_vp, c_vp, c_vp])
       for t in ("", "_i16")},
    **{"vad_stream_hops_forest" + t: (c_int, [c_vp, c_vp, c_vp, c_i64, c_i32, c_vp, c_i64, c_i32, c_i64, c_i32,
                                              c_i64, c_vp, c_vp, c_vp, c_i64, c_i32, c_i32, c_vp, c_i64, c_vp,
                                              c_vp, c_vp, c_vp, c_f32, c_i32, c_i32, c_vp, c_vp, c_vp])
       for t in ("", "_i16")},
    "vad_stream_hop_forest_table_bytes": (c_i64, [c_vp, c_vp, c_i32]),
    "vad_stream_forest_lds_trees": (c_i32, [c_vp, c_vp]),
    **{"vad_stream_noise_load" + t: (c_int, [c_vp, c_vp, c_i64, c_i64, c_i32, c_i32, c_i64, c_vp, c_vp, c_vp, c_f32,
                                             c_vp])
       for t in ("", "_i16")},
    "vad_graph_launch": (c_int, [c_vp, c_vp]),
    "vad_graph_plan_create": (c_int, [c_vp, c_vp, c_vp]),
    "vad_graph_plan_launch": (c_int, [c_vp, c_vp]),
    "vad_graph_plan_direct": (c_i32, [c_vp]),
    "vad_graph_plan_destroy": (c_int, [c_vp]),
    "vad_segments_workspace_bytes": (c_sz, [c_i64]),
    "vad_label_smooth": (c_int, [c_vp, c_i64, c_i32, c_i64, c_i64, c_vp, c_vp, c_sz, c_vp]),
    "vad_label_segments": (c_int, [c_vp, c_i64, c_i32, c_i64, c_i64, c_i32, c_i32, c_i64, c_vp, c_i64, c_vp, c_vp,
                                   c_sz, c_vp]),
    "vad_gather_segments_f32": (c_int, [c_vp, c_i64, c_vp, c_vp, c_i64, c_vp, c_i64, c_vp]),
    "vad_gather_segments_i16": (c_int, [c_vp, c_i64, c_vp, c_vp, c_i64, c_vp, c_i64, c_vp]),
    "vad_gather_active_frames_f32": (c_int, [c_vp, c_i64, c_vp, c_i64, c_i32, c_i32, c_i32, c_vp, c_i64, c_vp, c_vp,
                                             c_sz, c_vp]),
    "vad_gather_active_frames_i16": (c_int, [c_vp, c_i64, c_vp, c_i64, c_i32, c_i32, c_i32, c_vp, c_i64, c_vp, c_vp,
                                             c_sz, c_vp]),
    "vad_batch_pack_f32": (c_int, [c_vp, c_vp, c_vp, c_i64, c_vp, c_i64, c_vp]),
    "vad_batch_pack_i16": (c_int, [c_vp, c_vp, c_vp, c_i64, c_vp, c_i64, c_vp]),
    "vad_batch_compact_rows": (c_int, [c_vp, c_i64, c_i64, c_vp, c_vp, c_vp, c_i64, c_vp, c_i64, c_vp]),
    "vad_batch_segments_workspace_bytes": (c_sz, [c_i64, c_i64]),
    "vad_batch_label_smooth": (c_int, [c_vp, c_i64, c_vp, c_vp, c_i64, c_i32, c_i64, c_i64, c_vp, c_vp, c_sz, c_vp]),
    "vad_batch_label_segments": (c_int, [c_vp, c_i64, c_vp, c_vp, c_vp, c_i64, c_i32, c_i64, c_i64, c_i32, c_i32,
                                         c_vp, c_vp, c_i64, c_vp, c_vp, c_vp, c_vp, c_vp, c_sz, c_vp]),
    "vad_scores_from_logits": (c_int, [c_vp, c_i64, c_i32, c_i32, c_vp, c_vp]),
    "vad_tree_train_features": (c_int, [c_vp, c_vp, c_i64, c_i32, c_i32, c_vp, c_vp, c_vp, c_i32, c_vp, c_vp, c_vp,
                                        c_sz, c_vp, c_vp]),
    "vad_tree_train_weighted_workspace_bytes": (c_sz, [c_i64, c_i32, c_i32, c_i32, c_vp]),
    "vad_tree_train_weighted": (c_int, [c_vp, c_vp, c_i64, c_i32, c_i32, c_vp, c_vp, c_vp, c_i32, c_vp, c_vp, c_vp,
                                        c_sz, c_vp, c_vp]),
    "vad_forest_create": (c_int, [c_i32, c_vp, c_vp, c_vp, c_vp, c_vp, c_i32, c_vp, c_i32, c_vp, c_i32, c_vp]),
    "vad_forest_destroy": (c_int, [c_vp]),
    "vad_forest_predict": (c_int, [c_vp, c_vp, c_i64, c_i32, c_vp, c_vp, c_vp]),
    "vad_features_forest": (c_int, [c_vp, c_vp, c_i64, c_i32, c_i32, c_i32, c_vp, c_vp, c_vp]),
    "vad_features_tree_scores": (c_int, [c_vp, c_vp, c_vp, c_i64, c_i32, c_i32, c_vp, c_vp]),
    "vad_tree_predict_scores": (c_int, [c_vp, c_vp, c_vp, c_i64, c_vp, c_vp]),
    "vad_scores_workspace_bytes": (c_sz, [c_i64]),
    "vad_score_labels": (c_int, [c_vp, c_i64, c_f32, c_f32, c_vp, c_vp, c_sz, c_vp]),
    "vad_label_dilate": (c_int, [c_vp, c_i64, c_i32, c_i64, c_i64, c_vp, c_vp, c_sz, c_vp]),
    "vad_batch_score_labels": (c_int, [c_vp, c_i64, c_vp, c_vp, c_i64, c_f32, c_f32, c_vp, c_vp, c_sz, c_vp]),
    "vad_batch_label_dilate": (c_int, [c_vp, c_i64, c_vp, c_vp, c_i64, c_i32, c_i64, c_i64, c_vp, c_vp, c_sz,
                                       c_vp]),
    "vad_reference_labels": (c_int, [c_vp, c_i64, c_i64, c_i32, c_i32, c_vp, c_vp]),
    "vad_batch_reference_labels": (c_int, [c_vp, c_i64, c_vp, c_vp, c_vp, c_i64, c_i64, c_i32, c_i32, c_vp, c_vp]),
    "vad_score_histogram_f32": (c_int, [c_vp, c_vp, c_i64, c_i32, c_vp, c_vp]),
    "vad_score_histogram_u8": (c_int, [c_vp, c_vp, c_i64, c_i32, c_vp, c_vp]),
    "vad_stream_seg_delay": (c_i64, [c_i64, c_i64, c_i32, c_i32]),
    "vad_stream_seg_flush_rows": (c_i64, [c_i64, c_i64, c_i32, c_i32]),
    "vad_stream_seg_state_bytes": (c_sz, [c_i64]),
    "vad_stream_seg_history_elems": (c_i64, [c_i64, c_i32, c_i64, c_i64, c_i32, c_i32]),
    "vad_stream_segments": (c_int, [c_vp, c_i64, c_i64, c_i32, c_i32, c_i64, c_i64, c_i32, c_i32, c_vp, c_vp, c_i64,
                                    c_vp, c_vp]),
    "vad_stream_segments_f32": (c_int, [c_vp, c_i64, c_i64, c_i32, c_i32, c_i64, c_i64, c_i32, c_i32, c_vp, c_vp,
                                        c_i64, c_vp, c_vp, c_i64, c_i64, c_vp, c_i64, c_vp, c_vp, c_vp]),
    "vad_stream_segments_i16": (c_int, [c_vp, c_i64, c_i64, c_i32, c_i32, c_i64, c_i64, c_i32, c_i32, c_vp, c_vp,
                                        c_i64, c_vp, c_vp, c_i64, c_i64, c_vp, c_i64, c_vp, c_vp, c_vp]),
    "vad_stream_segments_flush": (c_int, [c_i64, c_i64, c_i64, c_i32, c_i32, c_vp, c_vp, c_i64, c_vp, c_vp]),
    "vad_stream_segments_flush_f32": (c_int, [c_i64, c_i64, c_i64, c_i32, c_i32, c_vp, c_vp, c_i64, c_vp, c_vp,
                                              c_i64, c_vp, c_vp, c_vp]),
    "vad_stream_segments_flush_i16": (c_int, [c_i64, c_i64, c_i64, c_i32, c_i32, c_vp, c_vp, c_i64, c_vp, c_vp,
                                              c_i64, c_vp, c_vp, c_vp]),
    "vad_stream_seg_delay_pad": (c_i64, [c_i64, c_i64, c_i32, c_i32, c_i64, c_i64]),
    "vad_stream_seg_flush_rows_pad": (c_i64, [c_i64, c_i64, c_i32, c_i32, c_i64, c_i64]),
    "vad_stream_seg_history_elems_pad": (c_i64, [c_i64, c_i32, c_i64, c_i64, c_i32, c_i32, c_i64, c_i64]),
    # block, is_scores, stride, S, n_hops, active, max_gap, min_run, L, H, on, off, pad_before, pad_after, tables
    "vad_stream_segments_op": (c_int, [c_vp, c_i32, c_i64, c_i64, c_i32, c_i32, c_i64, c_i64, c_i32, c_i32, c_f32,
                                       c_f32, c_i64, c_i64, c_vp, c_vp, c_i64, c_vp, c_vp]),
    **{"vad_stream_segments_op_" + t: (c_int, [c_vp, c_i32, c_i64, c_i64, c_i32, c_i32, c_i64, c_i64, c_i32, c_i32,
                                               c_f32, c_f32, c_i64, c_i64, c_vp, c_vp, c_i64, c_vp, c_vp, c_i64,
                                               c_i64, c_vp, c_i64, c_vp, c_vp, c_vp])
       for t in ("f32", "i16")},
    "vad_stream_segments_op_flush": (c_int, [c_i64, c_i32, c_i64, c_i64, c_i32, c_i32, c_f32, c_f32, c_i64, c_i64,
                                             c_vp, c_vp, c_i64, c_vp, c_vp]),
    **{"vad_stream_segments_op_flush_" + t: (c_int, [c_i64, c_i32, c_i64, c_i64, c_i32, c_i32, c_f32, c_f32, c_i64,
                                                     c_i64, c_vp, c_vp, c_i64, c_vp, c_vp, c_i64, c_vp, c_vp, c_vp])
       for t in ("f32", "i16")},
    # sessions: the sibling's arguments, then hop_counts, restart, (end_voiced,) end_len, table_session, stream
    "vad_stream_segments_sessions": (c_int, [c_vp, c_i64, c_i64, c_i32, c_i32, c_i64, c_i64, c_i32, c_i32, c_vp,
                                             c_vp, c_i64, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp]),
    **{"vad_stream_segments_sessions_" + t: (c_int, [c_vp, c_i64, c_i64, c_i32, c_i32, c_i64, c_i64, c_i32, c_i32,
                                                     c_vp, c_vp, c_i64, c_vp, c_vp, c_i64, c_i64, c_vp, c_i64, c_vp,
                                                     c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp])
       for t in ("f32", "i16")},
    "vad_stream_segments_op_sessions": (c_int, [c_vp, c_i32, c_i64, c_i64, c_i32, c_i32, c_i64, c_i64, c_i32, c_i32,
                                                c_f32, c_f32, c_i64, c_i64, c_vp, c_vp, c_i64, c_vp, c_vp, c_vp,
                                                c_vp, c_vp, c_vp]),
    **{"vad_stream_segments_op_sessions_" + t: (c_int, [c_vp, c_i32, c_i64, c_i64, c_i32, c_i32, c_i64, c_i64, c_i32,
                                                        c_i32, c_f32, c_f32, c_i64, c_i64, c_vp, c_vp, c_i64, c_vp,
                                                        c_vp, c_i64, c_i64, c_vp, c_i64, c_vp, c_vp, c_vp, c_vp,
                                                        c_vp, c_vp, c_vp, c_vp])
       for t in ("f32", "i16")},
    "vad_resample_tile_outputs": (c_i32, []),
    "vad_resample_plan_create": (c_int, [c_i32, c_i32, c_vp, c_i32, c_vp]),
    "vad_resample_plan_upload": (c_int, [c_vp]),
    "vad_resample_plan_destroy": (c_int, [c_vp]),
    "vad_resample_n_out": (c_i64, [c_vp, c_i64]),
    "vad_resample_delay": (c_i32, [c_vp]),
    **{f"vad_resample_batch_{i}_{o}": (c_int, [c_vp, c_vp, c_vp, c_vp, c_i64, c_vp, c_i64, c_vp])
       for i in ("f32", "i16") for o in ("f32", "i16")},
    "vad_resample_stream_state_bytes": (c_sz, [c_vp, c_i64]),
    **{f"vad_resample_stream_{i}_{o}": (c_int, [c_vp, c_vp, c_i64, c_i64, c_i64, c_i32, c_i32, c_vp, c_vp, c_vp])
       for i in ("f32", "i16") for o in ("f32", "i16")},
    "vad_resample_sessions_grid": (c_i32, []),
    "vad_resample_sessions_state_bytes": (c_sz, [c_vp, c_i32, c_i64]),
    **{f"vad_resample_stream_sessions_{i}_{o}": (c_int, [c_vp, c_i32, c_vp, c_i64, c_i64, c_i64, c_i32, c_i32, c_vp,
                                                         c_vp, c_vp, c_vp, c_vp, c_vp])
       for i in ("f32", "i16") for o in ("f32", "i16")},
    "vad_rccl_available": (c_int, []),
    "vad_rccl_error_string": (ctypes.c_char_p, []),
    "vad_rccl_unique_id": (c_int, [c_vp]),
    "vad_rccl_init": (c_int, [c_vp, c_i32, c_vp, c_i32]),
    "vad_rccl_gather_u8": (c_int, [c_vp, c_vp, c_vp, c_sz, c_i32, c_vp]),
    "vad_rccl_destroy": (c_int, [c_vp]),
}


class VadError(RuntimeError):
    """A libvad_amd call failed (negative VAD_E* code or a hipError_t)."""


_lib = None


def lib():
    """The loaded library (raises if it was not built)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                f"libvad_amd.so not found at {LIB_PATH}: build it with "
                "`python -m vad_amd.build` (there is no CPU fallback)")
        handle = ctypes.CDLL(LIB_PATH, mode=ctypes.RTLD_GLOBAL)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(handle, name)
            fn.restype = res
            fn.argtypes = args
        _lib = handle
    return _lib


def check(code, what):
    if code != VAD_OK:
        names = {VAD_EINVAL: "invalid argument", VAD_EUNSUPPORTED: "unsupported configuration",
                 VAD_ENOMEM: "out of memory"}
        if code == VAD_ERCCL:
            raise VadError(f"{what} failed: RCCL: {lib().vad_rccl_error_string().decode()}")
        raise VadError(f"{what} failed: {names.get(code, f'hipError_t {code}')}")


def ptr(t):
    """Device pointer of a torch tensor (None -> NULL)."""
    return None if t is None else ctypes.c_void_p(t.data_ptr())


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def stream_ptr(stream=None):
    """hipStream_t of a torch stream (default: the current stream of the
    current device, read without building a Stream object: this sits on
    every per-hop launch path)."""
    if stream is None and _raw_stream is not None:
        return ctypes.c_void_p(_raw_stream(torch.cuda.current_device()))
    s = stream if stream is not None else torch.cuda.current_stream()
    return ctypes.c_void_p(s.cuda_stream)
