"""ctypes binding of libivr_hip.so (include/ivr_api.h).

The product path has no CPU fallback: if the HIP library is missing or a call
fails, this module raises.  Status codes map to the exception types the
reference raises at the same places (IVR_ERR_INVALID -> ValueError as in
core.py:1178-1191, everything else -> RuntimeError as in core.py:894-896).
"""
import ctypes as C
import operator
import os
import threading

_HERE = os.path.dirname(os.path.abspath(__file__))
# IVR_LIB: diagnostics only (e.g. a -DIVR_GEMM_STAMPS build for tools/gemm_stamps.py)
LIB_PATH = os.environ.get("IVR_LIB") or os.path.join(os.path.dirname(_HERE), "lib", "libivr_hip.so")

IVR_MAX_K = 2048
IVR_GRAPH_MAX_EF, IVR_GRAPH_MAX_CAND, IVR_GRAPH_MAX_DEGREE = 256, 64, 64       # include/ivr_api.h
IVR_PQ_MAX_M = 128
IVR_PQFS_MAX_M = 256
IVR_SQ_MAX_D = 1024
IVR_SEQ_MAX_LEN = 64
IVR_EVENT_MAX_LEN = 8
IVR_EVENT_MAX_GAP = 4096
IVR_KNN_MAX_K = 64
IVR_TAG_MAX_LABELS, IVR_TAG_MAX_TOP = 4096, 64
IVR_TAG_RANK = {"mass": 0, "votes": 1}                    # rank of ivr_index_tag_segments (_staging.check_tag_segments)
IVR_GROUP_MAX_ROWS = 64
IVR_PHASH_MAX_SIDE = 8192
IVR_KEEPWIN_MAX_WINDOW = 64
IVR_DIVERSE_MMR, IVR_DIVERSE_SUPPRESS = 0, 1              # mode of ivr_index_diversify
IVR_FUSE_MAX_MEMBERS = 16
IVR_FUSE_FOLD = {"max": 0, "min": 1, "sum": 2}            # fold / combine of ivr_index_search_fused
IVR_FUSE_COMBINE = {"margin": 0, "veto": 1}
IVR_MOMENT_RANK = {"peak": 0, "count": 1}                 # rank of ivr_index_search_moments
IVR_VIDEO_MAX_MEMBERS = 4096
IVR_VIDEO_MODE = {"forward": 0, "backward": 1, "symmetric": 2}        # mode of ivr_index_video_scores / ivr_index_video_search
# flags of ivr_preprocess
PP_MODE = {"identity": 0, "shortest_edge_crop": 1, "stretch": 2, "letterbox": 3}
PP_BGR, PP_OUT_F32, PP_OUT_PATCH_MAJOR, PP_BILINEAR = 1 << 4, 1 << 5, 1 << 6, 1 << 7


class TowerDesc(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("kind", "width", "layers", "heads", "mlp", "tokens", "out_dim", "act", "pool",
                                       "image", "patch", "pre_ln", "patch_bias", "vocab", "eos_id", "causal",
                                       "compute")] + [("ln_eps", C.c_float), ("fp8_sites", C.c_int), ("fp8_mlp_cls_bf16", C.c_int),
                                                                      ("fp8_first_layer", C.c_int)]


class GemmDesc(C.Structure):
    """ivr_gemm_desc (include/ivr_api.h)."""
    _fields_ = ([(n, C.c_int) for n in ("dtype", "epilogue", "act", "M", "N", "K")]
                + [("A", C.c_void_p), ("lda", C.c_int), ("W", C.c_void_p), ("ldw", C.c_int), ("bias", C.c_void_p),
                   ("colscale", C.c_void_p), ("out", C.c_void_p), ("ldo", C.c_int), ("out8", C.c_int), ("resid", C.c_void_p),
                   ("ldr", C.c_int), ("pos", C.c_void_p)]
                + [(n, C.c_int) for n in ("T", "G2", "skip_mod", "reverse_m")])


class IdFilter(C.Structure):
    """ivr_id_filter (include/ivr_api.h): allowed ids [lo, hi), and bits[id >> 3] >> (id & 7) & 1 when bits is set (id < nbits)."""
    _fields_ = [("lo", C.c_int64), ("hi", C.c_int64), ("bits", C.c_void_p), ("nbits", C.c_int64)]


API_VERSION = 11
FP8_SITE = {"qkv": 1, "o": 2, "fc1": 4, "fc2": 8}
# IVR_SITE_* of ivr_tower_debug_capture
TOWER_SITE = {"embed": 0, "eos_pos": 1, "stream": 2, "ln1": 3, "qkv": 4, "att": 5, "attn_out": 6, "ln2": 7, "ln2_cls": 8, "hid": 9,
              "hid8": 10, "hid_cls": 11, "hid_cls8": 12, "fc2": 13, "pool_ln": 14, "pooled": 15}


_p = C.c_void_p
_i, _i64, _f = C.c_int, C.c_int64, C.c_float
_SIGS = {
    "ivr_api_version": (_i, []),
    "ivr_init": (_i, [_i, C.POINTER(_p)]),
    "ivr_destroy": (_i, [_p]),
    "ivr_last_error": (C.c_char_p, [_p]),
    "ivr_device_info": (_i, [_p, C.POINTER(_i), C.POINTER(_i64), C.c_char_p, _i]),
    "ivr_release_stream_scratch": (_i, [_p, _p]),
    "ivr_profile_enable": (_i, [_p, _i]),
    "ivr_profile_reset": (_i, [_p]),
    "ivr_profile_json": (_i, [_p, C.c_char_p, _i]),
    "ivr_preprocess": (_i, [_p, _p, _i, _i, _i, _i, C.POINTER(_f), C.POINTER(_f), _i, _i, _p, _p]),
    "ivr_preprocess_scratch_bytes": (_i64, [_i, _i, _i, _i, _i]),
    "ivr_resize_u8": (_i, [_p, _p, _i, _i, _i, _i, _i, _p, _p]),
    "ivr_phash_scratch_bytes": (_i64, [_i, _i, _i]),
    "ivr_phash": (_i, [_p, _p, _i, _i, _i, _i, _p, _p, _p]),
    "ivr_phash_cos_table": (_i, [C.POINTER(C.c_double)]),
    "ivr_tower_create": (_i, [_p, C.POINTER(TowerDesc), C.POINTER(_p)]),
    "ivr_tower_set_weight": (_i, [_p, C.c_char_p, _p, _i64]),
    "ivr_tower_finalize": (_i, [_p, _i]),
    "ivr_tower_destroy": (_i, [_p]),
    "ivr_tower_encode_image": (_i, [_p, _p, _i, _i, _p, _p]),
    "ivr_tower_encode_text": (_i, [_p, _p, _i, _i, _i, _p, _p]),
    "ivr_tower_debug_hidden": (_i, [_p, _i, _i, _p, _p]),
    "ivr_tower_debug_capture": (_i, [_p, _i, _i, _p, _i64]),
    "ivr_tower_debug_capture_result": (_i, [_p, _i, C.POINTER(_i64), C.POINTER(_i)]),
    "ivr_tower_workspace_bytes": (_i64, [_p]),
    "ivr_linear": (_i, [_p, _i, _i, _p, _p, _p, _i, _i, _i, _i, _p, _p, _p]),
    "ivr_quantize_e4m3_host": (_i, [_p, _p, _i64]),
    "ivr_attention": (_i, [_p, _i, _p, _i, _i, _i, _i, _i, _i, _p, _p]),
    "ivr_qkv_attention": (_i, [_p, _p, _p, _p, _i, _i, _i, _i, _i, _p, _p]),
    "ivr_layernorm": (_i, [_p, _i, _p, _i, _p, _p, _p, _f, _i, _i, _i, _p, _p]),
    "ivr_linear_fp8": (_i, [_p, _i, _p, _p, _p, _p, _i, _i, _i, _i, _p, _i, _p, _p]),
    "ivr_gemm": (_i, [_p, C.POINTER(GemmDesc), _p]),
    "ivr_l2_normalize": (_i, [_p, _p, _i64, _i, _p, _p]),
    "ivr_index_create": (_i, [_p, _i, _i64, C.POINTER(_p)]),
    "ivr_index_destroy": (_i, [_p]),
    "ivr_index_scan_stats": (_i, [_p, _p]),
    "ivr_index_reset": (_i, [_p]),
    "ivr_index_ntotal": (_i64, [_p]),
    "ivr_index_dim": (_i, [_p]),
    "ivr_index_capacity": (_i64, [_p]),
    "ivr_index_add": (_i, [_p, _p, _i64, _i, _p]),
    "ivr_index_write": (_i, [_p, _i64, _p, _i64, _i, _p]),
    "ivr_index_write_ring": (_i, [_p, _p, _i64, _i, _p, _p]),
    "ivr_index_reconstruct": (_i, [_p, _i64, _i64, _p, _p]),
    "ivr_index_reserve_search": (_i, [_p, _i, _i]),
    "ivr_index_search": (_i, [_p, _p, _i, _i, _i, _i64, _p, _p, _p]),
    "ivr_index_range_search": (_i, [_p, _p, _i, _f, _i, _i64, _p, _p, _p, _i64, _p]),
    "ivr_index_search_filtered": (_i, [_p, _p, _i, _i, _i, _i64, C.POINTER(IdFilter), _p, _p, _p]),
    "ivr_index_range_search_filtered": (_i, [_p, _p, _i, _f, _i, _i64, C.POINTER(IdFilter), _p, _p, _p, _i64, _p]),
    "ivr_index_remove_ids": (_i, [_p, _i64, C.POINTER(IdFilter), C.POINTER(_i64), _p]),
    "ivr_index_add_with_ids": (_i, [_p, _p, _p, _i64, _i, _p]),
    "ivr_index_has_ids": (_i, [_p]),
    "ivr_index_get_ids": (_i, [_p, _i64, _i64, _p, _p]),
    "ivr_index_find_ids": (_i, [_p, _p, _i64, _p, _p]),
    "ivr_index_gather": (_i, [_p, _p, _i64, _p, _p]),
    "ivr_index_scatter": (_i, [_p, _p, _p, _i64, _i, _p]),
    "ivr_index_search_reconstruct": (_i, [_p, _p, _i, _i, _i, _i64, C.POINTER(IdFilter), _p, _p, _p, _p]),
    "ivr_index_search_lists": (_i, [_p, _p, _i, _p, _i, _p, _i, _i64, _i, _i, _p, _p, _p]),
    "ivr_segment_mean": (_i, [_p, _p, _i64, _p, _i, _i, _i, _p, _p]),
    "ivr_index_rescore": (_i, [_p, _p, _i, _p, _i, _i, _i, _p, _p, _p, _p]),
    "ivr_index_search_sequences": (_i, [_p, _p, _i, _i, _p, _i, _i, _i, _p, _p, _p]),
    "ivr_index_range_search_sequences": (_i, [_p, _p, _i, _i, _p, _i, _f, _i, _p, _p, _p, _i64, _p]),
    "ivr_index_search_events": (_i, [_p, _p, _i, _i, _i, _i, _p, _i, _i, _i, _p, _p, _p]),
    "ivr_index_best_events_per_segment": (_i, [_p, _p, _i, _i, _i, _i, _p, _i, _i, _p, _p, _p]),
    "ivr_group_piece_rows": (_i, []),
    "ivr_index_search_groups": (_i, [_p, _p, _i, _p, _i, _i, _i, _i, _p, _p, _p, _p]),
    "ivr_index_best_per_segment": (_i, [_p, _p, _i, _p, _i, _i, _p, _p, _p]),
    "ivr_moment_block_rows": (_i, []),
    "ivr_index_search_moments": (_i, [_p, _p, _i, _p, _i, _f, _i, _i, _i, _i, _i, _p, _p, _p, _p, _p, _p]),
    "ivr_index_range_search_moments": (_i, [_p, _p, _i, _p, _i, _f, _i, _i, _p, _p, _p, _p, _p, _p, _i64, _p]),
    "ivr_index_search_fused": (_i, [_p, _p, _i, _i, _p, _p, _i, _i, _i, _i, _p, _p, _p]),
    "ivr_index_range_search_fused": (_i, [_p, _p, _i, _i, _p, _p, _i, _i, _f, _i, _p, _p, _p, _i64, _p]),
    "ivr_index_dbscan": (_i, [_p, _f, _i, _p, _i, _p, _p, _p, _p]),
    "ivr_segment_best_cosine": (_i, [_p, _p, _i64, _p, _i, _i, _p, _p, _p, _p]),
    "ivr_knn_max_k": (_i, []),
    "ivr_knn_piece_rows": (_i, []),
    "ivr_index_knn_graph": (_i, [_p, _i, _p, _i, _f, _p, _p, _p, _p]),
    "ivr_tag_max_labels": (_i, []),
    "ivr_tag_max_top": (_i, []),
    "ivr_index_tag_rows": (_i, [_p, _p, _i, _i, _f, _i, _f, _i64, _i64, _p, _p, _p, _p, _p, _p]),
    "ivr_index_tag_segments": (_i, [_p, _p, _i, _i, _f, _i, _f, _p, _i, _i, _i, _p, _p, _p, _p, _p]),
    "ivr_index_video_scores": (_i, [_p, _p, _i, _p, _i, _p, _i, _i, _i, _p, _p]),
    "ivr_index_video_search": (_i, [_p, _p, _i, _p, _i, _p, _i, _i, _i, _i, _p, _p, _p, _p]),
    "ivr_bin_index_create": (_i, [_p, _i, _i64, C.POINTER(_p)]),
    "ivr_bin_index_destroy": (_i, [_p]),
    "ivr_bin_index_reset": (_i, [_p]),
    "ivr_bin_index_ntotal": (_i64, [_p]),
    "ivr_bin_index_block_rows": (_i, []),
    "ivr_bin_index_add": (_i, [_p, _p, _i64, _p]),
    "ivr_bin_index_get_codes": (_i, [_p, _i64, _i64, _p, _p]),
    "ivr_bin_index_search": (_i, [_p, _p, _i, _i, _p, _p, _p]),
    "ivr_sign_encode": (_i, [_p, _p, _i64, _i, _p, _p, _i, _p, _p, _p]),
    "ivr_pq_encode": (_i, [_p, _p, _i64, _i, _p, _i, _p, _p]),
    "ivr_pq_tables": (_i, [_p, _p, _i, _i, _p, _i, _p, _p]),
    "ivr_bin_index_search_pq": (_i, [_p, _p, _i, _i, _i, _p, _p, _p]),
    "ivr_ivfpq_create": (_i, [_p, _i, _i, C.POINTER(_p)]),
    "ivr_ivfpq_destroy": (_i, [_p]),
    "ivr_ivfpq_reset": (_i, [_p]),
    "ivr_ivfpq_ntotal": (_i64, [_p]),
    "ivr_ivfpq_probe_queries": (_i, []),
    "ivr_ivfpq_set_lists": (_i, [_p, _p, _p, _p, _i64, _p]),
    "ivr_ivfpq_get_codes": (_i, [_p, _i64, _i64, _p, _p, _p]),
    "ivr_ivfpq_search": (_i, [_p, _p, _p, _p, _i, _i, _i, _p, _p, _p]),
    "ivr_ivfsq_create": (_i, [_p, _i, _i, C.POINTER(_p)]),
    "ivr_ivfsq_destroy": (_i, [_p]),
    "ivr_ivfsq_reset": (_i, [_p]),
    "ivr_ivfsq_ntotal": (_i64, [_p]),
    "ivr_ivfsq_set_lists": (_i, [_p, _p, _p, _p, _i64, _p]),
    "ivr_ivfsq_get_codes": (_i, [_p, _i64, _i64, _p, _p, _p]),
    "ivr_ivfsq_search": (_i, [_p, _p, _p, _p, _p, _p, _i, _i, _i, _p, _p, _p]),
    "ivr_sq_encode": (_i, [_p, _p, _i64, _i, _p, _p, _p, _p]),
    "ivr_sq_query": (_i, [_p, _p, _i, _i, _p, _p, _p, _p, _p, _p]),
    "ivr_sq_index_create": (_i, [_p, _i, C.POINTER(_p)]),
    "ivr_sq_index_destroy": (_i, [_p]),
    "ivr_sq_index_reset": (_i, [_p]),
    "ivr_sq_index_ntotal": (_i64, [_p]),
    "ivr_sq_index_add": (_i, [_p, _p, _i64, _p]),
    "ivr_sq_index_get_codes": (_i, [_p, _i64, _i64, _p, _p]),
    "ivr_sq_index_search": (_i, [_p, _p, _p, _p, _i, _i, _p, _p, _p]),
    "ivr_pqfs_pass_queries": (_i, []),
    "ivr_pqfs_encode": (_i, [_p, _p, _i64, _i, _p, _i, _p, _p]),
    "ivr_pqfs_tables": (_i, [_p, _p, _i, _i, _p, _i, _p, _p, _p, _p, _p]),
    "ivr_pqfs_quantize": (_i, [_p, _p, _i, _i, _p, _p, _p, _p]),
    "ivr_pqfs_index_create": (_i, [_p, _i, C.POINTER(_p)]),
    "ivr_pqfs_index_destroy": (_i, [_p]),
    "ivr_pqfs_index_reset": (_i, [_p]),
    "ivr_pqfs_index_ntotal": (_i64, [_p]),
    "ivr_pqfs_index_add": (_i, [_p, _p, _i64, _p]),
    "ivr_pqfs_index_get_codes": (_i, [_p, _i64, _i64, _p, _p]),
    "ivr_pqfs_index_search": (_i, [_p, _p, _p, _p, _i, _i, _p, _p, _p]),
    "ivr_graph_max_ef": (_i, []),
    "ivr_graph_max_cand": (_i, []),
    "ivr_graph_create": (_i, [_p, _i, _i, C.POINTER(_p)]),
    "ivr_graph_destroy": (_i, [_p]),
    "ivr_graph_reset": (_i, [_p]),
    "ivr_graph_ntotal": (_i64, [_p]),
    "ivr_graph_set_rows": (_i, [_p, _p, _i64, _p]),
    "ivr_graph_prune": (_i, [_p, _p, _i, _i, _p, _p, _p]),
    "ivr_graph_set_neighbors": (_i, [_p, _p, _i64, _p]),
    "ivr_graph_search": (_i, [_p, _p, _i, _i, _i, _p, _i, _i, _i, _p, _p, _p, _p]),
    "ivr_topk_merge": (_i, [_p, _p, _p, _i, _i, _i, _p, _p, _p]),
    "ivr_topk_pack": (_i, [_p, _p, _p, _i, _i, _p, _p]),
    "ivr_topk_merge_packed": (_i, [_p, _p, _i, _i, _i, _p, _p, _p]),
    "ivr_rowwise_cosine": (_i, [_p, _p, _p, _i, _i, _p, _p]),
    "ivr_dedup_keep_mask": (_i, [_p, _p, _i, _i, _f, _p, _p, _p]),
    "ivr_scene_keep_mask": (_i, [_p, _p, _i, _i, _f, _i, _p, _p]),
    "ivr_scene_keep_mask_window": (_i, [_p, _p, _i, _i, _f, _i, _p, _p]),
    "ivr_hash_keep_mask": (_i, [_p, _p, _i64, _p, _i, _i, _i, _p, _p]),
    "ivr_kept_window_mask": (_i, [_p, _p, _i64, _i, _p, _i, _f, _i, _p, _p]),
    "ivr_frame_quality_scratch_bytes": (_i64, [_i, _i, _i]),
    "ivr_frame_quality": (_i, [_p, _p, _i, _i, _i, _i, _i, _i, _p, _p, _p]),
    "ivr_index_diversify": (_i, [_p, _p, _i, _p, _i, _i, _i, _f, _i, _p, _p, _p, _p]),
}
EXPORTS = tuple(_SIGS)
# the exports that return a value; every other one returns a status that call() hands to check()
_VALUE = frozenset(("ivr_api_version", "ivr_last_error", "ivr_preprocess_scratch_bytes", "ivr_tower_workspace_bytes", "ivr_index_ntotal",
                    "ivr_index_dim", "ivr_index_capacity", "ivr_index_has_ids", "ivr_bin_index_ntotal", "ivr_bin_index_block_rows",
                    "ivr_graph_max_ef", "ivr_graph_max_cand", "ivr_graph_ntotal", "ivr_frame_quality_scratch_bytes",
                    "ivr_sq_index_ntotal", "ivr_ivfpq_ntotal", "ivr_ivfpq_probe_queries", "ivr_ivfsq_ntotal",
                    "ivr_pqfs_pass_queries", "ivr_pqfs_index_ntotal", "ivr_knn_max_k", "ivr_knn_piece_rows",
                    "ivr_phash_scratch_bytes", "ivr_group_piece_rows", "ivr_moment_block_rows", "ivr_tag_max_labels",
                    "ivr_tag_max_top"))
# the slot of the ivr_stream argument (the last one wherever there is one): call() fills it when the caller leaves it out
_STREAM = {n: len(_SIGS[n][1]) - 1 for n in (
    "ivr_release_stream_scratch", "ivr_preprocess", "ivr_tower_encode_image", "ivr_tower_encode_text", "ivr_tower_debug_hidden",
    "ivr_linear", "ivr_attention", "ivr_qkv_attention", "ivr_layernorm", "ivr_linear_fp8", "ivr_gemm", "ivr_l2_normalize",
    "ivr_index_add", "ivr_index_write", "ivr_index_write_ring", "ivr_index_reconstruct", "ivr_index_search", "ivr_index_range_search",
    "ivr_index_search_filtered", "ivr_index_range_search_filtered", "ivr_index_remove_ids", "ivr_index_add_with_ids",
    "ivr_index_get_ids", "ivr_index_find_ids", "ivr_index_gather", "ivr_index_scatter", "ivr_index_search_reconstruct",
    "ivr_index_search_lists", "ivr_segment_mean", "ivr_index_rescore", "ivr_index_search_sequences",
    "ivr_index_range_search_sequences", "ivr_index_search_events", "ivr_index_best_events_per_segment",
    "ivr_index_search_groups", "ivr_index_best_per_segment", "ivr_index_dbscan", "ivr_segment_best_cosine", "ivr_index_knn_graph", "ivr_bin_index_add", "ivr_bin_index_get_codes", "ivr_bin_index_search",
    "ivr_sign_encode", "ivr_pq_encode", "ivr_pq_tables", "ivr_bin_index_search_pq", "ivr_ivfpq_set_lists", "ivr_ivfpq_get_codes",
    "ivr_ivfpq_search", "ivr_ivfsq_set_lists", "ivr_ivfsq_get_codes", "ivr_ivfsq_search", "ivr_sq_encode", "ivr_sq_query", "ivr_sq_index_add",
    "ivr_sq_index_get_codes", "ivr_sq_index_search", "ivr_pqfs_encode", "ivr_pqfs_tables", "ivr_pqfs_quantize", "ivr_pqfs_index_add",
    "ivr_pqfs_index_get_codes", "ivr_pqfs_index_search", "ivr_graph_set_rows", "ivr_graph_prune",
    "ivr_graph_set_neighbors", "ivr_graph_search", "ivr_topk_merge",
    "ivr_topk_pack", "ivr_topk_merge_packed", "ivr_rowwise_cosine", "ivr_dedup_keep_mask", "ivr_scene_keep_mask",
    "ivr_scene_keep_mask_window", "ivr_frame_quality", "ivr_resize_u8", "ivr_phash", "ivr_hash_keep_mask", "ivr_kept_window_mask",
    "ivr_index_diversify", "ivr_index_search_fused", "ivr_index_range_search_fused", "ivr_index_search_moments",
    "ivr_index_range_search_moments", "ivr_index_tag_rows", "ivr_index_tag_segments", "ivr_index_video_scores",
    "ivr_index_video_search")}

_lib = None
_lock = threading.Lock()


class IvrError(RuntimeError):
    pass


def load():
    """Load libivr_hip.so; raises ImportError (never falls back) when it has not been built."""
    global _lib
    with _lock:
        if _lib is None:
            if not os.path.exists(LIB_PATH):
                raise ImportError(f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                                  "(hipcc --offload-arch=gfx950); there is no CPU fallback")
            # torch must load its HIP runtime first: the process has to end up with ONE libamdhip64, the one
            # torch's allocator and streams live in (loading ours first leaves two runtimes and no visible device)
            import torch  # noqa: F401
            lib = C.CDLL(LIB_PATH)
            for name, (res, args) in _SIGS.items():
                fn = getattr(lib, name)
                fn.restype = res
                fn.argtypes = args
            _lib = lib
    return _lib


def check(rc, what=""):
    if rc == 0:
        return
    msg = (load().ivr_last_error(None) or b"").decode("utf-8", "replace")
    text = f"{what}: {msg}" if what else msg
    if rc == -1:
        raise ValueError(text)
    if rc == -3:
        raise MemoryError(text)
    raise IvrError(text)


_ctxs = {}


def context(device=0):
    """One ivr_ctx per device per process."""
    with _lock:
        ctx = _ctxs.get(device)
    if ctx is None:
        lib = load()
        h = _p()
        check(lib.ivr_init(int(device), C.byref(h)), "ivr_init")
        with _lock:
            ctx = _ctxs.setdefault(device, h)
    return ctx


def device_info(device=0):
    lib = load()
    cu, hbm = _i(), _i64()
    arch = C.create_string_buffer(64)
    check(lib.ivr_device_info(context(device), C.byref(cu), C.byref(hbm), arch, 64))
    return {"cu_count": cu.value, "hbm_bytes": hbm.value, "arch": arch.value.decode()}


def stream_ptr(stream=None):
    """hipStream_t of a torch stream (default: torch's current stream) as an integer for ctypes."""
    import torch
    s = stream if stream is not None else torch.cuda.current_stream()
    return C.c_void_p(s.cuda_stream)


def f3(v):
    return (_f * 3)(*[float(x) for x in v])


CTX = object()      # in an ivr_ctx* slot of call(): the context of `device`, made (on first use) with that device current


def _plan(argtypes):
    """The slots of one export by how call() treats them: addresses (c_void_p), integers, floats, and (slot, T) for POINTER(T).
    What is left (char*, and a POINTER slot given anything but a T) goes to ctypes as it is."""
    at = lambda *ts: tuple(i for i, t in enumerate(argtypes) if t in ts)     # noqa: E731
    refs = tuple((i, t._type_) for i, t in enumerate(argtypes) if isinstance(getattr(t, "_type_", None), type))
    return len(argtypes), at(_p), at(_i, _i64), at(_f), refs


_PLANS = {n: _plan(sig[1]) for n, sig in _SIGS.items()}


def _call(name, args, device, what):
    n, ptrs, ints, floats, refs = _PLANS[name]
    slot = _STREAM.get(name)
    if len(args) == n - 1 and slot is not None:
        args = args[:slot] + (stream_ptr(),) + args[slot:]
    elif len(args) != n:
        raise TypeError(f"{name} takes {n} arguments{' (the stream may be left out)' if slot is not None else ''}, got {len(args)}")
    out = list(args)
    for i in ptrs:
        a = out[i]
        ptr = getattr(a, "data_ptr", None)
        if ptr is not None:
            out[i] = ptr()
        elif a is CTX and device is not None:
            out[i] = context(device if isinstance(device, int) else device.index)
        elif not (a is None or isinstance(a, (int, C.c_void_p, C.Array))):
            raise TypeError(f"{name}: argument {i} takes a tensor, None, an address or a c_void_p, got {type(a).__name__}")
    for i in ints:
        if not isinstance(out[i], int):                 # bool included; anything else must be an integer type (numpy.int64), as for ctypes
            try:
                out[i] = operator.index(out[i])
            except TypeError:
                raise TypeError(f"{name}: argument {i} takes an int, got {type(out[i]).__name__}") from None
    for i in floats:
        if not isinstance(out[i], float):
            raise TypeError(f"{name}: argument {i} takes a float, got {type(out[i]).__name__}")
    for i, T in refs:
        if isinstance(out[i], T):
            out[i] = C.byref(out[i])
    rc = getattr(_lib or load(), name)(*out)
    if name in _VALUE:
        return rc
    check(rc, what or name)


def call(name, *args, device=None, what=None):
    """The one way the package calls the library: lib.<name>(*args), marshalled from _SIGS[name].
      c_void_p slot      a torch tensor (its data_ptr()), None, an address, a c_void_p, or CTX (the ivr_ctx of `device`)
      int / float slot   an int, a bool or a numpy integer / a float
      POINTER(T) slot    a T (passed by reference), or whatever ctypes takes there (None, an array)
    device: the call runs under torch.cuda.device(device).  A stream slot the caller leaves out is filled with the current stream
    (of `device` when given).  A status goes through check(rc, what or name); the value exports (_VALUE) return their value."""
    if device is None:
        return _call(name, args, None, what)
    import torch
    with torch.cuda.device(device):
        return _call(name, args, device, what)


class Handle:
    """Base of the objects that own one library handle (an index, a tower): _lib, _h, device, close() / __del__, and _call, which
    supplies the handle, the device and the stream.  A subclass names its destroy export and opens the handle with _open."""
    _DESTROY = None
    _h = None

    def _open(self, create, device, *args):
        """self._h = the handle that `create`(ctx, *args, &handle) makes on `device` (None: the current device)."""
        import torch
        self._lib = load()
        self.device = torch.device("cuda", torch.cuda.current_device() if device is None else int(device))
        h = _p()
        call(create, CTX, *args, h, device=self.device)
        self._h = h

    def _call(self, name, *args, what=None):
        import torch
        with torch.cuda.device(self.device):
            return _call(name, (self._h,) + args, self.device, what)

    def close(self):
        h, self._h = self._h, None
        if h:
            getattr(self._lib, self._DESTROY)(h)        # the status of a destroy is dropped

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def profile_enable(on=True, device=0):
    """on: False / True (level 1: the kernels that carry a step) / 2 (also the short search-tail and append launches)."""
    check(load().ivr_profile_enable(context(device), int(on)))


def profile_reset(device=0):
    check(load().ivr_profile_reset(context(device)))


def profile_read(device=0):
    """{"kernel": {"launches", "ms", "work"}} measured with HIP events on the launch stream."""
    import json
    buf = C.create_string_buffer(1 << 16)
    check(load().ivr_profile_json(context(device), buf, len(buf)))
    return json.loads(buf.value.decode())
