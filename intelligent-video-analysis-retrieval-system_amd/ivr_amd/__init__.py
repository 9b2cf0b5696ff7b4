"""ivr_amd: the HIP-backed pieces of the retrieval system.  The submodules are imported by name (ivr_amd.index, ivr_amd.tower, ...);
the inverted-file indexes (flat rows, product-quantised and scalar-quantised codes), the binary / LSH indexes, the graph index, the re-ranking index, the product-quantisation (8- and 4-bit codes) and scalar-quantisation indexes
and the clip search, the event search, the grouped search, the moment search, the diversified search, the fused search, the frame clustering, the neighbour graph, the zero-shot tagging, the video search and the perceptual hash with its look-back filters are also reachable from the package itself, resolved on first use so that importing the package stays free of side effects."""
_IVF = ("IVFFlatIndex", "IndexIVFFlat", "SearchParametersIVF", "METRIC_INNER_PRODUCT", "METRIC_L2")
_BINARY = ("BinaryFlatIndex", "IndexBinaryFlat", "IndexLSH", "lsh_rotation")
_GRAPH = ("GraphFlatIndex", "IndexHNSWFlat", "SearchParametersHNSW", "graph_prune_ref", "graph_link_ref", "graph_build_ref",
          "graph_search_ref")
_REFINE = ("RefineFlatIndex", "IndexRefineFlat", "IndexRefineSearchParameters", "refine_order_ref")
_PQ = ("PQIndex", "IndexPQ", "pq_encode_ref", "pq_tables_ref", "pq_scan_ref")
_PQFS = ("PQFastScanIndex", "IndexPQFastScan", "pqfs_pack_ref", "pqfs_unpack_ref", "pqfs_encode_ref", "pqfs_tables_ref",
         "pqfs_quantize_ref", "pqfs_scan_ref", "pqfs_score_bound")
_SQ = ("SQIndex", "IndexScalarQuantizer", "ScalarQuantizer", "sq_encode_ref", "sq_decode_ref", "sq_query_ref", "sq_scan_ref")
_IVFPQ = ("IVFPQIndex", "IndexIVFPQ", "ivfpq_scan_ref", "ivfpq_pack_ref", "ivfpq_unpack_ref")
_IVFSQ = ("IVFSQIndex", "IndexIVFScalarQuantizer", "ivfsq_scan_ref", "ivfsq_pack_ref", "ivfsq_unpack_ref", "ivfsq_score_bound")
_TEMPORAL = ("TemporalAnalyzer", "sequence_search", "sequence_search_device", "sequence_range_search", "sequence_range_search_device",
             "sequence_scores_ref", "sequence_search_ref", "sequence_range_ref", "event_search", "event_search_device",
             "event_best_per_segment", "event_best_per_segment_device", "event_scores_ref", "event_search_ref",
             "event_best_per_segment_ref")
_GROUPING = ("group_search", "group_search_device", "best_per_segment", "best_per_segment_device", "group_search_ref",
             "best_per_segment_ref", "seg_off_from_labels")
_MOMENTS = ("moment_search", "moment_search_device", "moment_range_search", "moment_range_search_device", "moments_ref",
            "moment_search_ref", "moment_range_search_ref", "moment_block_rows")
_DIVERSIFY = ("mmr_search", "mmr_search_device", "dedup_search", "dedup_search_device", "mmr_rerank", "mmr_rerank_device",
              "suppress_rerank", "suppress_rerank_device", "mmr_ref", "suppress_ref")
_FUSION = ("fused_search", "fused_search_device", "fused_range_search", "fused_range_search_device", "fused_scores_ref",
           "fused_search_ref", "fused_range_search_ref", "fused_tables")
_CLUSTER = ("dbscan", "dbscan_device", "dbscan_ref", "cluster_members", "select_representatives", "representatives_ref",
            "cluster_similar_frames", "select_representative_frame")
_NEIGHBORS = ("knn_graph", "knn_graph_device", "knn_graph_ref", "similarity_graphs", "build_similarity_relationships")
_TAGGING = ("tag_rows", "tag_rows_device", "tag_segments", "tag_segments_device", "tag_rows_ref", "tag_segments_ref", "tag_prob_bound",
            "zero_shot_labels")
_VIDEOS = ("video_scores", "video_scores_device", "video_search", "video_search_device", "related_videos", "video_scores_ref",
           "video_search_ref", "video_sums_ref")
_KEYFRAMES = ("phash", "phash_device", "phash_ref", "hash_keep_mask", "hash_keep_mask_device", "hash_keep_mask_ref", "kept_window_mask",
              "kept_window_mask_device", "kept_window_mask_ref", "select_keyframes", "select_keyframes_ref", "AdvancedKeyframeExtractor",
              "PerceptualHash")
__all__ = list(_IVF + _BINARY + _GRAPH + _REFINE + _PQ + _PQFS + _SQ + _IVFPQ + _IVFSQ + _TEMPORAL + _GROUPING + _MOMENTS + _DIVERSIFY + _FUSION + _CLUSTER + _NEIGHBORS + _TAGGING + _VIDEOS + _KEYFRAMES)


def __getattr__(name):
    if name in _IVF:
        from . import ivf
        return getattr(ivf, name)
    if name in _BINARY:
        from . import binary
        return getattr(binary, name)
    if name in _GRAPH:
        from . import graph
        return getattr(graph, name)
    if name in _REFINE:
        from . import refine
        return getattr(refine, name)
    if name in _PQ:
        from . import pq
        return getattr(pq, name)
    if name in _PQFS:
        from . import pqfs
        return getattr(pqfs, name)
    if name in _SQ:
        from . import sq
        return getattr(sq, name)
    if name in _IVFPQ:
        from . import ivfpq
        return getattr(ivfpq, name)
    if name in _IVFSQ:
        from . import ivfsq
        return getattr(ivfsq, name)
    if name in _TEMPORAL:
        from . import temporal
        return getattr(temporal, name)
    if name in _GROUPING:
        from . import grouping
        return getattr(grouping, name)
    if name in _MOMENTS:
        from . import moments
        return getattr(moments, name)
    if name in _DIVERSIFY:
        from . import diversify
        return getattr(diversify, name)
    if name in _FUSION:
        from . import fusion
        return getattr(fusion, name)
    if name in _CLUSTER:
        from . import cluster
        return getattr(cluster, name)
    if name in _NEIGHBORS:
        from . import neighbors
        return getattr(neighbors, name)
    if name in _TAGGING:
        from . import tagging
        return getattr(tagging, name)
    if name in _VIDEOS:
        from . import videos
        return getattr(videos, name)
    if name in _KEYFRAMES:
        from . import keyframes
        return getattr(keyframes, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
