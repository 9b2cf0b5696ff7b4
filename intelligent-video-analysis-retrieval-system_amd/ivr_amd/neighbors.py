"""The neighbour graph: for every stored row of a FlatIPIndex its k best other rows of the same segment, optionally above a score.

Stands in for the reference's `MetadataManager._build_similarity_relationships` (`core.py:3493-3531`), which per folder builds the full
cosine matrix, sorts every row and keeps the top 10 others with cosine `> 0.7` (`get_similar_frames`, `core.py:3206`, reads the
result).  Here all folders are segments of one index and one call (ivr_index_knn_graph, csrc/knn.hip) runs a tiled self-join of the
stored rows with a running top-k per row: no matrix, no index per folder, no copy of the rows into a query buffer.

Definition (`knn_graph_ref` below is this in numpy, given the scores):

  S[j, i]     the float32 inner product `FlatIPIndex.search` / `rescore_device` report for (query = stored row j, stored row i).  S[j, i]
              is read with j as the query for every ordered pair; S[i, j] is never used in its place
  segments    seg_off (int64 [nseg+1], ascending, empty runs allowed) marks the folders, as in `dbscan` and clip search; rows outside
              [seg_off[0], seg_off[nseg]) have no neighbours and are nobody's neighbour.  None: the whole index is one segment
  candidates  of row j: the rows i != j of j's segment with i < ntotal whose score is not NaN, and S[j, i] > float32(threshold) when a
              threshold is given: strict, as the reference's `> 0.7`
  the row     itself is left out by its row number, not by its place in the order.  The reference drops the first entry of its
              descending sort, which among duplicate frames may be another row (the one stated departure)
  order       score descending, equal scores to the lower row: the project's key order
  D           float32 [ntotal, k], unused slots -FLT_MAX (a score of -0.0 is reported as +0.0, as by every top-k of the project)
  I           int64 [ntotal, k]: row numbers, on an id-mapped index too (as the labels of `dbscan`), unused slots -1
  count       int32 [ntotal]: the used slots of each row

The candidates of a row are totally ordered by unique keys, so every output has the same bits on every run and stream.
1 <= k <= ivr_knn_max_k() (64); ntotal < 2^31.
"""
import numpy as np
import torch

from . import _ffi, _staging
from .index import FlatIPIndex

SIMILAR_TOP = 10            # core.py:3522: [1:11]
SIMILAR_THRESHOLD = 0.7     # core.py:3524
NEG_FLT_MAX = -np.finfo(np.float32).max


def knn_max_k():
    return _ffi.call("ivr_knn_max_k")


# -- the definition in numpy ---------------------------------------------------------------------------------------------------
def knn_graph_ref(S, k, seg_off=None, threshold=None):
    """S float32 [N,N] scores (S[j, i]: query row j, stored row i) -> (D float32 [N,k], I int64 [N,k], count int32 [N]): the
    definition of the module docstring."""
    S = np.asarray(S, np.float32)
    if S.ndim != 2 or S.shape[0] != S.shape[1]:
        raise ValueError(f"knn_graph_ref: S {S.shape} must be [N,N]")
    n = S.shape[0]
    k, threshold = _staging.check_knn(k, threshold, _ffi.IVR_KNN_MAX_K, "knn_graph_ref")
    lo, hi = _staging.segment_bounds(n, seg_off)
    D = np.full((n, k), NEG_FLT_MAX, np.float32)
    I = np.full((n, k), -1, np.int64)
    count = np.zeros(n, np.int32)
    for j in range(n):
        i = np.arange(lo[j], hi[j], dtype=np.int64)
        s = S[j, lo[j]:hi[j]] + np.float32(0)                      # -0.0 counts and is reported as +0.0
        ok = (i != j) & ~np.isnan(s)
        if threshold != float("-inf"):
            with np.errstate(invalid="ignore"):
                ok &= s > np.float32(threshold)
        i, s = i[ok], s[ok]
        order = np.lexsort((i, -s.astype(np.float64)))[:k]         # score descending, then row ascending
        count[j] = len(order)
        D[j, :len(order)] = s[order]
        I[j, :len(order)] = i[order]
    return D, I, count


# -- the library calls ---------------------------------------------------------------------------------------------------------
def knn_graph_device(index, k, seg_off=None, threshold=None):
    """The neighbour graph of the stored rows on the device: (D float32 [ntotal,k], I int64 [ntotal,k], count int32 [ntotal]) CUDA
    tensors, the definition of the module docstring.  seg_off: integers [nseg+1], ascending (checked when it is a host array), or
    None.  No host synchronisation unless seg_off had to be staged."""
    if not isinstance(index, FlatIPIndex):
        raise ValueError(f"knn_graph: index must be a FlatIPIndex, got {type(index).__name__}")
    k, threshold = _staging.check_knn(k, threshold, knn_max_k(), "knn_graph")
    seg, staged, nseg = _staging.segments(seg_off, index.device, "knn_graph")
    n = index.ntotal
    D, I = _staging.alloc_DI(max(n, 1), k, index.device)             # never a NULL pointer, even for an empty index
    count = torch.empty(max(n, 1), dtype=torch.int32, device=index.device)
    index._call("ivr_index_knn_graph", k, seg, nseg, threshold, D, I, count)
    _staging.sync_if_staged(staged, index.device)
    return D[:n], I[:n], count[:n]


def knn_graph(index, k, seg_off=None, threshold=None):
    """knn_graph_device as numpy arrays (D, I, count)."""
    D, I, count = knn_graph_device(index, k, seg_off, threshold)
    return D.cpu().numpy(), I.cpu().numpy(), count.cpu().numpy()


# -- the reference's function ----------------------------------------------------------------------------------------------------
def similarity_graphs(index, seg_off, keys, top=SIMILAR_TOP, threshold=SIMILAR_THRESHOLD):
    """core.py:3493-3531 for all folders in one call: seg_off marks the folders among the stored rows, keys[r] names row r ->
    {key: [keys of its `top` most similar other rows of its folder with score > threshold, in rank order]} for every row inside a
    folder of at least two rows (the reference skips smaller ones).  One copy of the row numbers and counts to the host."""
    if len(keys) != index.ntotal:
        raise ValueError(f"similarity_graphs: {len(keys)} keys for {index.ntotal} rows")
    _, I, count = knn_graph_device(index, top, seg_off, threshold)
    host = torch.cat([I, count.to(torch.int64).reshape(-1, 1)], 1).cpu().numpy()
    off = seg_off.cpu().numpy() if isinstance(seg_off, torch.Tensor) else np.asarray(seg_off)
    lo, hi = _staging.segment_bounds(index.ntotal, off)
    out = {}
    for r in np.flatnonzero(hi - lo >= 2).tolist():
        out[keys[r]] = [keys[i] for i in host[r, :host[r, -1]].tolist()]
    return out


def build_similarity_relationships(folders, top=SIMILAR_TOP, threshold=SIMILAR_THRESHOLD):
    """core.py:3493-3531: folders = {folder name: (features [m,d], keys [m])} -> the merged {key: [similar keys]} of all folders.
    Folders of fewer than two rows are skipped, as in the reference; the rest are the segments of one temporary FlatIPIndex
    (normalize=True: the scores are cosines)."""
    feats, keys, off = [], [], [0]
    for features, names in folders.values():
        f = np.asarray(features, dtype=np.float32)
        if f.ndim != 2 or len(f) != len(names):
            raise ValueError(f"build_similarity_relationships: features {f.shape} for {len(names)} keys")
        if len(f) < 2:
            continue
        feats.append(f)
        keys.extend(names)
        off.append(off[-1] + len(f))
    if not feats:
        return {}
    x = np.ascontiguousarray(np.concatenate(feats))
    index = FlatIPIndex(x.shape[1], capacity=len(x))
    try:
        index.add(x, normalize=True)
        return similarity_graphs(index, np.asarray(off, np.int64), keys, top, threshold)
    finally:
        index.close()
