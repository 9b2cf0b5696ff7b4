"""Frame clustering: which stored rows of a FlatIPIndex are the same shot, and which row stands for each group?

Stands in for the reference's `AdvancedKeyframeExtractor.cluster_similar_frames` / `select_representative_frame`
(`filter_research_update.py:113-155`): per scene the full `1 - cosine_similarity` matrix, sklearn's
`DBSCAN(eps=0.05, min_samples=2, metric="precomputed")` on it, and per cluster the frame closest to the cluster's mean.  Here the scores
are the float32 inner products of the flat index, the clustering is a tiled self-join of the stored rows in three passes on the GPU
(ivr_index_dbscan, csrc/cluster.hip) that never holds a matrix, and the representative is a gather, a segment mean and one
best-cosine kernel (ivr_segment_best_cosine).

Definition (`dbscan_ref` below is this in numpy, given the scores):

  S[q, r]   the float32 inner product `FlatIPIndex.search` reports for (query = stored row q, stored row r)
  edge      for rows i < j, {i, j} is an edge iff both lie in the same segment and float32(1) - S[j, i] <= float32(eps): one rounded
            float32 subtraction, `<=` as sklearn's test.  Only S[j, i] is read, the higher row as the query, so adjacency is symmetric
            by construction; S[i, i] is not read
  segments  seg_off (int64 [nseg+1], ascending, empty runs allowed) marks the scenes, as in clip search; rows outside
            [seg_off[0], seg_off[nseg]) belong to nothing: not core, label -1.  None: the whole index is one segment
  core      row i is core iff 1 + (edges at i) >= min_samples.  A row always counts itself; sklearn reads the diagonal distance instead,
            so it differs for a zero row or an eps below about 1e-6 (the one departure)
  cluster   a connected component of the core rows under edges; its root is its lowest core row
  border    a non-core row with at least one core neighbour takes the cluster with the lowest root among its core neighbours (sklearn
            grows cluster 0 completely before it starts cluster 1, so this is its rule); every other non-core row is noise
  labels    int32: the rank of the cluster's root among the roots of the row's own segment, ascending from 0, -1 for noise.  Numbering
            restarts in every segment, because the reference clusters scene by scene

With unit rows S is the cosine and 1 - S sklearn's precomputed distance.  Labels are indexed by row on plain and id-mapped indexes
alike.  Every result is an integer: the same output on every run.
"""
import numpy as np
import torch

from . import _ffi, _staging
from .index import FlatIPIndex

CLUSTER_EPS = 0.05          # filter_research_update.py: CLUSTER_EPS
MIN_CLUSTER_SIZE = 2        # filter_research_update.py: MIN_CLUSTER_SIZE


# -- the definition in numpy ---------------------------------------------------------------------------------------------------
def dbscan_ref(S, eps, min_samples, seg_off=None):
    """S float32 [N,N] scores (S[q, r]: query row q, stored row r) -> (labels int32 [N], core uint8 [N], nclusters int32
    [max(nseg, 1)]): the definition of the module docstring."""
    S = np.asarray(S, np.float32)
    if S.ndim != 2 or S.shape[0] != S.shape[1]:
        raise ValueError(f"dbscan_ref: S {S.shape} must be [N,N]")
    eps, min_samples = _staging.check_dbscan(eps, min_samples, "dbscan_ref")
    n = S.shape[0]
    lo, _ = _staging.segment_bounds(n, seg_off)                    # the start of row j's segment, j + 1 outside every segment
    adj = np.zeros((n, n), bool)
    for j in range(n):
        if lo[j] < j:
            adj[j, lo[j]:j] = (np.float32(1) - S[j, lo[j]:j]) <= np.float32(eps)
    adj |= adj.T
    rows = np.arange(n)
    core = (lo <= rows) & (1 + adj.sum(1) >= min_samples)
    root = np.full(n, -1, np.int64)                                # of the row's cluster; -1: noise
    for i in rows[core]:                                           # ascending, so a component is first met at its lowest row
        if root[i] >= 0:
            continue
        root[i] = i
        todo = [i]
        while todo:
            nb = np.flatnonzero(adj[todo.pop()] & core & (root < 0))
            root[nb] = i
            todo.extend(nb.tolist())
    for i in rows[~core]:
        nb = np.flatnonzero(adj[i] & core)
        if len(nb):
            root[i] = root[nb].min()
    is_root = core & (root == rows)
    before = np.concatenate([[0], np.cumsum(is_root)])             # roots among the rows below
    labels = np.full(n, -1, np.int32)
    got = root >= 0
    labels[got] = before[root[got]] - before[lo[got]]
    if seg_off is None:
        ncl = before[n:]
    else:
        off = np.clip(np.asarray(seg_off).astype(np.int64).reshape(-1), 0, n)
        ncl = before[off[1:]] - before[off[:-1]]
    return labels, core.astype(np.uint8), ncl.astype(np.int32)


def _fma32(x, y, acc):
    """float32 fma(x, y, acc) of float32 arrays with its single rounding: the exact product and the sum in float64, rounded to odd
    (the float64 sum's error decides the last bit) so that the rounding to float32 is the only one that counts."""
    p = x.astype(np.float64) * y.astype(np.float64)
    a = acc.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        s = p + a
        t = s - p
        err = (p - (s - t)) + (a - t)
        even = (s.view(np.int64) & 1) == 0
        s = np.where((err != 0) & even, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
    return s.astype(np.float32)


def _wave_dot(a, b):
    """float32 [n]: sum_k a[i, k] b[i, k] as one wave computes it (rowwise_cosine_kernel): lane l runs an fma chain over the columns
    l, l + 64, ..., then the 64 lane sums are added pairwise in a balanced tree."""
    n, d = a.shape
    pad = -d % 64
    a = np.pad(a, ((0, 0), (0, pad))).reshape(n, -1, 64)
    b = np.pad(b, ((0, 0), (0, pad))).reshape(n, -1, 64)
    v = np.zeros((n, 64), np.float32)
    for c in range(a.shape[1]):
        live = np.arange(64) + 64 * c < d
        v = np.where(live, _fma32(a[:, c], b[:, c], v), v)
    while v.shape[1] > 1:
        v = (v[:, 0::2] + v[:, 1::2]).astype(np.float32)
    return v[:, 0]


def _cosine32(a, b):
    """cos(a[i], b[i]) with the arithmetic of ivr_rowwise_cosine (a zero norm counts as 1)."""
    dot, sa, sb = _wave_dot(a, b), _wave_dot(a, a), _wave_dot(b, b)
    one = np.float32(1)
    na = np.where(sa > 0, np.sqrt(sa), one).astype(np.float32)
    nb = np.where(sb > 0, np.sqrt(sb), one).astype(np.float32)
    with np.errstate(invalid="ignore", divide="ignore"):
        return (dot / (na * nb).astype(np.float32)).astype(np.float32)


def _mean32(rows):
    """The normalised mean of float32 rows [cnt,d] with the arithmetic of ivr_segment_mean(normalize=1): columns summed in ascending
    row order in float64, the squares summed per thread (columns t, t + 256, ...) and over 256 threads by a halving tree."""
    cnt, d = rows.shape
    s = np.zeros(d, np.float64)
    for r in rows.astype(np.float64):
        s = s + r
    m = (s * (1.0 / cnt)).astype(np.float32)
    red = np.zeros(256, np.float64)
    for c in range(d):
        red[c % 256] += float(m[c]) * float(m[c])
    w = 128
    while w:
        red[:w] += red[w:2 * w]
        w >>= 1
    nrm = np.float32(np.sqrt(red[0])) if red[0] > 0 else np.float32(1)
    return (m / nrm).astype(np.float32)


def representatives_ref(X, cluster_off, members):
    """select_representatives in numpy, with the roundings of its kernels: X float32 [N,d] the stored rows, cluster c = the rows
    members[cluster_off[c] : cluster_off[c+1]] -> int64 [nclusters], per cluster the member with the largest float32 cosine to the
    cluster's normalised mean, equal cosines the earlier member, -1 for an empty cluster."""
    X = np.asarray(X, np.float32)
    off = np.asarray(cluster_off).astype(np.int64).reshape(-1)
    members = np.asarray(members).astype(np.int64).reshape(-1)
    reps = np.full(len(off) - 1, -1, np.int64)
    for c in range(len(off) - 1):
        m = members[off[c]:off[c + 1]]
        if not len(m):
            continue
        rows = X[m]
        cos = _cosine32(rows, np.broadcast_to(_mean32(rows), rows.shape))
        if not np.isnan(cos).all():
            reps[c] = m[int(np.nanargmax(cos))]
    return reps


# -- the library calls ---------------------------------------------------------------------------------------------------------
def dbscan_device(index, eps, min_samples=2, seg_off=None):
    """DBSCAN over the stored rows on the device: (labels int32 [ntotal], core uint8 [ntotal], nclusters int32 [max(nseg, 1)]) CUDA
    tensors, the definition of the module docstring.  seg_off: integers [nseg+1], ascending (checked when it is a host array), or
    None.  No host synchronisation unless seg_off had to be staged."""
    if not isinstance(index, FlatIPIndex):
        raise ValueError(f"dbscan: index must be a FlatIPIndex, got {type(index).__name__}")
    eps, min_samples = _staging.check_dbscan(eps, min_samples, "dbscan")
    seg, staged, nseg = _staging.segments(seg_off, index.device, "dbscan")
    n = index.ntotal
    labels = torch.empty(max(n, 1), dtype=torch.int32, device=index.device)            # never a NULL pointer, even for an empty index
    core = torch.empty(max(n, 1), dtype=torch.uint8, device=index.device)
    nclusters = torch.zeros(max(nseg, 1), dtype=torch.int32, device=index.device)      # an empty index writes nothing
    index._call("ivr_index_dbscan", eps, min_samples, seg, nseg, labels, core, nclusters)
    _staging.sync_if_staged(staged, index.device)
    return labels[:n], core[:n], nclusters


def dbscan(index, eps, min_samples=2, seg_off=None):
    """dbscan_device as numpy arrays (labels, core, nclusters)."""
    labels, core, nclusters = dbscan_device(index, eps, min_samples, seg_off)
    return labels.cpu().numpy(), core.cpu().numpy(), nclusters.cpu().numpy()


def _tensor(a, dtype):
    return (a if isinstance(a, torch.Tensor) else torch.as_tensor(np.asarray(a))).to(dtype)


def cluster_members(labels, nclusters, seg_off=None):
    """The output of dbscan as lists: (cluster_off int64 [total+1], members int64 [clustered rows]) on the device of `labels`.  The
    clusters are numbered segment by segment (total = nclusters.sum()), cluster c holds the rows members[cluster_off[c] :
    cluster_off[c+1]], ascending: the clustered rows in (segment, cluster, row) order.  Noise rows are left out.  One host
    synchronisation (the sizes depend on the labels)."""
    labels = _tensor(labels, torch.int64)
    dev = labels.device
    ncl = _tensor(nclusters, torch.int64).to(dev)
    rows = torch.nonzero(labels >= 0).reshape(-1)
    first = torch.cumsum(ncl, 0) - ncl                              # the number of the first cluster of each segment
    if seg_off is None:
        cluster = labels[rows]
    else:
        off = _tensor(seg_off, torch.int64).to(dev).contiguous()
        seg = torch.searchsorted(off, rows, right=True) - 1         # the last offset <= row
        cluster = first[seg] + labels[rows]
    cluster, order = torch.sort(cluster, stable=True)
    counts = torch.bincount(cluster, minlength=int(ncl.sum()))
    cluster_off = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(counts, 0)])
    return cluster_off, rows[order].contiguous()


def select_representatives(index, cluster_off, members):
    """Per cluster the member closest to the cluster's mean (filter_research_update.py:136-155), on the device: int64 CUDA tensor
    [nclusters] of row numbers, -1 for an empty cluster.  Four steps: ivr_index_gather of the members, ivr_segment_mean(normalize=1)
    with cluster_off as the segments, ivr_segment_best_cosine, and the map back to row numbers.  Equal cosines go to the lower
    position in `members`.  cluster_off / members: int64 CUDA tensors as cluster_members returns them.  No host synchronisation."""
    if not isinstance(index, FlatIPIndex):
        raise ValueError(f"select_representatives: index must be a FlatIPIndex, got {type(index).__name__}")
    dev = index.device
    for name, t in (("cluster_off", cluster_off), ("members", members)):
        if not (isinstance(t, torch.Tensor) and t.dtype == torch.int64 and t.dim() == 1 and t.is_contiguous() and t.device == dev):
            raise ValueError(f"select_representatives: {name} must be a contiguous int64 tensor [n] on {dev}")
    nclu = len(cluster_off) - 1
    if nclu < 1:
        return torch.empty(0, dtype=torch.int64, device=dev)
    rows = index.gather_device(members)
    centers = torch.empty((nclu, index.d), dtype=torch.float32, device=dev)
    _ffi.call("ivr_segment_mean", _ffi.CTX, rows, len(rows), cluster_off, nclu, index.d, True, centers, device=dev)
    best = torch.empty(nclu, dtype=torch.int64, device=dev)
    score = torch.empty(nclu, dtype=torch.float32, device=dev)
    _ffi.call("ivr_segment_best_cosine", _ffi.CTX, rows, len(rows), cluster_off, nclu, index.d, centers, best, score, device=dev)
    if not len(members):
        return best                                                 # every cluster empty: all -1
    return torch.where(best >= 0, members[best.clamp(min=0)], best)


# -- the reference's functions -------------------------------------------------------------------------------------------------
def _embedding_index(embeddings, normalize):
    x = np.ascontiguousarray(np.asarray(embeddings, dtype=np.float32))
    if x.ndim != 2:
        raise ValueError(f"embeddings must be [n,d], got {x.shape}")
    index = FlatIPIndex(x.shape[1])
    index.add(x, normalize=normalize)
    return index


def cluster_similar_frames(embeddings, frame_indices=None, eps=CLUSTER_EPS, min_samples=MIN_CLUSTER_SIZE):
    """filter_research_update.py:113-134: the frames of one scene as lists of positions, one list per DBSCAN label in order of first
    appearance; the noise frames (label -1) form one more list, as in the reference.  [[0]] for one frame, [] for none.  The rows go
    through a temporary FlatIPIndex with normalize=True (a zero row stays zero: cosine 0, as sklearn gives).  frame_indices is not
    read, as in the reference."""
    if len(embeddings) < 2:
        return [[0]] if len(embeddings) else []
    index = _embedding_index(embeddings, True)
    try:
        labels, _, _ = dbscan(index, eps, min_samples)
    finally:
        index.close()
    clusters = {}
    for idx, label in enumerate(labels.tolist()):
        clusters.setdefault(label, []).append(idx)
    return list(clusters.values())


def select_representative_frame(cluster_indices, embeddings, frame_info=None):
    """filter_research_update.py:136-155: the entry of cluster_indices whose embedding is closest (cosine) to the mean of the
    cluster's embeddings; equal cosines keep the earlier entry, a single entry is returned as it is.  frame_info is not read, as in
    the reference."""
    if len(cluster_indices) == 1:
        return cluster_indices[0]
    index = _embedding_index([embeddings[i] for i in cluster_indices], False)      # row p of the index = entry p of the cluster
    try:
        members = torch.arange(len(cluster_indices), dtype=torch.int64, device=index.device)
        off = torch.tensor([0, len(cluster_indices)], dtype=torch.int64, device=index.device)
        best = int(select_representatives(index, off, members).item())
    finally:
        index.close()
    return cluster_indices[max(best, 0)]                   # -1: every cosine is NaN; the reference keeps entry 0 then
