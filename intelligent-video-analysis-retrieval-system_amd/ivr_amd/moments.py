"""Moment search: the ranked time intervals of a query, over a FlatIPIndex.

Every other search of the library answers with rows (frames) or with whole videos; a retrieval page shows moments, "video X, frames
412 - 447".  A text query that matches a shot matches a run of adjacent keyframes: `search` fills its list with that run,
`group_search` collapses it to the video, `range_search` leaves the merging of neighbours to the host.  Here the rows above a score
are merged into intervals on the device (ivr_index_search_moments / ivr_index_range_search_moments, csrc/search_moments.hip).  The
reference attaches the +-3 neighbouring frames to a hit as an unscored `temporal_context` (system.py:1967-1974); a moment is the
scored form of that: the extent around a hit inside which the query keeps matching.

Definition (the `*_ref` functions below are this in numpy, to the bit, given the frame scores):

  S[q, r]    the float32 inner product `FlatIPIndex.search` reports for (query q, stored row r)
  segments   seg_off (int64 [nseg+1], ascending) marks the videos; empty segments are allowed, rows outside
             [seg_off[0], seg_off[nseg]) belong to nothing, offsets beyond the stored rows are clipped; without seg_off the index is
             one segment
  hot        row r is hot for q when it belongs to a segment and S[q, r] >= threshold (a NaN score is never hot)
  head       prev(r) = the greatest hot row below r; a hot row is a head when prev(r) is none, lies in another segment, or
             r - prev(r) > max_gap + 1 (more than max_gap cold rows between them: max_gap bridges a blink or one bad keyframe)
  moment     a head and the hot rows behind it up to the next head: lo (the head), hi (its last hot row, inclusive), cnt (its hot
             rows), peak (its best hot row in the order of every top-k: score descending, row ascending, -0.0 equal to +0.0)

Per moment D = S[q, peak] + 0.0, I = the peak's row number, or its stored id on an id-mapped index; Lo, Hi and Cnt are always row
numbers and counts.  `moment_range_search` returns every moment of every query in ascending lo (lims / cap as `range_search`);
`moment_search` the best k per query among those with cnt >= min_count, by peak key (rank="peak": equal scores, the lower peak row
first) or by cnt descending (rank="count": equal counts, the lower lo first); unused slots hold -FLT_MAX / -1 / -1 / -1 / 0.  A mean
score per moment is left out on purpose: a float sum over a moment has no parallel order that is also the obvious numpy one; the
caller can `rescore_device` over [Lo, Hi].
"""
import numpy as np
import torch

from . import _ffi, _staging
from ._faiss import FLT_MAX
from .grouping import _labels, _ranges, _scores
from .index import FlatIPIndex
from .refine import _ordered

MAX_GAP_LIMIT = 2**31 - 2


def moment_block_rows():
    """Stored rows one workgroup of the run passes covers (tests size their cases from it)."""
    return _ffi.call("ivr_moment_block_rows")


# -- argument checks ---------------------------------------------------------------------------------------------------------------
def _check_int(v, name, what):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
        raise ValueError(f"{what}: {name} must be an integer, got {type(v).__name__}")
    return int(v)


def _check_threshold(threshold, what):
    if isinstance(threshold, bool) or not isinstance(threshold, (int, float, np.integer, np.floating)):
        raise ValueError(f"{what}: threshold must be a number, got {type(threshold).__name__}")
    threshold = float(np.float32(threshold))
    if threshold != threshold:
        raise ValueError(f"{what}: threshold={threshold} is NaN")
    return threshold


def _check_gap(max_gap, what):
    max_gap = _check_int(max_gap, "max_gap", what)
    if max_gap < 0 or max_gap > MAX_GAP_LIMIT:
        raise ValueError(f"{what}: max_gap={max_gap} outside [0,2^31-2]")
    return max_gap


def _check_topk(k, min_count, rank, what):
    k = _check_int(k, "k", what)
    if k < 1 or k > _ffi.IVR_MAX_K:
        raise ValueError(f"{what}: k={k} outside [1,{_ffi.IVR_MAX_K}]")
    min_count = _check_int(min_count, "min_count", what)
    if min_count < 1:
        raise ValueError(f"{what}: min_count={min_count} < 1")
    if rank not in _ffi.IVR_MOMENT_RANK:
        raise ValueError(f"{what}: rank={rank!r} is neither 'peak' nor 'count'")
    return k, min(min_count, 2**31 - 1), _ffi.IVR_MOMENT_RANK[rank]


# -- the definition in numpy -------------------------------------------------------------------------------------------------------
def moments_ref(S, threshold, max_gap, seg_off=None):
    """S float32 [nq,N] frame scores -> per query the int64 array [m,4] of its moments (lo, hi, cnt, peak row) in ascending lo: the
    definition of the module docstring."""
    S = _scores(S, "moments_ref")
    threshold = np.float32(_check_threshold(threshold, "moments_ref"))
    max_gap = _check_gap(max_gap, "moments_ref")
    nq, N = S.shape
    seg = np.full(N, -1, np.int64)
    for j, (lo, hi) in enumerate(_ranges(N, seg_off)):
        seg[lo:hi] = j
    out = []
    for q in range(nq):
        with np.errstate(invalid="ignore"):
            hot = np.flatnonzero((seg >= 0) & (S[q] >= threshold))
        if not len(hot):
            out.append(np.zeros((0, 4), np.int64))
            continue
        head = np.ones(len(hot), bool)
        head[1:] = (seg[hot[1:]] != seg[hot[:-1]]) | (hot[1:] - hot[:-1] > max_gap + 1)
        starts = np.flatnonzero(head)
        ends = np.append(starts[1:], len(hot))
        key = _ordered(S[q, hot]).astype(np.int64)
        rows = np.empty((len(starts), 4), np.int64)
        for i, (a, b) in enumerate(zip(starts, ends)):
            rows[i] = hot[a], hot[b - 1], b - a, hot[a + np.argmax(key[a:b])]       # argmax: the first = the lowest row of the best score
        out.append(rows)
    return out


def moment_search_ref(S, k, threshold, max_gap=0, min_count=1, rank="peak", seg_off=None, ids=None):
    """(D float32 [nq,k], I int64 [nq,k], Lo, Hi, Cnt int64 [nq,k]): the best k moments per query.  ids: the labels of an id-mapped
    index (I = ids[peak])."""
    S = _scores(S, "moment_search_ref")
    k, min_count, rank = _check_topk(k, min_count, rank, "moment_search_ref")
    nq = S.shape[0]
    D = np.full((nq, k), -FLT_MAX, np.float32)
    I, Lo, Hi = (np.full((nq, k), -1, np.int64) for _ in range(3))
    Cnt = np.zeros((nq, k), np.int64)
    for q, m in enumerate(moments_ref(S, threshold, max_gap, seg_off)):
        m = m[m[:, 2] >= min_count]
        if rank == _ffi.IVR_MOMENT_RANK["count"]:
            order = np.lexsort((m[:, 0], -m[:, 2]))
        else:
            order = np.lexsort((m[:, 3], -_ordered(S[q, m[:, 3]]).astype(np.int64)))
        m = m[order[:k]]
        n = len(m)
        D[q, :n] = S[q, m[:, 3]] + np.float32(0.0)
        I[q, :n] = _labels(m[:, 3], ids)
        Lo[q, :n], Hi[q, :n], Cnt[q, :n] = m[:, 0], m[:, 1], m[:, 2]
    return D, I, Lo, Hi, Cnt


def moment_range_search_ref(S, threshold, max_gap=0, seg_off=None, ids=None):
    """(lims int64 [nq+1], D float32 [total], I, Lo, Hi, Cnt int64 [total]): every moment of every query in ascending lo."""
    S = _scores(S, "moment_range_search_ref")
    per = moments_ref(S, threshold, max_gap, seg_off)
    lims = np.zeros(len(per) + 1, np.int64)
    lims[1:] = np.cumsum([len(m) for m in per])
    m = np.concatenate(per) if per else np.zeros((0, 4), np.int64)
    qs = np.repeat(np.arange(len(per)), [len(p) for p in per])
    D = (S[qs, m[:, 3]] + np.float32(0.0)).astype(np.float32)
    return lims, D, _labels(m[:, 3], ids).astype(np.int64), m[:, 0].copy(), m[:, 1].copy(), m[:, 2].copy()


# -- the library calls -------------------------------------------------------------------------------------------------------------
def _stage(index, x, threshold, max_gap, seg_off, what):
    """The checked arguments of both calls: (queries tensor [nq,d], staged, nq, seg_off tensor or None, nseg, threshold, max_gap)."""
    if not isinstance(index, FlatIPIndex):
        raise ValueError(f"{what}: index must be a FlatIPIndex, got {type(index).__name__}")
    threshold = _check_threshold(threshold, what)
    max_gap = _check_gap(max_gap, what)
    seg, seg_staged, nseg = _staging.segments(seg_off, index.device, what)
    t, staged = _staging.queries_f32(_staging.as_rows(x), index.d, index.device)
    _staging.check_nq(t.shape[0], what)
    return t, staged or seg_staged, int(t.shape[0]), seg, nseg, threshold, max_gap


def moment_search_device(index, x, k, threshold, max_gap=0, min_count=1, rank="peak", seg_off=None, normalize=False):
    """The best k moments per query on the device: x float32 [nq,d] (numpy or torch) -> (D float32 [nq,k], I, Lo, Hi, Cnt int64
    [nq,k]) CUDA tensors, the definition of moment_search_ref.  seg_off: integers [nseg+1], ascending (checked when it is a host
    array), or None.  No host synchronisation unless an argument had to be staged."""
    k, min_count, rank = _check_topk(k, min_count, rank, "moment_search")
    t, staged, nq, seg, nseg, threshold, max_gap = _stage(index, x, threshold, max_gap, seg_off, "moment_search")
    D = torch.empty((nq, k), dtype=torch.float32, device=index.device)
    I, Lo, Hi, Cnt = (torch.empty((nq, k), dtype=torch.int64, device=index.device) for _ in range(4))
    index._call("ivr_index_search_moments", t, nq, seg, nseg, threshold, max_gap, min_count, rank, k, bool(normalize), D, I, Lo, Hi, Cnt)
    _staging.sync_if_staged(staged, index.device)
    return D, I, Lo, Hi, Cnt


def moment_search(index, x, k, threshold, max_gap=0, min_count=1, rank="peak", seg_off=None, normalize=False):
    """moment_search_device as numpy arrays (D, I, Lo, Hi, Cnt)."""
    return tuple(t.cpu().numpy() for t in moment_search_device(index, x, k, threshold, max_gap, min_count, rank, seg_off, normalize))


def moment_range_search_device(index, x, threshold, max_gap=0, seg_off=None, normalize=False, cap=None):
    """Every moment of every query on the device: (lims int64 [nq+1], D float32 [cap], I, Lo, Hi, Cnt int64 [cap], total) CUDA
    tensors, total = lims[nq:] (the number of moments; entries at positions >= cap are counted but not written).  No host
    synchronisation when `cap` is given; cap=None sizes the outputs exactly: a counting pass with cap 0, one synchronisation, then
    the exact pass."""
    t, staged, nq, seg, nseg, threshold, max_gap = _stage(index, x, threshold, max_gap, seg_off, "moment_range_search")
    if cap is not None:
        cap = _check_int(cap, "cap", "moment_range_search")
        if cap < 0:
            raise ValueError(f"moment_range_search: cap={cap} < 0")
    lims = torch.empty(nq + 1, dtype=torch.int64, device=index.device)

    def run(c):
        D = torch.empty(max(c, 1), dtype=torch.float32, device=index.device)      # never a NULL pointer, even for cap 0
        I, Lo, Hi, Cnt = (torch.empty(max(c, 1), dtype=torch.int64, device=index.device) for _ in range(4))
        index._call("ivr_index_range_search_moments", t, nq, seg, nseg, threshold, max_gap, bool(normalize), lims, D, I, Lo, Hi, Cnt, c)
        return D[:c], I[:c], Lo[:c], Hi[:c], Cnt[:c]

    with torch.cuda.device(index.device):
        if cap is None:
            run(0)
            cap = int(lims[nq].item())
        out = run(cap)
        _staging.sync_if_staged(staged)
    return (lims,) + out + (lims[nq:],)


def moment_range_search(index, x, threshold, max_gap=0, seg_off=None, normalize=False):
    """(lims, D, I, Lo, Hi, Cnt) numpy arrays, sized in two passes as FlatIPIndex.range_search_device(cap=None) does."""
    return tuple(t.cpu().numpy() for t in moment_range_search_device(index, x, threshold, max_gap, seg_off, normalize)[:6])
