"""Grouped search: the best videos per query with their best frames, over a FlatIPIndex.

Every other search of the library ranks rows; a results page or a submission file ranks videos.  Adjacent keyframes of one shot sit
within a hair of each other in cosine, so the head of a row list routinely comes from three or four videos.  Here the rows are reduced
per segment (video) while they are scored and the best segments are returned with their best rows (ivr_index_search_groups /
ivr_index_best_per_segment, csrc/search_groups.hip).  Vector stores call this grouping search (Milvus) or collapse with inner hits
(Elasticsearch).

Definition (the `*_ref` functions below are this in numpy, to the bit, given the frame scores):

  S[q, r]    the float32 inner product `FlatIPIndex.search` reports for (query q, stored row r)
  order      rows rank by (S descending, row ascending), -0.0 equal to +0.0: the order of every top-k of the library
  segments   seg_off (int64 [nseg+1], ascending) marks the videos; empty segments form no group, rows outside
             [seg_off[0], seg_off[nseg]) belong to no group, offsets beyond the stored rows are clipped; without seg_off the index is one
             segment
  groups     a segment ranks by its best row in that order (equal best scores: the lower segment first); per query the best
             n_groups segments, and within each the group_size best rows of that segment

Rows are labelled with their number, or with their stored id on an id-mapped index; Gseg always holds segment numbers.  Unused group
slots hold -1 / -FLT_MAX / -1, unused row slots of a short segment -FLT_MAX / -1.
"""
import numpy as np
import torch

from . import _ffi, _staging
from ._faiss import FLT_MAX
from .index import FlatIPIndex
from .refine import _ordered

GROUP_MAX_ROWS = _ffi.IVR_GROUP_MAX_ROWS


def group_piece_rows():
    """Stored rows one workgroup's piece of a long segment covers at least (tests size their cases from it)."""
    return _ffi.call("ivr_group_piece_rows")


# -- the definition in numpy ---------------------------------------------------------------------------------------------------
def _scores(S, what):
    S = np.asarray(S, np.float32)
    if S.ndim != 2:
        raise ValueError(f"{what}: S {S.shape} must be [nq,N]")
    return S


def _ranges(N, seg_off):
    """[(lo, hi)] of every segment, clipped to [0, N]."""
    if seg_off is None:
        return [(0, N)]
    off = np.asarray(seg_off).astype(np.int64).reshape(-1)
    if len(off) < 2 or (off[1:] < off[:-1]).any():
        raise ValueError("seg_off must be [nseg+1] with nseg >= 1, ascending")
    return [(int(min(max(a, 0), N)), int(min(max(b, 0), N))) for a, b in zip(off[:-1], off[1:])]


def _check_sizes(n_groups, group_size, what):
    for name, v in (("n_groups", n_groups), ("group_size", group_size)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError(f"{what}: {name} must be an integer, got {type(v).__name__}")
    n_groups, group_size = int(n_groups), int(group_size)
    if n_groups < 1:
        raise ValueError(f"{what}: n_groups={n_groups} < 1")
    if group_size < 1 or group_size > GROUP_MAX_ROWS:
        raise ValueError(f"{what}: group_size={group_size} outside [1,{GROUP_MAX_ROWS}]")
    if n_groups * group_size > _ffi.IVR_MAX_K:
        raise ValueError(f"{what}: n_groups * group_size = {n_groups * group_size} > {_ffi.IVR_MAX_K}")
    return n_groups, group_size


def _ranked(s, lo, hi):
    """The rows [lo, hi) of one query's scores s, best first."""
    rows = np.arange(lo, hi, dtype=np.int64)
    return rows[np.lexsort((rows, -_ordered(s[lo:hi]).astype(np.int64)))]


def _labels(rows, ids):
    return rows if ids is None else np.asarray(ids).astype(np.int64)[rows]


def group_search_ref(S, n_groups, group_size, seg_off=None, ids=None):
    """S float32 [nq,N] frame scores -> (Gseg int64 [nq,G], D float32 [nq,G,g], I int64 [nq,G,g]), the definition of the module
    docstring.  ids: the labels of an id-mapped index (I = ids[row])."""
    S = _scores(S, "group_search_ref")
    G, g = _check_sizes(n_groups, group_size, "group_search_ref")
    nq, N = S.shape
    ranges = _ranges(N, seg_off)
    Gseg = np.full((nq, G), -1, np.int64)
    D = np.full((nq, G, g), -FLT_MAX, np.float32)
    I = np.full((nq, G, g), -1, np.int64)
    for q in range(nq):
        groups = []                                                # (-ordered best score, best row, segment, its rows best first)
        for j, (lo, hi) in enumerate(ranges):
            if lo < hi:
                rows = _ranked(S[q], lo, hi)
                groups.append((-int(_ordered(S[q, rows[0]])), int(rows[0]), j, rows[:g]))
        groups.sort(key=lambda t: t[:2])
        for slot, (_, _, j, rows) in enumerate(groups[:G]):
            Gseg[q, slot] = j
            D[q, slot, :len(rows)] = S[q, rows] + np.float32(0.0)
            I[q, slot, :len(rows)] = _labels(rows, ids)
    return Gseg, D, I


def best_per_segment_ref(S, seg_off=None, ids=None):
    """(D float32 [nq,nseg], I int64 [nq,nseg]): the best row of every segment and its score, (-FLT_MAX, -1) for an empty one.
    nseg = 1 without seg_off."""
    S = _scores(S, "best_per_segment_ref")
    nq, N = S.shape
    ranges = _ranges(N, seg_off)
    D = np.full((nq, len(ranges)), -FLT_MAX, np.float32)
    I = np.full((nq, len(ranges)), -1, np.int64)
    for q in range(nq):
        for j, (lo, hi) in enumerate(ranges):
            if lo < hi:
                r = _ranked(S[q], lo, hi)[0]
                D[q, j] = S[q, r] + np.float32(0.0)
                I[q, j] = _labels(r, ids)
    return D, I


def seg_off_from_labels(labels):
    """Per-row labels (folder names, video ids, ...) -> seg_off int64 [nseg+1]: one segment per run of equal labels, in row order.
    Raises ValueError when the rows of a label are not contiguous."""
    labels = list(labels)
    off, seen = [0], set()
    for i, lab in enumerate(labels):
        if i and lab == labels[i - 1]:
            continue
        if lab in seen:
            raise ValueError(f"seg_off_from_labels: the rows of label {lab!r} are not contiguous (row {i} starts a second run)")
        seen.add(lab)
        if i:
            off.append(i)
    off.append(len(labels))                                        # no rows: one empty segment
    return np.asarray(off, np.int64)


# -- the library calls ---------------------------------------------------------------------------------------------------------
def _stage(index, x, seg_off, what):
    """The checked arguments of both calls: (queries tensor [nq,d], staged, nq, seg_off tensor or None, nseg)."""
    if not isinstance(index, FlatIPIndex):
        raise ValueError(f"{what}: index must be a FlatIPIndex, got {type(index).__name__}")
    seg, seg_staged, nseg = _staging.segments(seg_off, index.device, what)
    t, staged = _staging.queries_f32(_staging.as_rows(x), index.d, index.device)
    _staging.check_nq(t.shape[0], what)
    return t, staged or seg_staged, int(t.shape[0]), seg, nseg


def group_search_device(index, x, n_groups, group_size=1, seg_off=None, normalize=False):
    """Grouped search on the device: x float32 [nq,d] (numpy or torch) -> (Gseg int64 [nq,G], D float32 [nq,G,g], I int64 [nq,G,g])
    CUDA tensors, the definition of group_search_ref.  seg_off: integers [nseg+1], ascending (checked when it is a host array), or
    None.  No host synchronisation unless an argument had to be staged."""
    G, g = _check_sizes(n_groups, group_size, "group_search")
    t, staged, nq, seg, nseg = _stage(index, x, seg_off, "group_search")
    Gseg = torch.empty((nq, G), dtype=torch.int64, device=index.device)
    D = torch.empty((nq, G, g), dtype=torch.float32, device=index.device)
    I = torch.empty((nq, G, g), dtype=torch.int64, device=index.device)
    index._call("ivr_index_search_groups", t, nq, seg, nseg, G, g, bool(normalize), Gseg, D, I)
    _staging.sync_if_staged(staged, index.device)
    return Gseg, D, I


def group_search(index, x, n_groups, group_size=1, seg_off=None, normalize=False):
    """group_search_device as numpy arrays (Gseg, D, I)."""
    Gseg, D, I = group_search_device(index, x, n_groups, group_size, seg_off, normalize)
    return Gseg.cpu().numpy(), D.cpu().numpy(), I.cpu().numpy()


def best_per_segment_device(index, x, seg_off, normalize=False):
    """The best row of every segment on the device: (D float32 [nq,nseg], I int64 [nq,nseg]) CUDA tensors, the definition of
    best_per_segment_ref: the video-level score of every video in one call.  nseg = 1 without seg_off."""
    t, staged, nq, seg, nseg = _stage(index, x, seg_off, "best_per_segment")
    if nq * max(nseg, 1) >= 2**31:
        raise ValueError(f"best_per_segment: nq * nseg = {nq * nseg} >= 2^31")
    D, I = _staging.alloc_DI(nq, max(nseg, 1), index.device)
    index._call("ivr_index_best_per_segment", t, nq, seg, nseg, bool(normalize), D, I)
    _staging.sync_if_staged(staged, index.device)
    return D, I


def best_per_segment(index, x, seg_off, normalize=False):
    """best_per_segment_device as numpy arrays (D, I)."""
    D, I = best_per_segment_device(index, x, seg_off, normalize)
    return D.cpu().numpy(), I.cpu().numpy()
