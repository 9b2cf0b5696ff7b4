"""Clip search: where in the stored rows of a FlatIPIndex does a run of L consecutive query frames occur?

Stands in for the reference's `TemporalAnalyzer` (`core.py:3560-3828`), whose `find_similar_sequences` (`core.py:3644-3702`) takes
every window of `sequence_length` target frames against every window of database frames in three nested Python loops around sklearn's
`cosine_similarity`.  Here the frame scores are the float32 inner products of the flat index, and the window sums, the segment test
and the top-k / threshold tails run on the GPU (ivr_index_search_sequences / ivr_index_range_search_sequences,
csrc/search_seq.hip).

Definition (the `*_ref` functions below are this in numpy, to the bit, given the frame scores):

  S[t, s]   the float32 inner product `FlatIPIndex.search` reports for (query frame t, stored row s)
  W[t, s]   (((S[t, s] + S[t+1, s+1]) + ...) + S[t+L-1, s+L-1]) / float32(L) for target window t in [0, T-L] and start row s in
            [0, N-L]: L-1 float32 additions in ascending order, each rounded on its own, then one float32 division
  segments  seg_off (int64 [nseg+1], ascending) marks the videos: a start s is a candidate only when [s, s+L) lies inside one
            [seg_off[j], seg_off[j+1]); rows outside [seg_off[0], seg_off[nseg]) start nothing; without seg_off the index is one segment

Results are labelled with the start row, or with the stored id of that row on an id-mapped index.  Equal scores rank the lower start
ROW first; -0.0 is reported as +0.0.  The threshold test of the range call is `>=`, as the reference's is, not the strict `>` of
`FlatIPIndex.range_search`.

Event search (event_search, event_best_per_segment; the `event_*_ref` functions are its definition) is the gapped form: m query events
in order, consecutive events between min_gap and max_gap rows apart, inside one segment; a result is an end row's chain score and the
path of m rows behind it.
"""
import numpy as np
import torch

from . import _ffi, _staging
from ._faiss import FLT_MAX
from .index import FlatIPIndex
from .refine import _ordered

SEQ_MAX_LEN = _ffi.IVR_SEQ_MAX_LEN
EVENT_MAX_LEN = _ffi.IVR_EVENT_MAX_LEN
EVENT_MAX_GAP = _ffi.IVR_EVENT_MAX_GAP


# -- the definition in numpy ---------------------------------------------------------------------------------------------------
def _segments_ok(nstart, L, seg_off):
    """bool [nstart]: start s is a candidate."""
    ok = np.ones(nstart, bool)
    if seg_off is None:
        return ok
    off = np.asarray(seg_off).astype(np.int64).reshape(-1)
    s = np.arange(nstart, dtype=np.int64)
    j = np.searchsorted(off, s, side="right") - 1                  # the last offset <= s: with empty segments the run that holds s
    inside = (j >= 0) & (j < len(off) - 1)
    end = off[np.clip(j + 1, 0, len(off) - 1)]
    return inside & (s + L <= end)


def sequence_scores_ref(S, L, seg_off=None):
    """S float32 [T,N] frame scores -> (W float32 [T-L+1, max(N-L+1, 0)], ok bool [max(N-L+1, 0)]): the window score of every (target
    window, start row) with its roundings, and which starts are candidates."""
    S = np.asarray(S, np.float32)
    L = int(L)
    if S.ndim != 2 or L < 1 or S.shape[0] < L:
        raise ValueError(f"sequence_scores_ref: S {S.shape} must be [T,N] with T >= L={L} >= 1")
    T, N = S.shape
    nwin, nstart = T - L + 1, max(N - L + 1, 0)
    acc = S[0:nwin, 0:nstart].copy()
    for i in range(1, L):
        acc = (acc + S[i:i + nwin, i:i + nstart]).astype(np.float32)
    return (acc / np.float32(L)).astype(np.float32), _segments_ok(nstart, L, seg_off)


def _labels(rows, ids):
    return rows if ids is None else np.asarray(ids).astype(np.int64)[rows]


def sequence_search_ref(S, L, k, seg_off=None, ids=None):
    """(D float32 [T-L+1,k], I int64 [T-L+1,k]): per target window the k best candidate starts by W, descending, equal scores the
    lower start row first, (-FLT_MAX, -1) in unused slots.  ids: the labels of an id-mapped index (I = ids[start])."""
    W, ok = sequence_scores_ref(S, L, seg_off)
    k = int(k)
    nwin = W.shape[0]
    D = np.full((nwin, k), -FLT_MAX, np.float32)
    I = np.full((nwin, k), -1, np.int64)
    rows = np.flatnonzero(ok).astype(np.int64)
    for t in range(nwin):
        keys = _ordered(W[t, rows]).astype(np.int64)
        order = np.lexsort((rows, -keys))[:k]
        D[t, :len(order)] = W[t, rows[order]] + np.float32(0.0)
        I[t, :len(order)] = _labels(rows[order], ids)
    return D, I


def sequence_range_ref(S, L, threshold, seg_off=None, ids=None):
    """(lims int64 [T-L+2], D float32 [lims[-1]], I int64 [lims[-1]]): every candidate with W >= float32(threshold); the results of
    window t at [lims[t], lims[t+1]) in ascending start row.  A NaN score matches nothing."""
    W, ok = sequence_scores_ref(S, L, seg_off)
    W = W + np.float32(0.0)
    thr = np.float32(threshold)
    if thr != thr:
        raise ValueError("sequence_range_ref: threshold is NaN")
    lims, D, I = [0], [], []
    for t in range(W.shape[0]):
        with np.errstate(invalid="ignore"):
            rows = np.flatnonzero(ok & (W[t] >= thr)).astype(np.int64)
        D.append(W[t, rows])
        I.append(_labels(rows, ids))
        lims.append(lims[-1] + len(rows))
    return (np.asarray(lims, np.int64), np.concatenate(D).astype(np.float32) if D else np.zeros(0, np.float32),
            np.concatenate(I).astype(np.int64) if I else np.zeros(0, np.int64))


# -- event search: the definition in numpy ----------------------------------------------------------------------------------------
# m query events in order, consecutive events min_gap .. max_gap rows apart, all inside the segment of the end row
# (ivr_index_search_events / ivr_index_best_events_per_segment, csrc/search_events.hip; the definition is in include/ivr_api.h):
#   C[0, r] = S[0, r] for the rows inside a segment
#   P[j, r] = the candidate p of step j-1 in [max(lo(r), r - max_gap), r - min_gap] with the greatest C[j-1, p], -0.0 equal to +0.0,
#             equal values the lower row; no candidate in the window: r is no candidate of step j
#   C[j, r] = float32((C[j-1, P[j, r]] + 0.0) + S[j, r]),   W[r] = C[m-1, r] / float32(m)
def _event_args(S, min_gap, max_gap, what):
    S = np.asarray(S, np.float32)
    if S.ndim != 2 or not 1 <= S.shape[0] <= EVENT_MAX_LEN:
        raise ValueError(f"{what}: S {S.shape} must be [m,N] with 1 <= m <= {EVENT_MAX_LEN}")
    min_gap, max_gap = _staging.check_gaps(min_gap, max_gap, EVENT_MAX_GAP, what)
    return S, min_gap, max_gap


def event_scores_ref(S, min_gap, max_gap, seg_off=None):
    """S float32 [m,N] frame scores of one chain -> (C float32 [m,N], P int64 [m,N], ok bool [m,N]): the best left-to-right float32
    sum of an admissible chain whose event j lies on row r, the row of its event j-1 (-1 in row 0 and for a row that is no candidate)
    and which (step, row) pairs are candidates."""
    S, min_gap, max_gap = _event_args(S, min_gap, max_gap, "event_scores_ref")
    m, N = S.shape
    lo, _ = _staging.segment_bounds(N, seg_off)
    rows = np.arange(N, dtype=np.int64)
    C = np.zeros((m, N), np.float32)
    P = np.full((m, N), -1, np.int64)
    ok = np.zeros((m, N), bool)
    ok[0] = lo <= rows
    C[0, ok[0]] = S[0, ok[0]]
    zero = np.float32(0.0)
    for j in range(1, m):
        keys = np.where(ok[j - 1], _ordered(C[j - 1]).astype(np.int64), -1)
        for r in range(N):
            a, b = max(int(lo[r]), r - max_gap), r - min_gap
            if a > b:
                continue
            i = int(np.argmax(keys[a:b + 1]))                      # the first of equal maxima: the lower row
            if keys[a + i] < 0:
                continue
            ok[j, r], P[j, r] = True, a + i
            C[j, r] = np.float32(np.float32(C[j - 1, a + i] + zero) + S[j, r])
    return C, P, ok


def _event_paths(P, ends, ids):
    """int64 [len(ends), m]: the path behind every end row, in event order."""
    m = P.shape[0]
    out = np.empty((len(ends), m), np.int64)
    r = np.asarray(ends, np.int64).copy()
    for j in range(m - 1, -1, -1):
        out[:, j] = r
        if j:
            r = P[j, r]
    return _labels(out, ids)


def _event_chains(S, what):
    S = np.asarray(S, np.float32)
    if S.ndim == 2:
        S = S[None]
    if S.ndim != 3:
        raise ValueError(f"{what}: S {S.shape} must be [B,m,N] or [m,N]")
    return S


def _event_ranked(Sb, min_gap, max_gap, seg_off):
    """(W float32 [N] + 0.0, P, the candidate end rows by (W descending, row ascending)) of one chain."""
    C, P, ok = event_scores_ref(Sb, min_gap, max_gap, seg_off)
    m = C.shape[0]
    W = (C[m - 1] / np.float32(m)).astype(np.float32)
    rows = np.flatnonzero(ok[m - 1]).astype(np.int64)
    order = np.lexsort((rows, -_ordered(W[rows]).astype(np.int64)))
    return W + np.float32(0.0), P, rows[order]


def event_search_ref(S, k, min_gap, max_gap, seg_off=None, ids=None):
    """S float32 [B,m,N] (or [m,N]: one chain) -> (D float32 [B,k], I int64 [B,k,m]): per chain the k best end rows by W, descending,
    equal scores the lower end row first, with the path behind each in event order; (-FLT_MAX, -1 in all m entries) in unused
    slots.  ids: the labels of an id-mapped index."""
    S = _event_chains(S, "event_search_ref")
    k = int(k)
    B, m = S.shape[:2]
    D = np.full((B, k), -FLT_MAX, np.float32)
    I = np.full((B, k, m), -1, np.int64)
    for b in range(B):
        W, P, ends = _event_ranked(S[b], min_gap, max_gap, seg_off)
        ends = ends[:k]
        D[b, :len(ends)] = W[ends]
        I[b, :len(ends)] = _event_paths(P, ends, ids)
    return D, I


def event_best_per_segment_ref(S, min_gap, max_gap, seg_off=None, ids=None):
    """(D float32 [B,nseg], I int64 [B,nseg,m]): for every segment its best end row by the order of event_search_ref and the path behind
    it; (-FLT_MAX, -1) for a segment without a chain.  nseg = 1 without seg_off."""
    S = _event_chains(S, "event_best_per_segment_ref")
    B, m, N = S.shape
    off = np.array([0, N], np.int64) if seg_off is None else np.asarray(seg_off).astype(np.int64).reshape(-1)
    nseg = len(off) - 1
    D = np.full((B, nseg), -FLT_MAX, np.float32)
    I = np.full((B, nseg, m), -1, np.int64)
    for b in range(B):
        W, P, ends = _event_ranked(S[b], min_gap, max_gap, seg_off)
        for s in range(nseg):
            inside = ends[(ends >= off[s]) & (ends < off[s + 1])]
            if len(inside):
                D[b, s] = W[inside[0]]
                I[b, s] = _event_paths(P, inside[:1], ids)[0]
    return D, I


# -- the library calls ---------------------------------------------------------------------------------------------------------
def _stage_events(index, x, min_gap, max_gap, seg_off, what):
    """The checked arguments of both event calls: (frames tensor [B*m,d], staged, B, m, min_gap, max_gap, seg_off tensor or None,
    nseg)."""
    if not isinstance(index, FlatIPIndex):
        raise ValueError(f"{what}: index must be a FlatIPIndex, got {type(index).__name__}")
    t, staged, B, m = _staging.chains_f32(x, index.d, index.device, EVENT_MAX_LEN, what)
    min_gap, max_gap = _staging.check_gaps(min_gap, max_gap, EVENT_MAX_GAP, what)
    seg, seg_staged, nseg = _staging.segments(seg_off, index.device, what)
    return t, staged or seg_staged, B, m, min_gap, max_gap, seg, nseg


def event_search_device(index, x, k, max_gap, min_gap=1, seg_off=None, normalize=False):
    """Top-k event search on the device: x float32 [B,m,d] chains of m events (numpy or torch; [m,d] is one chain) -> (D float32
    [B,k], I int64 [B,k,m]) CUDA tensors, the definition of event_search_ref.  seg_off as for sequence_search_device.  No host
    synchronisation unless an argument had to be staged."""
    t, staged, B, m, min_gap, max_gap, seg, nseg = _stage_events(index, x, min_gap, max_gap, seg_off, "event_search")
    k = _staging.check_k(k, _ffi.IVR_MAX_K)
    D, I = _staging.alloc_DI_paths(B, k, m, index.device)
    index._call("ivr_index_search_events", t, B, m, min_gap, max_gap, seg, nseg, k, bool(normalize), D, I)
    _staging.sync_if_staged(staged, index.device)
    return D, I


def event_search(index, x, k, max_gap, min_gap=1, seg_off=None, normalize=False):
    """event_search_device as numpy arrays (D, I)."""
    D, I = event_search_device(index, x, k, max_gap, min_gap, seg_off, normalize)
    return D.cpu().numpy(), I.cpu().numpy()


def event_best_per_segment_device(index, x, max_gap, min_gap=1, seg_off=None, normalize=False):
    """The best chain of every segment on the device: (D float32 [B,nseg], I int64 [B,nseg,m]) CUDA tensors, the definition of
    event_best_per_segment_ref: which videos hold the sequence, all videos in one call.  nseg = 1 without seg_off."""
    t, staged, B, m, min_gap, max_gap, seg, nseg = _stage_events(index, x, min_gap, max_gap, seg_off, "event_best_per_segment")
    D, I = _staging.alloc_DI_paths(B, max(nseg, 1), m, index.device)
    index._call("ivr_index_best_events_per_segment", t, B, m, min_gap, max_gap, seg, nseg, bool(normalize), D, I)
    _staging.sync_if_staged(staged, index.device)
    return D, I


def event_best_per_segment(index, x, max_gap, min_gap=1, seg_off=None, normalize=False):
    """event_best_per_segment_device as numpy arrays (D, I)."""
    D, I = event_best_per_segment_device(index, x, max_gap, min_gap, seg_off, normalize)
    return D.cpu().numpy(), I.cpu().numpy()


def _stage(index, x, L, seg_off, what):
    """The checked arguments of both calls: (frames tensor, staged, T, L, seg_off tensor or None, nseg)."""
    if not isinstance(index, FlatIPIndex):
        raise ValueError(f"{what}: index must be a FlatIPIndex, got {type(index).__name__}")
    t, staged = _staging.queries_f32(x, index.d, index.device)
    L = _staging.check_window(L, t.shape[0], SEQ_MAX_LEN, what)
    seg, seg_staged, nseg = _staging.segments(seg_off, index.device, what)
    return t, staged or seg_staged, t.shape[0], L, seg, nseg


def sequence_search_device(index, x, L, k, seg_off=None, normalize=False):
    """Top-k clip search on the device: x float32 [T,d] query frames (numpy or torch) -> (D float32 [T-L+1,k], I int64 [T-L+1,k])
    CUDA tensors, the definition of the module docstring.  seg_off: integers [nseg+1], ascending (checked when it is a host array), or
    None.  No host synchronisation unless an argument had to be staged."""
    t, staged, T, L, seg, nseg = _stage(index, x, L, seg_off, "sequence_search")
    k = _staging.check_k(k, _ffi.IVR_MAX_K)
    D, I = _staging.alloc_DI(T - L + 1, k, index.device)
    index._call("ivr_index_search_sequences", t, T, L, seg, nseg, k, bool(normalize), D, I)
    _staging.sync_if_staged(staged, index.device)
    return D, I


def sequence_search(index, x, L, k, seg_off=None, normalize=False):
    """sequence_search_device as numpy arrays (D, I)."""
    D, I = sequence_search_device(index, x, L, k, seg_off, normalize)
    return D.cpu().numpy(), I.cpu().numpy()


def sequence_range_search_device(index, x, L, threshold, seg_off=None, normalize=False, cap=None):
    """Threshold clip search on the device: (lims int64 [T-L+2], D float32 [cap], I int64 [cap], total) CUDA tensors, total =
    lims[T-L+1:] (the number of results; entries at positions >= cap are counted but not written).  No host synchronisation when `cap`
    is given; cap=None sizes D and I exactly: a counting pass with cap 0, one synchronisation, then the full pass."""
    threshold = float(threshold)
    if threshold != threshold:
        raise ValueError("sequence_range_search: threshold is NaN")
    t, staged, T, L, seg, nseg = _stage(index, x, L, seg_off, "sequence_range_search")
    if cap is not None and int(cap) < 0:
        raise ValueError(f"sequence_range_search: cap={cap} < 0")
    nwin = T - L + 1
    lims = torch.empty(nwin + 1, dtype=torch.int64, device=index.device)

    def run(c):
        D = torch.empty(max(c, 1), dtype=torch.float32, device=index.device)      # never a NULL pointer, even for cap 0
        I = torch.empty(max(c, 1), dtype=torch.int64, device=index.device)
        index._call("ivr_index_range_search_sequences", t, T, L, seg, nseg, threshold, bool(normalize), lims, D, I, int(c))
        return D[:c], I[:c]

    with torch.cuda.device(index.device):
        if cap is None:
            run(0)
            cap = int(lims[nwin].item())
        D, I = run(int(cap))
        _staging.sync_if_staged(staged)
    return lims, D, I, lims[nwin:]


def sequence_range_search(index, x, L, threshold, seg_off=None, normalize=False):
    """(lims, D, I) numpy arrays: every candidate start with W >= threshold, per target window in ascending start row.  Sized in two
    passes as FlatIPIndex.range_search_device(cap=None) does: a counting pass, one synchronisation, the exact pass."""
    lims, D, I, _ = sequence_range_search_device(index, x, L, threshold, seg_off, normalize)
    return lims.cpu().numpy(), D.cpu().numpy(), I.cpu().numpy()


# -- the reference's class -----------------------------------------------------------------------------------------------------
class _NullLogger:
    def __getattr__(self, _):
        return lambda *a, **k: None


class TemporalAnalyzer:
    """core.TemporalAnalyzer (core.py:3560): the same signatures and return shapes.  The cosines come from the HIP kernels; the list
    bookkeeping is the reference's own and stays on the host.  Unlike the reference, an error of the library propagates instead of
    being logged and turned into an empty result.  analyze_temporal_patterns reads metadata only and is not provided."""

    def __init__(self, config=None, logger=None):
        self.config = config
        self.logger = logger or _NullLogger()

    def detect_scene_boundaries(self, features, threshold=0.3, min_scene_length=5, validate_inputs=True):
        """core.py:3584-3642: [(start_frame, end_frame), ...].  A scene ends at frame i when cos(frame i, frame i+1) < threshold and
        it is at least min_scene_length frames long by then; otherwise the cut is ignored and the scene runs on (the reference's
        bookkeeping, which differs from filter.py's group_into_scenes)."""
        if validate_inputs:
            if not isinstance(features, np.ndarray):
                raise ValueError("Features must be numpy array")
            if features.ndim != 2:
                raise ValueError("Features must be 2D array")
            if len(features) < min_scene_length * 2:
                self.logger.warning(f"Too few features ({len(features)}) for scene detection")
                return [(0, len(features) - 1)]
        n = len(features)
        similarities = []
        if n >= 2:
            from .filters import rowwise_cosine
            similarities = rowwise_cosine(features[:-1], features[1:]).cpu().numpy().tolist()
        boundaries, current_start = [], 0
        for i, sim in enumerate(similarities):
            if sim < threshold and i - current_start >= min_scene_length:
                boundaries.append((current_start, i))
                current_start = i + 1
        if current_start < n:
            boundaries.append((current_start, n - 1))
        return boundaries

    def find_similar_sequences(self, target_features, database_features, sequence_length=5, similarity_threshold=0.8,
                               validate_inputs=True):
        """core.py:3644-3702: [(db_start, score), ...] for every (target window, database window) pair whose mean frame-wise cosine
        is >= similarity_threshold, best first; equal scores keep (target start, db start) order, as the reference's stable sort
        leaves them.  Both arrays go through a temporary FlatIPIndex with normalize=True (a zero row stays zero: cosine 0, as
        sklearn gives).  sequence_length is at most SEQ_MAX_LEN here."""
        if validate_inputs:
            if not isinstance(target_features, np.ndarray) or not isinstance(database_features, np.ndarray):
                raise ValueError("Features must be numpy arrays")
            if target_features.ndim != 2 or database_features.ndim != 2:
                raise ValueError("Features must be 2D arrays")
        if len(target_features) < sequence_length or len(database_features) < sequence_length:
            self.logger.warning("Insufficient features for sequence comparison")
            return []
        index = FlatIPIndex(database_features.shape[1])
        try:
            index.add(database_features, normalize=True)
            lims, D, I = sequence_range_search(index, target_features, sequence_length, similarity_threshold, normalize=True)
        finally:
            index.close()
        similar_sequences = [(int(s), float(w)) for s, w in zip(I, D)]      # (target start, db start) order
        similar_sequences.sort(key=lambda x: x[1], reverse=True)
        return similar_sequences

    def find_event_sequences(self, event_features, database_features, max_gap, min_gap=1, k=10, validate_inputs=True):
        """Not in the reference: [(path, score), ...], best first, for the k best places where the m rows of event_features occur in
        order in database_features, consecutive events min_gap .. max_gap rows apart.  path is a tuple of m database rows, score the mean
        cosine along it.  Both arrays go through a temporary FlatIPIndex with normalize=True, as find_similar_sequences does; fewer
        than k chains give a shorter list."""
        if validate_inputs:
            if not isinstance(event_features, np.ndarray) or not isinstance(database_features, np.ndarray):
                raise ValueError("Features must be numpy arrays")
            if event_features.ndim != 2 or database_features.ndim != 2:
                raise ValueError("Features must be 2D arrays")
        if len(event_features) < 1 or len(database_features) < 1:
            self.logger.warning("Insufficient features for event search")
            return []
        index = FlatIPIndex(database_features.shape[1])
        try:
            index.add(database_features, normalize=True)
            D, I = event_search(index, event_features, k, max_gap, min_gap, normalize=True)
        finally:
            index.close()
        return [(tuple(int(r) for r in path), float(w)) for path, w in zip(I[0], D[0]) if path[0] >= 0]

    def get_transition_frames(self, features, scene_boundaries, validate_inputs=True):
        """core.py:3704-3739: the frames within two before and three after every cut between consecutive scenes, ascending."""
        if validate_inputs:
            if not isinstance(features, np.ndarray):
                raise ValueError("Features must be numpy array")
            if not isinstance(scene_boundaries, list):
                raise ValueError("Scene boundaries must be a list")
        frames = set()
        for (_, current_end), (next_start, _) in zip(scene_boundaries[:-1], scene_boundaries[1:]):
            frames.update(range(max(0, current_end - 2), min(len(features), next_start + 3)))
        return sorted(frames)

    def _compute_sequence_similarity(self, seq1, seq2):
        """core.py:3812-3828 on the host, in float64: the mean of the frame-wise cosines; 0.0 for sequences of different shape."""
        seq1, seq2 = np.asarray(seq1, np.float64), np.asarray(seq2, np.float64)
        if seq1.shape != seq2.shape or seq1.ndim != 2:
            return 0.0
        n1, n2 = np.linalg.norm(seq1, axis=1), np.linalg.norm(seq2, axis=1)
        n1[n1 == 0] = 1.0
        n2[n2 == 0] = 1.0
        return float(np.mean((seq1 * seq2).sum(1) / (n1 * n2)))
