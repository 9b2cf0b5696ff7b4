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
"""
import numpy as np
import torch

from . import _ffi, _staging
from ._faiss import FLT_MAX
from .index import FlatIPIndex
from .refine import _ordered

SEQ_MAX_LEN = _ffi.IVR_SEQ_MAX_LEN


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


# -- the library calls ---------------------------------------------------------------------------------------------------------
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
