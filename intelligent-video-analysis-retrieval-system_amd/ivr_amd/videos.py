"""Video search: stored videos ranked against a SET of query vectors, over a FlatIPIndex.

Every other search of the library takes one vector per query; the `seg_off` family (clip search, event search, grouped search, moment
search, per-video tags) answers per video, but for a single vector.  Here both sides hold several vectors: "which stored videos look
like this video or clip, whatever the order, frame rate or cut?", "which videos contain all of these sub-queries somewhere?", and
the related-videos list of every stored video (ivr_index_video_scores / ivr_index_video_search, csrc/search_videos.hip).  The measure
is the two-sided reduction of the frame score matrix that Qdrant, Vespa and Milvus ship for multi-vector documents: MaxSim in one
direction, Chamfer similarity in both.

Definition (the `*_ref` functions below are this in numpy, to the bit, given the frame scores):

  S[i, r]     the float32 inner product `FlatIPIndex.search` / `rescore_device` report for (query member i, stored row r), -0.0
              counted as +0.0.  Precondition |S| <= 256; beyond it nothing faults and the result is unspecified
  sets        set_off (integers [nsets+1], ascending) marks the query sets: set s is the members [set_off[s], set_off[s+1]) of x,
              1 <= m_s <= VIDEO_MAX_MEMBERS; without set_off all of x is one set
  videos      seg_off (integers [nseg+1], ascending) marks the stored videos as everywhere in the family: rows outside
              [seg_off[0], seg_off[nseg]) belong to no video, offsets beyond the stored rows are clipped, n_j is the row count of
              video j; without seg_off the index is one video
  fix(t)      int64(rint(float32(t * 2^24))): the fixed point of tagging.MASS_ONE.  The scaling is exact in float32, so a term is
              rounded by at most 2^-25
  Fsum[s, j]  the sum over the members i of s of fix(max over the rows r of j of S[i, r]): every query frame finds its best match
  Bsum[s, j]  the sum over the rows r of j of fix(max over the members i of s of S[i, r]): every stored frame finds its best match
  V[s, j]     with F64 = float64(Fsum) / (m_s * 2^24) and B64 = float64(Bsum) / (n_j * 2^24):
                mode="forward"    float32(F64)                  MaxSim, the answer to "contains all of these"
                mode="backward"   float32(B64)
                mode="symmetric"  float32((F64 + B64) * 0.5)    Chamfer, the default
              an empty video scores -FLT_MAX and is never ranked
  order       videos rank by (V descending, video ascending), with the library's 64-bit key

Maxima do not depend on the order of arrival and integer sums do not either: every output has the same bits on every run and
stream.  The price is the 2^-25 rounding of each term: with one member, mode="forward" is the score `best_per_segment` reports for
that video WITHIN 2^-25, NOT TO THE BIT.  Unused slots hold -1 / -FLT_MAX.
"""
import numpy as np
import torch

from . import _ffi, _staging
from ._faiss import FLT_MAX
from .index import FlatIPIndex
from .refine import _ordered
from .tagging import MASS_ONE

VIDEO_MAX_MEMBERS = _ffi.IVR_VIDEO_MAX_MEMBERS
MODES = tuple(_ffi.IVR_VIDEO_MODE)


# -- the definition in numpy ---------------------------------------------------------------------------------------------------
def _mode(mode, what):
    if not isinstance(mode, str) or mode not in _ffi.IVR_VIDEO_MODE:
        raise ValueError(f"{what}: mode must be 'forward', 'backward' or 'symmetric', got {mode!r}")
    return _ffi.IVR_VIDEO_MODE[mode]


def _sets(set_off, nq, what):
    """The checked sets of nq members: int64 [nsets+1]; [0, nq] without set_off."""
    if set_off is None:
        off = np.array([0, nq], np.int64)
    else:
        if isinstance(set_off, torch.Tensor):
            set_off = set_off.cpu().numpy()
        off = np.asarray(set_off)
        if not np.issubdtype(off.dtype, np.integer) or off.ndim != 1 or len(off) < 2:
            raise ValueError(f"{what}: set_off must be integers [nsets+1] with nsets >= 1, got {off.dtype} {off.shape}")
        off = off.astype(np.int64)
    m = np.diff(off)
    if (m < 0).any():
        i = int(np.flatnonzero(m < 0)[0])
        raise ValueError(f"{what}: set_off must ascend, got set_off[{i}]={off[i]} > set_off[{i + 1}]={off[i + 1]}")
    if off[0] < 0 or off[-1] > nq:
        raise ValueError(f"{what}: set_off [{off[0]},{off[-1]}] outside the {nq} members")
    if (m == 0).any():
        raise ValueError(f"{what}: set {int(np.flatnonzero(m == 0)[0])} is empty")
    if (m > VIDEO_MAX_MEMBERS).any():
        i = int(np.flatnonzero(m > VIDEO_MAX_MEMBERS)[0])
        raise ValueError(f"{what}: set {i} has {int(m[i])} members > {VIDEO_MAX_MEMBERS}")
    return off


def _ranges(N, seg_off):
    if seg_off is None:
        return [(0, N)]
    off = np.asarray(seg_off).astype(np.int64).reshape(-1)
    if len(off) < 2 or (off[1:] < off[:-1]).any():
        raise ValueError("seg_off must be [nseg+1] with nseg >= 1, ascending")
    return [(int(min(max(a, 0), N)), int(min(max(b, 0), N))) for a, b in zip(off[:-1], off[1:])]


def fix(t):
    """float32 -> int64: rint(float32(t * 2^24))."""
    return np.rint(np.asarray(t, np.float32) * np.float32(MASS_ONE)).astype(np.int64)


def video_sums_ref(S, seg_off=None, set_off=None):
    """S float32 [members,N] -> (Fsum int64 [nsets,nseg], Bsum int64 [nsets,nseg], m int64 [nsets], n int64 [nseg])."""
    S = np.asarray(S, np.float32)
    if S.ndim != 2:
        raise ValueError(f"video_scores_ref: S {S.shape} must be [members,N]")
    S = S + np.float32(0.0)                                        # -0.0 counts as +0.0
    off = _sets(set_off, S.shape[0], "video_scores_ref")
    ranges = _ranges(S.shape[1], seg_off)
    nsets, nseg = len(off) - 1, len(ranges)
    Fsum = np.zeros((nsets, nseg), np.int64)
    Bsum = np.zeros((nsets, nseg), np.int64)
    for s in range(nsets):
        Ss = S[off[s]:off[s + 1]]
        back = fix(Ss.max(axis=0))                                 # [N]: the best member of the set for every stored row
        for j, (lo, hi) in enumerate(ranges):
            if lo < hi:
                Fsum[s, j] = fix(Ss[:, lo:hi].max(axis=1)).sum()
                Bsum[s, j] = back[lo:hi].sum()
    return Fsum, Bsum, np.diff(off), np.array([max(hi - lo, 0) for lo, hi in ranges], np.int64)


def video_scores_ref(S, seg_off=None, set_off=None, mode="symmetric", sums=None):
    """S float32 [members,N] frame scores -> V float32 [nsets,nseg], the definition of the module docstring.  sums: what
    video_sums_ref returned for the same S, seg_off and set_off (the three modes share it)."""
    _mode(mode, "video_scores_ref")
    Fsum, Bsum, m, n = sums if sums is not None else video_sums_ref(S, seg_off, set_off)
    with np.errstate(divide="ignore", invalid="ignore"):
        F64 = Fsum.astype(np.float64) / (m.astype(np.float64) * float(MASS_ONE))[:, None]
        B64 = Bsum.astype(np.float64) / (n.astype(np.float64) * float(MASS_ONE))[None, :]
    V64 = F64 if mode == "forward" else B64 if mode == "backward" else (F64 + B64) * 0.5
    V = V64.astype(np.float32)
    V[:, n == 0] = -FLT_MAX
    return V


def video_search_ref(S, k, seg_off=None, set_off=None, mode="symmetric", exclude=None, sums=None):
    """(Vseg int64 [nsets,k], D float32 [nsets,k]): the k best videos of every set by (V descending, video ascending).  exclude:
    integers [nsets], one video left out per set (a value that is no video leaves none out).  sums: as for video_scores_ref."""
    k = _staging.check_k(k, _ffi.IVR_MAX_K)
    sums = sums if sums is not None else video_sums_ref(S, seg_off, set_off)
    V = video_scores_ref(S, seg_off, set_off, mode, sums)
    n = sums[3]
    nsets, nseg = V.shape
    Vseg = np.full((nsets, k), -1, np.int64)
    D = np.full((nsets, k), -FLT_MAX, np.float32)
    for s in range(nsets):
        ok = n > 0
        if exclude is not None and 0 <= int(exclude[s]) < nseg:
            ok = ok.copy()
            ok[int(exclude[s])] = False
        js = np.flatnonzero(ok)
        js = js[np.lexsort((js, -_ordered(V[s, js]).astype(np.int64)))][:k]
        Vseg[s, :len(js)] = js
        D[s, :len(js)] = V[s, js] + np.float32(0.0)
    return Vseg, D


# -- the library calls ---------------------------------------------------------------------------------------------------------
def _stage(index, x, seg_off, set_off, mode, what):
    """The checked arguments of both calls: (members tensor [nq,d], staged, nq, set_off tensor or None, nsets, seg_off tensor or
    None, nseg, the library's mode number)."""
    if not isinstance(index, FlatIPIndex):
        raise ValueError(f"{what}: index must be a FlatIPIndex, got {type(index).__name__}")
    mode = _mode(mode, what)
    seg, seg_staged, nseg = _staging.segments(seg_off, index.device, what)
    t, staged = _staging.queries_f32(_staging.as_rows(x), index.d, index.device)
    nq = int(t.shape[0])
    _staging.check_nq(nq, what)
    off = _sets(set_off, nq, what)
    sets = None if set_off is None else torch.from_numpy(off).to(index.device)
    return t, staged or seg_staged or sets is not None, nq, sets, len(off) - 1, seg, nseg, mode


def video_scores_device(index, x, seg_off=None, set_off=None, mode="symmetric", normalize=False):
    """The score of every stored video for every query set, on the device: x float32 [members,d] (numpy or torch) -> V float32
    [nsets,nseg] CUDA tensor, the definition of video_scores_ref.  set_off is checked on the host (a CUDA tensor is copied back);
    the library reads it back once more: one host synchronisation per call."""
    t, staged, nq, sets, nsets, seg, nseg, mode = _stage(index, x, seg_off, set_off, mode, "video_scores")
    V = torch.empty((nsets, max(nseg, 1)), dtype=torch.float32, device=index.device)
    index._call("ivr_index_video_scores", t, nq, sets, nsets, seg, nseg, mode, bool(normalize), V)
    _staging.sync_if_staged(staged, index.device)
    return V


def video_scores(index, x, seg_off=None, set_off=None, mode="symmetric", normalize=False):
    """video_scores_device as a numpy array."""
    return video_scores_device(index, x, seg_off, set_off, mode, normalize).cpu().numpy()


def video_search_device(index, x, k, seg_off=None, set_off=None, mode="symmetric", exclude=None, normalize=False):
    """The k best stored videos of every query set, on the device: (Vseg int64 [nsets,k], D float32 [nsets,k]) CUDA tensors, the
    definition of video_search_ref.  exclude: integers [nsets] (numpy or torch), one video left out per set, or None."""
    k = _staging.check_k(k, _ffi.IVR_MAX_K)
    t, staged, nq, sets, nsets, seg, nseg, mode = _stage(index, x, seg_off, set_off, mode, "video_search")
    ex = None
    if exclude is not None:
        ex = _staging.int_tensor(exclude, "video_search: exclude")
        if ex.dim() != 1 or ex.shape[0] != nsets:
            raise ValueError(f"video_search: exclude must be [{nsets}], got {tuple(ex.shape)}")
        ex = ex.to(device=index.device, dtype=torch.int64).contiguous()
        staged = staged or _staging.is_staged(ex, exclude)
    Vseg, D = torch.empty((nsets, k), dtype=torch.int64, device=index.device), torch.empty((nsets, k), dtype=torch.float32, device=index.device)
    index._call("ivr_index_video_search", t, nq, sets, nsets, seg, nseg, mode, bool(normalize), k, ex, Vseg, D)
    _staging.sync_if_staged(staged, index.device)
    return Vseg, D


def video_search(index, x, k, seg_off=None, set_off=None, mode="symmetric", exclude=None, normalize=False):
    """video_search_device as numpy arrays (Vseg, D)."""
    Vseg, D = video_search_device(index, x, k, seg_off, set_off, mode, exclude, normalize)
    return Vseg.cpu().numpy(), D.cpu().numpy()


RELATED_CHUNK_ROWS = 1 << 14        # members of one call of related_videos: the gathered copy of the query videos stays at 32 MiB at d = 512


def related_videos(index, seg_off, k, mode="symmetric", videos=None):
    """For every stored video, or for those listed in `videos`, its k best OTHER videos: (Vseg int64 [n,k], D float32 [n,k]) numpy
    arrays, line i for video i (or videos[i]); a listed video without stored rows gets unused slots.  Chunks of query videos are
    gathered on the device (FlatIPIndex.gather_device, no host copy of rows) into one set each and go through video_search with
    `exclude` set to the video itself; a video of more than VIDEO_MAX_MEMBERS rows raises ValueError.  With videos=None every stored
    row is scored against every stored row: the cost is QUADRATIC in the rows."""
    if not isinstance(index, FlatIPIndex):
        raise ValueError(f"related_videos: index must be a FlatIPIndex, got {type(index).__name__}")
    _mode(mode, "related_videos")
    k = _staging.check_k(k, _ffi.IVR_MAX_K)
    N = index.ntotal
    host = seg_off.cpu().numpy() if isinstance(seg_off, torch.Tensor) else None if seg_off is None else np.asarray(seg_off)
    ranges = _ranges(N, host)
    seg, _, _ = _staging.segments(seg_off, index.device, "related_videos")
    which = np.arange(len(ranges), dtype=np.int64) if videos is None else np.asarray(videos).astype(np.int64).reshape(-1)
    if len(which) and (which.min() < 0 or which.max() >= len(ranges)):
        raise ValueError(f"related_videos: videos must lie in [0, {len(ranges)})")
    Vseg = np.full((len(which), k), -1, np.int64)
    D = np.full((len(which), k), -FLT_MAX, np.float32)
    full = [i for i, j in enumerate(which) if ranges[j][0] < ranges[j][1]]
    pos = 0
    while pos < len(full):
        take, rows = [], 0
        while pos < len(full) and (not take or rows + ranges[which[full[pos]]][1] - ranges[which[full[pos]]][0] <= RELATED_CHUNK_ROWS):
            lo, hi = ranges[which[full[pos]]]
            take.append(full[pos])
            rows += hi - lo
            pos += 1
        set_off = np.concatenate(([0], np.cumsum([ranges[which[i]][1] - ranges[which[i]][0] for i in take]))).astype(np.int64)
        _sets(set_off, rows, "related_videos")
        gather = torch.cat([torch.arange(*ranges[which[i]], dtype=torch.int64) for i in take]).to(index.device)
        x = index.gather_device(gather)
        vs, d = video_search_device(index, x, k, seg, set_off, mode, exclude=which[take])
        Vseg[take], D[take] = vs.cpu().numpy(), d.cpu().numpy()
    return Vseg, D
