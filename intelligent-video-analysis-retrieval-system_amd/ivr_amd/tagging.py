"""Zero-shot tagging: for every stored row of a FlatIPIndex the best t of C label vectors with their softmax probabilities, and per
video (segment) the top labels.  The other standard use of a CLIP model, `logits_per_image.softmax(dim=1)`, for frames that are
already in the index.

The reference has the place for the answer and nothing local that fills it: `KeyframeMetadata.scene_tags` (`core.py:101`),
`MetadataManager.add_semantic_tags` (`core.py:3278`), the exports (`system.py:2066`, `system.py:2130`) and the tag-matching search of
`api.py:2851` all read `scene_tags`, and only the remote vision call writes them.  Here one call (ivr_index_tag_rows, csrc/tags.hip)
streams the label tiles past blocks of stored rows: the stored rows are read once, nothing N x C is ever held, and every score
carries the index's bits.

Definition (`tag_rows_ref` and `tag_segments_ref` below are this in numpy, given the scores):

  labels      float32 [C, d], 1 <= C <= tag_max_labels() (4096); normalize=True L2-normalises them as `add(normalize=True)` does
  S[j, i]     the float32 inner product a FlatIPIndex HOLDING THE LABELS reports for (query = stored row j, stored row = label i):
              `FlatIPIndex(labels).rescore_device(index.reconstruct_n(), all labels)`.  -0.0 counts as +0.0
  candidates  of row j: the labels whose score is not NaN.  Scores of +-inf are outside the definition
  order       score descending, equal scores to the lower label: the project's key order
  probability m_j = the best score of row j, Z_j = sum over the candidates of exp(scale (S[j, i] - m_j)),
              P[j, i] = exp(scale (S[j, i] - m_j)) / Z_j.  scale is CLIP's logit_scale.exp() (default 100), rounded to float32.
              Defined mathematically: exp is not reproducible to the bit.  P and Z lie within `tag_prob_bound(C, scale, spread)` (relative,
              plus FLT_MIN absolute for P) of the float64 value on the same float32 scores, and have the same bits on every run and stream
  D, P, J     float32 / float32 / int64 [n, t]: score (to the bit), probability and label number of the row's best t = `top` labels,
              1 <= t <= tag_max_top() (64).  A slot is used while P >= float32(min_prob): P descends with the rank, so min_prob cuts
              the list at the first slot below it.  Unused slots hold -FLT_MAX / 0 / -1
  count, Z    int32 / float32 [n]: the used slots of each row and Z_j (0 for a row without candidates).  With D[:, 0] = m_j, Z gives
              the probability of any other label later
  rows        [row0, row1), default all: only these rows are computed; the others' lines of the outputs hold the unused values
              (tag_rows) or what the caller's tensors held (the `out` of tag_rows_device).  Row numbers, on an id-mapped index too

  tag_segments  the tags of a video: seg_off as in `grouping` / `neighbors` (empty runs allowed, rows outside every run count nowhere)
    votes[s, i] the rows of segment s whose first label is i
    mass[s, i]  the sum, over the rows of s and their used slots that name i, of rint(P 2^24) as an integer (P 2^24 is exact in float32)
    result      the top g = `top_labels` <= 64 labels per segment by (mass or votes, per `rank`) descending, equal values to the lower
                label, among the labels whose value is not 0: L int64 [nseg, g] (unused -1), mass uint64 [nseg, g], votes int32 [nseg, g]
                (unused 0), rows int32 [nseg] (the stored rows of each segment), mean_prob = mass / (2^24 rows) float64 [nseg, g]
    Both sums are integer sums: numpy reproduces both from the kernel's own P and J exactly, whatever the arrival order.  nseg x C may
    not exceed 2^25 table entries: beyond that the call raises ValueError (IVR_ERR_INVALID); tag the videos in groups then.

The probability bound (`tag_prob_bound`), with u = 2^-24 the unit roundoff of float32 and spread >= max_i (m_j - S[j, i]):
  argument    x = scale (s - m) is two roundings: |x^ - x| <= 2u |x| <= 2u scale spread.  Every term of Z reaches the final maximum
              through a chain of such arguments (its own, the rescalings of the online softmax, the final merge) whose magnitudes add
              up to scale (m_j - s): so the arguments of one term contribute 2u scale spread in all, whatever the number of rescalings,
              and exp(x^) = exp(x) exp(x^ - x) turns that into the same RELATIVE error (times exp's own conditioning, 1 + the error)
  exp         expf of the device library (OCML), documented at 1 ulp = 2u relative; one per link of the chain
  chain       a lane folds at most T = ceil(ceil(C / 16) / 8) tiles, then the 32 partial pairs of a column are merged: at most T + 1
              rescalings of a term, each one expf and one multiplication (3u), on top of the term's own expf (2u)
  sum         every term is non-negative: a sum of m terms in any fixed order has relative error <= (m - 1) u.  4 terms per tile and
              lane, T tiles, then 32 partials: depth 4 T + 32
  P           numerator exp(scale (s - m_j)): 2u scale spread + 2u; the division u; Z as above
  bound = 1.01 (2 (2u scale spread) + u (3 (T + 1) + 2 + 4 T + 32 + 3)): 5.4e-5 at C = 1000, scale = 100, spread = 2, of which 4.8e-5 are
  the two argument terms: at scale 100 a float32 cosine difference simply carries that much.  A numerator below FLT_MIN may be flushed
  where float64 keeps it, hence the absolute FLT_MIN in the test of P.
"""
import math

import numpy as np
import torch

from . import _ffi, _staging
from .index import FlatIPIndex

NEG_FLT_MAX = -np.finfo(np.float32).max
FLT_MIN = float(np.finfo(np.float32).tiny)
MASS_ONE = 1 << 24          # the fixed point of the mass: rint(P 2^24)
DEFAULT_SCALE = 100.0       # CLIP's logit_scale.exp()


def tag_max_labels():
    return _ffi.call("ivr_tag_max_labels")


def tag_max_top():
    return _ffi.call("ivr_tag_max_top")


def tag_prob_bound(C, scale, spread):
    """The relative error bound of P and Z (module docstring): C labels, `scale`, spread >= the largest m_j - S[j, i] of a row (2 for
    cosines of unit rows)."""
    u = 2.0 ** -24
    tiles = (int(C) + 15) // 16
    T = (tiles + 7) // 8
    return 1.01 * (2.0 * (2.0 * u * float(scale) * float(spread)) + u * (3 * (T + 1) + 2 + 4 * T + 32 + 3))


# -- the definition in numpy ---------------------------------------------------------------------------------------------------
def softmax64(S, scale):
    """(P64 float64 [n,C], Z64 float64 [n]) of the float32 scores S: the definition's probabilities in float64, a NaN score is no
    candidate (P64 = 0)."""
    S = np.asarray(S, np.float32).astype(np.float64)
    ok = ~np.isnan(S)
    m = np.where(ok, S, -np.inf).max(axis=1, keepdims=True, initial=-np.inf)
    with np.errstate(invalid="ignore"):
        e = np.where(ok, np.exp(float(np.float32(scale)) * (S - m)), 0.0)
    Z = e.sum(axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        P = np.where(Z[:, None] > 0, e / Z[:, None], 0.0)
    return P, Z


def tag_rows_ref(S, scale=DEFAULT_SCALE, t=5, min_prob=0.0):
    """S float32 [n,C] scores (S[j, i]: stored row j as the query, label i) -> (D float32 [n,t], P float32 [n,t], J int64 [n,t], count
    int32 [n], Z float32 [n]): the definition of the module docstring, P and Z the float64 values rounded to float32."""
    S = np.asarray(S, np.float32)
    if S.ndim != 2 or S.shape[1] < 1:
        raise ValueError(f"tag_rows_ref: S {S.shape} must be [n,C] with C >= 1")
    scale, t, min_prob = _staging.check_tags(S.shape[1], scale, t, min_prob, _ffi.IVR_TAG_MAX_LABELS, _ffi.IVR_TAG_MAX_TOP, "tag_rows_ref")
    n, C = S.shape
    S = S + np.float32(0)                                              # -0.0 counts and is reported as +0.0
    P64, Z64 = softmax64(S, scale)
    D = np.full((n, t), NEG_FLT_MAX, np.float32)
    P = np.zeros((n, t), np.float32)
    J = np.full((n, t), -1, np.int64)
    count = np.zeros(n, np.int32)
    lab = np.arange(C, dtype=np.int64)
    for j in range(n):
        ok = ~np.isnan(S[j])
        i, s = lab[ok], S[j, ok]
        order = np.lexsort((i, -s.astype(np.float64)))[:t]             # score descending, then label ascending
        p = P64[j, i[order]].astype(np.float32)
        below = np.flatnonzero(~(p >= np.float32(min_prob)))
        c = int(below[0]) if len(below) else len(order)
        count[j] = c
        D[j, :c], P[j, :c], J[j, :c] = s[order][:c], p[:c], i[order][:c]
    return D, P, J, count, Z64.astype(np.float32)


def tag_segments_ref(P, J, count, seg_off, C, g, rank="mass"):
    """The rows' lists P float32 [n,t], J int64 [n,t], count int32 [n] -> (L int64 [nseg,g], mass uint64 [nseg,g], votes int32
    [nseg,g], rows int32 [nseg]): the definition of the module docstring in integers.  seg_off None: one segment."""
    P, J, count = np.asarray(P, np.float32), np.asarray(J, np.int64), np.asarray(count, np.int32)
    n, t = P.shape
    g, by = _staging.check_tag_segments(g, rank, _ffi.IVR_TAG_MAX_TOP, "tag_segments_ref")
    lo, hi = _staging.segment_bounds(n, seg_off)
    starts = np.zeros(1, np.int64) if seg_off is None else np.asarray(seg_off, np.int64)[:-1]
    nseg = len(starts)
    # the segment of row j: the last run whose start is <= j, when the row lies in a run at all
    seg = np.searchsorted(np.asarray([0, n] if seg_off is None else seg_off, np.int64), np.arange(n), side="right") - 1
    inside = lo <= np.arange(n)
    fixed = np.rint(P.astype(np.float32) * np.float32(MASS_ONE)).astype(np.uint64)
    mass = np.zeros((nseg, C), np.uint64)
    votes = np.zeros((nseg, C), np.int32)
    rows = np.zeros(nseg, np.int32)
    for j in np.flatnonzero(inside & (hi > lo)):
        s = int(seg[j])
        rows[s] += 1
        c = int(count[j])
        np.add.at(mass[s], J[j, :c], fixed[j, :c])
        if c:
            votes[s, J[j, 0]] += 1
    L = np.full((nseg, g), -1, np.int64)
    M = np.zeros((nseg, g), np.uint64)
    V = np.zeros((nseg, g), np.int32)
    for s in range(nseg):
        value = votes[s].astype(np.uint64) if by else mass[s]
        order = [i for i in sorted(range(C), key=lambda i: (-int(value[i]), i)) if value[i] != 0][:g]
        L[s, :len(order)], M[s, :len(order)], V[s, :len(order)] = order, mass[s, order], votes[s, order]
    return L, M, V, rows


# -- the library calls ---------------------------------------------------------------------------------------------------------
def _labels(index, labels, what):
    if not isinstance(index, FlatIPIndex):
        raise ValueError(f"{what}: index must be a FlatIPIndex, got {type(index).__name__}")
    _staging.check_rows(labels, index.d, f"{what}: labels")
    t = _staging.dev_f32(labels, index.device)
    return t, _staging.is_staged(t, labels)


def tag_rows_device(index, labels, top=5, scale=DEFAULT_SCALE, min_prob=0.0, normalize=False, row0=0, row1=None, out=None):
    """The tags of the stored rows [row0, row1) on the device: (D, P, J, count, Z) CUDA tensors over ALL ntotal rows, the definition of
    the module docstring.  out: the five tensors of an earlier call, whose lines outside the range are then left as they are;
    without it those lines hold the unused values.  No host synchronisation unless the labels had to be staged."""
    lab, staged = _labels(index, labels, "tag_rows")
    C = int(lab.shape[0])
    scale, t, min_prob = _staging.check_tags(C, scale, top, min_prob, tag_max_labels(), tag_max_top(), "tag_rows")
    n = index.ntotal
    row0, row1 = _staging.check_row_range(row0, row1, n, "tag_rows")
    if out is None:
        dev, m = index.device, max(n, 1)                               # never a NULL pointer, even for an empty index
        out = (torch.full((m, t), NEG_FLT_MAX, dtype=torch.float32, device=dev), torch.zeros((m, t), dtype=torch.float32, device=dev),
               torch.full((m, t), -1, dtype=torch.int64, device=dev), torch.zeros(m, dtype=torch.int32, device=dev),
               torch.zeros(m, dtype=torch.float32, device=dev))
    else:
        shapes = [(torch.float32, (n, t)), (torch.float32, (n, t)), (torch.int64, (n, t)), (torch.int32, (n,)), (torch.float32, (n,))]
        if len(out) != 5 or any(not (isinstance(o, torch.Tensor) and o.device == index.device and o.dtype == dt and tuple(o.shape) == sh
                                     and o.is_contiguous()) for o, (dt, sh) in zip(out, shapes)):
            raise ValueError(f"tag_rows: out must be the five tensors of a call on {n} rows with top={t}")
        if n == 0:
            return tuple(out)
    index._call("ivr_index_tag_rows", lab, C, bool(normalize), scale, t, min_prob, row0, row1, *out)
    _staging.sync_if_staged(staged, index.device)
    return tuple(o[:n] for o in out)


def tag_rows(index, labels, top=5, scale=DEFAULT_SCALE, min_prob=0.0, normalize=False, row0=0, row1=None):
    """tag_rows_device as numpy arrays (D, P, J, count, Z)."""
    return tuple(o.cpu().numpy() for o in tag_rows_device(index, labels, top, scale, min_prob, normalize, row0, row1))


def tag_segments_device(index, labels, seg_off=None, top_labels=5, rank="mass", top=5, scale=DEFAULT_SCALE, min_prob=0.0,
                        normalize=False):
    """The tags of every segment on the device: (L int64 [nseg,g], mass int64 [nseg,g] (the uint64 sums, below 2^55), votes int32
    [nseg,g], rows int32 [nseg]) CUDA tensors, the definition of the module docstring with g = top_labels.  seg_off: integers
    [nseg+1], ascending (checked when it is a host array), or None for one segment."""
    lab, staged = _labels(index, labels, "tag_segments")
    C = int(lab.shape[0])
    scale, t, min_prob = _staging.check_tags(C, scale, top, min_prob, tag_max_labels(), tag_max_top(), "tag_segments")
    g, by = _staging.check_tag_segments(top_labels, rank, tag_max_top(), "tag_segments")
    seg, seg_staged, nseg = _staging.segments(seg_off, index.device, "tag_segments")
    ns, dev = max(nseg, 1), index.device
    L = torch.full((ns, g), -1, dtype=torch.int64, device=dev)          # what an empty index leaves: the call writes nothing then
    mass = torch.zeros((ns, g), dtype=torch.int64, device=dev)
    votes = torch.zeros((ns, g), dtype=torch.int32, device=dev)
    rows = torch.zeros(ns, dtype=torch.int32, device=dev)
    index._call("ivr_index_tag_segments", lab, C, bool(normalize), scale, t, min_prob, seg, nseg, g, by, L, mass, votes, rows)
    _staging.sync_if_staged(staged or seg_staged, index.device)
    return L, mass, votes, rows


def tag_segments(index, labels, seg_off=None, top_labels=5, rank="mass", top=5, scale=DEFAULT_SCALE, min_prob=0.0, normalize=False):
    """tag_segments_device as numpy arrays (L, mass uint64, votes, rows, mean_prob): mean_prob float64 [nseg,g] = mass / (2^24 rows),
    the mean probability of the label over the rows of the segment (0 for an empty segment)."""
    L, mass, votes, rows = (o.cpu().numpy() for o in tag_segments_device(index, labels, seg_off, top_labels, rank, top, scale, min_prob,
                                                                         normalize))
    mass = mass.view(np.uint64)
    mean = mass.astype(np.float64) / (float(MASS_ONE) * np.maximum(rows, 1)[:, None])
    return L, mass, votes, rows, mean


# -- the labels ------------------------------------------------------------------------------------------------------------------
def zero_shot_labels(extractor, names, template="a photo of a {}"):
    """The label vectors of a list of class names: extractor.encode_text (compat.CLIPFeatureExtractor: L2-normalised text features)
    of `template.format(name)` -> float32 [C, d]."""
    names = list(names)
    if not names or not all(isinstance(n, str) and n.strip() for n in names):
        raise ValueError("zero_shot_labels: names must be non-empty strings")
    feats = np.asarray(extractor.encode_text([template.format(n) for n in names]), dtype=np.float32)
    if feats.ndim != 2 or feats.shape[0] != len(names):
        raise ValueError(f"zero_shot_labels: encode_text returned {feats.shape} for {len(names)} names")
    return np.ascontiguousarray(feats)


def bound_ratio(got, want64, bound, absolute=0.0):
    """The largest |got - want64| / (bound want64 + absolute) over the entries (0 when there is none): what the tests print."""
    got, want64 = np.asarray(got, np.float64), np.asarray(want64, np.float64)
    if got.size == 0:
        return 0.0
    lim = bound * np.abs(want64) + absolute
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.where(lim > 0, np.abs(got - want64) / lim, np.where(got == want64, 0.0, math.inf))
    return float(r.max())
