"""ORACLE (test infrastructure, never shipped, never imported by the product path).

float64 restatement of the small reducing kernels and a derived per-element bound for each: the cosine of row pairs
(rowwise_cosine_kernel, band_cosine_kernel and the chain of dedup_kernel, csrc/dedup.hip), the in-place row normalisation
(l2_normalize_kernel, csrc/search_index.hip) and the centroid update of k-means (segment_mean_kernel, csrc/search_ivf.hip).
Everything is numpy float64 on the float32 operands exactly as the kernels read them, so the only difference between kernel and
reference is the kernel's own rounding.

U = 2^-24 is the unit roundoff of float32.  A row of d floats is reduced by one wave: lane l runs an fma chain over the columns
l, l + 64, ... (ceil(d / 64) links, one rounding each) and ivr_wave_sum adds the 64 lane sums in a tree of six levels, so every
input passes through at most

    m(d) = ceil(d / 64) + 6

roundings.  All bounds are first order in U (the terms of order (m U)^2 are below 2e-11 of the bound for d <= 4099).

Cosine.  cos = dot / (na nb), na = sqrtf(sa) (1 where sa = 0), the sklearn convention of video_frame_filter.py:63-70.
  * dot: a float32 sum of d products in any order with at most m roundings on every path is within m U sum_k |a_k b_k| of the exact
    one: m U sum|a b| / (na nb) in the quotient.
  * sa, sb: sums of non-negative terms, so relative m U each; the root halves that (0.5 m U each, m U for the product na nb).
  * two roots, the product na nb and the quotient: correctly rounded operations are U each; 2 U each is allowed (8 U).
        |out - cos| <= U (m sum|a_k b_k| / (na nb) + (m + 8) |cos|)
    A zero row has dot = 0 exactly and norm 1: cos = 0 and the bound is 0.

Row normalisation.  out_k = x_k / sqrtf(ss): ss relative m U, halved by the root, the root and the quotient U each:
        |out - ref| <= (0.5 m + 2) U |ref|
    and the float64 norm of an output row is within (0.5 m + 3) U of 1 (the quotient roundings move the norm by at most U more).

Segment mean.  A column is summed over the cnt rows of the segment in double (cnt - 1 additions), multiplied by the double
1 / cnt (two roundings) and rounded to float32 once:
        |out - mean| <= 2^-24 |mean| + eps,     eps = (cnt + 2) 2^-53 sum|x| / cnt
With normalize the reference is m32 / ||m32||, m32 = float32(mean), the norm in float64.  The kernel's own float32 mean lies
between float32(mean - eps) and float32(mean + eps) (rounding is monotone): almost always that is m32 itself, and where a rounding
boundary falls inside the interval the difference `dev` enters the bound directly and through the norm.  The kernel's norm is a
double sum of the squares (relative error of a few 2^-53) rounded to float32 once, the quotient once more:
        |out - ref| <= dev / ||m32|| + |ref| ||dev|| / ||m32|| + 2^-23 (1 + 2^-20) |ref|
A zero mean stays zero (norm taken as 1), an empty segment is a row of NaNs, seg_off is clipped to [0, n] (include/ivr_api.h).

tests/test_reduce_ref_cpu.py checks on the CPU that a numpy float32 emulation of the kernels as written stays inside these bounds and
that eleven typical faults leave them (or flip a decision).
"""
import math

import numpy as np

U = 2.0 ** -24


def m(d):
    """Roundings on the longest path of a wave's row reduction: the lane's fma chain and the six levels of ivr_wave_sum."""
    return -(-int(d) // 64) + 6


def _f64(x):
    x = np.asarray(x)
    if x.dtype != np.float32:
        raise TypeError(f"the references take the float32 operands the kernels read, got {x.dtype}")
    return x.astype(np.float64)


def _norms(x):
    n = np.sqrt((x * x).sum(axis=-1))
    return np.where(n > 0, n, 1.0)


def cosine_ref(a, b):
    """float64 cos(a[i], b[i]) of float32 [n,d] (or [d]) operands, zero norm -> 1 as sklearn's cosine_similarity."""
    a, b = _f64(a), _f64(b)
    return (a * b).sum(axis=-1) / (_norms(a) * _norms(b))


def cosine_bound(a, b):
    """Per-pair bound of |float32 kernel - cosine_ref| (module docstring)."""
    a, b = _f64(a), _f64(b)
    md = m(a.shape[-1])
    nn = _norms(a) * _norms(b)
    return U * (md * np.abs(a * b).sum(axis=-1) / nn + (md + 8) * np.abs((a * b).sum(axis=-1) / nn))


def l2_normalize_ref(x):
    """float64 x / ||x|| per row of a float32 [n,d] array; zero rows stay zero (signs kept)."""
    x = _f64(x)
    return x / _norms(x)[..., None]


def l2_normalize_bound(x):
    return (0.5 * m(np.asarray(x).shape[-1]) + 2) * U * np.abs(l2_normalize_ref(x))


def unit_norm_bound(d):
    """How far the float64 norm of a normalised float32 row may lie from 1."""
    return (0.5 * m(d) + 3) * U


def flat_score_bound(d, row_norm):
    """What the flat index states for one float32 inner product with a unit-norm query (acc_eps of csrc/search_internal.h, the
    bound tests/test_ivf_gpu.py holds the list scan to): dp * 1.2e-7 * ||row||, dp = d rounded up to a multiple of 16."""
    return (-(-int(d) // 16) * 16) * 1.2e-7 * np.asarray(row_norm, dtype=np.float64)


def _segments(n, seg_off):
    off = np.asarray(seg_off, dtype=np.int64)
    for s in range(len(off) - 1):
        s0 = min(max(int(off[s]), 0), n)
        yield s, s0, min(max(int(off[s + 1]), s0), n)


def _segment_stats(rows, seg_off):
    """(mean float64 [nseg,d] with NaN rows for empty segments, eps [nseg,d]) - eps as in the module docstring."""
    rows = _f64(rows)
    n, d = rows.shape
    nseg = len(seg_off) - 1
    mean = np.full((nseg, d), np.nan)
    eps = np.zeros((nseg, d))
    for s, s0, s1 in _segments(n, seg_off):
        if s1 > s0:
            cnt = s1 - s0
            mean[s] = np.array([math.fsum(col) for col in rows[s0:s1].T.tolist()]) / cnt       # exactly rounded column sums
            eps[s] = (cnt + 2) * 2.0 ** -53 * np.abs(rows[s0:s1]).sum(axis=0) / cnt
    return mean, eps


def segment_mean_ref(rows, seg_off, normalize):
    """out[s] = mean of rows[seg_off[s] : seg_off[s+1]] in float64 (offsets clipped to [0, n], an empty segment a NaN row); with
    normalize the float32-rounded mean divided by its float64 norm (a zero mean stays zero)."""
    return segment_mean_ref_bound(rows, seg_off, normalize)[0]


def segment_mean_bound(rows, seg_off, normalize):
    """Per-element bound of |kernel - segment_mean_ref| (module docstring); NaN rows of empty segments have bound 0."""
    return segment_mean_ref_bound(rows, seg_off, normalize)[1]


def segment_mean_ref_bound(rows, seg_off, normalize):
    """(segment_mean_ref, segment_mean_bound) from one pass over the rows."""
    mean, eps = _segment_stats(rows, seg_off)
    if not normalize:
        return mean, 2.0 ** -24 * np.abs(np.nan_to_num(mean)) + eps
    m32 = mean.astype(np.float32).astype(np.float64)
    return m32 / _norms(np.nan_to_num(m32))[:, None], _normalized_bound(mean, eps)


def _normalized_bound(mean, eps):
    empty = np.isnan(mean[:, 0])
    mean = np.nan_to_num(mean)
    m32 = mean.astype(np.float32).astype(np.float64)
    lo, hi = (mean - eps).astype(np.float32).astype(np.float64), (mean + eps).astype(np.float32).astype(np.float64)
    dev = np.maximum(np.abs(lo - m32), np.abs(hi - m32))
    nrm = _norms(m32)[:, None]
    ref = m32 / nrm
    b = dev / nrm + np.abs(ref) * np.sqrt((dev * dev).sum(axis=1))[:, None] / nrm + 2.0 ** -23 * (1 + 2.0 ** -20) * np.abs(ref)
    b[empty] = 0.0
    return b


class Comparisons:
    """The cosines a keep / drop chain compared with its threshold: float64 `sim`, their `bound` (cosine_bound) and the rows
    (`i`, `j`; j = -1 is the carried frame) of each."""

    def __init__(self):
        self.sim, self.bound, self.i, self.j = [], [], [], []

    def add(self, E, i, j, other=None):
        b = E[j] if other is None else other
        self.sim.append(float(cosine_ref(E[i], b)))
        self.bound.append(float(cosine_bound(E[i], b)))
        self.i.append(i)
        self.j.append(-1 if other is not None else j)
        return self.sim[-1]

    def margin(self, thr):
        """(min |sim - float32 thr|, 4 * the largest bound): decisions are comparable across float32 summation orders when the
        first exceeds the second.  (inf, 0) when nothing was compared."""
        if not self.sim:
            return np.inf, 0.0
        return float(np.abs(np.array(self.sim) - float(np.float32(thr))).min()), 4.0 * max(self.bound)

    def clear_of(self, thr):
        gap, need = self.margin(thr)
        return gap > need


def keep_chain_ref(E, thr, min_distance=1, prev=None):
    """The sequential keep / drop chain (video_frame_filter.py:63-70; with min_distance, filter.py:178-222 without its "always
    keep the last frame"): a frame is kept iff its cosine to the last kept frame is below the float32 threshold; the first frame
    of a chain without a carried frame `prev` is always kept; a frame closer than min_distance rows to the last frame kept in this
    call is dropped without a comparison.  Returns (mask bool [n], Comparisons, the last kept row of E or None)."""
    E = np.asarray(E)
    thr = float(np.float32(thr))
    cmp = Comparisons()
    mask = np.zeros(len(E), dtype=bool)
    last, cur = None, prev
    for i in range(len(E)):
        keep = True
        if cur is not None or last is not None:
            if min_distance > 1 and last is not None and i - last < min_distance:
                keep = False
            else:
                sim = cmp.add(E, i, last, None if last is not None else cur)
                keep = sim < thr
        if keep:
            last = i
            mask[i] = True
    return mask, cmp, last


def keep_window_ref(E, thr, window):
    """filter.py:224-258: frame i is kept iff no KEPT frame j in [i - window, i) has cosine >= the float32 threshold (window clipped
    to the number of frames).  Every kept j of the window is compared (a superset of what either scan order looks at before it
    stops).  Returns (mask bool [n], Comparisons)."""
    E = np.asarray(E)
    thr = float(np.float32(thr))
    n = len(E)
    window = min(int(window), n)
    cmp = Comparisons()
    mask = np.zeros(n, dtype=bool)
    for i in range(n):
        keep = True
        for j in range(max(0, i - window), i):
            if mask[j] and cmp.add(E, i, j) >= thr:
                keep = False
        mask[i] = keep
    return mask, cmp
