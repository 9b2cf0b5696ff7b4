"""Fused search: one ranking of the stored rows from a SET of query vectors per query, over a FlatIPIndex.

Every other search of the library ranks the rows against one vector per query.  Several expansions of one text, a text together with
an example image, "like these frames but not like that one" and "all of these concepts in one frame" bring a set of vectors, and
joining their result lists on the host invents a score for a row that misses a list; for a minimum the best row is typically in the
head of no list at all.  Here every stored row is scored against every member and the scores are folded while they are still in
registers (ivr_index_search_fused / ivr_index_range_search_fused, csrc/search_fused.hip): the result is exact over all rows.

Definition (the `*_ref` functions below are this in numpy, to the bit, given the member scores).  This is the library's own
definition; `combine="veto"` has the shape of the best_score strategy of Qdrant's recommend API, without any claim of parity.

  slots      a fused query is a set of at most 16 members.  Its positive members occupy the slots 0 .. m-1 and its negative members
             the slots m .. m+mn-1, m and mn being the widths of the (padded) arrays of the call; a slot is positive (role 1),
             negative (role -1) or absent (role 0).  slots_pad = the next power of two of m + mn; the slots beyond m + mn are absent
  S[j, r]    the float32 inner product `FlatIPIndex.search` / `rescore_device` report for (member j, stored row r), -0.0 as +0.0
  T[j]       w[j] * S[j, r]: one float32 product, rounded on its own (never fused with what follows); w finite, 1 by default
  P          the fold of T over the positive members: fold="max" the maximum (expansion, OR), fold="min" the minimum (AND),
             fold="sum" the BALANCED PAIRWISE TREE over the slots_pad slots, ((T0 + T1) + (T2 + T3)) + ..., in which a slot that is
             absent or negative contributes +0.0: the order a butterfly of lane exchanges produces.  It is not an ascending sum, and
             the same members in other slots may differ in the last bit
  Nn         the maximum of T over the negative members
  F          without negative members P; combine="margin": P - Nn, one float32 subtraction; combine="veto": P when P > Nn, else
             -(Nn * Nn): a row that resembles a negative example at least as much as any positive one sinks, the further the more
  order      rows rank by (F descending, row ascending), -0.0 equal to +0.0: the order of every top-k of the library; reported
             scores are F + 0.0

Rows are labelled with their number, or with their stored id on an id-mapped index.  Unused result slots hold -FLT_MAX / -1.  The
range form returns every row with F >= threshold in FAISS's (lims, D, I) form, per fused query in ascending row order.
"""
import numpy as np
import torch

from . import _ffi, _staging
from ._faiss import FLT_MAX
from .index import FlatIPIndex
from .refine import _ordered

FUSE_MAX_MEMBERS = _ffi.IVR_FUSE_MAX_MEMBERS
FOLDS = tuple(_ffi.IVR_FUSE_FOLD)
COMBINES = tuple(_ffi.IVR_FUSE_COMBINE)


def slots_pad(n):
    """The columns a set of n slots occupies in the query tile: the next power of two (1, 2, 4, 8 or 16)."""
    p = 1
    while p < n:
        p *= 2
    return p


# -- checks shared by the definition and the library calls -----------------------------------------------------------------------
def _check_modes(fold, combine, what):
    if fold not in _ffi.IVR_FUSE_FOLD:
        raise ValueError(f"{what}: fold={fold!r} is none of {FOLDS}")
    if combine not in _ffi.IVR_FUSE_COMBINE:
        raise ValueError(f"{what}: combine={combine!r} is none of {COMBINES}")


def _check_tables(W, R, what):
    """weights float32 [nq,slots] and roles int8 [nq,slots] of a call: at most 16 slots, roles 1 / -1 / 0, every weight finite, a
    positive member in every set."""
    W = np.asarray(W)
    R = np.asarray(R)
    if R.ndim != 2 or W.shape != R.shape:
        raise ValueError(f"{what}: weights {W.shape} and roles {R.shape} must both be [nq,slots]")
    if R.shape[0] < 1:
        raise ValueError(f"{what}: no queries")
    if R.shape[1] < 1 or R.shape[1] > FUSE_MAX_MEMBERS:
        raise ValueError(f"{what}: {R.shape[1]} members outside [1,{FUSE_MAX_MEMBERS}]")
    if not np.isin(R, (-1, 0, 1)).all():
        raise ValueError(f"{what}: roles must be 1 (positive), -1 (negative) or 0 (absent)")
    W = W.astype(np.float32)
    if not np.isfinite(W).all():
        raise ValueError(f"{what}: weights must be finite")
    none = np.flatnonzero(~(R > 0).any(axis=1))
    if len(none):
        raise ValueError(f"{what}: set {int(none[0])} has no positive member")
    return np.ascontiguousarray(W), np.ascontiguousarray(R.astype(np.int8))


def _check_scores(S, W, R, what):
    S = np.asarray(S, np.float32)
    if S.ndim != 3:
        raise ValueError(f"{what}: S {S.shape} must be [nq,slots,N]")
    W, R = _check_tables(W, R, what)
    if S.shape[:2] != R.shape:
        raise ValueError(f"{what}: S {S.shape} does not match the tables {R.shape}")
    return S, W, R


# -- the definition in numpy ---------------------------------------------------------------------------------------------------
def fused_scores_ref(S, weights, roles, fold="max", combine="margin"):
    """S float32 [nq,slots,N] member scores, weights [nq,slots], roles [nq,slots] (1, -1, 0) -> F float32 [nq,N], the definition of
    the module docstring, before the + 0.0 of a reported score.  fold="sum" is the pairwise tree over slots_pad(slots) slots."""
    _check_modes(fold, combine, "fused_scores_ref")
    S, W, R = _check_scores(S, weights, roles, "fused_scores_ref")
    nq, slots, N = S.shape
    pos, neg = (R > 0)[:, :, None], (R < 0)[:, :, None]
    with np.errstate(invalid="ignore", over="ignore"):
        T = W[:, :, None] * (S + np.float32(0.0))                 # float32 * float32: one rounding
        if fold == "max":
            P = np.where(pos, T, np.float32(-np.inf)).max(axis=1)
        elif fold == "min":
            P = np.where(pos, T, np.float32(np.inf)).min(axis=1)
        else:
            terms = np.zeros((nq, slots_pad(slots), N), np.float32)
            terms[:, :slots] = np.where(pos, T, np.float32(0.0))
            while terms.shape[1] > 1:
                terms = terms[:, 0::2] + terms[:, 1::2]            # neighbours first: ((T0 + T1) + (T2 + T3)) + ...
            P = terms[:, 0]
        Nn = np.where(neg, T, np.float32(-np.inf)).max(axis=1)
        has = neg.any(axis=1)                                       # [nq,1]
        if combine == "margin":
            F = np.where(has, P - Nn, P)
        else:
            F = np.where(has & ~(P > Nn), -(Nn * Nn), P)
    return F.astype(np.float32)


def _labels(rows, ids):
    return rows if ids is None else np.asarray(ids).astype(np.int64)[rows]


def fused_search_ref(S, weights, roles, k, fold="max", combine="margin", ids=None):
    """(D float32 [nq,k], I int64 [nq,k]): the k best rows of every fused query by (F descending, row ascending), (-FLT_MAX, -1)
    beyond the stored rows.  ids: the labels of an id-mapped index (I = ids[row])."""
    k = _staging.check_k(k, _ffi.IVR_MAX_K)
    F = fused_scores_ref(S, weights, roles, fold, combine)
    nq, N = F.shape
    D = np.full((nq, k), -FLT_MAX, np.float32)
    I = np.full((nq, k), -1, np.int64)
    rows = np.arange(N, dtype=np.int64)
    for q in range(nq):
        best = rows[np.lexsort((rows, -_ordered(F[q]).astype(np.int64)))][:k]
        D[q, :len(best)] = F[q, best] + np.float32(0.0)
        I[q, :len(best)] = _labels(best, ids)
    return D, I


def fused_range_search_ref(S, weights, roles, threshold, fold="max", combine="margin", ids=None):
    """(lims int64 [nq+1], D float32, I int64): every row with F >= threshold, per fused query in ascending row order."""
    threshold = np.float32(threshold)
    if threshold != threshold:
        raise ValueError("fused_range_search_ref: threshold is NaN")
    F = fused_scores_ref(S, weights, roles, fold, combine) + np.float32(0.0)
    lims, D, I = [0], [], []
    for q in range(F.shape[0]):
        rows = np.flatnonzero(F[q] >= threshold).astype(np.int64)
        D.append(F[q, rows])
        I.append(_labels(rows, ids))
        lims.append(lims[-1] + len(rows))
    return np.asarray(lims, np.int64), np.concatenate(D).astype(np.float32), np.concatenate(I).astype(np.int64)


# -- the tables of a call ------------------------------------------------------------------------------------------------------
def _shape_of(x, what, name):
    """(members, present bool [nq,m], ragged) of a member argument: an array / tensor [nq,m,d] as it is, or a list of [m_i,d]
    arrays as a list."""
    if isinstance(x, (list, tuple)):
        if not len(x):
            raise ValueError(f"{what}: no queries")
        sets = [_staging.as_rows(s) for s in x]
        if any(s.ndim != 2 for s in sets):
            raise ValueError(f"{what}: every entry of the {name} list must be [m,d]")
        counts = [int(s.shape[0]) for s in sets]
        present = np.zeros((len(sets), max(counts)), bool)
        for i, c in enumerate(counts):
            present[i, :c] = True
        return sets, present, True
    if not isinstance(x, (np.ndarray, torch.Tensor)) or x.ndim != 3:
        raise ValueError(f"{what}: {name} must be [nq,m,d] or a list of [m,d] arrays, got {tuple(getattr(x, 'shape', ()))}")
    return x, np.ones(tuple(x.shape[:2]), bool), False


def _weights_of(w, present, ragged, what, name):
    """float32 [nq,m] weights of one side: None (all 1), [nq,m] / [m], or for ragged sets a list of per-set sequences; 0 where absent."""
    nq, m = present.shape
    out = np.zeros((nq, m), np.float32)
    if w is None:
        out[present] = 1.0
        return out
    if ragged and isinstance(w, (list, tuple)) and len(w) == nq and all(np.ndim(v) == 1 for v in w):
        for i, v in enumerate(w):
            v = np.asarray(v, np.float32)
            if len(v) != int(present[i].sum()):
                raise ValueError(f"{what}: {name}[{i}] has {len(v)} entries for a set of {int(present[i].sum())}")
            out[i, :len(v)] = v
        return out
    w = np.asarray(w.cpu() if isinstance(w, torch.Tensor) else w, np.float32)
    if w.ndim == 1 and w.shape[0] == m:
        w = np.broadcast_to(w, (nq, m))
    if w.shape != (nq, m):
        raise ValueError(f"{what}: {name} {w.shape} must be [{nq},{m}]")
    return np.where(present, w, np.float32(0.0)).astype(np.float32)


def _layout(positives, weights, negatives, negative_weights, mask, what):
    """(pos, neg or None, W float32 [nq,m+mn], R int8 [nq,m+mn], m): the member arguments and the tables in slot order."""
    pos, ppres, pragged = _shape_of(positives, what, "positives")
    nq, m = ppres.shape
    if mask is not None:
        if pragged:
            raise ValueError(f"{what}: mask goes with the array form of positives; ragged sets are given as a list")
        mk = np.asarray(mask.cpu() if isinstance(mask, torch.Tensor) else mask)
        if mk.dtype != bool or mk.shape != (nq, m):
            raise ValueError(f"{what}: mask must be bool [{nq},{m}], got {mk.dtype} {mk.shape}")
        ppres = ppres & mk
    neg, npres = None, np.zeros((nq, 0), bool)
    if negatives is not None:
        neg, npres, nragged = _shape_of(negatives, what, "negatives")
        if npres.shape[0] != nq:
            raise ValueError(f"{what}: negatives hold {npres.shape[0]} sets for {nq} fused queries")
        nw = _weights_of(negative_weights, npres, nragged, what, "negative_weights")
    elif negative_weights is not None:
        raise ValueError(f"{what}: negative_weights without negatives")
    if m + npres.shape[1] > FUSE_MAX_MEMBERS or m + npres.shape[1] < 1:
        raise ValueError(f"{what}: {m + npres.shape[1]} members outside [1,{FUSE_MAX_MEMBERS}]")
    W = _weights_of(weights, ppres, pragged, what, "weights")
    R = ppres.astype(np.int8)
    if neg is not None and npres.shape[1]:
        W = np.concatenate([W, nw], axis=1)
        R = np.concatenate([R, -npres.astype(np.int8)], axis=1)
    else:
        neg = None
    W, R = _check_tables(W, R, what)
    return pos, neg, W, R, m


def fused_tables(positives, weights=None, negatives=None, negative_weights=None, mask=None):
    """(weights float32 [nq,m+mn], roles int8 [nq,m+mn]) of a fused_search call with these arguments, in slot order: the tables the
    `*_ref` functions take and the order of the last axis of the `explain` output.  Raises the ValueErrors of the call."""
    return _layout(positives, weights, negatives, negative_weights, mask, "fused_search")[2:4]


# -- the library calls ---------------------------------------------------------------------------------------------------------
def _fill(Q, x, col0, d, device, what):
    """The member vectors x (array / tensor [nq,m,d], or the list of [m_i,d] sets) into Q[:, col0 : col0 + m]."""
    if isinstance(x, list):
        for i, s in enumerate(x):
            if s.shape[0]:
                t = _staging.dev_f32(s, device)
                if t.shape[1] != d:
                    raise ValueError(f"{what}: member dimension ({tuple(t.shape)}) != index dimension ({d})")
                Q[i, col0:col0 + t.shape[0]] = t
        return
    t = _staging.dev_f32(x, device)
    if t.shape[2] != d:
        raise ValueError(f"{what}: member dimension ({tuple(t.shape)}) != index dimension ({d})")
    Q[:, col0:col0 + t.shape[1]] = t


def _stage(index, positives, weights, negatives, negative_weights, mask, fold, combine, what):
    """The staged arguments of both calls: (Q float32 [nq,sp,d], W float32 [nq,sp], R int8 [nq,sp] CUDA tensors, nq, sp, slots =
    m + mn, R on the host)."""
    if not isinstance(index, FlatIPIndex):
        raise ValueError(f"{what}: index must be a FlatIPIndex, got {type(index).__name__}")
    _check_modes(fold, combine, what)
    pos, neg, W, R, m = _layout(positives, weights, negatives, negative_weights, mask, what)
    nq, slots = R.shape
    sp = slots_pad(slots)
    if nq * sp >= 2**31:
        raise ValueError(f"{what}: nq * slots = {nq * sp} >= 2^31")
    dev = index.device
    Q = torch.zeros((nq, sp, index.d), dtype=torch.float32, device=dev)
    _fill(Q, pos, 0, index.d, dev, what)
    if neg is not None:
        _fill(Q, neg, m, index.d, dev, what)
    Wp = np.zeros((nq, sp), np.float32)
    Rp = np.zeros((nq, sp), np.int8)
    Wp[:, :slots], Rp[:, :slots] = W, R
    Rd = torch.from_numpy(Rp).to(dev)
    Q = torch.where((Rd != 0)[:, :, None], Q, torch.zeros((), dtype=torch.float32, device=dev)).contiguous()     # absent slots: zero rows
    return Q, torch.from_numpy(Wp).to(dev), Rd, nq, sp, slots, R


def _explain(index, Q, R, I, slots, normalize):
    """E float32 [nq,k,slots]: the member scores S of every hit from rescore_device, -FLT_MAX for an absent slot / an unused hit."""
    nq, sp, d = Q.shape
    k = I.shape[1]
    rows = I
    if index.has_ids:                                               # labels -> the lowest row stored under each
        rows = torch.where(I >= 0, index._find_device(I.reshape(-1).contiguous()).reshape(I.shape), I)
    cand = rows.repeat_interleave(slots, dim=0).contiguous()        # [nq * slots, k]
    E = index.rescore_device(Q[:, :slots].reshape(nq * slots, d).contiguous(), cand, normalize=normalize)[0].reshape(nq, slots, k)
    E = torch.where(torch.from_numpy(R != 0).to(index.device)[:, :, None], E, torch.full((), -FLT_MAX, dtype=torch.float32, device=index.device))
    return E.permute(0, 2, 1).contiguous()


def fused_search_device(index, positives, k, fold="max", weights=None, negatives=None, negative_weights=None, combine="margin", mask=None,
                        normalize=False, explain=False):
    """Top-k fused search on the device -> (D float32 [nq,k], I int64 [nq,k]) CUDA tensors, the definition of fused_search_ref.
      positives         float32 [nq,m,d] (numpy or torch), or a list of [m_i,d] arrays for ragged sets (padded; the padding is absent)
      weights           None (all 1), [nq,m] or [m]; for the list form also a list of per-set sequences
      negatives         [nq,mn,d] or a list, with negative_weights likewise; m + mn <= 16
      mask              bool [nq,m] for the array form: False makes the member absent
      normalize         scale every member vector to unit length first
      explain           a third output E float32 [nq,k,m+mn]: the member scores S of every hit (rescore_device; -FLT_MAX for an absent
                        slot or an unused hit), which tell WHICH member matched.  Folding E by the definition (fused_scores_ref with
                        fused_tables) reproduces D to the bit.  On an id-mapped index a hit is looked up by its label: the lowest row
                        stored under it
    The tables are staged from the host, so the call synchronises with the stream."""
    what = "fused_search"
    k = _staging.check_k(k, _ffi.IVR_MAX_K)
    Q, W, R, nq, sp, slots, Rh = _stage(index, positives, weights, negatives, negative_weights, mask, fold, combine, what)
    D, I = _staging.alloc_DI(nq, k, index.device)
    index._call("ivr_index_search_fused", Q, nq, sp, W, R, _ffi.IVR_FUSE_FOLD[fold], _ffi.IVR_FUSE_COMBINE[combine], k, bool(normalize), D, I)
    E = _explain(index, Q, Rh, I, slots, normalize) if explain else None
    _staging.sync_if_staged(True, index.device)
    return (D, I, E) if explain else (D, I)


def fused_search(index, positives, k, fold="max", weights=None, negatives=None, negative_weights=None, combine="margin", mask=None,
                 normalize=False, explain=False):
    """fused_search_device as numpy arrays (D, I), or (D, I, E) with explain."""
    out = fused_search_device(index, positives, k, fold, weights, negatives, negative_weights, combine, mask, normalize, explain)
    return tuple(t.cpu().numpy() for t in out)


def fused_range_search_device(index, positives, threshold, fold="max", weights=None, negatives=None, negative_weights=None, combine="margin",
                              mask=None, normalize=False, cap=None):
    """Threshold fused search on the device: (lims int64 [nq+1], D float32 [cap], I int64 [cap], total) CUDA tensors, total = lims[nq:]
    (the number of results; entries at positions >= cap are counted but not written).  cap=None sizes D and I exactly: a counting pass
    with cap 0, one synchronisation, then the full pass.  The other arguments as for fused_search_device."""
    what = "fused_range_search"
    threshold = float(threshold)
    if threshold != threshold:
        raise ValueError(f"{what}: threshold is NaN")
    if cap is not None and int(cap) < 0:
        raise ValueError(f"{what}: cap={cap} < 0")
    Q, W, R, nq, sp, slots, _ = _stage(index, positives, weights, negatives, negative_weights, mask, fold, combine, what)
    lims = torch.empty(nq + 1, dtype=torch.int64, device=index.device)

    def run(c):
        D = torch.empty(max(c, 1), dtype=torch.float32, device=index.device)      # never a NULL pointer, even for cap 0
        I = torch.empty(max(c, 1), dtype=torch.int64, device=index.device)
        index._call("ivr_index_range_search_fused", Q, nq, sp, W, R, _ffi.IVR_FUSE_FOLD[fold], _ffi.IVR_FUSE_COMBINE[combine], threshold,
                    bool(normalize), lims, D, I, int(c))
        return D[:c], I[:c]

    with torch.cuda.device(index.device):
        if cap is None:
            run(0)
            cap = int(lims[nq].item())
        D, I = run(int(cap))
        _staging.sync_if_staged(True)
    return lims, D, I, lims[nq:]


def fused_range_search(index, positives, threshold, fold="max", weights=None, negatives=None, negative_weights=None, combine="margin",
                       mask=None, normalize=False):
    """(lims, D, I) numpy arrays: every row with F >= threshold, per fused query in ascending row order."""
    lims, D, I, _ = fused_range_search_device(index, positives, threshold, fold, weights, negatives, negative_weights, combine, mask, normalize)
    return lims.cpu().numpy(), D.cpu().numpy(), I.cpu().numpy()
