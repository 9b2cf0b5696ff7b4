"""Diversified search: maximal marginal relevance (MMR) and near-duplicate suppression over a FlatIPIndex, at query time.

Every search of the library ranks rows by relevance alone, and in a keyframe index the head of such a list is routinely one shot
repeated.  `keyframes.py`, `cluster.py` and `dedup.py` treat that when the index is built and `grouping.py` per video; two videos that
show one scene, or one long video with a recurring shot, still fill a results page with one picture.  Here a candidate list (the top
fetch_k of a search, or the labels any base index of the package proposes) is re-ranked greedily by what the frames look like
(ivr_index_diversify, csrc/search_diverse.hip).  Vector stores call this max_marginal_relevance_search (LangChain's FAISS wrapper) or
MMR (Qdrant, Elasticsearch, OpenSearch); the plainer relative drops a hit that is nearly the same as a better hit.

Definition (the `*_ref` functions below are this in numpy, to the bit, given R and P), per query q with its list cand[q, 0 .. kc):

  candidates  entries are storage rows, positional like `FlatIPIndex.rescore_device`; an entry outside [0, ntotal) is absent; a row
              named twice is two candidates
  R[j]        the float32 score `rescore_device` reports for (query q, row cand[j]): the relevance, with the bits of `search`
  P[i, j]     the float32 score `rescore_device` reports for (query = the stored float32 row cand[i], row cand[j]): the chosen row is
              the query operand.  R and P enter the arithmetic as reported, -0.0 as +0.0
  order       candidates rank by (value descending, -0.0 equal to +0.0; row ascending; position in cand ascending)
  selection   greedy, t = 0 .. k-1; m[j] = the greatest P[s, j] over the candidates s chosen so far, by float compare
  MMR         lambda_mult in [0, 1] as float32, mu = float32(1) - lambda_mult.  The first choice is the best candidate by R, what
              `search` returns first whatever lambda_mult is; from the second on the value of a candidate not yet chosen is
              (lambda_mult * R[j]) - (mu * m[j]): two float32 products and one float32 subtraction, each rounded on its own
  suppress    the value is R[j]; a candidate with m[j] >= threshold is out for good; the selection ends early when nothing is left

Output, in the order chosen: D = R of the chosen candidate, I = its row (its stored id on an id-mapped index), M = its m at the moment
it was chosen (how redundant is this hit?), -FLT_MAX in slot 0.  Unused slots hold -FLT_MAX / -1 / -FLT_MAX.  lambda_mult = 1, and a
threshold above every P, give the order of `refine_order_ref`.
"""
import numpy as np
import torch

from . import _ffi, _staging
from ._faiss import FLT_MAX
from .index import FlatIPIndex
from .refine import _ordered

MMR, SUPPRESS = _ffi.IVR_DIVERSE_MMR, _ffi.IVR_DIVERSE_SUPPRESS


# -- the definition in numpy ---------------------------------------------------------------------------------------------------
def _check_param(mode, param, what):
    name = "lambda_mult" if mode == MMR else "threshold"
    if isinstance(param, bool) or not isinstance(param, (int, float, np.integer, np.floating)):
        raise ValueError(f"{what}: {name} must be a number, got {type(param).__name__}")
    p = np.float32(param)
    if p != p:
        raise ValueError(f"{what}: {name}={param} is NaN")
    if mode == MMR and not 0.0 <= p <= 1.0:
        raise ValueError(f"{what}: lambda_mult={param} outside [0,1]")
    return p


def _select_ref(R, P, cand, k, mode, param, ntotal, ids, what):
    R = np.asarray(R, np.float32)
    P = np.asarray(P, np.float32)
    cand = np.asarray(cand).astype(np.int64)
    if R.ndim != 2 or R.shape != cand.shape or P.shape != R.shape + R.shape[1:]:
        raise ValueError(f"{what}: R {R.shape} and cand {cand.shape} must be [nq,kc] and P {P.shape} [nq,kc,kc]")
    nq, kc = R.shape
    k = int(k)
    if k < 1 or k > kc:
        raise ValueError(f"{what}: k={k} outside [1,{kc}]")
    param = _check_param(mode, param, what)
    mu = np.float32(1.0) - param
    R = R + np.float32(0.0)
    P = P + np.float32(0.0)
    D = np.full((nq, k), -FLT_MAX, np.float32)
    I = np.full((nq, k), -1, np.int64)
    M = np.full((nq, k), -FLT_MAX, np.float32)
    for q in range(nq):
        rows = cand[q]
        live = rows >= 0
        if ntotal is not None:
            live &= rows < int(ntotal)
        m = np.full(kc, -FLT_MAX, np.float32)
        for t in range(k):
            j = np.flatnonzero(live)
            if not len(j):
                break
            value = R[q, j]
            if mode == MMR and t > 0:
                value = (param * R[q, j]).astype(np.float32) - (mu * m[j]).astype(np.float32)
            s = j[np.lexsort((j, rows[j], -_ordered(value).astype(np.int64)))[0]]
            D[q, t], M[q, t] = R[q, s], m[s]
            I[q, t] = rows[s] if ids is None else np.asarray(ids).astype(np.int64)[rows[s]]
            live[s] = False
            j = np.flatnonzero(live)
            m[j] = np.where(P[q, s, j] > m[j], P[q, s, j], m[j])
            if mode == SUPPRESS:
                live[j[m[j] >= param]] = False
    return D, I, M


def mmr_ref(R, P, cand, k, lambda_mult, ntotal=None, ids=None):
    """R float32 [nq,kc], P float32 [nq,kc,kc], cand integers [nq,kc] -> (D float32 [nq,k], I int64 [nq,k], M float32 [nq,k]), the MMR
    of the module docstring.  ntotal: entries at or above it are absent too; ids: the labels of an id-mapped index (I = ids[row])."""
    return _select_ref(R, P, cand, k, MMR, lambda_mult, ntotal, ids, "mmr_ref")


def suppress_ref(R, P, cand, k, threshold, ntotal=None, ids=None):
    """As mmr_ref for the near-duplicate suppression of the module docstring."""
    return _select_ref(R, P, cand, k, SUPPRESS, threshold, ntotal, ids, "suppress_ref")


# -- the library calls ---------------------------------------------------------------------------------------------------------
def _check_index(index, what):
    if not isinstance(index, FlatIPIndex):
        raise ValueError(f"{what}: index must be a FlatIPIndex, got {type(index).__name__}")


def _rerank(index, x, cand, k, mode, param, normalize, what):
    _check_index(index, what)
    param = _check_param(mode, param, what)
    t, staged = _staging.queries_f32(_staging.as_rows(x), index.d, index.device)
    nq = int(t.shape[0])
    _staging.check_nq(nq, what)
    if not (isinstance(cand, torch.Tensor) and cand.is_cuda and cand.device == index.device and cand.dtype == torch.int64
            and cand.dim() == 2 and cand.shape[0] == nq and cand.is_contiguous()):
        raise ValueError(f"{what} expects cand as a contiguous int64 CUDA tensor [{nq},kc] on {index.device}")
    kc = int(cand.shape[1])
    if kc < 1 or kc > _ffi.IVR_MAX_K:
        raise ValueError(f"{what}: kc={kc} outside [1,{_ffi.IVR_MAX_K}]")
    k = _staging.check_k(k, kc)
    D, I = _staging.alloc_DI(nq, k, index.device)
    M = torch.empty((nq, k), dtype=torch.float32, device=index.device)
    index._call("ivr_index_diversify", t, nq, cand, kc, k, mode, float(param), bool(normalize), D, I, M)
    _staging.sync_if_staged(staged, index.device)
    return D, I, M


def mmr_rerank_device(index, x, cand, k, lambda_mult=0.5, normalize=False):
    """MMR over candidate lists on the device: x float32 [nq,d] (numpy or torch), cand a contiguous int64 CUDA tensor [nq,kc] of row
    POSITIONS (the labels any base index of the package proposes, as RefineFlatIndex passes them on) -> (D float32 [nq,k], I int64
    [nq,k], M float32 [nq,k]) CUDA tensors, the definition of mmr_ref.  No host synchronisation unless x had to be staged."""
    return _rerank(index, x, cand, k, MMR, lambda_mult, normalize, "mmr_rerank")


def suppress_rerank_device(index, x, cand, k, threshold, normalize=False):
    """Near-duplicate suppression over candidate lists on the device, arguments and results as for mmr_rerank_device; the definition
    of suppress_ref."""
    return _rerank(index, x, cand, k, SUPPRESS, threshold, normalize, "suppress_rerank")


def _search(index, x, k, fetch_k, mode, param, normalize, what):
    _check_index(index, what)
    _check_param(mode, param, what)
    fetch_k = _staging.check_k(fetch_k, _ffi.IVR_MAX_K)
    if int(k) < 1 or int(k) > fetch_k:
        raise ValueError(f"{what}: k={int(k)} outside [1,fetch_k={fetch_k}]")
    t, staged = _staging.queries_f32(_staging.as_rows(x), index.d, index.device)
    _staging.check_nq(t.shape[0], what)
    with torch.cuda.device(index.device):
        rows = index.search_device(t, fetch_k, normalize=normalize)[1]
        if index.has_ids:                                          # labels -> rows, as reconstruct_batch_device: the lowest row under the id
            rows = index._find_device(rows.reshape(-1)).reshape(rows.shape)
        out = _rerank(index, t, rows.contiguous(), k, mode, param, normalize, what)
        _staging.sync_if_staged(staged, index.device)
    return out


def mmr_search_device(index, x, k, fetch_k, lambda_mult=0.5, normalize=False):
    """index.search_device(x, fetch_k) followed by mmr_rerank_device at k: (D, I, M) CUDA tensors.  On an id-mapped index the labels of
    the search are turned back into rows on the device (an id stored twice stands for its lowest row) and I holds stored ids.  No host
    synchronisation unless x had to be staged.  lambda_mult = 1 is index.search(x, k) to the bit."""
    return _search(index, x, k, fetch_k, MMR, lambda_mult, normalize, "mmr_search")


def dedup_search_device(index, x, k, fetch_k, threshold=0.95, normalize=False):
    """index.search_device(x, fetch_k) followed by suppress_rerank_device at k: the best k hits none of which scores `threshold` or
    more against a better one; unused slots when fewer are left.  Otherwise as mmr_search_device."""
    return _search(index, x, k, fetch_k, SUPPRESS, threshold, normalize, "dedup_search")


def _numpy(out):
    return tuple(t.cpu().numpy() for t in out)


def mmr_rerank(index, x, cand, k, lambda_mult=0.5, normalize=False):
    """mmr_rerank_device as numpy arrays (D, I, M)."""
    return _numpy(mmr_rerank_device(index, x, cand, k, lambda_mult, normalize))


def suppress_rerank(index, x, cand, k, threshold, normalize=False):
    """suppress_rerank_device as numpy arrays (D, I, M)."""
    return _numpy(suppress_rerank_device(index, x, cand, k, threshold, normalize))


def mmr_search(index, x, k, fetch_k, lambda_mult=0.5, normalize=False):
    """mmr_search_device as numpy arrays (D, I, M)."""
    return _numpy(mmr_search_device(index, x, k, fetch_k, lambda_mult, normalize))


def dedup_search(index, x, k, fetch_k, threshold=0.95, normalize=False):
    """dedup_search_device as numpy arrays (D, I, M)."""
    return _numpy(dedup_search_device(index, x, k, fetch_k, threshold, normalize))
