"""FAISS-shaped IndexRefineFlat resident in MI355X HBM: a cheap base index proposes k * k_factor candidates per query, a flat index
over the same rows scores exactly those and returns the best k.

Stands in for `faiss.IndexRefineFlat(base)`.  The base is one of the approximate indexes of this package (`IndexLSH`, `PQIndex`,
`SQIndex`, `IVFFlatIndex`, `IVFPQIndex`, `IVFSQIndex`, `GraphFlatIndex`) or a plain `FlatIPIndex`; the refine index is a plain `FlatIPIndex` that receives every row the
base receives, in the same order, so a base label is a row of the refine index (there is no add_with_ids, as in faiss).  The base's
labels never leave the device: they go straight into `FlatIPIndex.rescore_device` (ivr_index_rescore, csrc/search_refine.hip), whose
scores carry the bits of `FlatIPIndex.search` and whose ordering is pinned to `refine_order_ref` below.
"""
import numpy as np
import torch

from . import _ffi, _staging
from ._coded import CodedIndex
from ._faiss import FLT_MAX, METRIC_INNER_PRODUCT, search_numpy, typed_params
from .graph import GraphFlatIndex, SearchParametersHNSW
from .index import FlatIPIndex, SearchParameters, _selector
from .ivf import IVFFlatIndex, SearchParametersIVF
from .ivfpq import IVFPQIndex
from .ivfsq import IVFSQIndex


def _ordered(s):
    """float32 -> uint32 that orders like the scores (larger score, larger key), -0.0 folded onto +0.0: ivr_f2ord of the library."""
    u = (np.asarray(s, np.float32) + np.float32(0.0)).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000))


def refine_order_ref(S, cand, k, ntotal=None):
    """The ordering pass of a re-ranking, pure numpy: S float32 [nq,kc] = the score of every candidate, cand integers [nq,kc] = the
    candidate rows -> (D float32 [nq,k], I int64 [nq,k]).  An entry of cand below 0 (or at / above ntotal, when given) is absent
    and its score is ignored.  The present candidates of a query are ranked by score descending (-0.0 counts as +0.0 and is
    reported as +0.0), equal scores by the lower row first; the position in cand has no influence.  A row named m times appears m
    times, in adjacent slots.  Slots beyond the present candidates hold (-FLT_MAX, -1).  1 <= k <= kc."""
    S = np.asarray(S, np.float32)
    cand = np.asarray(cand).astype(np.int64)
    if S.ndim != 2 or S.shape != cand.shape:
        raise ValueError(f"refine_order_ref: S {S.shape} and cand {cand.shape} must both be [nq,kc]")
    nq, kc = S.shape
    k = int(k)
    if k < 1 or k > kc:
        raise ValueError(f"refine_order_ref: k={k} outside [1,{kc}]")
    D = np.full((nq, k), -FLT_MAX, np.float32)
    I = np.full((nq, k), -1, np.int64)
    for i in range(nq):
        here = cand[i] >= 0
        if ntotal is not None:
            here &= cand[i] < int(ntotal)
        j = np.flatnonzero(here)
        rows, keys = cand[i, j], _ordered(S[i, j]).astype(np.int64)
        order = np.lexsort((rows, -keys))[:k]
        D[i, :len(order)] = S[i, j[order]] + np.float32(0.0)
        I[i, :len(order)] = rows[order]
    return D, I


class IndexRefineSearchParameters:
    """faiss.IndexRefineSearchParameters(k_factor=..., base_index_params=...): k_factor overrides the index attribute for one call,
    base_index_params is what the base index's own search() takes as params (SearchParametersIVF for IVFFlatIndex, IVFPQIndex and IVFSQIndex,
    SearchParametersHNSW, or
    SearchParameters(sel=...) for a flat base; None for IndexLSH, PQIndex and SQIndex).  A selector on the refine level is not supported: search raises
    ValueError when sel is set."""

    def __init__(self, k_factor=None, base_index_params=None, sel=None):
        self.k_factor = None if k_factor is None else _check_k_factor(k_factor, "IndexRefineSearchParameters")
        self.base_index_params = base_index_params
        self.sel = sel


def _check_k_factor(v, who):
    v = float(v)
    if not v >= 1.0:
        raise ValueError(f"{who}: k_factor={v} < 1")
    return v


def _base_kwargs(base, params):
    """The keyword arguments of base.search_device that carry base_index_params."""
    if isinstance(base, CodedIndex):                # IndexLSH, PQIndex, SQIndex
        if params is not None:
            raise ValueError(f"base_index_params must be None for {type(base).__name__}, got {type(params).__name__}")
        return {}
    if isinstance(base, (IVFFlatIndex, IVFPQIndex, IVFSQIndex)):
        params = typed_params(params, SearchParametersIVF, type(base).__name__)
        return {} if params is None else {"nprobe": params.nprobe}
    if isinstance(base, GraphFlatIndex):
        params = typed_params(params, SearchParametersHNSW, "GraphFlatIndex")
        return {} if params is None else {"efSearch": params.efSearch}
    if params is not None and not isinstance(params, SearchParameters):
        raise ValueError(f"base_index_params must be a SearchParameters for a flat base, got {type(params).__name__}")
    sel = _selector(params)
    return {} if sel is None else {"sel": sel}


class RefineFlatIndex:
    """Base index + exact re-ranking (FAISS IndexRefineFlat contract) on one GPU.

    search(x, k) asks the base for int(k * k_factor) labels per query, scores those rows exactly in refine_index and returns the
    best k under the contract of FlatIPIndex.search: float32 descending, int64 row numbers, equal scores the lower row first, -1
    padding.  The base must be empty when it is wrapped and receives its rows through add() of this object only."""

    def __init__(self, base_index, device=None):
        if not isinstance(base_index, (CodedIndex, IVFFlatIndex, IVFPQIndex, IVFSQIndex, GraphFlatIndex, FlatIPIndex)):
            raise ValueError(f"RefineFlatIndex: the base must be an IndexLSH, PQIndex, SQIndex, IVFFlatIndex, IVFPQIndex, IVFSQIndex, GraphFlatIndex or FlatIPIndex, "
                             f"got {type(base_index).__name__}")
        if isinstance(base_index, FlatIPIndex) and base_index.has_ids:
            raise ValueError("RefineFlatIndex: a flat base must be a plain index, this one is id-mapped")
        if base_index.ntotal != 0:
            raise ValueError(f"RefineFlatIndex: the base must be empty, it holds {base_index.ntotal} rows")
        dev = base_index.device.index
        if device is not None and int(device) != dev:
            raise ValueError(f"RefineFlatIndex: device={device}, the base lives on device {dev}")
        self.base_index = base_index
        self.d = int(base_index.d)
        self.metric_type = METRIC_INNER_PRODUCT
        self._k_factor = 1.0
        self.refine_index = FlatIPIndex(self.d, device=dev)
        self.device = self.refine_index.device

    # -- attributes ------------------------------------------------------------------------------
    @property
    def ntotal(self):
        return self.refine_index.ntotal

    @property
    def is_trained(self):
        return bool(getattr(self.base_index, "is_trained", True))

    @property
    def k_factor(self):
        return self._k_factor

    @k_factor.setter
    def k_factor(self, v):
        self._k_factor = _check_k_factor(v, "RefineFlatIndex")

    # -- FAISS surface ---------------------------------------------------------------------------
    def train(self, x):
        return self.base_index.train(x)

    def add(self, x):
        """Append rows to the base and then to refine_index, labelled ntotal, ntotal + 1, ... in both.  RuntimeError when the two do
        not hold the same number of rows beforehand (rows reached one of them behind this object's back)."""
        nb, nr = self.base_index.ntotal, self.refine_index.ntotal
        if nb != nr:
            raise RuntimeError(f"add: the base holds {nb} rows, refine_index {nr}: labels and rows no longer agree")
        _staging.check_rows(x, self.d, "add")
        self.base_index.add(x)
        self.refine_index.add(x)

    def search(self, x, k, params=None):
        """(D, I) numpy arrays under the contract of FlatIPIndex.search.  params = IndexRefineSearchParameters(k_factor=...,
        base_index_params=...) overrides k_factor and hands the base its own parameters for this call; a selector raises ValueError."""
        params = typed_params(params, IndexRefineSearchParameters, "RefineFlatIndex")
        if params is None:
            return search_numpy(self, x, k)
        return search_numpy(self, x, k, k_factor=params.k_factor, base_index_params=params.base_index_params)

    def search_device(self, x, k, k_factor=None, base_index_params=None):
        """Device-resident search: CUDA tensors, no host synchronisation of its own (the base may have one; x is staged once).
        ValueError when int(k * k_factor) exceeds IVR_MAX_K; a base with a lower limit of its own raises its own error."""
        kw = _base_kwargs(self.base_index, base_index_params)
        t, staged = _staging.queries_f32(_staging.as_rows(x), self.d, self.device)
        _staging.check_nq(t.shape[0])
        k = _staging.check_k(k, _ffi.IVR_MAX_K)
        kf = self._k_factor if k_factor is None else _check_k_factor(k_factor, "search")
        k_base = int(k * kf)
        if k_base > _ffi.IVR_MAX_K:
            raise ValueError(f"search: k * k_factor = {k_base} outside [1,{_ffi.IVR_MAX_K}]")
        with torch.cuda.device(self.device):
            I_base = self.base_index.search_device(t, k_base, **kw)[1]
            D, I = self.refine_index.rescore_device(t, I_base.contiguous(), k)
            _staging.sync_if_staged(staged)
        return D, I

    def reconstruct(self, i):
        return self.refine_index.reconstruct(i)

    def reconstruct_n(self, start=0, n=None):
        return self.refine_index.reconstruct_n(start, n)

    def reconstruct_batch(self, keys):
        return self.refine_index.reconstruct_batch(keys)

    def reset(self):
        """Drop the rows of both indexes; what the base was trained to stays."""
        self.base_index.reset()
        self.refine_index.reset()

    def close(self):
        """Release refine_index; the base belongs to the caller."""
        x = getattr(self, "refine_index", None)
        if x is not None:
            x.close()


def IndexRefineFlat(base_index):
    """faiss.IndexRefineFlat(base_index) drop-in: base_index is an EMPTY IndexLSH, PQIndex, SQIndex, IVFFlatIndex, IVFPQIndex, IVFSQIndex, GraphFlatIndex or plain
    FlatIPIndex
    (ValueError otherwise)."""
    return RefineFlatIndex(base_index)
