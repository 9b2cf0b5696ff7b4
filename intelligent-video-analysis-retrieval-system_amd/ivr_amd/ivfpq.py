"""FAISS-shaped inverted-file index over product-quantised codes (IndexIVFPQ, inner product, 8-bit codes) resident in MI355X HBM.

The reference's `_create_index` (`core.py:1198-1230`) never builds an `IndexIVFPQ`; it is here because it is the compressed index
faiss users deploy at scale, and the base `IndexRefineFlat` is usually paired with.  It joins the coarse side of `InvertedFileIndex`
(`_ivf.py`, shared with `IVFFlatIndex`: quantizer, k-means, offsets, probe step) with the codes of `PQIndex`: a row is stored in the
list of its best centroid as the `M`-byte code of its residual against that centroid (`by_residual`, the default, as in faiss) or of
the row itself, and a search scores only the rows of the `nprobe` lists whose centroids score best against the query.

With the inner product residual coding costs nothing at search time: `<q, c_l + r> = <q, c_l> + <q, r>`, so the `M x 256` lookup
table of a query (`PQIndex.compute_tables_device`, unchanged) serves every list, and the only per-list term is the coarse score the
coarse search has produced already.  `ivfpq_scan_ref` below states the scan to the bit; the list store, the probe table and the scan
are HIP kernels of libivr_hip.so (csrc/search_ivfpq.hip), the encoder and the table builder are those of `PQIndex`; torch stages
arrays, subtracts centroids and orders rows by list.

Tie rule: equal scores rank the row in the LOWER LIST first, and within a list the row ADDED EARLIER, as on `IVFFlatIndex`: a result
does not depend on the order in which lists were probed.
"""
import numpy as np
import torch

from . import _ffi, _staging
from ._faiss import FLT_MAX, METRIC_INNER_PRODUCT, require_inner_product
from ._ivf import CodedInvertedFileIndex, _check_off, check_quantizer, ivfpq_positions_ref
from ._staging import dev_f32 as _dev_f32
from .index import FlatIPIndex
from .pq import KSUB, PQIndex


# -- pure numpy definitions (no GPU) -------------------------------------------------------------------------------------------
def _words(M):
    """16-byte words per stored row: 1, 2, 3, 4 or 8 (the word counts of the binary store)."""
    w = (int(M) + 15) // 16
    return w if w <= 4 else 8


def ivfpq_pack_ref(codes, list_off):
    """The device layout of list-ordered codes: uint8 [n,M] -> uint8 [groups, W, 64, 16].  Every list is padded to whole 64-row
    groups; inside a group lane i holds row i of the group, and bytes 16 w .. 16 w + 15 of its code are word w (W = 1, 2, 3, 4 or 8
    words: M bytes rounded up).  Pad bytes and pad rows are zero."""
    codes = np.asarray(codes)
    if codes.ndim != 2 or codes.dtype != np.uint8:
        raise ValueError(f"ivfpq_pack_ref: codes must be uint8 [n,M], got {codes.dtype} {codes.shape}")
    n, M = codes.shape
    pos, goff = ivfpq_positions_ref(_check_off(list_off, n))
    W = _words(M)
    padded = np.zeros((int(goff[-1]) * 64, W * 16), np.uint8)
    padded[pos, :M] = codes
    return np.ascontiguousarray(padded.reshape(int(goff[-1]), 64, W, 16).transpose(0, 2, 1, 3))


def ivfpq_unpack_ref(packed, list_off, M):
    """The inverse of ivfpq_pack_ref: uint8 [groups, W, 64, 16] -> the list-ordered codes uint8 [n,M]."""
    packed = np.asarray(packed)
    M = int(M)
    if packed.ndim != 4 or packed.dtype != np.uint8 or packed.shape[1:] != (_words(M), 64, 16):
        raise ValueError(f"ivfpq_unpack_ref: packed must be uint8 [groups,{_words(M)},64,16], got {packed.dtype} {packed.shape}")
    off = np.asarray(list_off, np.int64).reshape(-1)
    pos, goff = ivfpq_positions_ref(_check_off(off, off[-1]))
    if goff[-1] != packed.shape[0]:
        raise ValueError(f"ivfpq_unpack_ref: list_off asks for {goff[-1]} groups, packed holds {packed.shape[0]}")
    rows = packed.transpose(0, 2, 1, 3).reshape(packed.shape[0] * 64, -1)
    return np.ascontiguousarray(rows[pos, :M])


def ivfpq_scan_ref(T, coarse, assign, list_off, codes, ids, k):
    """The search, to the bit.  T float32 [nq,M,256] (finite), coarse float32 [nq,p], assign int64 [nq,p], codes uint8 [n,M] in list
    order (list l = rows list_off[l] .. list_off[l + 1]), ids int64 [n] -> (D float32 [nq,k], I int64 [nq,k]).

    Query i probes the lists assign[i] names: -1 entries are skipped, and a list named twice counts once, with the coarse score of its
    first mention after an ascending STABLE sort of the row.  The score of row r of a list probed through entry j is
    ((coarse[i,j] + T[i,0,codes[r,0]]) + T[i,1,codes[r,1]]) + ...: plain float32 additions, coarse first, then ascending m (without
    by_residual the caller passes coarse = +0.0).  (D, I) is the ordering of refine_order_ref over the probed rows: score descending,
    -0.0 counted and reported as +0.0, equal scores the row in the lower list first and within a list the row added earlier; I holds
    ids[r].  Unused slots hold (-FLT_MAX, -1), as those of IVFFlatIndex.search do.  ValueError for an entry below -1 or >= nlist."""
    from .refine import refine_order_ref
    T = np.asarray(T, np.float32)
    codes = np.asarray(codes)
    assign = np.asarray(assign).astype(np.int64)
    coarse = np.asarray(coarse, np.float32)
    ids = np.asarray(ids, np.int64).reshape(-1)
    if T.ndim != 3 or T.shape[2] != KSUB or codes.ndim != 2 or codes.shape[1] != T.shape[1] or codes.dtype != np.uint8:
        raise ValueError(f"ivfpq_scan_ref: T {T.shape} must be [nq,M,{KSUB}] and codes {codes.shape} uint8 [n,M]")
    nq, M, _ = T.shape
    n, k = len(codes), int(k)
    off = _check_off(list_off, n)
    nlist = len(off) - 1
    if assign.ndim != 2 or assign.shape[0] != nq or assign.shape[1] < 1 or coarse.shape != assign.shape or len(ids) != n:
        raise ValueError(f"ivfpq_scan_ref: assign {assign.shape} and coarse {coarse.shape} must be [{nq},p], ids [{n}]")
    if assign.size and (assign.min() < -1 or assign.max() >= nlist):
        raise ValueError(f"ivfpq_scan_ref: assign entries must lie in [-1, {nlist})")
    if k < 1:
        raise ValueError(f"ivfpq_scan_ref: k={k} < 1")
    D = np.full((nq, k), -FLT_MAX, np.float32)
    I = np.full((nq, k), -1, np.int64)
    for i in range(nq):
        order = np.argsort(assign[i], kind="stable")
        a, c = assign[i, order], coarse[i, order]
        rows, base = [np.zeros(0, np.int64)], [np.zeros(0, np.float32)]
        for j, l in enumerate(a):
            if l < 0 or (j > 0 and a[j - 1] == l):
                continue
            rows.append(np.arange(off[l], off[l + 1], dtype=np.int64))
            base.append(np.full(off[l + 1] - off[l], c[j], np.float32))
        rows, S = np.concatenate(rows), np.concatenate(base)
        if len(rows) == 0:
            continue
        for m in range(M):
            S = S + T[i, m, codes[rows, m]]        # float32 + float32, rounded once: the kernel's addition
        kk = min(k, len(rows))
        Di, Ri = refine_order_ref(S[None], rows[None], kk)
        D[i, :kk], I[i, :kk] = Di[0], ids[Ri[0]]
    return D, I


class _CodebookPQ(PQIndex):
    """The PQIndex an IVFPQIndex holds for its codebooks, encoder, tables and decoder.  Its own row store stays empty; the rows its
    codebooks are bound to are the owner's, so that is what `centroids` and `train` ask about."""
    _owner = None

    def _require_empty(self, what, noun):
        n = self._owner.ntotal if self._owner is not None else 0
        if n:
            raise RuntimeError(f"{what}: the index holds {n} rows encoded with the current {noun}")


class IVFPQIndex(CodedInvertedFileIndex):
    """Inverted-file index over product-quantised codes (FAISS IndexIVFPQ contract, METRIC_INNER_PRODUCT, nbits = 8) on one GPU.

    search(x, k) looks at the rows of the nprobe lists nearest to each query and returns (D, I) as ivfpq_scan_ref defines them over
    the tables pq.compute_tables_device(x) and the quantizer's float32 scores of the probed centroids: float32 descending, int64
    labels, (-FLT_MAX, -1) padding.  Equal scores rank the row in the lower list first, and within a list the row added earlier.
    Every add() call regroups the whole index by list (one pass over all stored codes): add in large batches.  The store, the
    adding, the search surface and the reconstruction are CodedInvertedFileIndex's (_ivf.py)."""
    _PARTS = ("_lists", "pq", "quantizer")
    _ABI = "ivr_ivfpq"
    _NOUN = "codebooks"

    def __init__(self, d, nlist, M, device=None, _quantizer=None):
        self.pq = _CodebookPQ(d, M, device=device if _quantizer is None else _quantizer.device.index)
        super().__init__(d, nlist, self.pq, device, _quantizer)
        self.M = self.pq.M
        self.nbits = 8

    # -- training --------------------------------------------------------------------------------
    def train(self, x, niter=10, seed=1234, max_points_per_centroid=256, spherical=True):
        """Train the quantizer exactly as IVFFlatIndex.train does (same arguments; a quantizer that already holds nlist rows is taken
        as it is), form the training residuals x_i - centroids[assign(x_i)] (one float32 subtraction per coordinate; x itself without
        by_residual) and call pq.train on them with PQIndex.train's own defaults."""
        self._train(x, niter, seed, max_points_per_centroid, spherical)

    # -- search ----------------------------------------------------------------------------------
    def compute_tables_device(self, x):
        """pq.compute_tables_device(x): float32 CUDA [nq,M,256], the same for every list."""
        return self.pq.compute_tables_device(x)

    _query_form = compute_tables_device

    def search_tables_preassigned_device(self, T, coarse, assign, k):
        """The scan alone on caller-supplied tables: T float32 [nq,M,256] (finite), coarse float32 [nq,p] or None (+0.0), assign
        int64 [nq,p] -> (D, I) CUDA tensors, ivfpq_scan_ref(T, coarse, assign, list offsets, stored codes, stored ids, k) to the
        bit, whatever by_residual says."""
        self._require_trained("search")
        t = _dev_f32(T, self.device)
        if t.dim() != 3 or tuple(t.shape[1:]) != (self.M, KSUB):
            raise ValueError(f"search_tables_preassigned expects T [nq,{self.M},{KSUB}], got {tuple(t.shape)}")
        k = _staging.check_k(k, _ffi.IVR_MAX_K)
        _staging.check_nq(t.shape[0])
        with torch.cuda.device(self.device):
            assign = self._assign_arg(assign, t.shape[0], "search_tables_preassigned")
            out = self._scan(t, None if coarse is None else self._coarse_arg(coarse, assign, "search_tables_preassigned"), assign, k)
            _staging.sync_if_staged(True, self.device)       # T, coarse and assign may all be staged copies
            return out

    def _scan(self, T, coarse, assign, k):
        """assign: int64 CUDA [nq,p], entries in [-1, nlist).  The kernel wants every row ascending (a repeated list is then adjacent);
        the sort is stable, so the first mention of a list keeps its coarse score."""
        nq, p = assign.shape
        assign, coarse = self._ascending(assign, coarse, stable=True)
        D, I = _staging.alloc_DI(nq, k, self.device)
        self._lists._call("ivr_ivfpq_search", T, coarse, assign, nq, p, k, D, I)
        return D, I


def IndexIVFPQ(quantizer, d, nlist, M, nbits=8, metric=METRIC_INNER_PRODUCT):
    """faiss.IndexIVFPQ(quantizer, d, nlist, M, nbits, faiss.METRIC_INNER_PRODUCT) drop-in.  ValueError for nbits other than 8, for a
    metric other than inner product, for M outside [1, IVR_PQ_MAX_M] or not dividing d, and for a quantizer IndexIVFFlat refuses: it
    must be a plain (not id-mapped) FlatIPIndex of dimension d holding 0 rows (train() fills it) or exactly nlist rows."""
    if int(nbits) != 8:
        raise ValueError(f"IndexIVFPQ: only nbits=8 is supported, got {nbits}")
    require_inner_product(metric, "IndexIVFPQ")
    d, nlist, M = int(d), int(nlist), int(M)
    if M < 1 or M > _ffi.IVR_PQ_MAX_M:
        raise ValueError(f"IndexIVFPQ: M={M} outside [1,{_ffi.IVR_PQ_MAX_M}]")
    if d < 1 or d > 65536 or d % M != 0:
        raise ValueError(f"IndexIVFPQ: d={d} outside [1,65536] or not a multiple of M={M}")
    if nlist < 1:
        raise ValueError(f"IndexIVFPQ: nlist={nlist} < 1")
    if not isinstance(quantizer, FlatIPIndex):
        raise ValueError(f"IndexIVFPQ: the quantizer must be a FlatIPIndex, got {type(quantizer).__name__}")
    check_quantizer(quantizer, d, nlist, "IndexIVFPQ")
    return IVFPQIndex(d, nlist, M, _quantizer=quantizer)
