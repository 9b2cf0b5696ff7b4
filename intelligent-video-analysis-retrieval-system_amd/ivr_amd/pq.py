"""FAISS-shaped product-quantisation index (IndexPQ, inner product, 8-bit codes) resident in MI355X HBM.

The reference's `_create_index` (`core.py:1198-1230`) never builds an `IndexPQ`; it is here as the compressed base for
`IndexRefineFlat`: a row is stored as `M` bytes (32x smaller than float32 at `M = d / 8`), byte `m` naming one of the 256 centroids
of the codebook of slice `m` (coordinates `m * dsub .. (m + 1) * dsub`, `dsub = d / M`), and a search ranks the rows by a sum of `M`
table lookups: the asymmetric (query-to-code) inner product.  The encoder, the table builder and the scan are HIP kernels of
libivr_hip.so (csrc/search_pq.hip); the codes live in a `BinaryFlatIndex` of `8 * M` bits, as those of `IndexLSH` do; torch stages
arrays, orders the rows of a k-means step and gathers codebook rows for `sa_decode`.  The k-means around the encoder's assignment (sample,
segment means, repair of empty clusters) is `_kmeans.py`'s, shared with the coarse quantizer of the inverted-file indexes.

What the kernels are pinned to is stated by the numpy functions below: `pq_encode_ref`, `pq_tables_ref` (float64 references with the
tolerances in their docstrings) and `pq_scan_ref` (the float32 additions of the scan, which numpy reproduces to the bit).

faiss's own k-means draws from a random stream that cannot be reproduced here, so training is defined by `train` (_pqbase.py); a codebook
exported from a real faiss index can be assigned to `centroids` while the index is empty and then reproduces that index's codes up
to the rounding stated in `pq_encode_ref`.
"""
import numpy as np
import torch

from . import _ffi, _pqbase, _staging
from ._faiss import FLT_MAX, METRIC_INNER_PRODUCT, require_inner_product
from ._staging import dev_f32 as _dev_f32
from .binary import BinaryFlatIndex

KSUB = 256                    # centroids per slice: nbits = 8


# -- pure numpy definitions (no GPU) -------------------------------------------------------------------------------------------
def _codebooks(centroids):
    c = np.asarray(centroids)
    if c.ndim != 3 or c.shape[1] != KSUB:
        raise ValueError(f"centroids must be [M,{KSUB},dsub], got {c.shape}")
    return c


def pq_encode_ref(x, centroids):
    """The encoder's definition in float64: x [n,d], centroids [M,256,dsub] with M * dsub = d -> (codes uint8 [n,M], dist float64
    [n,M,256]).  dist[i,m,j] = sum_t (x[i, m*dsub + t] - centroids[m,j,t])^2 and codes[i,m] is the j of the smallest one, the LOWER j
    on equal distances.

    The kernel evaluates the distances in float32, so a code j of it is correct when
        dist[i,m,j] <= min_j' dist[i,m,j'] + 2 * (dsub + 3) * 2^-23 * (|x_m|^2 + max_j |centroids[m,j]|^2):
    the first-order float32 rounding bound of sum (x - c)^2 and of |c|^2 - 2 <x, c> alike, doubled because two distances are
    compared.  Two centroids with identical bits always resolve to the lower j."""
    return _pqbase.encode_ref("pq_encode_ref", x, _codebooks(centroids))


def pq_tables_ref(q, centroids):
    """The lookup tables in float64: T[i,m,j] = <slice m of q[i], centroids[m,j]>, [nq,M,256].  The kernel's float32 entry lies
    within (dsub + 2) * 2^-24 * sum_t |q_t * c_t| of it."""
    return _pqbase.tables_ref("pq_tables_ref", q, _codebooks(centroids))


def pq_scan_ref(T, codes, k):
    """The scan, to the bit: T float32 [nq,M,256], codes uint8 [n,M] -> (D float32 [nq,k], I int64 [nq,k]).  The score of row r for
    query i is (((T[i,0,codes[r,0]] + T[i,1,codes[r,1]]) + T[i,2,codes[r,2]]) + ...): plain float32 additions in ascending m.  (D, I)
    is the ordering of refine_order_ref over all rows: score descending, -0.0 counted and reported as +0.0, equal scores the lower
    row first, unused slots (k > n) hold (-FLT_MAX, -1).  The tables must be finite."""
    from .refine import refine_order_ref
    T = np.asarray(T, np.float32)
    codes = np.asarray(codes)
    if T.ndim != 3 or T.shape[2] != KSUB or codes.ndim != 2 or codes.shape[1] != T.shape[1] or codes.dtype != np.uint8:
        raise ValueError(f"pq_scan_ref: T {T.shape} must be [nq,M,{KSUB}] and codes {codes.shape} uint8 [n,M]")
    nq, M, _ = T.shape
    n, k = len(codes), int(k)
    if k < 1:
        raise ValueError(f"pq_scan_ref: k={k} < 1")
    D = np.full((nq, k), -FLT_MAX, np.float32)
    I = np.full((nq, k), -1, np.int64)
    if n == 0:
        return D, I
    S = T[:, 0, codes[:, 0]].copy()
    for m in range(1, M):
        S = S + T[:, m, codes[:, m]]          # float32 + float32, rounded once: the kernel's addition
    kk = min(k, n)
    D[:, :kk], I[:, :kk] = refine_order_ref(S, np.broadcast_to(np.arange(n, dtype=np.int64), (nq, n)), kk)
    return D, I


class PQIndex(_pqbase.ProductQuantizerIndex):
    """Product-quantisation index (FAISS IndexPQ contract, METRIC_INNER_PRODUCT, nbits = 8) on one GPU.

    search(x, k) returns (D float32, I int64): the asymmetric score pq_scan_ref defines, descending, equal scores the lower row
    first (quantised scores tie in bulk: rows with the same code always do), unused slots (-FLT_MAX, -1).  add() and search() raise
    RuntimeError until train() has run or `centroids` (numpy float32 [M,256,dsub]) has been assigned.  train(x) needs n >= 256 rows; the
    codebook state, train, sa_decode_device, search_tables and search_device are ProductQuantizerIndex's (_pqbase.py)."""
    _KSUB, _ENCODE = KSUB, "ivr_pq_encode"

    def __init__(self, d, M, nbits=8, metric=METRIC_INNER_PRODUCT, device=None):
        self.d, self.M = int(d), int(M)
        if int(nbits) != 8:
            raise ValueError(f"PQIndex: only nbits=8 is supported, got {nbits}")
        require_inner_product(metric, "PQIndex")
        if self.M < 1 or self.M > _ffi.IVR_PQ_MAX_M:
            raise ValueError(f"PQIndex: M={M} outside [1,{_ffi.IVR_PQ_MAX_M}]")
        self._setup("PQIndex", d, 8, self.M, lambda: BinaryFlatIndex(8 * self.M, device=device))

    @staticmethod
    def _slice_codes(codes):
        """codes uint8 CUDA [n,M] -> int64 CUDA [n,M]: a byte is the centroid of its slice."""
        return codes.to(torch.int64)

    # -- FAISS surface ---------------------------------------------------------------------------
    def compute_tables_device(self, x):
        """The lookup tables of the queries x [nq,d]: float32 CUDA [nq,M,256], T[i,m,j] = <slice m of x[i], centroids[m,j]>
        (pq_tables_ref states the tolerance)."""
        self._require_trained("compute_tables")
        t, staged = _staging.queries_f32(_staging.as_rows(x), self.d, self.device)
        nq = t.shape[0]
        _staging.check_nq(nq, "compute_tables")
        T = torch.empty((nq, self.M, KSUB), dtype=torch.float32, device=self.device)
        _ffi.call("ivr_pq_tables", _ffi.CTX, t, nq, self.d, self._codebooks_device(), self.M, T, device=self.device)
        _staging.sync_if_staged(staged, self.device)
        return T

    def compute_tables(self, x):
        """compute_tables_device as a numpy array."""
        return self.compute_tables_device(x).cpu().numpy()

    def search_tables_device(self, T, k):
        """The scan on caller-supplied tables T float32 [nq,M,256] (finite): (D, I) CUDA tensors, pq_scan_ref(T, codes, k) to the
        bit."""
        self._require_trained("search")
        t = _dev_f32(T, self.device)
        if t.dim() != 3 or tuple(t.shape[1:]) != (self.M, KSUB):
            raise ValueError(f"search_tables expects [nq,{self.M},{KSUB}], got {tuple(t.shape)}")
        k = _staging.check_k(k, _ffi.IVR_MAX_K)
        nq = t.shape[0]
        _staging.check_nq(nq)
        D, I = _staging.alloc_DI(nq, k, self.device)
        self._index._call("ivr_bin_index_search_pq", t, nq, self.M, k, D, I)
        _staging.sync_if_staged(_staging.is_staged(t, T), self.device)
        return D, I


def IndexPQ(d, M, nbits=8, metric=METRIC_INNER_PRODUCT):
    """faiss.IndexPQ(d, M, nbits, faiss.METRIC_INNER_PRODUCT) drop-in.  ValueError when M does not divide d or exceeds 128, for
    nbits other than 8 and for a metric other than inner product (faiss's own default, METRIC_L2, must be replaced explicitly)."""
    return PQIndex(d, M, nbits, metric)
