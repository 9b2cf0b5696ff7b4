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

faiss's own k-means draws from a random stream that cannot be reproduced here, so training is defined by `train` below; a codebook
exported from a real faiss index can be assigned to `centroids` while the index is empty and then reproduces that index's codes up
to the rounding stated in `pq_encode_ref`.
"""
import numpy as np
import torch

from . import _ffi, _kmeans, _staging
from ._coded import DecodableIndex
from ._faiss import FLT_MAX, METRIC_INNER_PRODUCT, require_inner_product
from ._staging import dev_f32 as _dev_f32, dev_u8 as _dev_u8
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
    c = _codebooks(centroids).astype(np.float64)
    M, _, dsub = c.shape
    x = np.asarray(x, np.float64)
    if x.ndim != 2 or x.shape[1] != M * dsub:
        raise ValueError(f"pq_encode_ref: x must be [n,{M * dsub}], got {x.shape}")
    xs = x.reshape(len(x), M, 1, dsub)
    dist = ((xs - c[None]) ** 2).sum(-1)
    return dist.argmin(-1).astype(np.uint8), dist


def pq_tables_ref(q, centroids):
    """The lookup tables in float64: T[i,m,j] = <slice m of q[i], centroids[m,j]>, [nq,M,256].  The kernel's float32 entry lies
    within (dsub + 2) * 2^-24 * sum_t |q_t * c_t| of it."""
    c = _codebooks(centroids).astype(np.float64)
    M, _, dsub = c.shape
    q = np.asarray(q, np.float64)
    if q.ndim != 2 or q.shape[1] != M * dsub:
        raise ValueError(f"pq_tables_ref: q must be [nq,{M * dsub}], got {q.shape}")
    return np.einsum("imt,mjt->imj", q.reshape(len(q), M, dsub), c)


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


class PQIndex(DecodableIndex):
    """Product-quantisation index (FAISS IndexPQ contract, METRIC_INNER_PRODUCT, nbits = 8) on one GPU.

    search(x, k) returns (D float32, I int64): the asymmetric score pq_scan_ref defines, descending, equal scores the lower row
    first (quantised scores tie in bulk: rows with the same code always do), unused slots (-FLT_MAX, -1).  add() and search() raise
    RuntimeError until train() has run or `centroids` has been assigned."""

    def __init__(self, d, M, nbits=8, metric=METRIC_INNER_PRODUCT, device=None):
        self.d, self.M = int(d), int(M)
        if int(nbits) != 8:
            raise ValueError(f"PQIndex: only nbits=8 is supported, got {nbits}")
        require_inner_product(metric, "PQIndex")
        if self.M < 1 or self.M > _ffi.IVR_PQ_MAX_M:
            raise ValueError(f"PQIndex: M={M} outside [1,{_ffi.IVR_PQ_MAX_M}]")
        if self.d < 1 or self.d > 65536 or self.d % self.M != 0:
            raise ValueError(f"PQIndex: d={d} outside [1,65536] or not a multiple of M={self.M}")
        self.dsub = self.d // self.M
        self.code_size = self.M
        self.nbits = 8
        self.metric_type = METRIC_INNER_PRODUCT
        self.is_trained = False
        self._index = BinaryFlatIndex(8 * self.M, device=device)
        self.device = self._index.device
        self._centroids = np.zeros((self.M, KSUB, self.dsub), np.float32)
        self._cb_dev = None

    # -- attributes ------------------------------------------------------------------------------
    @property
    def centroids(self):
        """numpy float32 [M,256,dsub]: the codebooks.  Assignable while the index is empty, which makes it trained."""
        return self._centroids

    @centroids.setter
    def centroids(self, c):
        self._require_empty("centroids", "codebooks")
        c = np.asarray(c)
        if c.shape != self._centroids.shape:
            raise ValueError(f"centroids expects [{self.M},{KSUB},{self.dsub}], got {c.shape}")
        self._set_centroids(np.ascontiguousarray(c, dtype=np.float32))

    def _set_centroids(self, c, dev=None):
        self._centroids, self._cb_dev = c, dev
        self.is_trained = True

    def _codebooks_device(self):
        if self._cb_dev is None:
            self._cb_dev = torch.from_numpy(self._centroids).to(self.device)
        return self._cb_dev

    # -- encoding --------------------------------------------------------------------------------
    def _encode_device(self, t, cb=None):
        """t: contiguous float32 CUDA tensor [n,d] -> codes uint8 CUDA [n,M] under the codebooks cb (default: the index's)."""
        codes = torch.empty((t.shape[0], self.M), dtype=torch.uint8, device=self.device)
        _ffi.call("ivr_pq_encode", _ffi.CTX, t, t.shape[0], self.d, self._codebooks_device() if cb is None else cb, self.M, codes,
                  device=self.device)
        return codes

    def sa_decode_device(self, codes):
        """float32 CUDA [n,d]: row i is the concatenation of centroids[m, codes[i,m]] over m (a gather, no arithmetic)."""
        self._require_trained("sa_decode")
        c = _dev_u8(codes, self.M, self.device, "sa_decode").to(torch.int64)
        m = torch.arange(self.M, device=self.device).expand(c.shape[0], -1)
        return self._codebooks_device()[m, c].reshape(c.shape[0], self.d)

    # -- training --------------------------------------------------------------------------------
    def train(self, x, niter=25, seed=1234, max_points_per_centroid=256):
        """Make the M codebooks by k-means on x [n,d], n >= 256 (ValueError otherwise):
          sample   _kmeans.kmeans_sample(n, 256, max_points_per_centroid, seed): one sample serves all slices, and the initial codebook of
                   slice m is slice m of its first 256 rows
          iterate  niter times: assign every sampled row's slices with the encoder (ivr_pq_encode: equal distances pick the lower
                   centroid), order the rows of each slice by code (stable), take the mean of every run (ivr_segment_mean with
                   spherical=False: fixed summation order, so a seed gives the same bits every time), repair empty clusters
                   (split_empty_clusters, per slice).  The loop's shared halves are those of _kmeans.py."""
        self._require_empty("train", "codebooks")
        _staging.check_rows(x, self.d, "train")
        n = len(x)
        if n < KSUB:
            raise ValueError(f"train: {n} training rows for {KSUB} centroids per slice")
        niter = _kmeans.check_niter(niter)
        with torch.cuda.device(self.device):
            xs = _kmeans.sample_rows(x, KSUB, max_points_per_centroid, seed, self.device)
            cent = xs[:KSUB].reshape(KSUB, self.M, self.dsub).permute(1, 0, 2).contiguous()
            for _ in range(niter):
                cent = self._kmeans_step(xs, cent)
            self._set_centroids(cent.cpu().numpy(), cent)

    def _kmeans_step(self, xs, cent):
        a = self._encode_device(xs, cent).t().contiguous().to(torch.int64)        # [M, ns]
        order = torch.argsort(a, dim=1, stable=True)        # one batched sort for all slices
        out = torch.empty_like(cent)
        counts = [_kmeans.segment_means(xs[:, m * self.dsub:(m + 1) * self.dsub], a[m], KSUB, out[m], order=order[m]) for m in range(self.M)]
        return _kmeans.repair_empty_clusters(out, torch.stack(counts).cpu().numpy())

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

    def search_tables(self, T, k):
        """search_tables_device as numpy arrays."""
        D, I = self.search_tables_device(T, k)
        return D.cpu().numpy(), I.cpu().numpy()

    def search_device(self, x, k):
        """search returning CUDA tensors: search_tables_device(compute_tables_device(x), k), bit for bit."""
        self._require_trained("search")
        k = _staging.check_k(k, _ffi.IVR_MAX_K)
        return self.search_tables_device(self.compute_tables_device(x), k)


def IndexPQ(d, M, nbits=8, metric=METRIC_INNER_PRODUCT):
    """faiss.IndexPQ(d, M, nbits, faiss.METRIC_INNER_PRODUCT) drop-in.  ValueError when M does not divide d or exceeds 128, for
    nbits other than 8 and for a metric other than inner product (faiss's own default, METRIC_L2, must be replaced explicitly)."""
    return PQIndex(d, M, nbits, metric)
