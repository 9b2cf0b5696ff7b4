"""FAISS-shaped 4-bit product-quantisation index (IndexPQFastScan, inner product) resident in MI355X HBM.

The reference's `_create_index` (`core.py:1198-1230`) never builds an `IndexPQFastScan`; it is here as the compressed base for
`IndexRefineFlat` whose lookups do not gather: a row is stored as `M` nibbles (`M / 2` bytes), nibble `m` naming one of the 16
centroids of the codebook of slice `m` (coordinates `m * dsub .. (m + 1) * dsub`, `dsub = d / M`).  A 16-entry table of 8-bit values
is 16 bytes: the scan reads it from a wave-uniform address into scalar registers and looks four rows up with two `v_perm_b32` and a
`v_bfi_b32`, where `PQIndex` gathers 4 bytes per lane from a 1 KiB table row in LDS.  The price is a second quantisation, of the
tables to 8 bits, whose error `pqfs_score_bound` states.  The encoder, the table builder and quantiser and the scan are HIP kernels of
libivr_hip.so (csrc/search_pqfs.hip); torch stages arrays, orders the rows of a k-means step, splits nibbles and gathers codebook rows
for `sa_decode`.  The k-means around the encoder's assignment (sample, segment means, repair of empty clusters) is `_kmeans.py`'s.

What the kernels are pinned to is stated by the numpy functions below: `pqfs_encode_ref` and `pqfs_tables_ref` (float64 references
with the tolerances in their docstrings), `pqfs_quantize_ref` and `pqfs_scan_ref` (to the bit), `pqfs_pack_ref` / `pqfs_unpack_ref`
(the byte form of a code).

faiss's own k-means draws from a random stream that cannot be reproduced here, so training is defined by `train` (_pqbase.py); a codebook
exported from a real faiss index can be assigned to `centroids` while the index is empty.
"""
import numpy as np
import torch

from . import _ffi, _pqbase, _staging
from ._coded import _CodeStore
from ._faiss import FLT_MAX, METRIC_INNER_PRODUCT, require_inner_product
from ._staging import dev_f32 as _dev_f32, dev_u8 as _dev_u8

KSUB = 16                     # centroids per slice: nbits = 4
_F = np.float32


# -- pure numpy definitions (no GPU) -------------------------------------------------------------------------------------------
def _codebooks(centroids):
    c = np.asarray(centroids)
    if c.ndim != 3 or c.shape[1] != KSUB or c.shape[0] % 2:
        raise ValueError(f"centroids must be [M,{KSUB},dsub] with M even, got {c.shape}")
    return c


def pqfs_pack_ref(codes):
    """The byte form of codes [n,M] (values 0..15, M even) -> uint8 [n,M/2]: byte j = codes[:,2j] | codes[:,2j+1] << 4, faiss's
    4-bit packing.  This is what sa_encode returns, `codes` holds and add stores."""
    c = np.asarray(codes)
    if c.ndim != 2 or c.shape[1] % 2 or (c.size and (c.min() < 0 or c.max() >= KSUB)):
        raise ValueError(f"pqfs_pack_ref: codes must be [n,M] with M even and values in [0,{KSUB}), got {c.shape}")
    c = c.astype(np.uint8)
    return (c[:, 0::2] | (c[:, 1::2] << 4)).astype(np.uint8)


def pqfs_unpack_ref(packed):
    """The inverse of pqfs_pack_ref: uint8 [n,M/2] -> uint8 [n,M]."""
    p = np.asarray(packed)
    if p.ndim != 2 or p.dtype != np.uint8:
        raise ValueError(f"pqfs_unpack_ref: packed codes must be uint8 [n,M/2], got {p.dtype} {p.shape}")
    out = np.empty((p.shape[0], 2 * p.shape[1]), np.uint8)
    out[:, 0::2] = p & 15
    out[:, 1::2] = p >> 4
    return out


def pqfs_encode_ref(x, centroids):
    """The encoder's definition in float64: x [n,d], centroids [M,16,dsub] with M * dsub = d -> (codes uint8 [n,M] (unpacked),
    dist float64 [n,M,16]).  dist[i,m,j] = sum_t (x[i, m*dsub + t] - centroids[m,j,t])^2 and codes[i,m] is the j of the smallest
    one, the LOWER j on equal distances.

    The kernel evaluates the distances in float32, so a code j of it is correct when
        dist[i,m,j] <= min_j' dist[i,m,j'] + 2 * (dsub + 3) * 2^-23 * (|x_m|^2 + max_j |centroids[m,j]|^2):
    the first-order float32 rounding bound of sum (x - c)^2, doubled because two distances are compared.  Two centroids with
    identical bits always resolve to the lower j."""
    return _pqbase.encode_ref("pqfs_encode_ref", x, _codebooks(centroids))


def pqfs_tables_ref(q, centroids):
    """The float tables in float64: T[i,m,j] = <slice m of q[i], centroids[m,j]>, [nq,M,16].  The kernel's float32 entry
    (accumulated from zero in ascending coordinate order) lies within (dsub + 2) * 2^-24 * sum_t |q_t * c_t| of it."""
    return _pqbase.tables_ref("pqfs_tables_ref", q, _codebooks(centroids))


def _tables(T):
    T = np.asarray(T, _F)
    if T.ndim != 3 or T.shape[2] != KSUB or T.shape[1] < 1:
        raise ValueError(f"T must be float32 [nq,M,{KSUB}], got {T.shape}")
    return T


def pqfs_quantize_ref(T):
    """The 8-bit tables, to the bit: T float32 [nq,M,16], finite -> (U uint8 [nq,M,16], scale float32 [nq], bias float32 [nq]).
    Every step is one individually rounded float32 operation, none fused:
        lo[m] = min_j T[m,j];  span = max_m (max_j T[m,j] - lo[m]);  a = 255 / span;
        U[m,j] = rint((T[m,j] - lo[m]) * a), ties to even, clamped to [0, 255];
        scale = span / 255;  bias = ((lo[0] + lo[1]) + lo[2]) + ... in ascending m.
    When span == 0 or 255 / span is not finite: a = 0, U = 0 and scale = 0.
    So T[m,j] ~ lo[m] + scale * U[m,j], and a row's score sum_m T[m,code_m] ~ scale * sum_m U[m,code_m] + bias."""
    T = _tables(T)
    lo = T.min(axis=2)
    rng = (T.max(axis=2) - lo).astype(_F)
    span = rng.max(axis=1)
    with np.errstate(divide="ignore", over="ignore"):
        a = (_F(255) / span).astype(_F)
    dead = (span == 0) | ~np.isfinite(a)
    a = np.where(dead, _F(0), a).astype(_F)
    scale = np.where(dead, _F(0), span / _F(255)).astype(_F)
    t = (T - lo[:, :, None]).astype(_F)
    U = np.clip(np.rint((t * a[:, None, None]).astype(_F)), 0, 255).astype(np.uint8)
    bias = lo[:, 0].copy()
    for m in range(1, T.shape[1]):
        bias = (bias + lo[:, m]).astype(_F)
    return U, scale, bias


def pqfs_scan_ref(U, scale, bias, codes, k):
    """The scan, to the bit: U uint8 [nq,M,16], scale and bias float32 [nq], codes uint8 [n,M/2] in the byte form of pqfs_pack_ref
    (what `codes` and sa_encode return) -> (D float32 [nq,k], I int64 [nq,k]).  With code[r,m] the nibbles of row r,
    acc[i,r] = sum_m U[i,m,code[r,m]] in exact integer arithmetic (at most 255 * M <= 65280).  Rows are ranked by (acc descending,
    row ascending): integers only.  D = float32(acc) * scale + bias: an exact conversion, then one float32 multiplication and one
    float32 addition.  Unused slots (k > n) hold (-FLT_MAX, -1)."""
    U = np.asarray(U)
    codes = np.asarray(codes)
    if U.ndim != 3 or U.shape[2] != KSUB or U.dtype != np.uint8 or codes.ndim != 2 or codes.dtype != np.uint8 \
            or 2 * codes.shape[1] != U.shape[1]:
        raise ValueError(f"pqfs_scan_ref: U {U.dtype} {U.shape} must be uint8 [nq,M,{KSUB}] and codes {codes.dtype} {codes.shape} uint8 [n,M/2]")
    nq, M, _ = U.shape
    n, k = len(codes), int(k)
    if k < 1:
        raise ValueError(f"pqfs_scan_ref: k={k} < 1")
    scale, bias = np.asarray(scale, _F).reshape(nq), np.asarray(bias, _F).reshape(nq)
    D = np.full((nq, k), -FLT_MAX, _F)
    I = np.full((nq, k), -1, np.int64)
    if n == 0:
        return D, I
    c = pqfs_unpack_ref(codes)
    acc = np.zeros((nq, n), np.int64)
    for m in range(M):
        acc += U[:, m, c[:, m]]
    kk = min(k, n)
    order = np.argsort(-acc, axis=1, kind="stable")[:, :kk]          # stable: equal acc, the lower row first
    top = np.take_along_axis(acc, order, axis=1)
    D[:, :kk] = (top.astype(_F) * scale[:, None]).astype(_F) + bias[:, None]
    I[:, :kk] = order
    return D, I


def pqfs_score_bound(T):
    """What the 8-bit tables cost: float64 [nq], a bound on |D - sum_m T[m,code_m]| for every code, where D is pqfs_scan_ref's score
    under pqfs_quantize_ref(T) and the sum is exact (float64) over the float32 tables T [nq,M,16].  Derived, with u = 2^-24 the unit
    roundoff, lo and span those of pqfs_quantize_ref and L = sum_m |lo[m]|:
        bound = M * span / 510  +  u * (7 * M * span + (M + 1) * L).
    Per sub-quantizer, t = T[m,j] - lo[m] in [0, span] is rounded once, multiplied by a = fl(255 / span) (two more roundings) and
    rounded to the integer U, off by at most 0.5; times scale = fl(span / 255) (one rounding) that is
        |scale * U - t| <= span / 510 * (1 + u) + 4.01 * u * span,
    the first term being the quantisation step, the only one that is not a float32 rounding.  acc = sum_m U is exact and so is its
    conversion (acc < 2^24).  The product float32(acc) * scale <= M * span * (1 + 2 u) is rounded once (u * M * span), the last
    addition once (u * (M * span + L) to first order), and bias, M - 1 additions in sequence, lies within (M - 1) * u * L of
    sum_m lo[m].  The roundings add up to (6.01 * M * span + M * L) * u and a second-order rest; 7 and M + 1 cover both.
    Where pqfs_quantize_ref gives up (span == 0 or 255 / span not finite: scale = 0, D = bias) the first term is M * span, the whole
    of what the tables vary by."""
    T = _tables(T).astype(np.float64)
    M = T.shape[1]
    lo = T.min(axis=2)
    span = (T.max(axis=2) - lo).max(axis=1)
    scale = pqfs_quantize_ref(T.astype(_F))[1]
    step = np.where(scale == 0, M * span, M * span / 510.0)
    return step + 2.0 ** -24 * (7.0 * M * span + (M + 1) * np.abs(lo).sum(axis=1))


class PQFastScanIndex(_pqbase.ProductQuantizerIndex):
    """4-bit product-quantisation index (FAISS IndexPQFastScan contract, METRIC_INNER_PRODUCT, nbits = 4) on one GPU.

    search(x, k) returns (D float32, I int64): the score pqfs_scan_ref defines under the query's 8-bit tables, descending by its
    integer part, equal integers the lower row first (rows with the same code always tie), unused slots (-FLT_MAX, -1).  add() and
    search() raise RuntimeError until train() has run or `centroids` (numpy float32 [M,16,dsub]) has been assigned.  train(x) needs
    n >= 16 rows; the codebook state, train, sa_decode_device, search_tables and search_device are ProductQuantizerIndex's
    (_pqbase.py)."""
    _KSUB, _ENCODE = KSUB, "ivr_pqfs_encode"

    def __init__(self, d, M, nbits=4, metric=METRIC_INNER_PRODUCT, device=None):
        self.d, self.M = int(d), int(M)
        if int(nbits) != 4:
            raise ValueError(f"PQFastScanIndex: only nbits=4 is supported, got {nbits}")
        require_inner_product(metric, "PQFastScanIndex")
        if self.M < 2 or self.M > _ffi.IVR_PQFS_MAX_M or self.M % 2:
            raise ValueError(f"PQFastScanIndex: M={self.M} odd or outside [2,{_ffi.IVR_PQFS_MAX_M}] "
                             "(255 * M must fit the 16-bit accumulator)")
        self.ksub = KSUB
        self._setup("PQFastScanIndex", self.d, 4, self.M // 2,
                    lambda: _CodeStore("ivr_pqfs_index", (self.M,), self.M // 2, "PQFastScanIndex", device))

    @staticmethod
    def _slice_codes(packed):
        """packed uint8 CUDA [n,M/2] -> int64 CUDA [n,M]: pqfs_unpack_ref."""
        return torch.stack((packed & 15, packed >> 4), dim=2).reshape(packed.shape[0], -1).to(torch.int64)

    # -- FAISS surface ---------------------------------------------------------------------------
    def add_codes(self, codes):
        """Append rows by their codes: uint8 [n,M/2] as sa_encode returns them (faiss's add_sa_codes)."""
        self._require_trained("add")
        self._index._add_device(_dev_u8(codes, self.code_size, self.device, "add_codes"))

    def _tables_out(self, nq):
        return (torch.empty((nq, self.M, KSUB), dtype=torch.uint8, device=self.device),
                torch.empty(nq, dtype=torch.float32, device=self.device), torch.empty(nq, dtype=torch.float32, device=self.device))

    def compute_tables_device(self, x, float_tables=False):
        """The 8-bit tables of the queries x [nq,d]: (U uint8 CUDA [nq,M,16], scale float32 CUDA [nq], bias float32 CUDA [nq]),
        pqfs_quantize_ref of the kernel's float tables.  float_tables=True returns those too, first: (T float32 CUDA [nq,M,16], U,
        scale, bias); pqfs_tables_ref states T's tolerance."""
        self._require_trained("compute_tables")
        t, staged = _staging.queries_f32(_staging.as_rows(x), self.d, self.device)
        nq = t.shape[0]
        _staging.check_nq(nq, "compute_tables")
        T = torch.empty((nq, self.M, KSUB), dtype=torch.float32, device=self.device) if float_tables else None
        U, scale, bias = self._tables_out(nq)
        _ffi.call("ivr_pqfs_tables", _ffi.CTX, t, nq, self.d, self._codebooks_device(), self.M, T, U, scale, bias, device=self.device)
        _staging.sync_if_staged(staged, self.device)
        return (T, U, scale, bias) if float_tables else (U, scale, bias)

    def compute_tables(self, x, float_tables=False):
        """compute_tables_device as numpy arrays."""
        return tuple(a.cpu().numpy() for a in self.compute_tables_device(x, float_tables))

    def quantize_tables_device(self, T):
        """The quantiser alone on float tables T float32 [nq,M,16] (finite): (U, scale, bias) CUDA tensors, pqfs_quantize_ref(T) to
        the bit."""
        t = _dev_f32(T, self.device)
        if t.dim() != 3 or tuple(t.shape[1:]) != (self.M, KSUB):
            raise ValueError(f"quantize_tables expects [nq,{self.M},{KSUB}], got {tuple(t.shape)}")
        nq = t.shape[0]
        _staging.check_nq(nq, "quantize_tables")
        U, scale, bias = self._tables_out(nq)
        _ffi.call("ivr_pqfs_quantize", _ffi.CTX, t, nq, self.M, U, scale, bias, device=self.device)
        _staging.sync_if_staged(_staging.is_staged(t, T), self.device)
        return U, scale, bias

    def search_tables_device(self, U, scale, bias, k):
        """The scan on caller-supplied 8-bit tables (U uint8 [nq,M,16], scale and bias float32 [nq]): (D, I) CUDA tensors,
        pqfs_scan_ref(U, scale, bias, codes, k) to the bit."""
        self._require_trained("search")
        if isinstance(U, np.ndarray):
            U = torch.from_numpy(np.ascontiguousarray(U))
        if not isinstance(U, torch.Tensor) or U.dtype != torch.uint8 or U.dim() != 3 or tuple(U.shape[1:]) != (self.M, KSUB):
            raise ValueError(f"search_tables expects U uint8 [nq,{self.M},{KSUB}], got {getattr(U, 'dtype', type(U).__name__)} "
                             f"{tuple(getattr(U, 'shape', ()))}")
        ud = U.to(device=self.device).contiguous()
        nq = ud.shape[0]
        _staging.check_nq(nq)
        sd, bd = _dev_f32(scale, self.device).reshape(-1), _dev_f32(bias, self.device).reshape(-1)
        if sd.shape[0] != nq or bd.shape[0] != nq:
            raise ValueError(f"search_tables expects scale and bias [{nq}], got {tuple(sd.shape)} and {tuple(bd.shape)}")
        k = _staging.check_k(k, _ffi.IVR_MAX_K)
        D, I = _staging.alloc_DI(nq, k, self.device)
        self._index._call("ivr_pqfs_index_search", ud, sd, bd, nq, k, D, I)
        staged = _staging.is_staged(ud, U) or _staging.is_staged(sd, scale) or _staging.is_staged(bd, bias)
        _staging.sync_if_staged(staged, self.device)
        return D, I


def IndexPQFastScan(d, M, nbits=4, metric=METRIC_INNER_PRODUCT):
    """faiss.IndexPQFastScan(d, M, 4, faiss.METRIC_INNER_PRODUCT) drop-in.  ValueError when M is odd, outside [2, 256] or does not
    divide d, for nbits other than 4 and for a metric other than inner product (faiss's own default, METRIC_L2, must be replaced
    explicitly)."""
    return PQFastScanIndex(d, M, nbits, metric)
