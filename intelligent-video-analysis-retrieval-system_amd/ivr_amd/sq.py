"""FAISS-shaped scalar-quantiser index (IndexScalarQuantizer, QT_8bit, inner product) resident in MI355X HBM.

The reference's `_create_index` (`core.py:1198-1230`) never builds an `IndexScalarQuantizer`; it is here as the compressed base
between the flat index and the 32 - 64 byte codes of `IndexLSH` / `PQIndex`: a row is stored as `d` bytes (4x smaller than float32),
byte `j` naming one of 256 buckets between `vmin[j]` and `vmin[j] + vdiff[j]`, and a search ranks the rows by an exact integer inner
product of the stored bytes with a 15-bit integer form of the query.  The encoder, the query preparation and the scan are HIP
kernels of libivr_hip.so (csrc/search_sq.hip: the scan runs on v_mfma_i32_16x16x64_i8); torch stages arrays, reduces the training
rows to their range and gathers decoded values from a host-made table.

What the kernels are pinned to is stated by the numpy functions below, all of them to the bit except the float32 sum `bias`:
`sq_encode_ref`, `sq_decode_ref`, `sq_query_ref`, `sq_scan_ref`.  Every "float32" step in them is one individually rounded IEEE
operation, which numpy reproduces.

Training is faiss's RS_minmax with rs_arg = 0; a table exported from a real faiss index (`faiss.vector_to_array(index.sq.trained)`)
can be assigned to `trained` while the index is empty and then reproduces that index's codes.
"""
import numpy as np
import torch

from . import _ffi, _staging
from ._coded import DecodableIndex, _CodeStore
from ._faiss import FLT_MAX, METRIC_INNER_PRODUCT, require_inner_product
from ._staging import dev_f32 as _dev_f32, dev_u8 as _dev_u8

T_MAX = 16256                 # 127 * 128: the largest |t| of a prepared query
_F = np.float32


class ScalarQuantizer:
    """faiss.ScalarQuantizer's quantiser types by value; IndexScalarQuantizer accepts QT_8bit only."""
    QT_8bit, QT_4bit, QT_8bit_uniform, QT_4bit_uniform, QT_fp16, QT_8bit_direct, QT_6bit, QT_bf16, QT_8bit_direct_signed = range(9)


QT_8bit = ScalarQuantizer.QT_8bit


# -- pure numpy definitions (no GPU) -------------------------------------------------------------------------------------------
def _split(trained):
    tr = np.asarray(trained, _F)
    if tr.ndim != 1 or tr.size % 2:
        raise ValueError(f"trained must be float32 [2d] = [vmin | vdiff], got {tr.shape}")
    d = tr.size // 2
    return tr[:d], tr[d:]


def sq_train_ref(x):
    """faiss RS_minmax with rs_arg = 0: x [n,d] -> trained float32 [2d] = [vmin | vdiff], vmin[j] = min_i x[i,j] and vdiff[j] =
    max_i x[i,j] - vmin[j] (one float32 subtraction)."""
    x = np.asarray(x, _F)
    vmin = x.min(axis=0)
    with np.errstate(invalid="ignore"):      # inf - inf of rows the caller refuses afterwards
        return np.concatenate([vmin, x.max(axis=0) - vmin])


def sq_encode_ref(x, trained):
    """The encoder, to the bit (faiss's Codec8bit behind the non-uniform quantiser): x float32 [n,d] -> codes uint8 [n,d].
        xi = (x - vmin) / vdiff in float32 (one subtraction, one division), 0 where vdiff == 0;  xi clamped to [0, 1];
        code = min(255, int(255f * xi)), one float32 multiplication, truncated.
    x must be finite: what a NaN encodes to is unspecified (the kernel and this function need not agree on it)."""
    vmin, vdiff = _split(trained)
    x = np.asarray(x, _F)
    if x.ndim != 2 or x.shape[1] != vmin.size:
        raise ValueError(f"sq_encode_ref: x must be [n,{vmin.size}], got {x.shape}")
    with np.errstate(divide="ignore", invalid="ignore"):
        xi = np.where(vdiff == 0, _F(0), (x - vmin) / vdiff).astype(_F)
    xi = np.clip(xi, _F(0), _F(1))
    return np.minimum(255, (_F(255) * xi).astype(np.int32)).astype(np.uint8)


def sq_decode_ref(codes, trained):
    """The decoder, to the bit: codes uint8 [n,d] -> float32 [n,d], vmin + vdiff * ((code + 0.5f) / 255f) with every operation in
    float32 in this order: one addition and one division (they depend on the code alone), one multiplication, one addition."""
    vmin, vdiff = _split(trained)
    xi = (np.asarray(codes).astype(_F) + _F(0.5)) / _F(255)
    return (vmin + vdiff * xi).astype(_F)


def sq_tables_ref(trained):
    """The two float32 [d] tables of the query preparation: gain = vdiff / 255f and offset = vmin + vdiff * (128.5f / 255f) (the
    quotient of the constants first, then one multiplication and one addition).  decode(code) = offset + gain * (code - 128) up to
    float32 rounding."""
    vmin, vdiff = _split(trained)
    return (vdiff / _F(255)).astype(_F), (vmin + vdiff * (_F(128.5) / _F(255))).astype(_F)


def sq_query_ref(q, trained):
    """The integer form of the queries q float32 [nq,d] -> (t int16 [nq,d], scale float32 [nq], bias float64 [nq]).
        w = q * gain in float32;  m = max_j |w_j|;  scale = m / 16256f in float32, 1.0 when m == 0;
        t = clamp(rint(w / scale), -16256, 16256): a float32 division, rounding half to even;
        bias = sum_j q_j * offset_j.
    t and scale are the kernel's to the bit.  bias is returned in float64; the kernel's float32 sum lies within
    (d + 2) * 2^-24 * sum_j |q_j * offset_j| of it.  q must be finite."""
    gain, offset = sq_tables_ref(trained)
    q = np.asarray(q, _F)
    if q.ndim != 2 or q.shape[1] != gain.size:
        raise ValueError(f"sq_query_ref: q must be [nq,{gain.size}], got {q.shape}")
    w = (q * gain).astype(_F)
    m = np.abs(w).max(axis=1)
    scale = np.where(m == 0, _F(1), m / _F(T_MAX)).astype(_F)
    t = np.clip(np.rint(w / scale[:, None]), -T_MAX, T_MAX).astype(np.int16)
    bias = (q.astype(np.float64) * offset.astype(np.float64)).sum(axis=1)
    return t, scale, bias


def sq_split_ref(t):
    """The two int8 halves the scan multiplies: t = 128 h + l with l = ((t + 64) & 127) - 64 in [-64, 63] and h = (t - l) >> 7 in
    [-127, 127] for |t| <= 16256."""
    t = np.asarray(t).astype(np.int32)
    l = ((t + 64) & 127) - 64
    return ((t - l) >> 7).astype(np.int8), l.astype(np.int8)


def sq_scan_ref(t, scale, bias, codes, k):
    """The scan, to the bit: t int16 [nq,d] (|t| <= 16256), scale and bias float32 [nq], codes uint8 [n,d] -> (D float32 [nq,k],
    I int64 [nq,k]).  With c' = code - 128, acc[i,r] = sum_j t[i,j] * c'[r,j] in exact integer arithmetic (|acc| <= 16256 * 128 * d,
    2,130,706,432 at d = 1024: inside int32).  Rows are ranked by (acc descending, row ascending): integers only.
    D = float32(acc) * scale + bias: the conversion rounds to nearest-even, then one float32 multiplication and one float32
    addition.  Unused slots (k > n) hold (-FLT_MAX, -1).

    Against faiss's score <q, decode(code)> (decode in exact arithmetic from the float32 vmin and vdiff), with (t, scale, bias)
    prepared from q:
        |D - <q, decode(code)>| <= 0.5 * scale * sum_j |c'_j| * (1 + 2^-8)  +  (d + 8) * 2^-24 * sum_j |q_j| * (|vmin_j| + |vdiff_j|).
    The first term is the rounding of w_j / scale to the integer t_j (at most 0.5 + 16256 * 2^-24 each, and the three relative
    roundings of float32(acc) * scale + bias on the integer part); the second collects the float32 roundings: d + 2 units for the
    bias sum, 2 for the offset table, 1 for gain and w, 1.02 + 1.5 for the two roundings of the product and the last addition, each
    on a quantity that sum_j |q_j| (|vmin_j| + |vdiff_j|) bounds (sq_score_bound evaluates it)."""
    t = np.asarray(t)
    codes = np.asarray(codes)
    if t.ndim != 2 or codes.ndim != 2 or codes.shape[1] != t.shape[1] or codes.dtype != np.uint8 or t.dtype != np.int16:
        raise ValueError(f"sq_scan_ref: t {t.shape} {t.dtype} must be int16 [nq,d] and codes {codes.shape} {codes.dtype} uint8 [n,d]")
    if t.size and np.abs(t.astype(np.int32)).max() > T_MAX:
        raise ValueError(f"sq_scan_ref: |t| must not exceed {T_MAX}")
    nq, n, k = len(t), len(codes), int(k)
    if k < 1:
        raise ValueError(f"sq_scan_ref: k={k} < 1")
    scale, bias = np.asarray(scale, _F).reshape(nq), np.asarray(bias, _F).reshape(nq)
    D = np.full((nq, k), -FLT_MAX, _F)
    I = np.full((nq, k), -1, np.int64)
    if n == 0:
        return D, I
    # float64 holds every partial sum exactly (integers below 2^53)
    acc = (t.astype(np.float64) @ (codes.astype(np.float64) - 128.0).T).astype(np.int64)
    kk = min(k, n)
    order = np.argsort(-acc, axis=1, kind="stable")[:, :kk]          # stable: equal acc, the lower row first
    top = np.take_along_axis(acc, order, axis=1)
    D[:, :kk] = (top.astype(_F) * scale[:, None]).astype(_F) + bias[:, None]
    I[:, :kk] = order
    return D, I


def sq_score_bound(q, codes, trained, scale):
    """The bound of sq_scan_ref's docstring for every (query, row): float64 [nq,n]."""
    vmin, vdiff = _split(trained)
    d = vmin.size
    cabs = np.abs(np.asarray(codes).astype(np.float64) - 128.0).sum(axis=1)
    a = (np.abs(np.asarray(q, np.float64)) * (np.abs(vmin.astype(np.float64)) + np.abs(vdiff.astype(np.float64)))).sum(axis=1)
    return 0.5 * np.asarray(scale, np.float64)[:, None] * cabs[None, :] * (1 + 2.0 ** -8) + (d + 8) * 2.0 ** -24 * a[:, None]


def _dev_i16(t, d, device):
    """numpy / torch int16 [nq,d] -> contiguous int16 tensor on `device` (a view when already there)."""
    if isinstance(t, np.ndarray):
        if t.dtype != np.int16:
            raise ValueError(f"search_codes: t must be int16, got {t.dtype}")
        t = torch.from_numpy(np.ascontiguousarray(t))
    if not isinstance(t, torch.Tensor) or t.dtype != torch.int16 or t.dim() != 2 or t.shape[1] != d:
        raise ValueError(f"search_codes expects t int16 [nq,{d}], got {getattr(t, 'dtype', type(t).__name__)} "
                         f"{tuple(getattr(t, 'shape', ()))}")
    return t.to(device=device).contiguous()


class SQIndex(DecodableIndex):
    """Scalar-quantiser index (FAISS IndexScalarQuantizer contract, QT_8bit, METRIC_INNER_PRODUCT) on one GPU.

    search(x, k) returns (D float32, I int64): the score sq_scan_ref defines, descending, equal integer scores the lower row first,
    unused slots (-FLT_MAX, -1).  add() and search() raise RuntimeError until train() has run or `trained` has been assigned."""

    def __init__(self, d, qtype=QT_8bit, metric=METRIC_INNER_PRODUCT, device=None):
        self.d = int(d)
        if qtype != QT_8bit:
            raise ValueError(f"SQIndex: only ScalarQuantizer.QT_8bit ({QT_8bit}) is supported, got {qtype}")
        require_inner_product(metric, "SQIndex")
        if self.d < 1 or self.d > _ffi.IVR_SQ_MAX_D:
            raise ValueError(f"SQIndex: d={d} outside [1,{_ffi.IVR_SQ_MAX_D}] (the int32 accumulator holds 16256 * 128 * d)")
        self.code_size = self.d
        self.qtype = QT_8bit
        self.metric_type = METRIC_INNER_PRODUCT
        self.is_trained = False
        self._trained = np.zeros(2 * self.d, _F)
        self._dev = None                     # (vmin, vdiff, gain, offset, decode table) on the device, made on first use
        self._index = _CodeStore("ivr_sq_index", (self.d,), self.d, "SQIndex", device)
        self.device = self._index.device

    # -- attributes ------------------------------------------------------------------------------
    @property
    def trained(self):
        """numpy float32 [2d] = [vmin | vdiff], as faiss stores it.  Assignable (finite values) while the index is empty, which makes
        it trained."""
        return self._trained

    @trained.setter
    def trained(self, tr):
        self._require_empty("trained", "table")
        tr = np.asarray(tr)
        if tr.shape != (2 * self.d,):
            raise ValueError(f"trained expects [{2 * self.d}], got {tr.shape}")
        tr = np.ascontiguousarray(tr, dtype=_F)
        if not np.isfinite(tr).all():
            raise ValueError("trained: the table must be finite")
        self._trained, self._dev = tr, None
        self.is_trained = True

    def _tables(self):
        if self._dev is None:
            vmin, vdiff = _split(self._trained)
            gain, offset = sq_tables_ref(self._trained)
            table = sq_decode_ref(np.repeat(np.arange(256, dtype=np.uint8)[:, None], self.d, axis=1), self._trained)
            self._dev = tuple(torch.from_numpy(np.ascontiguousarray(a)).to(self.device) for a in (vmin, vdiff, gain, offset, table))
        return self._dev

    # -- training --------------------------------------------------------------------------------
    def train(self, x):
        """trained = sq_train_ref(x): the per-coordinate minimum and range of x [n,d], n >= 1, finite (ValueError otherwise).
        RuntimeError when the index holds rows."""
        self._require_empty("train", "table")
        _staging.check_rows(x, self.d, "train")
        if len(x) < 1:
            raise ValueError("train: no training rows")
        if isinstance(x, torch.Tensor):
            xt = x.to(torch.float32)
            vmin = torch.amin(xt, dim=0)
            tr = torch.cat([vmin, torch.amax(xt, dim=0) - vmin]).cpu().numpy()
        else:
            tr = sq_train_ref(x)
        if not np.isfinite(tr).all():
            raise ValueError("train: the training rows must be finite")
        self._trained, self._dev = np.ascontiguousarray(tr, dtype=_F), None
        self.is_trained = True

    # -- encoding --------------------------------------------------------------------------------
    def _encode_device(self, t):
        """t: contiguous float32 CUDA tensor [n,d] -> codes uint8 CUDA [n,d]."""
        vmin, vdiff = self._tables()[:2]
        codes = torch.empty((t.shape[0], self.d), dtype=torch.uint8, device=self.device)
        _ffi.call("ivr_sq_encode", _ffi.CTX, t, t.shape[0], self.d, vmin, vdiff, codes, device=self.device)
        return codes

    def sa_decode_device(self, codes):
        """float32 CUDA [n,d]: sq_decode_ref(codes, trained) to the bit.  The 256 values a coordinate can decode to are computed on
        the host in sq_decode_ref's float32 order (vmin + vdiff * ((code + 0.5f) / 255f): addition, division, multiplication,
        addition) and gathered on the device: no arithmetic there."""
        self._require_trained("sa_decode")
        c = _dev_u8(codes, self.d, self.device, "sa_decode").to(torch.int64)
        j = torch.arange(self.d, device=self.device).expand(c.shape[0], -1)
        return self._tables()[4][c, j]

    # -- FAISS surface ---------------------------------------------------------------------------
    def add_codes(self, codes):
        """Append rows by their codes: uint8 [n,d] as sa_encode returns them (faiss's add_sa_codes)."""
        self._require_trained("add")
        self._index._add_device(_dev_u8(codes, self.d, self.device, "add_codes"))

    def compute_query_codes_device(self, x):
        """The integer form of the queries x [nq,d]: (t int16 CUDA [nq,d], scale float32 CUDA [nq], bias float32 CUDA [nq]);
        sq_query_ref states them."""
        self._require_trained("compute_query_codes")
        q, staged = _staging.queries_f32(_staging.as_rows(x), self.d, self.device)
        nq = q.shape[0]
        _staging.check_nq(nq, "compute_query_codes")
        gain, offset = self._tables()[2:4]
        t = torch.empty((nq, self.d), dtype=torch.int16, device=self.device)
        scale = torch.empty(nq, dtype=torch.float32, device=self.device)
        bias = torch.empty(nq, dtype=torch.float32, device=self.device)
        _ffi.call("ivr_sq_query", _ffi.CTX, q, nq, self.d, gain, offset, t, scale, bias, device=self.device)
        _staging.sync_if_staged(staged, self.device)
        return t, scale, bias

    def compute_query_codes(self, x):
        """compute_query_codes_device as numpy arrays."""
        return tuple(a.cpu().numpy() for a in self.compute_query_codes_device(x))

    def search_codes_device(self, t, scale, bias, k):
        """The scan on caller-supplied query codes (t int16 [nq,d], scale and bias float32 [nq]): (D, I) CUDA tensors,
        sq_scan_ref(t, scale, bias, codes, k) to the bit.  A |t| beyond 16256 is clamped to it."""
        self._require_trained("search")
        td = _dev_i16(t, self.d, self.device)
        nq = td.shape[0]
        _staging.check_nq(nq)
        sd, bd = _dev_f32(scale, self.device).reshape(-1), _dev_f32(bias, self.device).reshape(-1)
        if sd.shape[0] != nq or bd.shape[0] != nq:
            raise ValueError(f"search_codes expects scale and bias [{nq}], got {tuple(sd.shape)} and {tuple(bd.shape)}")
        k = _staging.check_k(k, _ffi.IVR_MAX_K)
        D, I = _staging.alloc_DI(nq, k, self.device)
        self._index._call("ivr_sq_index_search", td, sd, bd, nq, k, D, I)
        staged = _staging.is_staged(td, t) or _staging.is_staged(sd, scale) or _staging.is_staged(bd, bias)
        _staging.sync_if_staged(staged, self.device)
        return D, I

    def search_codes(self, t, scale, bias, k):
        """search_codes_device as numpy arrays."""
        D, I = self.search_codes_device(t, scale, bias, k)
        return D.cpu().numpy(), I.cpu().numpy()

    def search_device(self, x, k):
        """search returning CUDA tensors: search_codes_device(*compute_query_codes_device(x), k), bit for bit."""
        self._require_trained("search")
        k = _staging.check_k(k, _ffi.IVR_MAX_K)
        return self.search_codes_device(*self.compute_query_codes_device(x), k)


def IndexScalarQuantizer(d, qtype=QT_8bit, metric=METRIC_INNER_PRODUCT):
    """faiss.IndexScalarQuantizer(d, faiss.ScalarQuantizer.QT_8bit, faiss.METRIC_INNER_PRODUCT) drop-in.  ValueError for every other
    quantiser type, for a metric other than inner product (faiss's own default, METRIC_L2, must be replaced explicitly) and for d
    outside [1, 1024]."""
    return SQIndex(d, qtype, metric)
