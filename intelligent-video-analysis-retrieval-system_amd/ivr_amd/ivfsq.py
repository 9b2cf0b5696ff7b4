"""FAISS-shaped inverted-file index over scalar-quantiser codes (IndexIVFScalarQuantizer, QT_8bit, inner product; faiss's `IVFx,SQ8`)
resident in MI355X HBM.

The reference's `_create_index` (`core.py:1198-1230`) never builds an `IndexIVFScalarQuantizer`; it is here as the usual "compressed
but still accurate" deployment: `d` bytes per row, whose codes rank well by themselves (sq.py), read only in the `nprobe` lists whose
centroids score best against the query.  It joins the coarse side of `InvertedFileIndex` and the list store of
`CodedInvertedFileIndex` (`_ivf.py`, shared with `IVFPQIndex`) with the table, the encoder, the query form and the decoder of
`SQIndex`: a row is stored in the list of its best centroid as the `d`-byte code of its residual against that centroid
(`by_residual`, the default, as in faiss) or of the row itself.

With the inner product residual coding costs nothing at search time: `<q, c_l + decode(code)> = <q, c_l> + <q, decode(code)>`, and
the integer query form `(t, scale, bias)` of `sq_query_ref` depends on the query and the trained table only, so it serves every
list; the only per-list term is the coarse score the coarse search has produced already.  `ivfsq_scan_ref` below states the scan to
the bit; the list store, the probe tables and the scan are HIP kernels of libivr_hip.so (csrc/search_ivfsq.hip: the scan runs on
v_mfma_i32_16x16x64_i8 and reads a list once per 16 queries that probe it), the encoder and the query preparation are those of
`SQIndex`; torch stages arrays, subtracts centroids and orders rows by list.

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
from .sq import QT_8bit, T_MAX, SQIndex, _dev_i16, sq_score_bound

_F = np.float32


# -- pure numpy definitions (no GPU) -------------------------------------------------------------------------------------------
def _ksteps(d):
    return (int(d) + 63) // 64


def ivfsq_pack_ref(codes, list_off):
    """The device layout of list-ordered codes: uint8 [n,d] -> int8 [tiles, ksteps, 64, 16], tiles = 4 groups.  Every list is padded
    to whole 64-row groups and a row's packed position P is that of ivfpq_positions_ref (64 goff[l] + i for row i of list l).  Over
    the packed positions the layout is that of the scalar-quantiser store (csrc/search_sq.hip): the stored byte is code - 128, K is
    padded with zero bytes to ksteps = ceil(d / 64) steps of 64, and position P sits in tile P // 16, whose piece s holds bytes
    64 s + 16 c .. + 15 of the row in lane (P % 16) + 16 c, so one wave-wide 16-byte load of a piece is the A operand of one
    v_mfma_i32_16x16x64_i8.  Pad rows and pad bytes are zero."""
    codes = np.asarray(codes)
    if codes.ndim != 2 or codes.dtype != np.uint8 or codes.shape[1] < 1:
        raise ValueError(f"ivfsq_pack_ref: codes must be uint8 [n,d], got {codes.dtype} {codes.shape}")
    n, d = codes.shape
    pos, goff = ivfpq_positions_ref(_check_off(list_off, n))
    ks, tiles = _ksteps(d), 4 * int(goff[-1])
    padded = np.zeros((tiles * 16, ks * 64), np.int8)
    padded[pos, :d] = (codes.astype(np.int16) - 128).astype(np.int8)
    # [tile, row, step, chunk, byte] -> [tile, step, chunk, row, byte]: lane = row + 16 chunk
    return np.ascontiguousarray(padded.reshape(tiles, 16, ks, 4, 16).transpose(0, 2, 3, 1, 4)).reshape(tiles, ks, 64, 16)


def ivfsq_unpack_ref(packed, list_off, d):
    """The inverse of ivfsq_pack_ref: int8 [tiles, ksteps, 64, 16] -> the list-ordered codes uint8 [n,d]."""
    packed = np.asarray(packed)
    d = int(d)
    ks = _ksteps(d)
    if packed.ndim != 4 or packed.dtype != np.int8 or packed.shape[1:] != (ks, 64, 16) or packed.shape[0] % 4:
        raise ValueError(f"ivfsq_unpack_ref: packed must be int8 [4 groups,{ks},64,16], got {packed.dtype} {packed.shape}")
    off = np.asarray(list_off, np.int64).reshape(-1)
    pos, goff = ivfpq_positions_ref(_check_off(off, off[-1]))
    tiles = packed.shape[0]
    if 4 * goff[-1] != tiles:
        raise ValueError(f"ivfsq_unpack_ref: list_off asks for {goff[-1]} groups, packed holds {tiles // 4}")
    rows = packed.reshape(tiles, ks, 4, 16, 16).transpose(0, 3, 1, 2, 4).reshape(tiles * 16, ks * 64)
    return np.ascontiguousarray((rows[pos, :d].astype(np.int16) + 128).astype(np.uint8))


def ivfsq_scan_ref(t, scale, bias, coarse, assign, list_off, codes, ids, k):
    """The search, to the bit.  t int16 [nq,d] (|t| <= 16256), scale and bias float32 [nq], coarse float32 [nq,p] or None (+0.0),
    assign int64 [nq,p], codes uint8 [n,d] in list order (list l = rows list_off[l] .. list_off[l + 1]), ids int64 [n] ->
    (D float32 [nq,k], I int64 [nq,k]).

    Query i probes the lists assign[i] names: -1 entries are skipped, and a list named twice counts once, with the coarse score of its
    first mention after an ascending STABLE sort of the row.  For row r of a list probed through entry j, with c' = code - 128,
    acc = sum_m t[i,m] * c'[r,m] in exact integer arithmetic (inside int32, as in sq_scan_ref) and
        D = ((float32(acc) * scale[i]) + bias[i]) + coarse[i,j]:
    one conversion that rounds to nearest-even, one float32 multiplication and two float32 additions in this order, no fused
    multiply-add.  (D, I) is the ordering of refine_order_ref over the probed rows: D descending, -0.0 counted and reported as +0.0,
    equal D the row in the lower list first and within a list the row added earlier; I holds ids[r].  Rows are ranked by the float32
    D, not by acc: across lists only D is comparable, and two acc that round to one D rank by position.  Unused slots hold
    (-FLT_MAX, -1).  ValueError for an entry below -1 or >= nlist."""
    from .refine import refine_order_ref
    t = np.asarray(t)
    codes = np.asarray(codes)
    assign = np.asarray(assign).astype(np.int64)
    ids = np.asarray(ids, np.int64).reshape(-1)
    if t.ndim != 2 or codes.ndim != 2 or codes.shape[1] != t.shape[1] or codes.dtype != np.uint8 or t.dtype != np.int16:
        raise ValueError(f"ivfsq_scan_ref: t {t.shape} {t.dtype} must be int16 [nq,d] and codes {codes.shape} {codes.dtype} uint8 [n,d]")
    if t.size and np.abs(t.astype(np.int32)).max() > T_MAX:
        raise ValueError(f"ivfsq_scan_ref: |t| must not exceed {T_MAX}")
    nq, n, k = len(t), len(codes), int(k)
    scale, bias = np.asarray(scale, _F).reshape(nq), np.asarray(bias, _F).reshape(nq)
    off = _check_off(list_off, n)
    nlist = len(off) - 1
    if assign.ndim != 2 or assign.shape[0] != nq or assign.shape[1] < 1 or len(ids) != n:
        raise ValueError(f"ivfsq_scan_ref: assign {assign.shape} must be [{nq},p], ids [{n}]")
    coarse = np.zeros(assign.shape, _F) if coarse is None else np.asarray(coarse, _F)
    if coarse.shape != assign.shape:
        raise ValueError(f"ivfsq_scan_ref: coarse {coarse.shape} must be {assign.shape}")
    if assign.size and (assign.min() < -1 or assign.max() >= nlist):
        raise ValueError(f"ivfsq_scan_ref: assign entries must lie in [-1, {nlist})")
    if k < 1:
        raise ValueError(f"ivfsq_scan_ref: k={k} < 1")
    D = np.full((nq, k), -FLT_MAX, _F)
    I = np.full((nq, k), -1, np.int64)
    signed = codes.astype(np.float64) - 128.0
    for i in range(nq):
        order = np.argsort(assign[i], kind="stable")
        a, c = assign[i, order], coarse[i, order]
        rows, base = [np.zeros(0, np.int64)], [np.zeros(0, _F)]
        for j, l in enumerate(a):
            if l < 0 or (j > 0 and a[j - 1] == l):
                continue
            rows.append(np.arange(off[l], off[l + 1], dtype=np.int64))
            base.append(np.full(off[l + 1] - off[l], c[j], _F))
        rows, base = np.concatenate(rows), np.concatenate(base)
        if len(rows) == 0:
            continue
        acc = (signed[rows] @ t[i].astype(np.float64)).astype(np.int64)      # float64 holds every partial sum exactly
        S = ((acc.astype(_F) * scale[i]).astype(_F) + bias[i]).astype(_F) + base
        kk = min(k, len(rows))
        Di, Ri = refine_order_ref(S[None], rows[None], kk)
        D[i, :kk], I[i, :kk] = Di[0], ids[Ri[0]]
    return D, I


def ivfsq_score_bound(q, codes, trained, scale, cent, D):
    """A bound of the D of ivfsq_scan_ref against faiss's score <q, c_l + decode(code)> in float64 (decode in exact arithmetic from
    the float32 vmin and vdiff, c_l the float32 centroid of the row's list), with (t, scale, bias) prepared from q and the coarse
    score the float32 inner product <q, c_l> of the quantizer.  q [nq,d], codes uint8 [n,d], trained [2d], scale [nq], cent [n,d] =
    the centroid of every row's list, D [nq,n] (or broadcastable to it) -> float64 [nq,n]:
        sq_score_bound(q, codes, trained, scale)  +  (d + 2) * 2^-24 * sum_j |q_j * c_l,j|  +  2^-23 * |D|.
    With S = (float32(acc) * scale) + bias and C the coarse score, D = fl(S + C) and
        |D - <q, c_l + decode>| <= |D - (S + C)| + |S - <q, decode>| + |C - <q, c_l>|.
    The middle term is sq_scan_ref's own bound, unchanged: S is its D.  The last is the float32 accumulation of the quantizer's
    score under any summation order, fused or not: d products and d - 1 additions give at most gamma_d = d u / (1 - d u) relative to
    sum_j |q_j c_l,j|, u = 2^-24, below (d + 2) u for d <= 1024 (zero padding of the rows adds nothing).  The first is the rounding
    of the last addition, at most u |S + C| <= u |D| / (1 - u), taken with a factor 2 of slack.  No further term is needed: the
    scan adds nothing between S and D but that one addition, and the residual coding is exact in the identity above because
    decode and c_l enter it as the float32 values they are stored as (the float32 addition of reconstruct() is not part of D)."""
    q = np.asarray(q, np.float64)
    d = q.shape[1]
    c = (np.abs(q)[:, None, :] * np.abs(np.asarray(cent, np.float64))[None, :, :]).sum(axis=2)
    return sq_score_bound(q, codes, trained, scale) + (d + 2) * 2.0 ** -24 * c + 2.0 ** -23 * np.abs(np.asarray(D, np.float64))


class _TableSQ(SQIndex):
    """The SQIndex an IVFSQIndex holds for its table, encoder, query form and decoder.  Its own row store stays empty; the rows its
    table is bound to are the owner's, so that is what `trained` and `train` ask about."""
    _owner = None

    def _require_empty(self, what, noun):
        n = self._owner.ntotal if self._owner is not None else 0
        if n:
            raise RuntimeError(f"{what}: the index holds {n} rows encoded with the current {noun}")


class IVFSQIndex(CodedInvertedFileIndex):
    """Inverted-file index over scalar-quantiser codes (FAISS IndexIVFScalarQuantizer contract, QT_8bit, METRIC_INNER_PRODUCT) on one
    GPU.

    search(x, k) looks at the rows of the nprobe lists nearest to each query and returns (D, I) as ivfsq_scan_ref defines them over
    the query form sq.compute_query_codes_device(x) and the quantizer's float32 scores of the probed centroids: float32 descending,
    int64 labels, (-FLT_MAX, -1) padding.  Equal scores rank the row in the lower list first, and within a list the row added
    earlier.  `sq` is the SQIndex that holds the table (`sq.trained` is assignable while the index is empty).  Every add() call
    regroups the whole index by list (one pass over all stored codes): add in large batches.  The store, the adding, the search
    surface and the reconstruction are CodedInvertedFileIndex's (_ivf.py)."""
    _PARTS = ("_lists", "sq", "quantizer")
    _ABI = "ivr_ivfsq"
    _NOUN = "table"

    def __init__(self, d, nlist, device=None, _quantizer=None):
        self.sq = _TableSQ(d, device=device if _quantizer is None else _quantizer.device.index)
        super().__init__(d, nlist, self.sq, device, _quantizer)
        self.qtype = QT_8bit

    # -- training --------------------------------------------------------------------------------
    def train(self, x, niter=10, seed=1234, max_points_per_centroid=256, spherical=True):
        """Train the quantizer exactly as IVFFlatIndex.train does (same arguments; a quantizer that already holds nlist rows is taken
        as it is), form the training residuals x_i - centroids[assign(x_i)] (one float32 subtraction per coordinate; x itself without
        by_residual) and train the min / max table on them: sq.trained = sq_train_ref(residuals)."""
        self._train(x, niter, seed, max_points_per_centroid, spherical)

    # -- search ----------------------------------------------------------------------------------
    def compute_query_codes_device(self, x):
        """sq.compute_query_codes_device(x): (t int16 CUDA [nq,d], scale and bias float32 CUDA [nq]), the same for every list."""
        return self.sq.compute_query_codes_device(x)

    _query_form = compute_query_codes_device

    def search_codes_preassigned_device(self, t, scale, bias, coarse, assign, k):
        """The scan alone on caller-supplied query codes: t int16 [nq,d] (a |t| beyond 16256 is clamped to it), scale and bias
        float32 [nq], coarse float32 [nq,p] or None (+0.0), assign int64 [nq,p] -> (D, I) CUDA tensors, ivfsq_scan_ref(t, scale,
        bias, coarse, assign, list offsets, stored codes, stored ids, k) to the bit, whatever by_residual says."""
        self._require_trained("search")
        td = _dev_i16(t, self.d, self.device)
        nq = td.shape[0]
        _staging.check_nq(nq)
        sd, bd = _dev_f32(scale, self.device).reshape(-1), _dev_f32(bias, self.device).reshape(-1)
        if sd.shape[0] != nq or bd.shape[0] != nq:
            raise ValueError(f"search_codes_preassigned expects scale and bias [{nq}], got {tuple(sd.shape)} and {tuple(bd.shape)}")
        k = _staging.check_k(k, _ffi.IVR_MAX_K)
        with torch.cuda.device(self.device):
            assign = self._assign_arg(assign, nq, "search_codes_preassigned")
            out = self._scan((td, sd, bd), None if coarse is None else self._coarse_arg(coarse, assign, "search_codes_preassigned"), assign, k)
            _staging.sync_if_staged(True, self.device)       # every argument may be a staged copy
            return out

    def _scan(self, form, coarse, assign, k):
        """form = (t, scale, bias) on the device; assign: int64 CUDA [nq,p], entries in [-1, nlist).  The kernel wants every row
        ascending (a repeated list is then adjacent); the sort is stable, so the first mention of a list keeps its coarse score."""
        t, scale, bias = form
        nq, p = assign.shape
        assign, coarse = self._ascending(assign, coarse, stable=True)
        D, I = _staging.alloc_DI(nq, k, self.device)
        self._lists._call("ivr_ivfsq_search", t, scale, bias, coarse, assign, nq, p, k, D, I)
        return D, I


def IndexIVFScalarQuantizer(quantizer, d, nlist, qtype=QT_8bit, metric=METRIC_INNER_PRODUCT, by_residual=True):
    """faiss.IndexIVFScalarQuantizer(quantizer, d, nlist, faiss.ScalarQuantizer.QT_8bit, faiss.METRIC_INNER_PRODUCT, by_residual)
    drop-in.  ValueError for every other quantiser type, for a metric other than inner product (faiss's own default, METRIC_L2, must
    be replaced explicitly), for d outside [1, IVR_SQ_MAX_D] and for a quantizer IndexIVFFlat refuses: it must be a plain (not
    id-mapped) FlatIPIndex of dimension d holding 0 rows (train() fills it) or exactly nlist rows."""
    if qtype != QT_8bit:
        raise ValueError(f"IndexIVFScalarQuantizer: only ScalarQuantizer.QT_8bit ({QT_8bit}) is supported, got {qtype}")
    require_inner_product(metric, "IndexIVFScalarQuantizer")
    d, nlist = int(d), int(nlist)
    if d < 1 or d > _ffi.IVR_SQ_MAX_D:
        raise ValueError(f"IndexIVFScalarQuantizer: d={d} outside [1,{_ffi.IVR_SQ_MAX_D}] (the int32 accumulator holds 16256 * 128 * d)")
    if nlist < 1:
        raise ValueError(f"IndexIVFScalarQuantizer: nlist={nlist} < 1")
    if not isinstance(quantizer, FlatIPIndex):
        raise ValueError(f"IndexIVFScalarQuantizer: the quantizer must be a FlatIPIndex, got {type(quantizer).__name__}")
    check_quantizer(quantizer, d, nlist, "IndexIVFScalarQuantizer")
    index = IVFSQIndex(d, nlist, _quantizer=quantizer)
    index.by_residual = by_residual
    return index
