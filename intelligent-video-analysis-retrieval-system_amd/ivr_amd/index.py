"""FAISS-shaped flat inner-product index resident in MI355X HBM.

Stands in for the `faiss.IndexFlatIP` objects the reference creates at
`unified_index.py:1767` and `core.py:1208-1219`, and for `faiss.normalize_L2`
(`unified_index.py:1776`): same method names, same (D, I) contract -
float32 scores descending, int64 labels, -1 labels for unused slots - so the
call sites `index.add(x)`, `index.search(q, k)`, `index.ntotal`, `index.d`,
`index.is_trained`, `index.train(x)` run unchanged on this object.
`add_with_ids` / `IndexIDMap2` give the rows caller-chosen int64 labels that
survive `remove_ids` (what the reference's `id_to_metadata`, `core.py:722-723`,
and `search_by_id`, `core.py:932-958`, key on).
All arithmetic happens in libivr_hip.so; numpy arrays are staged through
torch CUDA tensors, torch CUDA tensors are used in place.
"""
import ctypes as C

import numpy as np
import torch

from . import _ffi, _staging
from ._faiss import METRIC_INNER_PRODUCT, search_numpy, to_numpy
from ._staging import dev_f32 as _dev_f32


def _ids_i64(ids, n, what):
    """ids (numpy / torch, any integer dtype) -> numpy int64 [n]; ValueError for a wrong length, a non-integer dtype or a negative id."""
    if isinstance(ids, torch.Tensor):
        if ids.dtype.is_floating_point or ids.dtype.is_complex or ids.dtype == torch.bool:
            raise ValueError(f"{what}: ids must be integers, got {ids.dtype}")
        ids = ids.detach().cpu().numpy()
    ids = np.asarray(ids)
    if not np.issubdtype(ids.dtype, np.integer):
        raise ValueError(f"{what}: ids must be integers, got {ids.dtype}")
    ids = ids.reshape(-1).astype(np.int64)
    if n is not None and len(ids) != n:
        raise ValueError(f"{what}: {len(ids)} ids for {n} rows")
    return ids


def normalize_L2(x):
    """faiss.normalize_L2(x): in-place row L2 normalisation of a float32 [n,d] array (zero rows stay zero)."""
    if isinstance(x, np.ndarray):
        if x.dtype != np.float32 or x.ndim != 2:
            raise ValueError("normalize_L2 expects a float32 [n,d] array")
        t = _dev_f32(x, torch.device("cuda", torch.cuda.current_device()))
        normalize_L2(t)
        x[...] = t.cpu().numpy()
        return
    if x.dtype != torch.float32 or x.dim() != 2 or not x.is_cuda or not x.is_contiguous():
        raise ValueError("normalize_L2 expects a contiguous float32 [n,d] CUDA tensor")
    _ffi.call("ivr_l2_normalize", _ffi.CTX, x, x.shape[0], x.shape[1], None, device=x.device)


def count_nonfinite_and_normalize(t):
    """In-place normalise a CUDA tensor and return how many input elements were NaN/Inf (N2 validation)."""
    flag = torch.zeros(1, dtype=torch.int32, device=t.device)
    _ffi.call("ivr_l2_normalize", _ffi.CTX, t, t.shape[0], t.shape[1], flag, device=t.device)
    return int(flag.item())


# -- faiss ID selectors (SearchParameters(sel=...)) --------------------------------------------------------------------------
# Each selector reduces to the filter of the C ABI: an id range [lo, hi) and an optional bitmap in faiss IDSelectorBitmap order
# (bit id & 7 of byte id >> 3).  The bitmap is uploaded once per device and kept.
class _IDSelector:
    lo = hi = 0
    _bits = None            # numpy uint8 bytes from byte _byte0 on (byte index id >> 3), or None: the range alone
    _byte0 = 0
    nbits = 0

    def __init__(self):
        self._dev = {}

    def _filter(self, device):
        """ivr_id_filter for `device` (the bitmap uploaded on first use)."""
        ptr = None
        if self._bits is not None:
            t = self._dev.get(device.index)
            if t is None:
                t = torch.from_numpy(np.ascontiguousarray(self._bits)).to(device) if len(self._bits) else torch.zeros(1, dtype=torch.uint8, device=device)
                self._dev[device.index] = t
            # bits[id >> 3] must address byte id >> 3: the upload starts at byte _byte0, and the kernels read bytes of ids in [lo, hi)
            # only, so lo is kept at or above the upload's first id whatever the attributes say
            ptr = t.data_ptr() - self._byte0
            return _ffi.IdFilter(max(int(self.lo), 8 * self._byte0), int(self.hi), ptr, int(self.nbits))
        return _ffi.IdFilter(int(self.lo), int(self.hi), None, 0)

    def is_member(self, i):
        i = int(i)
        if not (self.lo <= i < self.hi):
            return False
        if self._bits is None:
            return True
        b = (i >> 3) - self._byte0
        return i < self.nbits and 0 <= b < len(self._bits) and bool((self._bits[b] >> (i & 7)) & 1)


class IDSelectorRange(_IDSelector):
    """faiss.IDSelectorRange(imin, imax): ids imin <= id < imax.  Scanning is restricted to the rows of that range."""

    def __init__(self, imin, imax):
        super().__init__()
        self.imin, self.imax = int(imin), int(imax)
        self.lo, self.hi = self.imin, self.imax


class IDSelectorBitmap(_IDSelector):
    """faiss.IDSelectorBitmap(bitmap): id allowed iff bit (id & 7) of byte (id >> 3) is set; bitmap = numpy.packbits(mask,
    bitorder="little") as a uint8 numpy array or torch tensor.  IDSelectorBitmap(n, bitmap) (faiss's C++ argument order) is taken too.
    lo= / hi= (extension): also require lo <= id < hi, i.e. the bitmap intersected with IDSelectorRange(lo, hi); only the rows of that
    range are scanned, so giving the first and last set id as the range keeps a sparse bitmap from streaming the whole index."""

    def __init__(self, *args, lo=None, hi=None):
        super().__init__()
        if len(args) == 2:
            n, bitmap = args
        elif len(args) == 1:
            n, bitmap = None, args[0]
        else:
            raise ValueError("IDSelectorBitmap(bitmap) or IDSelectorBitmap(n, bitmap)")
        if isinstance(bitmap, torch.Tensor):
            if bitmap.dtype != torch.uint8:
                raise ValueError(f"IDSelectorBitmap: bitmap must be uint8, got {bitmap.dtype}")
            bitmap = bitmap.detach().cpu().numpy()
        if not isinstance(bitmap, np.ndarray) or bitmap.dtype != np.uint8:
            raise ValueError("IDSelectorBitmap: bitmap must be a uint8 numpy array or torch tensor")
        bitmap = np.ascontiguousarray(bitmap).reshape(-1)
        if n is not None:
            n = int(n)
            if n < 0 or n > len(bitmap):
                raise ValueError(f"IDSelectorBitmap: n={n} outside [0, {len(bitmap)}]")
            bitmap = bitmap[:n]
        self.bitmap = bitmap.copy()
        self._bits = self.bitmap
        self.nbits = 8 * len(self.bitmap)
        self.lo = 0 if lo is None else max(0, int(lo))
        self.hi = self.nbits if hi is None else min(self.nbits, int(hi))


class IDSelectorBatch(_IDSelector):
    """faiss.IDSelectorBatch(ids): the listed ids (duplicates are harmless).  Stored as a bitmap over [min(ids), max(ids)] plus that
    range, so an id list clustered in a few videos only scans the rows between its first and last id.  Negative ids never match.
    The bitmap takes (max(ids) - min(ids)) / 8 bytes on the host and on each device it is used on: one stray large id (say 10**9 among
    ids below 10**6) costs about 125 MB.  Drop ids at or above the index size first when that matters."""

    def __init__(self, ids):
        super().__init__()
        if isinstance(ids, torch.Tensor):
            ids = ids.detach().cpu().numpy()
        ids = np.asarray(ids).reshape(-1)
        if ids.size and not np.issubdtype(ids.dtype, np.integer):
            raise ValueError(f"IDSelectorBatch: ids must be integers, got {ids.dtype}")
        ids = ids.astype(np.int64)
        ids = np.unique(ids[ids >= 0])
        if ids.size == 0:
            self.lo = self.hi = 0
            self._bits = np.zeros(0, np.uint8)
            return
        lo, hi = int(ids[0]), int(ids[-1]) + 1
        self._byte0 = lo >> 3
        bits = np.zeros(((hi - 1) >> 3) - self._byte0 + 1, np.uint8)
        rel = ids - 8 * self._byte0
        np.bitwise_or.at(bits, rel >> 3, (1 << (rel & 7)).astype(np.uint8))
        self._bits = bits
        self.lo, self.hi, self.nbits = lo, hi, hi


class SearchParameters:
    """faiss.SearchParameters(sel=...): only `sel` is used (None = every id).  The ids a selector names are row positions (id_base + row)
    on a plain index and the stored ids on an id-mapped one (add_with_ids)."""

    def __init__(self, sel=None):
        if sel is not None and not isinstance(sel, _IDSelector):
            raise ValueError(f"SearchParameters: sel must be an IDSelectorRange / IDSelectorBatch / IDSelectorBitmap, got {type(sel).__name__}")
        self.sel = sel


def _selector(params=None, sel=None):
    """The selector of `params` (a SearchParameters) or `sel`; ValueError for anything else."""
    if params is not None:
        if not isinstance(params, SearchParameters):
            raise ValueError(f"params must be a SearchParameters, got {type(params).__name__}")
        if sel is not None:
            raise ValueError("give the selector either in params or as sel, not both")
        sel = params.sel
    if sel is not None and not isinstance(sel, _IDSelector):
        raise ValueError(f"sel must be an IDSelectorRange / IDSelectorBatch / IDSelectorBitmap, got {type(sel).__name__}")
    return sel


class FlatIPIndex(_ffi.Handle):
    """Exact inner-product index (FAISS IndexFlatIP contract) on one GPU."""
    _DESTROY = "ivr_index_destroy"

    def __init__(self, d, capacity=0, device=None):
        self.d = int(d)
        self.is_trained = True
        self.metric_type = METRIC_INNER_PRODUCT
        self._open("ivr_index_create", device, self.d, int(capacity))

    # -- FAISS surface ---------------------------------------------------------------------------
    @property
    def ntotal(self):
        return int(_ffi.call("ivr_index_ntotal", self._h))

    def scan_stats(self):
        """(has_bf16_scan_copy, queries of the last scan chunk that were redone by the exact float32 scan)."""
        out = (C.c_int * 2)()
        _ffi.call("ivr_index_scan_stats", self._h, out)
        return bool(out[0]), int(out[1])

    def train(self, x):  # core.py:817-820 calls train() when is_trained is False; flat indexes never need it
        return None

    def add(self, x, normalize=False, chunk_rows=1 << 20):
        """Append rows.  Host arrays are staged to HBM in chunks of `chunk_rows` so that a build of tens of millions of
        rows never needs a second full copy on either side (the reference adds 10k-row slices, unified_index.py:1770)."""
        if isinstance(x, np.ndarray) or (isinstance(x, torch.Tensor) and not x.is_cuda):
            n = len(x)
            _staging.check_rows(x, self.d, "add")
            for i in range(0, n, chunk_rows):
                self._add_device(_dev_f32(x[i:i + chunk_rows], self.device), normalize)
            return
        self._add_device(_dev_f32(x, self.device), normalize)

    def _add_device(self, t, normalize, ids=None):
        _staging.check_rows(t, self.d, "add")
        if ids is None:
            self._call("ivr_index_add", t, t.shape[0], bool(normalize))
        else:
            self._call("ivr_index_add_with_ids", t, torch.from_numpy(ids).to(self.device), t.shape[0], bool(normalize))
        torch.cuda.current_stream(self.device).synchronize()  # `t` may be a temporary staging copy

    def add_with_ids(self, x, ids, normalize=False, chunk_rows=1 << 20):
        """faiss add_with_ids(x, ids): append rows under caller-chosen int64 labels (numpy or torch, one per row, every id >= 0: -1 is
        the empty-slot label and the selectors never match a negative id; duplicates are allowed).  The first call on an empty index
        makes it id-mapped until reset(): search / range_search return the stored ids, selectors and remove_ids name stored ids, and
        add() is refused.  ValueError for a wrong length, a non-integer dtype or a negative id; refused on an index that already holds
        rows without ids."""
        _staging.check_rows(x, self.d, "add_with_ids")
        n = len(x)
        ids = _ids_i64(ids, n, "add_with_ids")
        if n and int(ids.min()) < 0:
            raise ValueError(f"add_with_ids: negative id {int(ids.min())} (-1 labels an unused result slot)")
        if n == 0:
            self._add_device(torch.empty((0, self.d), dtype=torch.float32, device=self.device), normalize, ids)
        for i in range(0, n, chunk_rows):
            self._add_device(_dev_f32(x[i:i + chunk_rows], self.device), normalize, np.ascontiguousarray(ids[i:i + chunk_rows]))

    @property
    def has_ids(self):
        """True once add_with_ids (or IndexIDMap / IndexIDMap2) has made the index id-mapped; False again after reset()."""
        return bool(_ffi.call("ivr_index_has_ids", self._h))

    @property
    def id_map(self):
        """The stored ids in row order as a numpy int64 copy: faiss.vector_to_array(index.id_map)."""
        n = self.ntotal
        out = torch.empty(n, dtype=torch.int64, device=self.device)
        self._call("ivr_index_get_ids", 0, n, out)
        return out.cpu().numpy()

    def find(self, ids):
        """rows[i] = the lowest row stored under ids[i], or -1 (numpy int64): the reference's search_by_id (core.py:932-958) for one
        key, a result list or a batch of labels for many.  Few keys scan the id table; IVR_FIND_TABLE_MIN_KEYS keys or more go through
        a device hash table that is rebuilt after add_with_ids / remove_ids / reset."""
        keys = _ids_i64(np.atleast_1d(ids) if not isinstance(ids, torch.Tensor) else ids, None, "find")
        return self._find_device(torch.from_numpy(np.ascontiguousarray(keys)).to(self.device)).cpu().numpy()

    def _find_device(self, keys):
        """keys: int64 CUDA tensor [n] of stored ids -> int64 CUDA tensor of their lowest rows (-1: not stored); no host sync."""
        rows = torch.empty(len(keys), dtype=torch.int64, device=self.device)
        self._call("ivr_index_find_ids", keys, len(keys), rows)
        return rows

    # -- row access by position / by key ---------------------------------------------------------
    def _rows_i64(self, rows, what):
        if not (isinstance(rows, torch.Tensor) and rows.is_cuda and rows.device == self.device and rows.dtype == torch.int64
                and rows.dim() == 1 and rows.is_contiguous()):
            raise ValueError(f"{what} expects a contiguous int64 CUDA tensor [n] on {self.device}")
        return rows

    def gather_device(self, rows):
        """Stored rows by POSITION (plain and id-mapped index alike): rows int64 CUDA tensor [n] -> float32 CUDA tensor [n,d] with the
        bits reconstruct_n returns; an entry outside [0, ntotal), -1 included, gives a NaN row.  Repeats are allowed.  No host sync."""
        rows = self._rows_i64(rows, "gather_device")
        out = torch.empty((len(rows), self.d), dtype=torch.float32, device=self.device)
        self._call("ivr_index_gather", rows, len(rows), out)
        return out

    def scatter_device(self, rows, x, normalize=False):
        """Replace the vectors at POSITIONS rows (int64 CUDA tensor [n]) by x (contiguous float32 CUDA tensor [n,d]) in one launch:
        the index ends up bit-identical to n single-row write() calls.  Entries outside [0, ntotal) are skipped, ids stay; with a row
        named twice, which vector it keeps is unspecified.  No host sync: rows and x must stay alive until the stream has run."""
        rows = self._rows_i64(rows, "scatter_device")
        if not (isinstance(x, torch.Tensor) and x.is_cuda and x.device == self.device and x.dtype == torch.float32 and x.is_contiguous()
                and x.dim() == 2 and x.shape == (len(rows), self.d)):
            raise ValueError(f"scatter_device expects a contiguous float32 CUDA tensor [{len(rows)},{self.d}]")
        self._call("ivr_index_scatter", rows, x, len(rows), bool(normalize))

    def _keys_device(self, keys, what):
        """keys (row numbers on a plain index, stored ids on an id-mapped one) -> (numpy int64 keys, int64 CUDA tensor of their rows,
        -1 where a key names no row)."""
        keys = _ids_i64(np.atleast_1d(keys) if not isinstance(keys, torch.Tensor) else keys, None, what)
        k = torch.from_numpy(np.ascontiguousarray(keys)).to(self.device)
        if self.has_ids:
            return keys, self._find_device(k)
        return keys, torch.where((k >= 0) & (k < self.ntotal), k, torch.full_like(k, -1))

    def reconstruct_batch_device(self, keys):
        """(rows, R) CUDA tensors without a host sync: rows int64 [n] = the position of each key (a row number on a plain index, the
        lowest row stored under the id on an id-mapped one; -1 when it names no row), R float32 [n,d] = those rows, NaN where -1."""
        _, rows = self._keys_device(keys, "reconstruct_batch")
        return rows, self.gather_device(rows)

    def reconstruct_batch(self, keys):
        """faiss reconstruct_batch(keys): numpy float32 [n,d].  Keys are row numbers on a plain index and stored ids on an id-mapped
        one (IndexIDMap2::reconstruct: the lowest row under the id).  RuntimeError for a key that names no row, as reconstruct."""
        keys, rows = self._keys_device(keys, "reconstruct_batch")
        R = self.gather_device(rows)
        missing = np.flatnonzero(rows.cpu().numpy() < 0)
        if len(missing):
            raise RuntimeError(f"reconstruct_batch: key {int(keys[missing[0]])} is not in the index ({len(missing)} of {len(keys)} missing)")
        return R.cpu().numpy()

    def update_vectors(self, keys, x, normalize=False):
        """faiss IndexIVF::update_vectors on the flat index: the vectors stored under keys (as for reconstruct_batch) become x [n,d];
        ids and every other row stay.  ValueError for duplicate keys or a wrong shape; RuntimeError when a key names no row, and then
        nothing has been written."""
        _staging.check_rows(x, self.d, "update_vectors")
        keys = _ids_i64(np.atleast_1d(keys) if not isinstance(keys, torch.Tensor) else keys, len(x), "update_vectors")
        if len(np.unique(keys)) != len(keys):
            raise ValueError("update_vectors: duplicate keys")
        keys, rows = self._keys_device(keys, "update_vectors")
        missing = np.flatnonzero(rows.cpu().numpy() < 0)
        if len(missing):
            raise RuntimeError(f"update_vectors: key {int(keys[missing[0]])} is not in the index ({len(missing)} of {len(keys)} missing)")
        t = _dev_f32(x, self.device)
        self.scatter_device(rows, t, normalize)
        torch.cuda.current_stream(self.device).synchronize()  # `t` and `rows` are temporaries

    # -- exact scores of candidate lists -----------------------------------------------------------
    def rescore_device(self, x, cand, k=None, normalize=False, want_all=False):
        """Exact re-ranking of candidate lists (what faiss IndexRefineFlat does behind its base index).  cand: contiguous int64 CUDA
        tensor [nq,kc] of row POSITIONS, kc <= IVR_MAX_K; an entry outside [0, ntotal), -1 included, is absent.  Every score has the
        bits search() reports for that (query, row).
          k given   (D, I) CUDA tensors [nq,k]: the best k candidates of each query in the order of search() (score descending, equal
                    scores the lower row first, whatever their place in cand); a row named m times appears m times; (-FLT_MAX, -1)
                    beyond the present candidates.  I holds positions.  want_all adds D_all from the same call: (D, I, D_all).
          k None    (D_all,): float32 [nq,kc], D_all[i, j] = the score of cand[i, j], -FLT_MAX for an absent entry.
        No host synchronisation unless x had to be staged."""
        t, staged = _staging.queries_f32(x, self.d, self.device)
        nq = t.shape[0]
        _staging.check_nq(nq, "rescore")
        if not (isinstance(cand, torch.Tensor) and cand.is_cuda and cand.device == self.device and cand.dtype == torch.int64
                and cand.dim() == 2 and cand.shape[0] == nq and cand.is_contiguous()):
            raise ValueError(f"rescore_device expects a contiguous int64 CUDA tensor [{nq},kc] on {self.device}")
        kc = cand.shape[1]
        if kc < 1 or kc > _ffi.IVR_MAX_K:
            raise ValueError(f"rescore: kc={kc} outside [1,{_ffi.IVR_MAX_K}]")
        D = I = D_all = None
        if k is not None:
            k = _staging.check_k(k, kc)
            D, I = _staging.alloc_DI(nq, k, self.device)
        if k is None or want_all:
            D_all = torch.empty((nq, kc), dtype=torch.float32, device=self.device)
        self._call("ivr_index_rescore", t, nq, cand, kc, 0 if k is None else k, bool(normalize), D_all, D, I)
        _staging.sync_if_staged(staged, self.device)
        if k is None:
            return (D_all,)
        return (D, I, D_all) if want_all else (D, I)

    def compute_distance_subset(self, x, labels):
        """faiss IndexFlat::compute_distance_subset(n, x, k, distances, labels): numpy float32 [nq,kc], entry [i, j] = the score of
        query i against the row labels[i, j] names, with the bits search() reports.  labels: integers [nq,kc] (numpy or torch), row
        numbers on a plain index and stored ids on an id-mapped one (the lowest row under the id, as reconstruct_batch); a label that
        names no row gives -FLT_MAX."""
        t = _dev_f32(_staging.as_rows(x, tensors_too=False), self.device)
        labels = _staging.int_tensor(labels, "compute_distance_subset: labels", np_dtype=np.int64)
        if labels.dim() != 2 or labels.shape[0] != t.shape[0] or labels.shape[1] < 1:
            raise ValueError(f"compute_distance_subset: labels must be [{t.shape[0]},kc] with kc >= 1, got {tuple(labels.shape)}")
        with torch.cuda.device(self.device):
            rows = labels.to(device=self.device, dtype=torch.int64).contiguous()
            if self.has_ids:
                rows = self._find_device(rows.reshape(-1)).reshape(rows.shape)
            out = self.rescore_device(t, rows)[0].cpu().numpy()       # the copy waits for the stream: t and rows may be temporaries
        return out

    def write(self, start, x, normalize=False):
        """Overwrite rows [start, start+n): ring-buffer maintenance for rolling indexes."""
        t = _dev_f32(x, self.device)
        self._call("ivr_index_write", int(start), t, t.shape[0], bool(normalize))
        torch.cuda.current_stream(self.device).synchronize()

    def write_device(self, start, rows, normalize=False):
        """Stream-ordered overwrite from a float32 CUDA tensor already on this device (no host sync)."""
        if not (isinstance(rows, torch.Tensor) and rows.is_cuda and rows.dtype == torch.float32 and rows.is_contiguous()
                and rows.dim() == 2 and rows.shape[1] == self.d):
            raise ValueError(f"write_device expects a contiguous float32 CUDA tensor [n,{self.d}]")
        self._call("ivr_index_write", int(start), rows, rows.shape[0], bool(normalize))

    def write_ring(self, rows, cursor, normalize=False):
        """Overwrite the rows at *cursor (int64 CUDA scalar tensor) and advance it, all stream-ordered (graph-capturable)."""
        if cursor.dtype != torch.int64 or not cursor.is_cuda or cursor.numel() != 1:
            raise ValueError("cursor must be a 1-element int64 CUDA tensor")
        self._call("ivr_index_write_ring", rows, rows.shape[0], bool(normalize), cursor)

    def search(self, x, k, params=None):
        """(D, I) numpy arrays, exactly like faiss: D float32 [nq,k] descending, I int64 [nq,k], -1 padded.  params =
        SearchParameters(sel=IDSelector...): the top k among the ids the selector allows.  On an id-mapped index (add_with_ids) the
        labels are the stored ids and the selector names stored ids; equal scores still rank the lower ROW first."""
        sel = _selector(params)
        q = _staging.as_rows(x, tensors_too=False)
        return search_numpy(self, q, k) if sel is None else search_numpy(self, q, k, sel=sel)

    def search_device(self, x, k, normalize=False, id_base=0, out=None, sel=None):
        """Device-resident variant: returns CUDA tensors and does not synchronise.  sel: an IDSelector (ids = id_base + row).  On an
        id-mapped index id_base is ignored: labels and selectors are stored ids (one extra pass over the id table per filtered call,
        still without a host synchronisation, and the whole index is scanned whatever the selector's range)."""
        sel = _selector(sel=sel)
        t, staged = _staging.queries_f32(x, self.d, self.device)
        k = _staging.check_k(k, _ffi.IVR_MAX_K)
        nq = t.shape[0]
        D, I = _staging.alloc_DI(nq, k, self.device) if out is None else out
        if sel is None:
            self._call("ivr_index_search", t, nq, k, bool(normalize), int(id_base), D, I)
        else:
            self._call("ivr_index_search_filtered", t, nq, k, bool(normalize), int(id_base), sel._filter(self.device), D, I)
        _staging.sync_if_staged(staged, self.device)
        return D, I

    def search_and_reconstruct(self, x, k, params=None):
        """faiss search_and_reconstruct(x, k): (D, I, R) numpy arrays, D and I exactly what search() returns and R float32 [nq,k,d]
        the stored row behind each slot (the row that scored, also where an id-mapped index stores a label twice), NaN rows for the
        -1 slots.  params = SearchParameters(sel=...) as for search."""
        sel = _selector(params)
        return to_numpy(self.search_and_reconstruct_device(_staging.as_rows(x, tensors_too=False), k, sel=sel))

    def search_and_reconstruct_device(self, x, k, normalize=False, id_base=0, sel=None):
        """Device-resident search_and_reconstruct: (D, I, R) CUDA tensors, arguments as for search_device."""
        sel = _selector(sel=sel)
        t, staged = _staging.queries_f32(x, self.d, self.device)
        k = _staging.check_k(k, _ffi.IVR_MAX_K)
        nq = t.shape[0]
        D, I = _staging.alloc_DI(nq, k, self.device)
        R = torch.empty((nq, k, self.d), dtype=torch.float32, device=self.device)
        f = None if sel is None else sel._filter(self.device)
        self._call("ivr_index_search_reconstruct", t, nq, k, bool(normalize), int(id_base), f, D, I, R)
        _staging.sync_if_staged(staged, self.device)
        return D, I, R

    def range_search(self, x, radius, params=None):
        """faiss range_search: every row with <q, row> > radius.  (lims int64 [nq+1], D float32 [lims[-1]], I int64 [lims[-1]])
        numpy arrays; query i's results are D/I[lims[i]:lims[i+1]], ids ascending.  One host sync to read the total; a second
        pass only when the first-guess capacity was too small.  params = SearchParameters(sel=...): only the allowed ids.  On an
        id-mapped index I holds stored ids (in ascending ROW order within a query) and the selector names stored ids."""
        sel = _selector(params)
        t = _dev_f32(_staging.as_rows(x, tensors_too=False), self.device)
        cap = max(1024, 64 * t.shape[0])
        lims, D, I, total = self.range_search_device(t, radius, cap=cap, sel=sel)
        n = int(total.item())
        if n > cap:
            lims, D, I, total = self.range_search_device(t, radius, cap=n, sel=sel)
        return lims.cpu().numpy(), D[:n].cpu().numpy(), I[:n].cpu().numpy()

    def range_search_device(self, x, radius, normalize=False, id_base=0, cap=None, sel=None):
        """Device-resident range search: (lims [nq+1], D [cap], I [cap], total) CUDA tensors, total = lims[nq:] (the number of
        results; entries at positions >= cap are counted but not written).  No host sync when `cap` is given; cap=None sizes
        D and I exactly (a counting pass, one sync, then the full pass).  sel: an IDSelector (ids = id_base + row; stored ids on an
        id-mapped index, where id_base is ignored)."""
        sel = _selector(sel=sel)
        radius = float(radius)
        if radius != radius:
            raise ValueError("range_search: radius is NaN")
        t, staged = _staging.queries_f32(x, self.d, self.device)
        nq = t.shape[0]
        _staging.check_nq(nq, "range_search")
        lims = torch.empty(nq + 1, dtype=torch.int64, device=self.device)

        def run(c):
            D = torch.empty(max(c, 1), dtype=torch.float32, device=self.device)   # never a NULL pointer, even for cap 0
            I = torch.empty(max(c, 1), dtype=torch.int64, device=self.device)
            if sel is None:
                self._call("ivr_index_range_search", t, nq, radius, bool(normalize), int(id_base), lims, D, I, int(c))
            else:
                self._call("ivr_index_range_search_filtered", t, nq, radius, bool(normalize), int(id_base), sel._filter(self.device),
                           lims, D, I, int(c))
            return D[:c], I[:c]

        with torch.cuda.device(self.device):
            if cap is None:
                run(0)
                cap = int(lims[nq].item())
            D, I = run(int(cap))
            _staging.sync_if_staged(staged)
        return lims, D, I, lims[nq:]

    def reserve_search(self, max_nq, max_k):
        self._call("ivr_index_reserve_search", int(max_nq), int(max_k))

    def reconstruct_n(self, start=0, n=None):
        n = self.ntotal - start if n is None else n
        out = torch.empty((n, self.d), dtype=torch.float32, device=self.device)
        self._call("ivr_index_reconstruct", int(start), int(n), out)
        return out.cpu().numpy()

    def reconstruct(self, i):
        """faiss reconstruct(i): the stored row i as a float32 [d] numpy array.  On an id-mapped index i is a stored id
        (IndexIDMap2::reconstruct): the lowest row stored under it, RuntimeError when no row is.  reconstruct_n stays positional."""
        if self.has_ids:
            row = int(self.find([int(i)])[0])
            if row < 0:
                raise RuntimeError(f"reconstruct: id {int(i)} is not in the index")
            return self.reconstruct_n(row, 1)[0]
        return self.reconstruct_n(int(i), 1)[0]

    def remove_ids(self, sel, id_base=0):
        """faiss remove_ids(sel): delete every stored row whose id (id_base + row) the selector names and return how many were removed.
        sel: an IDSelectorRange / IDSelectorBatch / IDSelectorBitmap, or an integer numpy array / torch tensor of ids (wrapped in an
        IDSelectorBatch, as faiss's Python wrapper does).  The surviving rows keep their order and their bits and move down, so the
        ids above a removed row shift; the capacity stays.  Synchronises the current stream once (not graph-capturable).
        On an id-mapped index the selector (or the integer array) names STORED ids, id_base is ignored, every row stored under a named
        id goes (duplicates each counted), and the surviving rows keep their ids: nothing shifts."""
        if isinstance(sel, (np.ndarray, torch.Tensor)):
            sel = IDSelectorBatch(sel)
        if not isinstance(sel, _IDSelector):
            raise ValueError(f"remove_ids: sel must be an IDSelectorRange / IDSelectorBatch / IDSelectorBitmap or an integer array, "
                             f"got {type(sel).__name__}")
        n = C.c_int64(0)
        self._call("ivr_index_remove_ids", int(id_base), sel._filter(self.device), n)
        return int(n.value)

    def reset(self):
        self._call("ivr_index_reset")


def IndexFlatIP(d):
    """faiss.IndexFlatIP(d) drop-in constructor."""
    return FlatIPIndex(d)


def IndexIDMap2(index):
    """faiss.IndexIDMap2(faiss.IndexFlatIP(d)) drop-in: the given EMPTY FlatIPIndex (ValueError otherwise, as faiss requires), made
    id-mapped: add_with_ids / search / remove_ids / reconstruct(id) work on stored ids and add() raises until the index is reset."""
    if not isinstance(index, FlatIPIndex):
        raise ValueError(f"IndexIDMap2 wraps a FlatIPIndex, got {type(index).__name__}")
    if index.ntotal != 0:
        raise ValueError(f"IndexIDMap2: the index must be empty, it holds {index.ntotal} rows")
    index.add_with_ids(np.zeros((0, index.d), np.float32), np.zeros(0, np.int64))
    return index


IndexIDMap = IndexIDMap2      # faiss.IndexIDMap differs only in lacking reconstruct(), which costs nothing to keep here


def topk_merge(D_parts, I_parts, k=None):
    """Merge per-shard candidates [parts,nq,k] (CUDA tensors, global ids, parts in ascending id order)."""
    parts, nq, kk = D_parts.shape
    k = kk if k is None else k
    D, I = _staging.alloc_DI(nq, k, D_parts.device)
    if k != kk:
        raise ValueError("merge k must equal the per-shard k")
    _ffi.call("ivr_topk_merge", _ffi.CTX, D_parts.contiguous(), I_parts.contiguous(), parts, nq, k, D, I, device=D_parts.device)
    return D, I


def topk_pack(D, I):
    """(D float32 [nq,k], I int64 [nq,k]) CUDA -> int32 [nq,k,3] (score bits, id lo, id hi): the wire format of the one all-gather."""
    nq, k = D.shape
    out = torch.empty((nq, k, 3), dtype=torch.int32, device=D.device)
    _ffi.call("ivr_topk_pack", _ffi.CTX, D.contiguous(), I.contiguous(), nq, k, out, device=D.device)
    return out


def topk_merge_packed(packed_parts):
    """Merge gathered candidates int32 [parts,nq,k,3] (parts in ascending id order) -> (D [nq,k], I [nq,k])."""
    parts, nq, k, _ = packed_parts.shape
    D, I = _staging.alloc_DI(nq, k, packed_parts.device)
    _ffi.call("ivr_topk_merge_packed", _ffi.CTX, packed_parts, parts, nq, k, D, I, device=packed_parts.device)
    return D, I
