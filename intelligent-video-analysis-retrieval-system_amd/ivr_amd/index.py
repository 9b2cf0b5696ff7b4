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

from . import _ffi


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


def _dev_f32(x, device):
    """numpy / torch -> contiguous float32 CUDA tensor on `device` (a view when already there)."""
    if isinstance(x, np.ndarray):
        x = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))
    if not isinstance(x, torch.Tensor):
        raise ValueError("expected a numpy array or a torch tensor")
    return x.to(device=device, dtype=torch.float32, non_blocking=False).contiguous()


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
    lib = _ffi.load()
    with torch.cuda.device(x.device):
        _ffi.check(lib.ivr_l2_normalize(_ffi.context(x.device.index), C.c_void_p(x.data_ptr()), x.shape[0], x.shape[1],
                                        None, _ffi.stream_ptr()), "ivr_l2_normalize")


def count_nonfinite_and_normalize(t):
    """In-place normalise a CUDA tensor and return how many input elements were NaN/Inf (N2 validation)."""
    lib = _ffi.load()
    flag = torch.zeros(1, dtype=torch.int32, device=t.device)
    with torch.cuda.device(t.device):
        _ffi.check(lib.ivr_l2_normalize(_ffi.context(t.device.index), C.c_void_p(t.data_ptr()), t.shape[0], t.shape[1],
                                        C.c_void_p(flag.data_ptr()), _ffi.stream_ptr()), "ivr_l2_normalize")
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


class FlatIPIndex:
    """Exact inner-product index (FAISS IndexFlatIP contract) on one GPU."""

    def __init__(self, d, capacity=0, device=None):
        self._lib = _ffi.load()
        self.device = torch.device("cuda", torch.cuda.current_device() if device is None else int(device))
        self.d = int(d)
        self.is_trained = True
        self.metric_type = 0  # faiss.METRIC_INNER_PRODUCT
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            _ffi.check(self._lib.ivr_index_create(_ffi.context(self.device.index), self.d, int(capacity), C.byref(h)),
                       "ivr_index_create")
        self._h = h

    # -- FAISS surface ---------------------------------------------------------------------------
    @property
    def ntotal(self):
        return int(self._lib.ivr_index_ntotal(self._h))

    def scan_stats(self):
        """(has_bf16_scan_copy, queries of the last scan chunk that were redone by the exact float32 scan)."""
        out = (C.c_int * 2)()
        _ffi.check(self._lib.ivr_index_scan_stats(self._h, out), "ivr_index_scan_stats")
        return bool(out[0]), int(out[1])

    def train(self, x):  # core.py:817-820 calls train() when is_trained is False; flat indexes never need it
        return None

    def add(self, x, normalize=False, chunk_rows=1 << 20):
        """Append rows.  Host arrays are staged to HBM in chunks of `chunk_rows` so that a build of tens of millions of
        rows never needs a second full copy on either side (the reference adds 10k-row slices, unified_index.py:1770)."""
        if isinstance(x, np.ndarray) or (isinstance(x, torch.Tensor) and not x.is_cuda):
            n = len(x)
            if x.ndim != 2 or x.shape[1] != self.d:
                raise ValueError(f"add expects [n,{self.d}], got {tuple(x.shape)}")
            for i in range(0, n, chunk_rows):
                self._add_device(_dev_f32(x[i:i + chunk_rows], self.device), normalize)
            return
        self._add_device(_dev_f32(x, self.device), normalize)

    def _add_device(self, t, normalize, ids=None):
        if t.dim() != 2 or t.shape[1] != self.d:
            raise ValueError(f"add expects [n,{self.d}], got {tuple(t.shape)}")
        with torch.cuda.device(self.device):
            if ids is None:
                _ffi.check(self._lib.ivr_index_add(self._h, C.c_void_p(t.data_ptr()), t.shape[0], int(bool(normalize)),
                                                   _ffi.stream_ptr()), "ivr_index_add")
            else:
                i = torch.from_numpy(ids).to(self.device)
                _ffi.check(self._lib.ivr_index_add_with_ids(self._h, C.c_void_p(t.data_ptr()), C.c_void_p(i.data_ptr()), t.shape[0],
                                                            int(bool(normalize)), _ffi.stream_ptr()), "ivr_index_add_with_ids")
            torch.cuda.current_stream().synchronize()  # `t` may be a temporary staging copy

    def add_with_ids(self, x, ids, normalize=False, chunk_rows=1 << 20):
        """faiss add_with_ids(x, ids): append rows under caller-chosen int64 labels (numpy or torch, one per row, every id >= 0: -1 is
        the empty-slot label and the selectors never match a negative id; duplicates are allowed).  The first call on an empty index
        makes it id-mapped until reset(): search / range_search return the stored ids, selectors and remove_ids name stored ids, and
        add() is refused.  ValueError for a wrong length, a non-integer dtype or a negative id; refused on an index that already holds
        rows without ids."""
        if not isinstance(x, (np.ndarray, torch.Tensor)) or x.ndim != 2 or x.shape[1] != self.d:
            raise ValueError(f"add_with_ids expects [n,{self.d}], got {tuple(getattr(x, 'shape', ()))}")
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
        return bool(self._lib.ivr_index_has_ids(self._h))

    @property
    def id_map(self):
        """The stored ids in row order as a numpy int64 copy: faiss.vector_to_array(index.id_map)."""
        n = self.ntotal
        out = torch.empty(n, dtype=torch.int64, device=self.device)
        with torch.cuda.device(self.device):
            _ffi.check(self._lib.ivr_index_get_ids(self._h, 0, n, C.c_void_p(out.data_ptr()), _ffi.stream_ptr()), "ivr_index_get_ids")
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
        with torch.cuda.device(self.device):
            _ffi.check(self._lib.ivr_index_find_ids(self._h, C.c_void_p(keys.data_ptr()), len(keys), C.c_void_p(rows.data_ptr()),
                                                    _ffi.stream_ptr()), "ivr_index_find_ids")
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
        with torch.cuda.device(self.device):
            _ffi.check(self._lib.ivr_index_gather(self._h, C.c_void_p(rows.data_ptr()), len(rows), C.c_void_p(out.data_ptr()),
                                                  _ffi.stream_ptr()), "ivr_index_gather")
        return out

    def scatter_device(self, rows, x, normalize=False):
        """Replace the vectors at POSITIONS rows (int64 CUDA tensor [n]) by x (contiguous float32 CUDA tensor [n,d]) in one launch:
        the index ends up bit-identical to n single-row write() calls.  Entries outside [0, ntotal) are skipped, ids stay; with a row
        named twice, which vector it keeps is unspecified.  No host sync: rows and x must stay alive until the stream has run."""
        rows = self._rows_i64(rows, "scatter_device")
        if not (isinstance(x, torch.Tensor) and x.is_cuda and x.device == self.device and x.dtype == torch.float32 and x.is_contiguous()
                and x.dim() == 2 and x.shape == (len(rows), self.d)):
            raise ValueError(f"scatter_device expects a contiguous float32 CUDA tensor [{len(rows)},{self.d}]")
        with torch.cuda.device(self.device):
            _ffi.check(self._lib.ivr_index_scatter(self._h, C.c_void_p(rows.data_ptr()), C.c_void_p(x.data_ptr()), len(rows),
                                                   int(bool(normalize)), _ffi.stream_ptr()), "ivr_index_scatter")

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
        if not isinstance(x, (np.ndarray, torch.Tensor)) or x.ndim != 2 or x.shape[1] != self.d:
            raise ValueError(f"update_vectors expects [n,{self.d}], got {tuple(getattr(x, 'shape', ()))}")
        keys = _ids_i64(np.atleast_1d(keys) if not isinstance(keys, torch.Tensor) else keys, len(x), "update_vectors")
        if len(np.unique(keys)) != len(keys):
            raise ValueError("update_vectors: duplicate keys")
        keys, rows = self._keys_device(keys, "update_vectors")
        missing = np.flatnonzero(rows.cpu().numpy() < 0)
        if len(missing):
            raise RuntimeError(f"update_vectors: key {int(keys[missing[0]])} is not in the index ({len(missing)} of {len(keys)} missing)")
        t = _dev_f32(x, self.device)
        self.scatter_device(rows, t, normalize)
        with torch.cuda.device(self.device):
            torch.cuda.current_stream().synchronize()  # `t` and `rows` are temporaries

    def write(self, start, x, normalize=False):
        """Overwrite rows [start, start+n): ring-buffer maintenance for rolling indexes."""
        t = _dev_f32(x, self.device)
        with torch.cuda.device(self.device):
            _ffi.check(self._lib.ivr_index_write(self._h, int(start), C.c_void_p(t.data_ptr()), t.shape[0],
                                                 int(bool(normalize)), _ffi.stream_ptr()), "ivr_index_write")
            torch.cuda.current_stream().synchronize()

    def write_device(self, start, rows, normalize=False):
        """Stream-ordered overwrite from a float32 CUDA tensor already on this device (no host sync)."""
        if not (isinstance(rows, torch.Tensor) and rows.is_cuda and rows.dtype == torch.float32 and rows.is_contiguous()
                and rows.dim() == 2 and rows.shape[1] == self.d):
            raise ValueError(f"write_device expects a contiguous float32 CUDA tensor [n,{self.d}]")
        with torch.cuda.device(self.device):
            _ffi.check(self._lib.ivr_index_write(self._h, int(start), C.c_void_p(rows.data_ptr()), rows.shape[0],
                                                 int(bool(normalize)), _ffi.stream_ptr()), "ivr_index_write")

    def write_ring(self, rows, cursor, normalize=False):
        """Overwrite the rows at *cursor (int64 CUDA scalar tensor) and advance it, all stream-ordered (graph-capturable)."""
        if cursor.dtype != torch.int64 or not cursor.is_cuda or cursor.numel() != 1:
            raise ValueError("cursor must be a 1-element int64 CUDA tensor")
        with torch.cuda.device(self.device):
            _ffi.check(self._lib.ivr_index_write_ring(self._h, C.c_void_p(rows.data_ptr()), rows.shape[0], int(bool(normalize)),
                                                      C.c_void_p(cursor.data_ptr()), _ffi.stream_ptr()), "ivr_index_write_ring")

    def search(self, x, k, params=None):
        """(D, I) numpy arrays, exactly like faiss: D float32 [nq,k] descending, I int64 [nq,k], -1 padded.  params =
        SearchParameters(sel=IDSelector...): the top k among the ids the selector allows.  On an id-mapped index (add_with_ids) the
        labels are the stored ids and the selector names stored ids; equal scores still rank the lower ROW first."""
        sel = _selector(params)
        q = np.asarray(x) if not isinstance(x, torch.Tensor) else x
        if isinstance(q, np.ndarray) and q.ndim == 1:
            q = q.reshape(1, -1)
        D, I = self.search_device(q, k) if sel is None else self.search_device(q, k, sel=sel)
        return D.cpu().numpy(), I.cpu().numpy()

    def search_device(self, x, k, normalize=False, id_base=0, out=None, sel=None):
        """Device-resident variant: returns CUDA tensors and does not synchronise.  sel: an IDSelector (ids = id_base + row).  On an
        id-mapped index id_base is ignored: labels and selectors are stored ids (one extra pass over the id table per filtered call,
        still without a host synchronisation, and the whole index is scanned whatever the selector's range)."""
        sel = _selector(sel=sel)
        t = _dev_f32(x, self.device)
        if t.dim() != 2 or t.shape[1] != self.d:
            raise ValueError(f"Query dimension ({tuple(t.shape)}) != index dimension ({self.d})")
        k = int(k)
        if k < 1 or k > _ffi.IVR_MAX_K:
            raise ValueError(f"k={k} outside [1,{_ffi.IVR_MAX_K}]")
        nq = t.shape[0]
        if out is None:
            D = torch.empty((nq, k), dtype=torch.float32, device=self.device)
            I = torch.empty((nq, k), dtype=torch.int64, device=self.device)
        else:
            D, I = out
        with torch.cuda.device(self.device):
            if sel is None:
                _ffi.check(self._lib.ivr_index_search(self._h, C.c_void_p(t.data_ptr()), nq, k, int(bool(normalize)),
                                                      int(id_base), C.c_void_p(D.data_ptr()), C.c_void_p(I.data_ptr()),
                                                      _ffi.stream_ptr()), "ivr_index_search")
            else:
                f = sel._filter(self.device)
                _ffi.check(self._lib.ivr_index_search_filtered(self._h, C.c_void_p(t.data_ptr()), nq, k, int(bool(normalize)), int(id_base),
                                                               C.byref(f), C.c_void_p(D.data_ptr()), C.c_void_p(I.data_ptr()),
                                                               _ffi.stream_ptr()), "ivr_index_search_filtered")
            if t.data_ptr() != (x.data_ptr() if isinstance(x, torch.Tensor) else 0):
                torch.cuda.current_stream().synchronize()  # staging copy must outlive the kernels
        return D, I

    def search_and_reconstruct(self, x, k, params=None):
        """faiss search_and_reconstruct(x, k): (D, I, R) numpy arrays, D and I exactly what search() returns and R float32 [nq,k,d]
        the stored row behind each slot (the row that scored, also where an id-mapped index stores a label twice), NaN rows for the
        -1 slots.  params = SearchParameters(sel=...) as for search."""
        sel = _selector(params)
        q = np.asarray(x) if not isinstance(x, torch.Tensor) else x
        if isinstance(q, np.ndarray) and q.ndim == 1:
            q = q.reshape(1, -1)
        D, I, R = self.search_and_reconstruct_device(q, k, sel=sel)
        return D.cpu().numpy(), I.cpu().numpy(), R.cpu().numpy()

    def search_and_reconstruct_device(self, x, k, normalize=False, id_base=0, sel=None):
        """Device-resident search_and_reconstruct: (D, I, R) CUDA tensors, arguments as for search_device."""
        sel = _selector(sel=sel)
        t = _dev_f32(x, self.device)
        if t.dim() != 2 or t.shape[1] != self.d:
            raise ValueError(f"Query dimension ({tuple(t.shape)}) != index dimension ({self.d})")
        k = int(k)
        if k < 1 or k > _ffi.IVR_MAX_K:
            raise ValueError(f"k={k} outside [1,{_ffi.IVR_MAX_K}]")
        nq = t.shape[0]
        D = torch.empty((nq, k), dtype=torch.float32, device=self.device)
        I = torch.empty((nq, k), dtype=torch.int64, device=self.device)
        R = torch.empty((nq, k, self.d), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            f = None if sel is None else sel._filter(self.device)
            _ffi.check(self._lib.ivr_index_search_reconstruct(self._h, C.c_void_p(t.data_ptr()), nq, k, int(bool(normalize)), int(id_base),
                                                              None if f is None else C.byref(f), C.c_void_p(D.data_ptr()),
                                                              C.c_void_p(I.data_ptr()), C.c_void_p(R.data_ptr()), _ffi.stream_ptr()),
                       "ivr_index_search_reconstruct")
            if t.data_ptr() != (x.data_ptr() if isinstance(x, torch.Tensor) else 0):
                torch.cuda.current_stream().synchronize()  # staging copy must outlive the kernels
        return D, I, R

    def range_search(self, x, radius, params=None):
        """faiss range_search: every row with <q, row> > radius.  (lims int64 [nq+1], D float32 [lims[-1]], I int64 [lims[-1]])
        numpy arrays; query i's results are D/I[lims[i]:lims[i+1]], ids ascending.  One host sync to read the total; a second
        pass only when the first-guess capacity was too small.  params = SearchParameters(sel=...): only the allowed ids.  On an
        id-mapped index I holds stored ids (in ascending ROW order within a query) and the selector names stored ids."""
        sel = _selector(params)
        q = np.asarray(x) if not isinstance(x, torch.Tensor) else x
        if isinstance(q, np.ndarray) and q.ndim == 1:
            q = q.reshape(1, -1)
        t = _dev_f32(q, self.device)
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
        t = _dev_f32(x, self.device)
        if t.dim() != 2 or t.shape[1] != self.d:
            raise ValueError(f"Query dimension ({tuple(t.shape)}) != index dimension ({self.d})")
        nq = t.shape[0]
        if nq < 1:
            raise ValueError("range_search: no queries")
        lims = torch.empty(nq + 1, dtype=torch.int64, device=self.device)

        def run(c):
            D = torch.empty(max(c, 1), dtype=torch.float32, device=self.device)   # never a NULL pointer, even for cap 0
            I = torch.empty(max(c, 1), dtype=torch.int64, device=self.device)
            if sel is None:
                _ffi.check(self._lib.ivr_index_range_search(self._h, C.c_void_p(t.data_ptr()), nq, C.c_float(radius), int(bool(normalize)),
                                                            int(id_base), C.c_void_p(lims.data_ptr()), C.c_void_p(D.data_ptr()),
                                                            C.c_void_p(I.data_ptr()), int(c), _ffi.stream_ptr()), "ivr_index_range_search")
            else:
                f = sel._filter(self.device)
                _ffi.check(self._lib.ivr_index_range_search_filtered(self._h, C.c_void_p(t.data_ptr()), nq, C.c_float(radius),
                                                                     int(bool(normalize)), int(id_base), C.byref(f), C.c_void_p(lims.data_ptr()),
                                                                     C.c_void_p(D.data_ptr()), C.c_void_p(I.data_ptr()), int(c),
                                                                     _ffi.stream_ptr()), "ivr_index_range_search_filtered")
            return D[:c], I[:c]

        with torch.cuda.device(self.device):
            if cap is None:
                run(0)
                cap = int(lims[nq].item())
            D, I = run(int(cap))
            if t.data_ptr() != (x.data_ptr() if isinstance(x, torch.Tensor) else 0):
                torch.cuda.current_stream().synchronize()  # staging copy must outlive the kernels
        return lims, D, I, lims[nq:]

    def reserve_search(self, max_nq, max_k):
        with torch.cuda.device(self.device):
            _ffi.check(self._lib.ivr_index_reserve_search(self._h, int(max_nq), int(max_k)), "ivr_index_reserve_search")

    def reconstruct_n(self, start=0, n=None):
        n = self.ntotal - start if n is None else n
        out = torch.empty((n, self.d), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _ffi.check(self._lib.ivr_index_reconstruct(self._h, int(start), int(n), C.c_void_p(out.data_ptr()),
                                                       _ffi.stream_ptr()), "ivr_index_reconstruct")
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
        with torch.cuda.device(self.device):
            f = sel._filter(self.device)
            _ffi.check(self._lib.ivr_index_remove_ids(self._h, int(id_base), C.byref(f), C.byref(n), _ffi.stream_ptr()),
                       "ivr_index_remove_ids")
        return int(n.value)

    def reset(self):
        with torch.cuda.device(self.device):
            _ffi.check(self._lib.ivr_index_reset(self._h), "ivr_index_reset")

    def close(self):
        if getattr(self, "_h", None):
            self._lib.ivr_index_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


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
    lib = _ffi.load()
    parts, nq, kk = D_parts.shape
    k = kk if k is None else k
    D = torch.empty((nq, k), dtype=torch.float32, device=D_parts.device)
    I = torch.empty((nq, k), dtype=torch.int64, device=D_parts.device)
    if k != kk:
        raise ValueError("merge k must equal the per-shard k")
    with torch.cuda.device(D_parts.device):
        _ffi.check(lib.ivr_topk_merge(_ffi.context(D_parts.device.index), C.c_void_p(D_parts.contiguous().data_ptr()),
                                      C.c_void_p(I_parts.contiguous().data_ptr()), parts, nq, k,
                                      C.c_void_p(D.data_ptr()), C.c_void_p(I.data_ptr()), _ffi.stream_ptr()),
                   "ivr_topk_merge")
    return D, I


def topk_pack(D, I):
    """(D float32 [nq,k], I int64 [nq,k]) CUDA -> int32 [nq,k,3] (score bits, id lo, id hi): the wire format of the one all-gather."""
    lib = _ffi.load()
    nq, k = D.shape
    out = torch.empty((nq, k, 3), dtype=torch.int32, device=D.device)
    with torch.cuda.device(D.device):
        _ffi.check(lib.ivr_topk_pack(_ffi.context(D.device.index), C.c_void_p(D.contiguous().data_ptr()), C.c_void_p(I.contiguous().data_ptr()),
                                     nq, k, C.c_void_p(out.data_ptr()), _ffi.stream_ptr()), "ivr_topk_pack")
    return out


def topk_merge_packed(packed_parts):
    """Merge gathered candidates int32 [parts,nq,k,3] (parts in ascending id order) -> (D [nq,k], I [nq,k])."""
    lib = _ffi.load()
    parts, nq, k, _ = packed_parts.shape
    D = torch.empty((nq, k), dtype=torch.float32, device=packed_parts.device)
    I = torch.empty((nq, k), dtype=torch.int64, device=packed_parts.device)
    with torch.cuda.device(packed_parts.device):
        _ffi.check(lib.ivr_topk_merge_packed(_ffi.context(packed_parts.device.index), C.c_void_p(packed_parts.data_ptr()), parts, nq, k,
                                             C.c_void_p(D.data_ptr()), C.c_void_p(I.data_ptr()), _ffi.stream_ptr()), "ivr_topk_merge_packed")
    return D, I
