"""What the inverted-file indexes (IVFFlatIndex, IVFPQIndex, IVFSQIndex) share: a coarse quantizer (a `FlatIPIndex` of `nlist` centroids) assigns
every row to the list of its best centroid, the rows are kept ordered by list (list l is the run `off[l] .. off[l+1]`), and a search
scans only the lists whose centroids score best against the query.
`InvertedFileIndex` owns the coarse side and the list bookkeeping: the quantizer and its k-means training (`_kmeans.py`), `nprobe`,
the offsets `_off_host` / `_off` (written by `_set_offsets` only), the checks of what is added and the probe step of a search.  A
subclass supplies `ntotal`, `is_trained`, `train`, its row store (named in `_PARTS`) with `add_with_ids` (around `_new_ids`,
`_assign_device` and `_regroup`), `_ids_device(start, n)`, its scan and `reset`.  `CodedInvertedFileIndex` below is that subclass for the two indexes that keep codes
in a list store of the library: everything but the coder, the query form and the scan call.
`_check_off` and `ivfpq_positions_ref` state the packed position of a row in that store (lists padded to whole 64-row groups).
"""
import numpy as np
import torch

from . import _ffi, _kmeans, _staging
from ._coded import ENCODE_CHUNK
from ._faiss import METRIC_INNER_PRODUCT, search_numpy, to_numpy, typed_params
from .index import FlatIPIndex, _ids_i64, normalize_L2

_ASSIGN_BLOCK = 1 << 16       # rows per coarse search when whole matrices are assigned: bounds the query workspace of the quantizer


def list_offsets(lists, nlist):
    """lists: the list number of every stored row (any order) -> int64 [nlist+1]: list l holds off[l+1] - off[l] rows, and once the
    rows are ordered by list it is the run off[l] .. off[l+1]."""
    lists = np.asarray(lists, dtype=np.int64).reshape(-1)
    if lists.size and (lists.min() < 0 or lists.max() >= nlist):
        raise ValueError(f"list numbers outside [0, {nlist})")
    off = np.zeros(nlist + 1, np.int64)
    np.cumsum(np.bincount(lists, minlength=nlist), out=off[1:])
    return off


def _check_off(list_off, n):
    off = np.asarray(list_off, np.int64).reshape(-1)
    if len(off) < 2 or off[0] != 0 or off[-1] != n or (np.diff(off) < 0).any():
        raise ValueError(f"list_off must ascend from 0 to n={n}")
    return off


def ivfpq_positions_ref(list_off):
    """The packed position of every list-ordered row: list l starts at group goff[l] = sum over the lists below it of
    ceil(size / 64), and its row i sits at 64 goff[l] + i.  -> (pos int64 [n], goff int64 [nlist + 1])."""
    off = np.asarray(list_off, np.int64).reshape(-1)
    sizes = np.diff(off)
    goff = np.concatenate([[0], np.cumsum((sizes + 63) // 64)]).astype(np.int64)
    pos = np.concatenate([64 * goff[l] + np.arange(sizes[l], dtype=np.int64) for l in range(len(sizes))] + [np.zeros(0, np.int64)])
    return pos, goff


def _nearest(index, t):
    """The best row of `index` for every row of the CUDA tensor t (int64 CUDA [n]): index.search_device(t, 1) in blocks."""
    return torch.cat([index.search_device(t[i:i + _ASSIGN_BLOCK], 1)[1][:, 0] for i in range(0, len(t), _ASSIGN_BLOCK)])


class SearchParametersIVF:
    """faiss.SearchParametersIVF(nprobe=..., sel=...): nprobe overrides the index attribute for one call.  Selectors are not
    supported on the inverted-file indexes: search raises ValueError when sel is set."""

    def __init__(self, nprobe=None, sel=None):
        if nprobe is not None and int(nprobe) < 1:
            raise ValueError(f"SearchParametersIVF: nprobe={nprobe} < 1")
        self.nprobe = None if nprobe is None else int(nprobe)
        self.sel = sel


def check_quantizer(quantizer, d, nlist, who):
    """What an inverted-file index asks of the FlatIPIndex that is its coarse quantizer (the factories check the type first, as the
    first of their refusals): plain (not id-mapped), of dimension d, holding 0 or exactly nlist rows.  ValueError otherwise, under
    the name `who`."""
    if quantizer.d != d:
        raise ValueError(f"{who}: the quantizer has dimension {quantizer.d}, expected {d}")
    if quantizer.has_ids:
        raise ValueError(f"{who}: the quantizer must not be id-mapped")
    if quantizer.ntotal not in (0, nlist):
        raise ValueError(f"{who}: the quantizer holds {quantizer.ntotal} rows, expected 0 or nlist={nlist}")


class InvertedFileIndex:
    """Base of the indexes that keep their rows in inverted lists.  Expects ntotal, is_trained and _ids_device on the subclass."""
    _PARTS = ("quantizer",)

    def __init__(self, d, nlist, device=None, _quantizer=None):
        self.d, self.nlist = int(d), int(nlist)
        if self.d < 1 or self.nlist < 1:
            raise ValueError(f"IVFFlatIndex: d={d} nlist={nlist}")       # the text both classes have always raised
        self.quantizer = FlatIPIndex(self.d, device=device) if _quantizer is None else _quantizer
        self.device = self.quantizer.device
        self.metric_type = METRIC_INNER_PRODUCT
        self._nprobe = 1
        self._set_offsets(np.zeros(self.nlist + 1, np.int64))

    # -- attributes ------------------------------------------------------------------------------
    @property
    def nprobe(self):
        return self._nprobe

    @nprobe.setter
    def nprobe(self, v):
        if int(v) < 1:
            raise ValueError(f"nprobe={v} < 1")
        self._nprobe = int(v)

    @property
    def centroids(self):
        """numpy float32 [nlist,d]: quantizer.reconstruct_n()."""
        return self.quantizer.reconstruct_n()

    def _require_trained(self, what):
        if not self.is_trained:
            raise RuntimeError(f"{what}: the index is not trained")

    def _set_offsets(self, off_host):
        """off_host: int64 numpy [nlist+1], the rows in front of every list.  The one place the offsets are set."""
        self._off_host = off_host
        self._off = torch.from_numpy(off_host).to(self.device)

    def _check_list(self, l):
        l = int(l)
        if not 0 <= l < self.nlist:
            raise ValueError(f"list {l} outside [0, {self.nlist})")
        return int(self._off_host[l]), int(self._off_host[l + 1])

    def list_sizes(self):
        """int64 [nlist]: rows per list."""
        return np.diff(self._off_host)

    def list_ids(self, l):
        """The labels of list l in stored order (numpy int64)."""
        a, b = self._check_list(l)
        return self._ids_device(a, b - a).cpu().numpy()

    # -- training --------------------------------------------------------------------------------
    def _train_quantizer(self, x, niter=10, seed=1234, max_points_per_centroid=256, spherical=True):
        """Fill the coarse quantizer as IVFFlatIndex.train states; one that already holds nlist rows is taken as it is."""
        if self.quantizer.ntotal == self.nlist:
            return
        if self.quantizer.ntotal != 0:
            raise ValueError(f"train: the quantizer holds {self.quantizer.ntotal} rows, expected 0 or nlist={self.nlist}")
        _staging.check_rows(x, self.d, "train")
        n = len(x)
        if n < self.nlist:
            raise ValueError(f"train: {n} training rows for nlist={self.nlist}")
        niter = _kmeans.check_niter(niter)
        with torch.cuda.device(self.device):
            xs = _kmeans.sample_rows(x, self.nlist, max_points_per_centroid, seed, self.device)
            cent = xs[:self.nlist].clone()
            if spherical:
                normalize_L2(cent)
            for _ in range(niter):
                cent = self._kmeans_step(xs, cent, bool(spherical))
            self.quantizer.add(cent)

    def _kmeans_step(self, xs, cent, spherical):
        tmp = FlatIPIndex(self.d, device=self.device.index)
        try:
            tmp.add(cent)
            a = _nearest(tmp, xs)
        finally:
            tmp.close()
        out = torch.empty((self.nlist, self.d), dtype=torch.float32, device=self.device)
        counts = _kmeans.segment_means(xs, a, self.nlist, out, spherical)
        return _kmeans.repair_empty_clusters(out, counts.cpu().numpy(), spherical)

    # -- adding ----------------------------------------------------------------------------------
    def assign(self, x):
        """The list of each row of x (numpy int64 [n]): the quantizer's own search(x, 1), so equal scores pick the lower list."""
        self._require_trained("assign")
        return self.quantizer.search(x, 1)[1][:, 0]

    def add(self, x, *args, **kw):
        """add(x, normalize=False) on IVFFlatIndex, add(x) on IVFPQIndex and IVFSQIndex: rows labelled ntotal, ntotal + 1, ... (see add_with_ids)."""
        n = len(x) if isinstance(x, (np.ndarray, torch.Tensor)) and x.ndim == 2 else 0
        self.add_with_ids(x, np.arange(self.ntotal, self.ntotal + n, dtype=np.int64), *args, _what="add", **kw)

    def _new_ids(self, x, ids, what):
        """The checks of add_with_ids(x, ids): trained, x [n,d], n labels >= 0.  Returns the labels as int64 numpy [n]."""
        self._require_trained(what)
        _staging.check_rows(x, self.d, what)
        ids = _ids_i64(ids, len(x), what)
        if len(ids) and int(ids.min()) < 0:
            raise ValueError(f"{what}: negative id {int(ids.min())} (-1 labels an unused result slot)")
        return ids

    def _assign_device(self, t):
        """The list of each row of the float32 CUDA tensor t (int64 CUDA [n])."""
        return _nearest(self.quantizer, t).clamp_(0, self.nlist - 1)

    def _regroup(self, lists):
        """lists: int64 CUDA [n], the list of every row, the stored ones (in stored order) first -> (order int64 CUDA [n]: row
        order[i] comes i-th in list order, rows of one list in the order given; the new offsets, int64 numpy [nlist+1])."""
        return torch.argsort(lists, stable=True), self._offsets(lists)

    def _offsets(self, lists):
        """list_offsets(lists, nlist) of an int64 CUDA tensor: one count on the device, one copy to the host."""
        sizes = torch.bincount(lists, minlength=self.nlist).cpu().numpy() if len(lists) else np.zeros(self.nlist, np.int64)
        return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)

    # -- search ----------------------------------------------------------------------------------
    def _queries(self, x, k, what):
        t, staged = _staging.queries_f32(_staging.as_rows(x), self.d, self.device)
        k = _staging.check_k(k, _ffi.IVR_MAX_K)
        self._require_trained(what)
        return t, k, staged

    def search(self, x, k, params=None):
        """(D, I) numpy arrays of search_device(x, k): over the rows of the nprobe lists nearest to each query.  params =
        SearchParametersIVF(nprobe=...) overrides nprobe for this call; a selector raises ValueError."""
        params = typed_params(params, SearchParametersIVF, type(self).__name__)
        return search_numpy(self, x, k, nprobe=None if params is None else params.nprobe)

    def _probe(self, t, nprobe, normalize=False):
        """The lists each query of t probes: nprobe (default: the attribute) clipped to nlist -> (coarse, assign), CUDA [nq,nprobe]:
        the quantizer's search, or every list in ascending order and coarse = None when nprobe >= nlist.  The caller has made the
        index's device the current one."""
        nprobe = min(self.nprobe if nprobe is None else int(nprobe), self.nlist)
        if nprobe < 1:
            raise ValueError(f"nprobe={nprobe} < 1")
        if nprobe >= self.nlist:     # every list: no coarse search
            return None, torch.arange(self.nlist, dtype=torch.int64, device=self.device).expand(t.shape[0], -1).contiguous()
        if nprobe > _ffi.IVR_MAX_K:
            raise ValueError(f"nprobe={nprobe} outside [1,{_ffi.IVR_MAX_K}] (or >= nlist)")
        return self.quantizer.search_device(t, nprobe, normalize=normalize)

    def _assign_arg(self, assign, nq, what):
        """A caller's assign -> int64 CUDA [nq,p], p >= 1, entries in [-1, nlist) (the range check synchronises once)."""
        assign = _staging.int_tensor(assign, f"{what}: assign", np_dtype=np.int64)
        if assign.dim() != 2 or assign.shape[0] != nq or assign.shape[1] < 1:
            raise ValueError(f"{what}: assign must be [{nq},p] with p >= 1, got {tuple(assign.shape)}")
        assign = assign.to(device=self.device, dtype=torch.int64)
        _staging.check_entries(assign, self.nlist, f"{what}: assign entries")
        return assign

    @staticmethod
    def _ascending(assign, coarse=None, stable=False):
        """Every row of assign ascending, which the scan kernels require (a repeated list is then adjacent), with the coarse scores
        carried along: under a stable sort the first mention of a list keeps its score.  -> (assign, coarse), contiguous."""
        assign, order = torch.sort(assign, dim=1, stable=stable)
        return assign.contiguous(), None if coarse is None else torch.gather(coarse, 1, order).contiguous()

    def close(self):
        """Release the index: the device objects _PARTS names, in that order."""
        for x in (getattr(self, name, None) for name in self._PARTS):
            if x is not None:
                x.close()


class _ListStore(_ffi.Handle):
    """The list store of a coded inverted-file index on the device: the object behind the exports `abi`_create / _destroy /
    _set_lists / _get_codes / _reset / _search (ivr_ivfpq of csrc/search_ivfpq.hip, ivr_ivfsq of csrc/search_ivfsq.hip)."""

    def __init__(self, abi, code_size, nlist, device):
        self._DESTROY = abi + "_destroy"
        self._open(abi + "_create", device, int(code_size), int(nlist))


class CodedInvertedFileIndex(InvertedFileIndex):
    """What the inverted-file indexes over codes (IVFPQIndex, IVFSQIndex) share: a row is stored in the list of its best centroid as
    the code of its residual against that centroid (`by_residual`, the default, as in faiss) or of the row itself; the codes live in
    a list store of the library (`_ABI` names its exports) and a search scans the probed lists with one query form that serves
    every list, the coarse score being the only per-list term.  The coder (a PQIndex / SQIndex whose own row store stays empty and
    whose tables are bound to the owner's rows) is handed to the constructor; a subclass supplies `_ABI`, `_NOUN`, `train` (around
    `_train`), `_query_form(t)` and `_scan(form, coarse, assign, k)`."""
    _ABI = None
    _NOUN = "tables"

    def __init__(self, d, nlist, coder, device=None, _quantizer=None):
        self._coder = coder
        coder._owner = self
        super().__init__(d, nlist, device, _quantizer)
        self.code_size = coder.code_size
        self._by_residual = True
        self._coarse_trained = False
        self._cent_dev = None
        self._lists = _ListStore(self._ABI, self.code_size, self.nlist, self.device.index)

    # -- attributes ------------------------------------------------------------------------------
    @property
    def ntotal(self):
        return int(self._off_host[-1])

    @property
    def is_trained(self):
        return bool(self._coder.is_trained and (self._coarse_trained or self.quantizer.ntotal == self.nlist))

    @property
    def by_residual(self):
        """True (faiss's default): a row is coded as its residual against its list's centroid.  Assignable only while the index is
        empty and untrained: the coder is trained on what is coded."""
        return self._by_residual

    @by_residual.setter
    def by_residual(self, v):
        if self.ntotal or self.is_trained:
            raise RuntimeError("by_residual: the index is trained or holds rows coded with the current setting")
        self._by_residual = bool(v)

    def _centroids_device(self):
        if self._cent_dev is None:
            self._cent_dev = self.quantizer.gather_device(torch.arange(self.nlist, dtype=torch.int64, device=self.device))
        return self._cent_dev

    def list_codes(self, l):
        """The codes of list l in stored order (numpy uint8 [size, code_size])."""
        a, b = self._check_list(l)
        return self._rows_device(a, b - a, ids=False)[0].cpu().numpy()

    def _rows_device(self, start=0, n=None, codes=True, ids=True):
        """(codes uint8 CUDA [n,code_size], ids int64 CUDA [n]) of the list-ordered rows [start, start + n); None for the half not asked for."""
        n = self.ntotal - start if n is None else n
        c = torch.empty((n, self.code_size), dtype=torch.uint8, device=self.device) if codes else None
        i = torch.empty(n, dtype=torch.int64, device=self.device) if ids else None
        if n:
            self._lists._call(self._ABI + "_get_codes", int(start), int(n), c, i)
        return c, i

    def _ids_device(self, start=0, n=None):
        return self._rows_device(start, n, codes=False)[1]

    def _set_lists(self, codes, ids, off_host):
        self._lists._call(self._ABI + "_set_lists", codes, ids, off_host.ctypes.data, len(codes))
        torch.cuda.current_stream(self.device).synchronize()      # codes and ids may be temporaries
        self._set_offsets(off_host)

    # -- training --------------------------------------------------------------------------------
    def _train(self, x, niter, seed, max_points_per_centroid, spherical):
        """Train the quantizer as IVFFlatIndex.train does (a quantizer that already holds nlist rows is taken as it is), then the
        coder on the residuals x_i - centroids[assign(x_i)] (one float32 subtraction per coordinate; x itself without by_residual)."""
        if self.ntotal:
            raise RuntimeError(f"train: the index holds {self.ntotal} rows encoded with the current {self._NOUN}")
        _staging.check_rows(x, self.d, "train")
        self._train_quantizer(x, niter, seed, max_points_per_centroid, spherical)
        self._coarse_trained = True
        self._cent_dev = None
        with torch.cuda.device(self.device):
            t = _staging.dev_f32(x, self.device)
            self._coder.train(self._residuals(t, self._assign_device(t)) if self._by_residual else t)

    def _residuals(self, t, lists):
        return t - self._centroids_device()[lists]

    # -- adding ----------------------------------------------------------------------------------
    def add_with_ids(self, x, ids, *, _what="add_with_ids"):
        """Append rows under caller-chosen int64 labels (>= 0, duplicates allowed).  Each row goes to the list of its best centroid
        and only its code is kept: the coder's encoder applied to its residual against that centroid (to the row itself without
        by_residual).  The whole index is regrouped by list in every call: one pass over all stored codes (unpack, a stable argsort
        of the list numbers, pack), so add in large batches.  RuntimeError while untrained."""
        ids = self._new_ids(x, ids, _what)
        if len(ids) == 0:
            return
        with torch.cuda.device(self.device):
            codes, lists = [], []
            for i in range(0, len(ids), ENCODE_CHUNK):
                t = _staging.dev_f32(x[i:i + ENCODE_CHUNK], self.device)
                l = self._assign_device(t)
                codes.append(self._coder._encode_device(self._residuals(t, l) if self._by_residual else t))
                lists.append(l)
            codes, lists = torch.cat(codes), torch.cat(lists)
            new_ids = torch.from_numpy(np.ascontiguousarray(ids)).to(self.device)
            if self.ntotal:
                old_codes, old_ids = self._rows_device()
                sizes = torch.from_numpy(self.list_sizes()).to(self.device)
                codes = torch.cat([old_codes, codes])
                new_ids = torch.cat([old_ids, new_ids])
                lists = torch.cat([torch.repeat_interleave(torch.arange(self.nlist, device=self.device), sizes), lists])
            order, off = self._regroup(lists)
            self._set_lists(codes[order].contiguous(), new_ids[order].contiguous(), off)

    # -- search ----------------------------------------------------------------------------------
    def _coarse_scores(self, t, assign):
        """float32 CUDA [nq,p]: the quantizer's inner product of query i with centroid assign[i,j], with the bits its search reports
        (-FLT_MAX for a -1 entry, which the scan skips)."""
        step = _ffi.IVR_MAX_K
        return torch.cat([self.quantizer.rescore_device(t, assign[:, j:j + step].contiguous())[0] for j in range(0, assign.shape[1], step)], dim=1)

    def search_device(self, x, k, nprobe=None):
        """Device-resident search: CUDA tensors, no host synchronisation (unless x had to be staged).  nprobe (default: the attribute)
        is clipped to nlist; below nlist it is the k of the coarse search and so at most IVR_MAX_K.  With nprobe >= nlist there is no
        coarse search: every list is probed, with the coarse scores search_preassigned computes."""
        t, k, staged = self._queries(x, k, "search")
        _staging.check_nq(t.shape[0])
        with torch.cuda.device(self.device):
            coarse, assign = self._probe(t, nprobe)
            if not self._by_residual:
                coarse = None
            elif coarse is None:         # every list: the scores search_preassigned computes
                coarse = self._coarse_scores(t, assign)
            out = self._scan(self._query_form(t), coarse, assign, k)
            _staging.sync_if_staged(staged, self.device)
            return out

    def search_preassigned(self, x, k, assign, coarse_dis=None):
        """faiss search_preassigned: assign int64 [nq,p] (numpy or CUDA tensor) names the lists to scan for each query; -1 entries
        are skipped and a list named twice is scanned once.  coarse_dis float32 [nq,p]: the coarse score that goes with each entry;
        when omitted it is the quantizer's float32 inner product for exactly the named lists (the bits its search reports).  Without
        by_residual it is not used.  ValueError for an entry >= nlist or < -1.  Returns (D, I) numpy arrays."""
        return to_numpy(self.search_preassigned_device(x, k, assign, coarse_dis))

    def search_preassigned_device(self, x, k, assign, coarse_dis=None):
        """search_preassigned returning CUDA tensors; the range check of assign synchronises once."""
        t, k, staged = self._queries(x, k, "search_preassigned")
        _staging.check_nq(t.shape[0])
        with torch.cuda.device(self.device):
            assign = self._assign_arg(assign, t.shape[0], "search_preassigned")
            coarse = None
            if self._by_residual:
                coarse = self._coarse_scores(t, assign) if coarse_dis is None else self._coarse_arg(coarse_dis, assign, "search_preassigned")
            out = self._scan(self._query_form(t), coarse, assign, k)
            _staging.sync_if_staged(staged, self.device)
            return out

    def _coarse_arg(self, coarse, assign, what):
        c = _staging.dev_f32(coarse, self.device)
        if tuple(c.shape) != tuple(assign.shape):
            raise ValueError(f"{what}: the coarse scores must be float32 {tuple(assign.shape)}, got {tuple(c.shape)}")
        return c

    # -- reconstruction --------------------------------------------------------------------------
    def reconstruct_batch(self, ids):
        """numpy float32 [n,d]: for every label centroids[l] + the coder's sa_decode(code) of the row stored under it, one float32 addition per
        coordinate (the decode alone without by_residual); the lowest stored position on duplicate labels.  RuntimeError when a label
        names no row.  Reads every stored label and code once per call."""
        keys = _ids_i64(np.atleast_1d(ids) if not isinstance(ids, torch.Tensor) else ids, None, "reconstruct_batch")
        miss, out = self._reconstruct(keys)
        if len(miss):
            raise RuntimeError(f"reconstruct_batch: key {int(keys[miss[0]])} is not in the index ({len(miss)} of {len(keys)} missing)")
        return out

    def reconstruct(self, i):
        """The decoded row stored under label i (the lowest stored position on duplicates); RuntimeError when none is."""
        miss, out = self._reconstruct(np.array([int(i)], np.int64))
        if len(miss):
            raise RuntimeError(f"reconstruct: id {int(i)} is not in the index")
        return out[0]

    def _reconstruct(self, keys):
        """keys int64 numpy [n] -> (the positions in keys of the labels that name no row, the decoded rows [n,d] or None when one is
        missing)."""
        if len(keys) == 0:
            return np.zeros(0, np.int64), np.zeros((0, self.d), np.float32)
        if self.ntotal == 0:
            return np.arange(len(keys)), None
        with torch.cuda.device(self.device):
            codes, stored = self._rows_device()
            k = torch.from_numpy(np.ascontiguousarray(keys)).to(self.device)
            sorted_ids, perm = torch.sort(stored, stable=True)
            at = torch.searchsorted(sorted_ids, k).clamp_(max=self.ntotal - 1)
            miss = np.flatnonzero((sorted_ids[at] != k).cpu().numpy())
            if len(miss):
                return miss, None
            rows = perm[at]
            out = self._coder.sa_decode_device(codes[rows].contiguous())
            if self._by_residual:
                out = self._centroids_device()[torch.searchsorted(self._off, rows, right=True) - 1] + out
            return miss, out.cpu().numpy()

    # -- maintenance -----------------------------------------------------------------------------
    def reset(self):
        """Drop the rows; the trained quantizer and coder stay."""
        self._lists._call(self._ABI + "_reset")
        self._set_offsets(np.zeros(self.nlist + 1, np.int64))
