"""What the inverted-file indexes (IVFFlatIndex, IVFPQIndex) share: a coarse quantizer (a `FlatIPIndex` of `nlist` centroids) assigns
every row to the list of its best centroid, the rows are kept ordered by list (list l is the run `off[l] .. off[l+1]`), and a search
scans only the lists whose centroids score best against the query.
`InvertedFileIndex` owns the coarse side and the list bookkeeping: the quantizer and its k-means training (`_kmeans.py`), `nprobe`,
the offsets `_off_host` / `_off` (written by `_set_offsets` only), the checks of what is added and the probe step of a search.  A
subclass supplies `ntotal`, `is_trained`, `train`, its row store (named in `_PARTS`) with `add_with_ids` (around `_new_ids`,
`_assign_device` and `_regroup`), `_ids_device(start, n)`, its scan and `reset`.
"""
import numpy as np
import torch

from . import _ffi, _kmeans, _staging
from ._faiss import METRIC_INNER_PRODUCT, search_numpy, typed_params
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
        """add(x, normalize=False) on IVFFlatIndex, add(x) on IVFPQIndex: rows labelled ntotal, ntotal + 1, ... (see add_with_ids)."""
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
