"""FAISS-shaped inverted-file index (IndexIVFFlat, inner product) resident in MI355X HBM.

Stands in for the `faiss.IndexIVFFlat(faiss.IndexFlatIP(d), d, nlist)` the reference builds from 10,000 vectors on
(`unified_index.py:910-921`) and accepts in `_create_index` (`core.py:1209`).  A coarse quantizer (a `FlatIPIndex` of `nlist`
centroids) assigns every row to the list of its best centroid; a search scores only the rows of the `nprobe` lists whose
centroids score best against the query.  Nothing is approximated in the arithmetic: a row's score is the float32 inner product
`FlatIPIndex.search` computes, to the bit, and with `nprobe >= nlist` the result is the flat result.

The rows live in one id-mapped `FlatIPIndex` (the storage), ordered by list, so that every list is a contiguous run of rows:
`off[l] .. off[l+1]`.  Row access, `remove_ids` and the id table are the storage's own; the list scan and the k-means centroid
update are HIP kernels of libivr_hip.so (csrc/search_ivf.hip), torch only orders and concatenates.

Tie rule: equal scores rank the row in the LOWER LIST first, and within a list the row ADDED EARLIER (the lower storage row).  A
result therefore does not depend on the order in which lists were probed.
"""
import numpy as np
import torch

from . import _ffi, _staging
from ._faiss import METRIC_INNER_PRODUCT, METRIC_L2, search_numpy, to_numpy, typed_params  # noqa: F401  (METRIC_L2: exported from here)
from .index import FlatIPIndex, _dev_f32, _ids_i64, normalize_L2


# -- pure numpy helpers (no GPU) ---------------------------------------------------------------------------------------------
def list_offsets(lists, nlist):
    """lists: the list number of every stored row (any order) -> int64 [nlist+1]: list l holds off[l+1] - off[l] rows, and once the
    rows are ordered by list it is the run off[l] .. off[l+1]."""
    lists = np.asarray(lists, dtype=np.int64).reshape(-1)
    if lists.size and (lists.min() < 0 or lists.max() >= nlist):
        raise ValueError(f"list numbers outside [0, {nlist})")
    off = np.zeros(nlist + 1, np.int64)
    np.cumsum(np.bincount(lists, minlength=nlist), out=off[1:])
    return off


def kmeans_sample(n, nlist, max_points_per_centroid=256, seed=1234):
    """The rows k-means trains on, as indices into the n training rows: the first min(n, max_points_per_centroid * nlist) entries of
    numpy.random.RandomState(seed).permutation(n).  The first nlist of them are the initial centroids."""
    perm = np.random.RandomState(seed).permutation(n).astype(np.int64)
    return perm[:min(n, int(max_points_per_centroid) * int(nlist))]


_SPLIT_EPS = 1.0 / 1024.0
_ASSIGN_BLOCK = 1 << 16       # rows per coarse search when whole matrices are assigned: bounds the query workspace of the quantizer


def _nearest(index, t):
    """The best row of `index` for every row of the CUDA tensor t (int64 CUDA [n]): index.search_device(t, 1) in blocks."""
    return torch.cat([index.search_device(t[i:i + _ASSIGN_BLOCK], 1)[1][:, 0] for i in range(0, len(t), _ASSIGN_BLOCK)])


def split_empty_clusters(centroids, counts):
    """faiss Clustering's repair of empty clusters, made deterministic: every cluster with counts == 0, in ascending order, takes a
    copy of the centroid of the currently largest cluster (the lowest such on a tie); the two copies are multiplied by 1 + 1/1024 and
    1 - 1/1024 on alternating coordinates (the new one starts with +, the old one with -) and the count is split, the old cluster
    keeping the larger half.  centroids float32 [nlist,d] and counts int64 [nlist] are changed in place; returns the clusters that
    were touched (new and split ones)."""
    touched = []
    sign = np.where(np.arange(centroids.shape[1]) % 2 == 0, 1.0, -1.0).astype(np.float32) * np.float32(_SPLIT_EPS)
    for ci in np.flatnonzero(counts == 0):
        cj = int(np.argmax(counts))
        if counts[cj] < 2:
            raise ValueError("split_empty_clusters: no cluster left to split")
        base = centroids[cj].copy()
        centroids[ci] = base * (np.float32(1) + sign)
        centroids[cj] = base * (np.float32(1) - sign)
        counts[ci] = counts[cj] // 2
        counts[cj] -= counts[ci]
        touched += [int(ci), cj]
    return sorted(set(touched))


class SearchParametersIVF:
    """faiss.SearchParametersIVF(nprobe=..., sel=...): nprobe overrides the index attribute for one call.  Selectors are not
    supported on IVFFlatIndex: search raises ValueError when sel is set."""

    def __init__(self, nprobe=None, sel=None):
        if nprobe is not None and int(nprobe) < 1:
            raise ValueError(f"SearchParametersIVF: nprobe={nprobe} < 1")
        self.nprobe = None if nprobe is None else int(nprobe)
        self.sel = sel


class IVFFlatIndex:
    """Inverted-file index with exact float32 inner-product scores (FAISS IndexIVFFlat contract) on one GPU.

    search(x, k) looks at the rows of the nprobe lists nearest to each query and returns (D, I) under the contract of
    FlatIPIndex.search: float32 descending, int64 labels, -1 padding.  Equal scores rank the row in the lower list first, and within
    a list the row added earlier.  Every add() call regroups the whole index by list (one pass over all stored rows, and about three
    times their bytes in flight): add in large batches."""

    def __init__(self, d, nlist, device=None, _quantizer=None):
        self.d, self.nlist = int(d), int(nlist)
        if self.d < 1 or self.nlist < 1:
            raise ValueError(f"IVFFlatIndex: d={d} nlist={nlist}")
        self.quantizer = FlatIPIndex(self.d, device=device) if _quantizer is None else _quantizer
        self.device = self.quantizer.device
        self._lib = _ffi.load()
        self._storage = FlatIPIndex(self.d, device=self.device.index)
        self.metric_type = METRIC_INNER_PRODUCT
        self._nprobe = 1
        self.is_trained = False
        self._set_lists(torch.zeros(0, dtype=torch.int64, device=self.device))

    # -- attributes ------------------------------------------------------------------------------
    @property
    def ntotal(self):
        return self._storage.ntotal

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

    def list_sizes(self):
        """int64 [nlist]: rows per list."""
        return np.diff(self._off_host)

    def list_ids(self, l):
        """The labels of list l in stored order (numpy int64)."""
        l = int(l)
        if not 0 <= l < self.nlist:
            raise ValueError(f"list {l} outside [0, {self.nlist})")
        a, b = int(self._off_host[l]), int(self._off_host[l + 1])
        return self._ids_device(a, b - a).cpu().numpy()

    def _ids_device(self, start=0, n=None):
        n = self.ntotal - start if n is None else n
        out = torch.empty(n, dtype=torch.int64, device=self.device)
        if n:
            self._storage._call("ivr_index_get_ids", int(start), int(n), out)
        return out

    def _set_lists(self, row_list):
        """row_list: int64 CUDA tensor, the list of every stored row, ascending."""
        self._row_list = row_list
        sizes = torch.bincount(row_list, minlength=self.nlist) if len(row_list) else torch.zeros(self.nlist, dtype=torch.int64, device=self.device)
        self._off_host = np.concatenate([[0], np.cumsum(sizes.cpu().numpy())]).astype(np.int64)       # = list_offsets(row_list, nlist)
        self._off = torch.from_numpy(self._off_host).to(self.device)
        self._by_size = np.concatenate([[0], np.cumsum(np.sort(np.diff(self._off_host))[::-1])])      # rows of the p longest lists

    # -- training --------------------------------------------------------------------------------
    def train(self, x, niter=10, seed=1234, max_points_per_centroid=256, spherical=True):
        """Make the coarse quantizer.  A quantizer that already holds nlist rows is taken as it is (faiss does the same), otherwise
        k-means runs on x [n,d] (n >= nlist) and its centroids are added to the quantizer:
          sample   kmeans_sample(n, nlist, max_points_per_centroid, seed); the initial centroids are its first nlist rows
          iterate  niter times: assign every sampled row to its best centroid (FlatIPIndex.search with k = 1: equal scores pick the
                   lower centroid), order the rows by assignment (stable), take the mean of every run (ivr_segment_mean: fixed
                   summation order, so a seed gives the same bits every time), repair empty clusters (split_empty_clusters)
          spherical=True L2-normalises the centroids after every update (and the initial ones): the reference stores unit-norm rows
                   and ranks by inner product, where unnormalised means would favour tight clusters.  spherical=False keeps faiss's
                   plain means."""
        if self.quantizer.ntotal == self.nlist:
            self.is_trained = True
            return
        if self.quantizer.ntotal != 0:
            raise ValueError(f"train: the quantizer holds {self.quantizer.ntotal} rows, expected 0 or nlist={self.nlist}")
        _staging.check_rows(x, self.d, "train")
        n = len(x)
        if n < self.nlist:
            raise ValueError(f"train: {n} training rows for nlist={self.nlist}")
        niter = int(niter)
        if niter < 0:
            raise ValueError(f"train: niter={niter} < 0")
        with torch.cuda.device(self.device):
            sample = torch.from_numpy(kmeans_sample(n, self.nlist, max_points_per_centroid, seed))
            if isinstance(x, torch.Tensor) and x.is_cuda:
                xs = _dev_f32(x, self.device)[sample.to(self.device)].contiguous()
            else:       # only the sample travels to the device
                xs = _dev_f32(x[sample.numpy()] if isinstance(x, np.ndarray) else x[sample], self.device)
            cent = xs[:self.nlist].clone()
            if spherical:
                normalize_L2(cent)
            for _ in range(niter):
                cent = self._kmeans_step(xs, cent, bool(spherical))
            self.quantizer.add(cent)
        self.is_trained = True

    def _kmeans_step(self, xs, cent, spherical):
        tmp = FlatIPIndex(self.d, device=self.device.index)
        try:
            tmp.add(cent)
            a = _nearest(tmp, xs)
        finally:
            tmp.close()
        order = torch.argsort(a, stable=True)
        rows = xs[order].contiguous()
        counts = torch.bincount(a, minlength=self.nlist)
        off = torch.cat([torch.zeros(1, dtype=torch.int64, device=self.device), torch.cumsum(counts, 0)]).contiguous()
        out = torch.empty((self.nlist, self.d), dtype=torch.float32, device=self.device)
        _ffi.call("ivr_segment_mean", _ffi.CTX, rows, len(rows), off, self.nlist, self.d, spherical, out, device=self.device)
        counts = counts.cpu().numpy()
        if (counts == 0).any():
            c = out.cpu().numpy()
            for i in split_empty_clusters(c, counts):
                if spherical:
                    nrm = np.float32(np.sqrt(np.dot(c[i].astype(np.float64), c[i].astype(np.float64))))
                    if nrm > 0:
                        c[i] /= nrm
            out = torch.from_numpy(c).to(self.device)
        return out

    # -- adding ----------------------------------------------------------------------------------
    def assign(self, x):
        """The list of each row of x (numpy int64 [n]): the quantizer's own search(x, 1), so equal scores pick the lower list."""
        if not self.is_trained:
            raise RuntimeError("assign: the index is not trained")
        return self.quantizer.search(x, 1)[1][:, 0]

    def add(self, x, normalize=False):
        """Append rows labelled ntotal, ntotal + 1, ... as faiss does.  See add_with_ids."""
        n = len(x) if isinstance(x, (np.ndarray, torch.Tensor)) and x.ndim == 2 else 0
        self.add_with_ids(x, np.arange(self.ntotal, self.ntotal + n, dtype=np.int64), normalize, _what="add")

    def add_with_ids(self, x, ids, normalize=False, _what="add_with_ids"):
        """Append rows under caller-chosen int64 labels (>= 0, duplicates allowed).  Each row goes to the list of its best centroid,
        decided on the bits that end up stored (after normalize).  The whole index is regrouped by list in every call: one pass over
        all stored rows (gather, a stable argsort of the list numbers, add_with_ids into the emptied storage) with about three times
        the index in flight, so add in large batches.  RuntimeError while untrained."""
        if not self.is_trained:
            raise RuntimeError(f"{_what}: the index is not trained")
        _staging.check_rows(x, self.d, _what)
        n = len(x)
        ids = _ids_i64(ids, n, _what)
        if n and int(ids.min()) < 0:
            raise ValueError(f"{_what}: negative id {int(ids.min())} (-1 labels an unused result slot)")
        if n == 0:
            return
        with torch.cuda.device(self.device):
            t = _dev_f32(x, self.device)
            if normalize:
                t = t.clone()
                normalize_L2(t)
            lists = _nearest(self.quantizer, t).clamp_(0, self.nlist - 1)
            new_ids = torch.from_numpy(np.ascontiguousarray(ids)).to(self.device)
            n_old = self._storage.ntotal
            if n_old:
                old = self._storage.gather_device(torch.arange(n_old, dtype=torch.int64, device=self.device))
                t = torch.cat([old, t])
                del old
                new_ids = torch.cat([self._ids_device(), new_ids])
                lists = torch.cat([self._row_list, lists])
            order = torch.argsort(lists, stable=True)
            t = t[order].contiguous()
            self._storage.reset()
            self._storage._add_device(t, False, np.ascontiguousarray(new_ids[order].cpu().numpy()))
            self._set_lists(lists[order].contiguous())

    # -- search ----------------------------------------------------------------------------------
    def _queries(self, x, k, what):
        t, staged = _staging.queries_f32(_staging.as_rows(x), self.d, self.device)
        k = _staging.check_k(k, _ffi.IVR_MAX_K)
        if not self.is_trained:
            raise RuntimeError(f"{what}: the index is not trained")
        return t, k, staged

    def search(self, x, k, params=None):
        """(D, I) numpy arrays under the contract of FlatIPIndex.search, over the rows of the nprobe lists nearest to each query.
        params = SearchParametersIVF(nprobe=...) overrides nprobe for this call; a selector raises ValueError."""
        params = typed_params(params, SearchParametersIVF, "IVFFlatIndex")
        return search_numpy(self, x, k, nprobe=None if params is None else params.nprobe)

    def search_device(self, x, k, normalize=False, nprobe=None):
        """Device-resident search: CUDA tensors, no host synchronisation (unless x had to be staged).  nprobe (default: the
        attribute) is clipped to nlist; below nlist it is the k of the coarse search and so at most IVR_MAX_K."""
        t, k, staged = self._queries(x, k, "search")
        nprobe = min(self.nprobe if nprobe is None else int(nprobe), self.nlist)
        if nprobe < 1:
            raise ValueError(f"nprobe={nprobe} < 1")
        with torch.cuda.device(self.device):
            if nprobe >= self.nlist:     # every list: no coarse search
                assign = torch.arange(self.nlist, dtype=torch.int64, device=self.device).expand(t.shape[0], -1).contiguous()
            else:
                if nprobe > _ffi.IVR_MAX_K:
                    raise ValueError(f"nprobe={nprobe} outside [1,{_ffi.IVR_MAX_K}] (or >= nlist)")
                assign = self.quantizer.search_device(t, nprobe, normalize=normalize)[1]
            return self._scan(t, k, assign, normalize, staged)

    def search_preassigned(self, x, k, assign):
        """faiss search_preassigned: assign int64 [nq,p] (numpy or CUDA tensor) names the lists to scan for each query; -1 entries
        are skipped and a list named twice is scanned once.  ValueError for an entry >= nlist or < -1 (checked on the tensor, before
        any kernel of the scan is launched).  Returns (D, I) numpy arrays."""
        return to_numpy(self.search_preassigned_device(x, k, assign))

    def search_preassigned_device(self, x, k, assign, normalize=False):
        """search_preassigned returning CUDA tensors; the range check of assign synchronises once."""
        t, k, staged = self._queries(x, k, "search_preassigned")
        assign = _staging.int_tensor(assign, "search_preassigned: assign", np_dtype=np.int64)
        if assign.dim() != 2 or assign.shape[0] != t.shape[0] or assign.shape[1] < 1:
            raise ValueError(f"search_preassigned: assign must be [{t.shape[0]},p] with p >= 1, got {tuple(assign.shape)}")
        with torch.cuda.device(self.device):
            assign = assign.to(device=self.device, dtype=torch.int64)
            _staging.check_entries(assign, self.nlist, "search_preassigned: assign entries")
            return self._scan(t, k, assign, normalize, staged)

    def _scan(self, t, k, assign, normalize, staged):
        """assign: int64 CUDA [nq,p], entries in [-1, nlist).  The kernel wants every row ascending (a repeated list is then adjacent)."""
        nq, p = assign.shape
        _staging.check_nq(nq)
        assign = torch.sort(assign, dim=1).values.contiguous()
        D, I = _staging.alloc_DI(nq, k, self.device)
        bound = int(self._by_size[min(p, self.nlist)])
        self._storage._call("ivr_index_search_lists", self._off, self.nlist, t, nq, assign, p, bound, k, bool(normalize), D, I)
        _staging.sync_if_staged(staged, self.device)
        return D, I

    # -- maintenance -----------------------------------------------------------------------------
    def remove_ids(self, sel):
        """faiss remove_ids: delete every row stored under a label the selector (or integer array) names; returns the count.  The
        surviving rows keep their labels and their list."""
        if self.ntotal == 0:
            return 0
        with torch.cuda.device(self.device):
            before = self._ids_device()
            n = self._storage.remove_ids(sel)
            if n:
                # removal goes by label value, so a label loses every row stored under it: the survivors are exactly the rows whose
                # label is still stored, and the storage's compaction keeps their order
                self._set_lists(self._row_list[torch.isin(before, self._ids_device())].contiguous())
        return n

    def reconstruct(self, i):
        """The row stored under label i (the lowest storage row on duplicates); RuntimeError when none is."""
        if not self._storage.has_ids:
            raise RuntimeError(f"reconstruct: id {int(i)} is not in the index")
        return self._storage.reconstruct(i)

    def reconstruct_batch(self, ids):
        """numpy float32 [n,d]: the rows stored under the labels; RuntimeError when one names no row."""
        if not self._storage.has_ids:
            ids = _ids_i64(np.atleast_1d(ids) if not isinstance(ids, torch.Tensor) else ids, None, "reconstruct_batch")
            if len(ids):
                raise RuntimeError(f"reconstruct_batch: key {int(ids[0])} is not in the index ({len(ids)} of {len(ids)} missing)")
            return np.zeros((0, self.d), np.float32)
        return self._storage.reconstruct_batch(ids)

    def reset(self):
        """Drop the rows; the trained quantizer stays."""
        self._storage.reset()
        self._set_lists(torch.zeros(0, dtype=torch.int64, device=self.device))

    def close(self):
        """Release the index (storage and quantizer)."""
        for x in (getattr(self, "_storage", None), getattr(self, "quantizer", None)):
            if x is not None:
                x.close()


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


def IndexIVFFlat(quantizer, d, nlist, metric=METRIC_INNER_PRODUCT):
    """faiss.IndexIVFFlat(quantizer, d, nlist, faiss.METRIC_INNER_PRODUCT) drop-in.  quantizer: a plain (not id-mapped) FlatIPIndex of
    dimension d holding 0 rows (train() fills it) or exactly nlist rows (the centroids; train() then only sets is_trained).
    ValueError for anything else and for a metric other than inner product."""
    if not isinstance(quantizer, FlatIPIndex):
        raise ValueError(f"IndexIVFFlat: the quantizer must be a FlatIPIndex, got {type(quantizer).__name__}")
    if metric != METRIC_INNER_PRODUCT:
        raise ValueError(f"IndexIVFFlat: only METRIC_INNER_PRODUCT ({METRIC_INNER_PRODUCT}) is supported, got {metric}")
    d, nlist = int(d), int(nlist)
    check_quantizer(quantizer, d, nlist, "IndexIVFFlat")
    return IVFFlatIndex(d, nlist, _quantizer=quantizer)
