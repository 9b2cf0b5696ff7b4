"""FAISS-shaped inverted-file index (IndexIVFFlat, inner product) resident in MI355X HBM.

Stands in for the `faiss.IndexIVFFlat(faiss.IndexFlatIP(d), d, nlist)` the reference builds from 10,000 vectors on
(`unified_index.py:910-921`) and accepts in `_create_index` (`core.py:1209`).  A coarse quantizer (a `FlatIPIndex` of `nlist`
centroids) assigns every row to the list of its best centroid; a search scores only the rows of the `nprobe` lists whose
centroids score best against the query.  Nothing is approximated in the arithmetic: a row's score is the float32 inner product
`FlatIPIndex.search` computes, to the bit, and with `nprobe >= nlist` the result is the flat result.

The rows live in one id-mapped `FlatIPIndex` (the storage), ordered by list, so that every list is a contiguous run of rows:
`off[l] .. off[l+1]`.  Row access, `remove_ids` and the id table are the storage's own; the list scan and the k-means centroid
update are HIP kernels of libivr_hip.so (csrc/search_ivf.hip), torch only orders and concatenates.  The coarse side (quantizer, k-means,
offsets, probe step) is `InvertedFileIndex`'s (`_ivf.py`, `_kmeans.py`), shared with `IVFPQIndex`, and its names are re-exported here.

Tie rule: equal scores rank the row in the LOWER LIST first, and within a list the row ADDED EARLIER (the lower storage row).  A
result therefore does not depend on the order in which lists were probed.
"""
import numpy as np
import torch

from . import _staging
from ._faiss import METRIC_INNER_PRODUCT, METRIC_L2, to_numpy  # noqa: F401  (METRIC_L2: exported from here)
from ._ivf import InvertedFileIndex, SearchParametersIVF, _nearest, check_quantizer, list_offsets  # noqa: F401  (exported from here)
from ._kmeans import kmeans_sample, split_empty_clusters  # noqa: F401  (exported from here)
from .index import FlatIPIndex, _dev_f32, _ids_i64, normalize_L2


class IVFFlatIndex(InvertedFileIndex):
    """Inverted-file index with exact float32 inner-product scores (FAISS IndexIVFFlat contract) on one GPU.

    search(x, k) looks at the rows of the nprobe lists nearest to each query and returns (D, I) under the contract of
    FlatIPIndex.search: float32 descending, int64 labels, -1 padding.  Equal scores rank the row in the lower list first, and within
    a list the row added earlier.  Every add() call regroups the whole index by list (one pass over all stored rows, and about three
    times their bytes in flight): add in large batches."""
    _PARTS = ("_storage", "quantizer")

    def __init__(self, d, nlist, device=None, _quantizer=None):
        super().__init__(d, nlist, device, _quantizer)
        self._storage = FlatIPIndex(self.d, device=self.device.index)
        self.is_trained = False
        self._set_lists(torch.zeros(0, dtype=torch.int64, device=self.device))

    # -- attributes ------------------------------------------------------------------------------
    @property
    def ntotal(self):
        return self._storage.ntotal

    def _ids_device(self, start=0, n=None):
        n = self.ntotal - start if n is None else n
        out = torch.empty(n, dtype=torch.int64, device=self.device)
        if n:
            self._storage._call("ivr_index_get_ids", int(start), int(n), out)
        return out

    def _set_lists(self, row_list, off_host=None):
        """row_list: int64 CUDA tensor, the list of every stored row, ascending; off_host: its list_offsets when the caller has them."""
        self._row_list = row_list
        self._set_offsets(self._offsets(row_list) if off_host is None else off_host)
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
        self._train_quantizer(x, niter, seed, max_points_per_centroid, spherical)
        self.is_trained = True

    # -- adding ----------------------------------------------------------------------------------
    def add_with_ids(self, x, ids, normalize=False, *, _what="add_with_ids"):
        """Append rows under caller-chosen int64 labels (>= 0, duplicates allowed).  Each row goes to the list of its best centroid,
        decided on the bits that end up stored (after normalize).  The whole index is regrouped by list in every call: one pass over
        all stored rows (gather, a stable argsort of the list numbers, add_with_ids into the emptied storage) with about three times
        the index in flight, so add in large batches.  RuntimeError while untrained."""
        ids = self._new_ids(x, ids, _what)
        if len(ids) == 0:
            return
        with torch.cuda.device(self.device):
            t = _dev_f32(x, self.device)
            if normalize:
                t = t.clone()
                normalize_L2(t)
            lists = self._assign_device(t)
            new_ids = torch.from_numpy(np.ascontiguousarray(ids)).to(self.device)
            n_old = self._storage.ntotal
            if n_old:
                old = self._storage.gather_device(torch.arange(n_old, dtype=torch.int64, device=self.device))
                t = torch.cat([old, t])
                del old
                new_ids = torch.cat([self._ids_device(), new_ids])
                lists = torch.cat([self._row_list, lists])
            order, off = self._regroup(lists)
            t = t[order].contiguous()
            self._storage.reset()
            self._storage._add_device(t, False, np.ascontiguousarray(new_ids[order].cpu().numpy()))
            self._set_lists(lists[order].contiguous(), off)

    # -- search ----------------------------------------------------------------------------------
    def search_device(self, x, k, normalize=False, nprobe=None):
        """Device-resident search: CUDA tensors, no host synchronisation (unless x had to be staged).  nprobe (default: the
        attribute) is clipped to nlist; below nlist it is the k of the coarse search and so at most IVR_MAX_K."""
        t, k, staged = self._queries(x, k, "search")
        with torch.cuda.device(self.device):
            return self._scan(t, k, self._probe(t, nprobe, normalize)[1], normalize, staged)

    def search_preassigned(self, x, k, assign):
        """faiss search_preassigned: assign int64 [nq,p] (numpy or CUDA tensor) names the lists to scan for each query; -1 entries
        are skipped and a list named twice is scanned once.  ValueError for an entry >= nlist or < -1 (checked on the tensor, before
        any kernel of the scan is launched).  Returns (D, I) numpy arrays."""
        return to_numpy(self.search_preassigned_device(x, k, assign))

    def search_preassigned_device(self, x, k, assign, normalize=False):
        """search_preassigned returning CUDA tensors; the range check of assign synchronises once."""
        t, k, staged = self._queries(x, k, "search_preassigned")
        with torch.cuda.device(self.device):
            return self._scan(t, k, self._assign_arg(assign, t.shape[0], "search_preassigned"), normalize, staged)

    def _scan(self, t, k, assign, normalize, staged):
        """assign: int64 CUDA [nq,p], entries in [-1, nlist).  The kernel wants every row ascending (a repeated list is then adjacent)."""
        nq, p = assign.shape
        _staging.check_nq(nq)
        assign = self._ascending(assign)[0]
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
