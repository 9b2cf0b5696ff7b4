"""What the product-quantisation indexes (PQIndex: 256 centroids per slice, a byte per slice; PQFastScanIndex: 16 centroids, a nibble)
share: the codebooks and their device copy, the k-means training around the encoder's assignment, the decoder's gather, the numpy
definitions of the encoder and of the float tables, and the search surface over a subclass's tables.

A subclass sets `_KSUB` (centroids per slice) and `_ENCODE` (the encoder's entry point: contiguous float32 rows and codebooks in, uint8
[n, code_size] out), maps a code byte array to one centroid number per slice (`_slice_codes`), checks its own limits on M, and supplies
`compute_tables_device` and `search_tables_device`.
"""
import numpy as np
import torch

from . import _ffi, _kmeans, _staging
from ._coded import DecodableIndex
from ._faiss import METRIC_INNER_PRODUCT
from ._staging import dev_u8 as _dev_u8


# -- pure numpy definitions (no GPU) -------------------------------------------------------------------------------------------
def encode_ref(who, x, c):
    """pq_encode_ref / pqfs_encode_ref over the checked codebooks c [M,ksub,dsub]."""
    c = c.astype(np.float64)
    M, _, dsub = c.shape
    x = np.asarray(x, np.float64)
    if x.ndim != 2 or x.shape[1] != M * dsub:
        raise ValueError(f"{who}: x must be [n,{M * dsub}], got {x.shape}")
    xs = x.reshape(len(x), M, 1, dsub)
    dist = ((xs - c[None]) ** 2).sum(-1)
    return dist.argmin(-1).astype(np.uint8), dist


def tables_ref(who, q, c):
    """pq_tables_ref / pqfs_tables_ref over the checked codebooks c [M,ksub,dsub]."""
    c = c.astype(np.float64)
    M, _, dsub = c.shape
    q = np.asarray(q, np.float64)
    if q.ndim != 2 or q.shape[1] != M * dsub:
        raise ValueError(f"{who}: q must be [nq,{M * dsub}], got {q.shape}")
    return np.einsum("imt,mjt->imj", q.reshape(len(q), M, dsub), c)


class ProductQuantizerIndex(DecodableIndex):
    """Base of PQIndex and PQFastScanIndex.  Expects d and M on the instance before _setup."""
    _KSUB = 0
    _ENCODE = None

    def _setup(self, who, d, nbits, code_size, make_store):
        """What both constructors end with, after their own checks of nbits, the metric and M; make_store() makes the row store."""
        if self.d < 1 or self.d > 65536 or self.d % self.M != 0:
            raise ValueError(f"{who}: d={d} outside [1,65536] or not a multiple of M={self.M}")
        self.dsub = self.d // self.M
        self.code_size, self.nbits = code_size, nbits
        self.metric_type = METRIC_INNER_PRODUCT
        self.is_trained = False
        self._index = make_store()
        self.device = self._index.device
        self._centroids = np.zeros((self.M, self._KSUB, self.dsub), np.float32)
        self._cb_dev = None

    # -- attributes ------------------------------------------------------------------------------
    @property
    def centroids(self):
        """numpy float32 [M,ksub,dsub] (ksub = 256 for PQIndex, 16 for PQFastScanIndex): the codebooks.  Assignable while the index is
        empty, which makes it trained."""
        return self._centroids

    @centroids.setter
    def centroids(self, c):
        self._require_empty("centroids", "codebooks")
        c = np.asarray(c)
        if c.shape != self._centroids.shape:
            raise ValueError(f"centroids expects [{self.M},{self._KSUB},{self.dsub}], got {c.shape}")
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
        """t: contiguous float32 CUDA tensor [n,d] -> codes uint8 CUDA [n,code_size] under the codebooks cb (default: the index's)."""
        codes = torch.empty((t.shape[0], self.code_size), dtype=torch.uint8, device=self.device)
        _ffi.call(self._ENCODE, _ffi.CTX, t, t.shape[0], self.d, self._codebooks_device() if cb is None else cb, self.M, codes,
                  device=self.device)
        return codes

    def sa_decode_device(self, codes):
        """float32 CUDA [n,d]: row i is the concatenation of centroids[m, code[i,m]] over m (a gather, no arithmetic)."""
        self._require_trained("sa_decode")
        c = self._slice_codes(_dev_u8(codes, self.code_size, self.device, "sa_decode"))
        m = torch.arange(self.M, device=self.device).expand(c.shape[0], -1)
        return self._codebooks_device()[m, c].reshape(c.shape[0], self.d)

    # -- training --------------------------------------------------------------------------------
    def train(self, x, niter=25, seed=1234, max_points_per_centroid=256):
        """Make the M codebooks of ksub centroids (256 for PQIndex, 16 for PQFastScanIndex) by k-means on x [n,d], n >= ksub
        (ValueError otherwise):
          sample   _kmeans.kmeans_sample(n, ksub, max_points_per_centroid, seed): one sample serves all slices, and the initial
                   codebook of slice m is slice m of its first ksub rows
          iterate  niter times: assign every sampled row's slices with the encoder (ivr_pq_encode / ivr_pqfs_encode: equal distances
                   pick the lower centroid), order the rows of each slice by code (stable), take the mean of every run
                   (ivr_segment_mean with spherical=False: fixed summation order, so a seed gives the same bits every time), repair
                   empty clusters (split_empty_clusters, per slice).  The loop's shared halves are those of _kmeans.py."""
        ksub = self._KSUB
        self._require_empty("train", "codebooks")
        _staging.check_rows(x, self.d, "train")
        n = len(x)
        if n < ksub:
            raise ValueError(f"train: {n} training rows for {ksub} centroids per slice")
        niter = _kmeans.check_niter(niter)
        with torch.cuda.device(self.device):
            xs = _kmeans.sample_rows(x, ksub, max_points_per_centroid, seed, self.device)
            cent = xs[:ksub].reshape(ksub, self.M, self.dsub).permute(1, 0, 2).contiguous()
            for _ in range(niter):
                cent = self._kmeans_step(xs, cent)
            self._set_centroids(cent.cpu().numpy(), cent)

    def _kmeans_step(self, xs, cent):
        a = self._slice_codes(self._encode_device(xs, cent)).t().contiguous()     # [M, ns]
        order = torch.argsort(a, dim=1, stable=True)        # one batched sort for all slices
        out = torch.empty_like(cent)
        counts = [_kmeans.segment_means(xs[:, m * self.dsub:(m + 1) * self.dsub], a[m], self._KSUB, out[m], order=order[m])
                  for m in range(self.M)]
        return _kmeans.repair_empty_clusters(out, torch.stack(counts).cpu().numpy())

    # -- FAISS surface ---------------------------------------------------------------------------
    def search_tables(self, *tables_k):
        """search_tables_device(*tables, k) as numpy arrays."""
        D, I = self.search_tables_device(*tables_k)
        return D.cpu().numpy(), I.cpu().numpy()

    def search_device(self, x, k):
        """search returning CUDA tensors: search_tables_device over the tables compute_tables_device(x) returns, bit for bit."""
        self._require_trained("search")
        k = _staging.check_k(k, _ffi.IVR_MAX_K)
        t = self.compute_tables_device(x)
        return self.search_tables_device(*(t if isinstance(t, tuple) else (t,)), k)
