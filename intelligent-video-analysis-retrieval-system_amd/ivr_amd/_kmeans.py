"""The k-means of the project: the coarse quantizer of the inverted-file indexes (_ivf.py) and the codebooks of PQIndex (pq.py) run the
same loop and differ only in who assigns a row to a centroid.  A trainer stages its sample (`sample_rows`), and per iteration assigns
the rows itself, takes the means (`segment_means`: the ivr_segment_mean kernel of csrc/search_ivf.hip, fixed summation order, so a seed
gives the same bits every time), brings the counts to the host once and repairs what came out empty (`repair_empty_clusters`).
"""
import numpy as np
import torch

from . import _ffi
from ._staging import dev_f32 as _dev_f32

_SPLIT_EPS = 1.0 / 1024.0


def kmeans_sample(n, nlist, max_points_per_centroid=256, seed=1234):
    """The rows k-means trains on, as indices into the n training rows: the first min(n, max_points_per_centroid * nlist) entries of
    numpy.random.RandomState(seed).permutation(n).  The first nlist of them are the initial centroids."""
    perm = np.random.RandomState(seed).permutation(n).astype(np.int64)
    return perm[:min(n, int(max_points_per_centroid) * int(nlist))]


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


def check_niter(niter):
    niter = int(niter)
    if niter < 0:
        raise ValueError(f"train: niter={niter} < 0")
    return niter


def sample_rows(x, k, max_points_per_centroid, seed, device):
    """Rows kmeans_sample(len(x), k, ...) of x as a contiguous float32 CUDA tensor; of a host x only the sample travels to the device."""
    sample = torch.from_numpy(kmeans_sample(len(x), k, max_points_per_centroid, seed))
    if isinstance(x, torch.Tensor) and x.is_cuda:
        return _dev_f32(x, device)[sample.to(device)].contiguous()
    return _dev_f32(x[sample.numpy()] if isinstance(x, np.ndarray) else x[sample], device)


def segment_means(x, a, k, out, spherical=False, order=None):
    """out[c] = the mean of the rows of x (float32 CUDA [n,dd], any strides) assigned to cluster c by a (int64 CUDA [n], in [0, k)),
    summed in ascending row order; a NaN row for an empty cluster, unit norm with spherical.  order: argsort(a, stable=True) when the
    caller has it already.  out: contiguous float32 CUDA [k,dd].  Returns the rows per cluster (int64 CUDA [k])."""
    rows = x[torch.argsort(a, stable=True) if order is None else order].contiguous()
    counts = torch.bincount(a, minlength=k)
    off = torch.zeros(k + 1, dtype=torch.int64, device=x.device)
    torch.cumsum(counts, 0, out=off[1:])
    _ffi.call("ivr_segment_mean", _ffi.CTX, rows, len(rows), off, k, rows.shape[1], bool(spherical), out, device=x.device)
    return counts


def repair_empty_clusters(cent, counts, spherical=False):
    """cent: float32 CUDA [k,dd] or a stack [M,k,dd] of segment_means results, counts: their counts on the host (int64 numpy [k] or
    [M,k]).  Nothing empty: cent itself.  Otherwise split_empty_clusters runs on the host on every set with an empty cluster (with
    spherical the touched centroids are renormalised: float64 norm, float32 division) and the repaired copy returns to the device."""
    if not (counts == 0).any():
        return cent
    c = cent.cpu().numpy()
    c3, n2 = c.reshape((-1,) + c.shape[-2:]), counts.reshape(-1, counts.shape[-1])
    for m in np.flatnonzero((n2 == 0).any(axis=1)):
        touched = split_empty_clusters(c3[m], n2[m])
        for i in touched if spherical else ():
            nrm = np.float32(np.sqrt(np.dot(c3[m, i].astype(np.float64), c3[m, i].astype(np.float64))))
            if nrm > 0:
                c3[m, i] /= nrm
    return torch.from_numpy(c).to(cent.device)
