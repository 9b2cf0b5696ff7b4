"""Staging and checking of what callers hand to an index: rows, queries, k, integer tables.

Host arrays are staged through torch tensors on the index's device; a tensor that is already there, contiguous and of the right
dtype is used in place.  A staged copy is a temporary that must outlive the kernels reading it: whoever stages asks is_staged and
ends with sync_if_staged.  Every check raises the ValueError text the index classes share.
"""
import numpy as np
import torch


# -- staging -------------------------------------------------------------------------------------------------------------------
def dev_f32(x, device):
    """numpy / torch -> contiguous float32 tensor on `device` (a view when already there)."""
    if isinstance(x, np.ndarray):
        x = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))
    if not isinstance(x, torch.Tensor):
        raise ValueError("expected a numpy array or a torch tensor")
    return x.to(device=device, dtype=torch.float32, non_blocking=False).contiguous()


def dev_u8(x, width, device, what):
    """numpy / torch uint8 [n, width] (or one code [width]) -> contiguous uint8 tensor on `device` (a view when already there)."""
    if isinstance(x, np.ndarray):
        if x.dtype != np.uint8:
            raise ValueError(f"{what}: codes must be uint8, got {x.dtype}")
        x = torch.from_numpy(np.ascontiguousarray(x))
    if not isinstance(x, torch.Tensor) or x.dtype != torch.uint8:
        raise ValueError(f"{what}: codes must be a uint8 numpy array or torch tensor")
    if x.dim() == 1 and width and x.shape[0] == width:
        x = x.reshape(1, -1)
    if x.dim() != 2 or x.shape[1] != width:
        raise ValueError(f"{what} expects uint8 [n,{width}], got {tuple(x.shape)}")
    return x.to(device=device).contiguous()


def as_rows(x, tensors_too=True):
    """The 1-D -> [1,d] rule of the query arguments: anything but a tensor goes through numpy.asarray, and a single vector becomes
    one row (a 1-D tensor only with tensors_too)."""
    q = x if isinstance(x, torch.Tensor) else np.asarray(x)
    if q.ndim == 1 and (tensors_too or isinstance(q, np.ndarray)):
        q = q.reshape(1, -1)
    return q


def is_staged(t, x):
    """Whether the device tensor t is a temporary copy of the caller's x (a host array, a converted or compacted tensor) and not
    x's own storage."""
    return not (isinstance(x, torch.Tensor) and t.data_ptr() == x.data_ptr())


def sync_if_staged(staged, device=None):
    """The staging copy must outlive the kernels: wait for the current stream (of `device`) when there was a copy."""
    if staged:
        torch.cuda.current_stream(device).synchronize()


def queries_f32(x, d, device):
    """Queries [nq,d] -> (contiguous float32 tensor on `device`, is_staged)."""
    t = dev_f32(x, device)
    if t.dim() != 2 or t.shape[1] != d:
        raise ValueError(f"Query dimension ({tuple(t.shape)}) != index dimension ({d})")
    return t, is_staged(t, x)


# -- checks --------------------------------------------------------------------------------------------------------------------
def check_rows(x, d, what):
    """x must be a numpy array or torch tensor [n,d]."""
    if not isinstance(x, (np.ndarray, torch.Tensor)) or x.ndim != 2 or x.shape[1] != d:
        raise ValueError(f"{what} expects [n,{d}], got {tuple(getattr(x, 'shape', ()))}")


def check_k(k, kmax):
    k = int(k)
    if k < 1 or k > kmax:
        raise ValueError(f"k={k} outside [1,{kmax}]")
    return k


def check_nq(nq, what="search"):
    if nq < 1:
        raise ValueError(f"{what}: no queries")


def check_window(L, T, lmax, what):
    """The window length of a clip search over T frames: an integer in [1, lmax], at most T."""
    if isinstance(L, bool) or not isinstance(L, (int, np.integer)):
        raise ValueError(f"{what}: L must be an integer, got {type(L).__name__}")
    L = int(L)
    if L < 1 or L > lmax:
        raise ValueError(f"{what}: L={L} outside [1,{lmax}]")
    if T < L:
        raise ValueError(f"{what}: T={T} frames < L={L}")
    return L


def chains_f32(x, d, device, mmax, what):
    """The chains of an event search: [B,m,d], or [m,d] for one chain, 1 <= m <= mmax -> (contiguous float32 tensor [B*m,d] on
    `device`, is_staged, B, m)."""
    t = dev_f32(x, device)
    if t.dim() == 2:
        t = t.unsqueeze(0)
    if t.dim() != 3 or t.shape[2] != d:
        raise ValueError(f"{what}: events must be [B,m,{d}] or [m,{d}], got {tuple(getattr(x, 'shape', ()))}")
    B, m = int(t.shape[0]), int(t.shape[1])
    if B < 1:
        raise ValueError(f"{what}: no chains")
    if m < 1 or m > mmax:
        raise ValueError(f"{what}: m={m} events outside [1,{mmax}]")
    return t.reshape(B * m, d), is_staged(t, x), B, m


def check_gaps(min_gap, max_gap, gmax, what):
    """The gaps of an event search: integers with 1 <= min_gap <= max_gap <= gmax -> (int min_gap, int max_gap)."""
    for name, g in (("min_gap", min_gap), ("max_gap", max_gap)):
        if isinstance(g, bool) or not isinstance(g, (int, np.integer)):
            raise ValueError(f"{what}: {name} must be an integer, got {type(g).__name__}")
    if not 1 <= min_gap <= max_gap <= gmax:
        raise ValueError(f"{what}: gaps [{min_gap},{max_gap}] outside 1 <= min_gap <= max_gap <= {gmax}")
    return int(min_gap), int(max_gap)


def check_dbscan(eps, min_samples, what):
    """The parameters of a DBSCAN call: eps a number >= 0 (not NaN), min_samples an integer >= 1 -> (float eps, int min_samples)."""
    if isinstance(eps, bool) or not isinstance(eps, (int, float, np.integer, np.floating)):
        raise ValueError(f"{what}: eps must be a number, got {type(eps).__name__}")
    eps = float(eps)
    if not eps >= 0.0:
        raise ValueError(f"{what}: eps={eps} is negative or NaN")
    if isinstance(min_samples, bool) or not isinstance(min_samples, (int, np.integer)):
        raise ValueError(f"{what}: min_samples must be an integer, got {type(min_samples).__name__}")
    if min_samples < 1 or min_samples >= 2**31:
        raise ValueError(f"{what}: min_samples={min_samples} outside [1,2^31)")
    return eps, int(min_samples)


def check_knn(k, threshold, kmax, what):
    """The parameters of a neighbour-graph call: k an integer in [1, kmax], threshold a number that is not NaN, or None -> (int k,
    float threshold, -inf for None)."""
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)):
        raise ValueError(f"{what}: k must be an integer, got {type(k).__name__}")
    if k < 1 or k > kmax:
        raise ValueError(f"{what}: k={k} outside [1,{kmax}]")
    if threshold is None:
        return int(k), float("-inf")
    if isinstance(threshold, bool) or not isinstance(threshold, (int, float, np.integer, np.floating)):
        raise ValueError(f"{what}: threshold must be a number, got {type(threshold).__name__}")
    threshold = float(threshold)
    if threshold != threshold:
        raise ValueError(f"{what}: threshold={threshold} is NaN")
    return int(k), threshold


def _is_number(v):
    return not isinstance(v, bool) and isinstance(v, (int, float, np.integer, np.floating))


def check_tags(C, scale, top, min_prob, cmax, tmax, what):
    """The parameters of a tagging call: C labels in [1, cmax], scale a positive finite number, top an integer in [1, tmax], min_prob a
    number that is not NaN -> (float scale and float min_prob, both rounded to float32, int top)."""
    if C < 1 or C > cmax:
        raise ValueError(f"{what}: C={C} labels outside [1,{cmax}]")
    if isinstance(top, bool) or not isinstance(top, (int, np.integer)):
        raise ValueError(f"{what}: top must be an integer, got {type(top).__name__}")
    if top < 1 or top > tmax:
        raise ValueError(f"{what}: top={top} outside [1,{tmax}]")
    if not _is_number(scale):
        raise ValueError(f"{what}: scale must be a number, got {type(scale).__name__}")
    scale = float(np.float32(scale))
    if not (scale > 0.0 and scale != float("inf")):
        raise ValueError(f"{what}: scale={scale} is not a positive finite number")
    if not _is_number(min_prob):
        raise ValueError(f"{what}: min_prob must be a number, got {type(min_prob).__name__}")
    min_prob = float(np.float32(min_prob))
    if min_prob != min_prob:
        raise ValueError(f"{what}: min_prob={min_prob} is NaN")
    return scale, int(top), min_prob


def check_tag_segments(g, rank, gmax, what):
    """top_labels an integer in [1, gmax], rank "mass" or "votes" -> (int g, the library's rank number)."""
    if isinstance(g, bool) or not isinstance(g, (int, np.integer)):
        raise ValueError(f"{what}: top_labels must be an integer, got {type(g).__name__}")
    if g < 1 or g > gmax:
        raise ValueError(f"{what}: top_labels={g} outside [1,{gmax}]")
    from ._ffi import IVR_TAG_RANK
    if rank not in IVR_TAG_RANK:
        raise ValueError(f"{what}: rank must be 'mass' or 'votes', got {rank!r}")
    return int(g), IVR_TAG_RANK[rank]


def check_row_range(row0, row1, n, what):
    """A row range [row0, row1) of n rows, row1 None = n: integers with 0 <= row0 <= row1 -> (int row0, int row1 clipped to n)."""
    row1 = n if row1 is None else row1
    for name, r in (("row0", row0), ("row1", row1)):
        if isinstance(r, bool) or not isinstance(r, (int, np.integer)):
            raise ValueError(f"{what}: {name} must be an integer, got {type(r).__name__}")
    if not 0 <= row0 <= row1:
        raise ValueError(f"{what}: rows [{row0},{row1}) are no range")
    return int(row0), int(min(row1, max(n, row0)))


def alloc_DI(nq, k, device, dtype=torch.float32):
    """The (D, I) pair of a search: D `dtype` [nq,k], I int64 [nq,k]."""
    return torch.empty((nq, k), dtype=dtype, device=device), torch.empty((nq, k), dtype=torch.int64, device=device)


def alloc_DI_paths(nq, k, m, device):
    """The (D, I) pair of an event search: D float32 [nq,k], I int64 [nq,k,m] (one row per event of the path)."""
    return torch.empty((nq, k), dtype=torch.float32, device=device), torch.empty((nq, k, m), dtype=torch.int64, device=device)


# -- caller-supplied integer tables ----------------------------------------------------------------------------------------------
def int_tensor(a, name, verb="be", np_dtype=None):
    """An integer numpy array or torch tensor -> torch tensor (where it lives; a numpy array as np_dtype when that is given).
    name: "who: the table"."""
    if isinstance(a, np.ndarray):
        if not np.issubdtype(a.dtype, np.integer):
            raise ValueError(f"{name} must {verb} integers, got {a.dtype}")
        a = torch.from_numpy(np.ascontiguousarray(a, dtype=np_dtype))
    if not isinstance(a, torch.Tensor) or a.dtype.is_floating_point or a.dtype.is_complex or a.dtype == torch.bool:
        raise ValueError(f"{name} must be an integer numpy array or torch tensor")
    return a


def segments(seg_off, device, what):
    """The segment argument of a library call: offsets (integers [nseg+1], nseg >= 1, ascending) or None -> (contiguous int64
    tensor on `device`, is_staged, nseg), (None, False, 0) for None.  The order is checked on a host array; a CUDA tensor is taken
    as it is (no host sync)."""
    if seg_off is None:
        return None, False, 0
    t = int_tensor(seg_off, f"{what}: seg_off")
    if t.dim() != 1 or t.shape[0] < 2:
        raise ValueError(f"{what}: seg_off must be [nseg+1] with nseg >= 1, got {tuple(t.shape)}")
    if not t.is_cuda and t.shape[0] > 1:
        bad = torch.nonzero(t[1:] < t[:-1])
        if len(bad):
            i = int(bad[0])
            raise ValueError(f"{what}: seg_off must ascend, got seg_off[{i}]={int(t[i])} > seg_off[{i + 1}]={int(t[i + 1])}")
    d = t.to(device=device, dtype=torch.int64).contiguous()
    return d, is_staged(d, seg_off), len(d) - 1


def segment_bounds(n, seg_off):
    """The definition of the segments in numpy: (lo, hi) int64 [n], the run [lo, hi) of seg_off that holds row j, clipped to [0, n);
    the empty range lo == hi == j + 1 for a row outside every run; [0, n) for every row without seg_off.  lo alone is the start array
    of DBSCAN: it ascends with the row, and lo[j] <= j exactly for the rows inside a segment."""
    j = np.arange(n, dtype=np.int64)
    if seg_off is None:
        return np.zeros(n, np.int64), np.full(n, n, np.int64)
    off = np.asarray(seg_off).astype(np.int64).reshape(-1)
    s = np.searchsorted(off, j, side="right") - 1                  # the last offset <= j: with empty segments the run that holds j
    inside = (s >= 0) & (s < len(off) - 1)
    s = np.clip(s, 0, len(off) - 2)
    return np.where(inside, np.maximum(off[s], 0), j + 1), np.where(inside, np.minimum(off[s + 1], n), j + 1)


def check_entries(t, n, name):
    """Every entry of the device tensor t must lie in [-1, n): checked on the tensor (one host sync) before anything is launched."""
    if bool(((t >= n) | (t < -1)).any().item()):
        raise ValueError(f"{name} must lie in [-1, {n})")


def entry_table(entries, nq, max_cols, what):
    """The entries of a graph walk: integers [nq, 1..max_cols] -> numpy int32, clipped to [-1, 2^31) (rows outside the index are
    skipped by the walk itself)."""
    e = np.asarray(entries)
    if not np.issubdtype(e.dtype, np.integer) or e.ndim != 2 or e.shape[0] != nq or not 1 <= e.shape[1] <= max_cols:
        raise ValueError(f"{what}: entries must be integers [{nq},1..{max_cols}]")
    return np.ascontiguousarray(e.clip(-1, 2**31 - 1), dtype=np.int32)
