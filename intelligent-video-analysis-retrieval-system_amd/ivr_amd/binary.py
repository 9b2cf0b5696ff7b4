"""FAISS-shaped binary indexes resident in MI355X HBM: IndexBinaryFlat (exact Hamming top-k) and IndexLSH (sign bits of a random
rotation, ranked by Hamming distance).

Stands in for the `faiss.IndexLSH(dimension, 256)` the reference accepts in `_create_index` (`core.py:1198-1230`).  A row is stored
as `nbits` sign bits (32 bytes at 256 bits), the search is popcount(xor) over the dense code array, and the top k is found by
counting, exactly: distances ascending, equal distances rank the LOWER ROW first, unused slots hold the largest int32 and -1 as
faiss's integer heap leaves them.  The encoder (float32 MFMA projection + sign packing) and every search pass are HIP kernels of
libivr_hip.so (csrc/search_binary.hip); torch stages arrays and sorts the training projections.

Codes are uint8 [n, code_size] in faiss order: bit j of a code is bit j & 7 of byte j >> 3, i.e.
numpy.packbits(bits, axis=1, bitorder="little").

faiss's own random stream cannot be reproduced here, so the default rotation is defined by `lsh_rotation` (numpy, seeded); a matrix
exported from a real faiss index can be assigned to `IndexLSH.rrot` while the index is empty and then reproduces that index's codes.
"""
import numpy as np
import torch

from . import _ffi, _staging
from ._coded import CodedIndex, _CodeStore, cat_chunks
from ._faiss import METRIC_L2, search_numpy
from ._staging import dev_u8 as _dev_u8


def lsh_rotation(d, nbits, seed=5):
    """The default rotation of IndexLSH, float32 [nbits, d], pure numpy: with m = max(d, nbits), A = RandomState(seed)
    .standard_normal((m, m)) in float64, Q R = A and the sign fixed so that diag(R) > 0, it is Q[:nbits, :d].  Its rows are
    orthonormal when nbits <= d and its columns when nbits > d (the shape of faiss's RandomRotationMatrix)."""
    d, nbits = int(d), int(nbits)
    if d < 1 or nbits < 1:
        raise ValueError(f"lsh_rotation: d={d} nbits={nbits}")
    m = max(d, nbits)
    a = np.random.RandomState(int(seed)).standard_normal((m, m))
    q, r = np.linalg.qr(a)
    q *= np.sign(np.diag(r))
    return np.ascontiguousarray(q[:nbits, :d], dtype=np.float32)


class BinaryFlatIndex(_ffi.Handle):
    """Exact Hamming-distance index over binary codes (FAISS IndexBinaryFlat contract) on one GPU.  d_bits is the code length in
    bits and must be a multiple of 8, as in faiss; a code is d_bits / 8 bytes."""
    _DESTROY, _abi = "ivr_bin_index_destroy", "ivr_bin_index"
    _add_device, _codes_device = _CodeStore._add_device, _CodeStore._codes_device     # the handle itself is opened at once, below

    def __init__(self, d_bits, device=None):
        d_bits = int(d_bits)
        if d_bits < 8 or d_bits % 8 != 0:
            raise ValueError(f"BinaryFlatIndex: d={d_bits} must be a positive multiple of 8")
        self.d = d_bits
        self.code_size = d_bits // 8
        self.is_trained = True
        self._open("ivr_bin_index_create", device, self.d, 0)

    @property
    def ntotal(self):
        return int(_ffi.call("ivr_bin_index_ntotal", self._h))

    def train(self, x):
        return None

    def add(self, codes):
        """Append codes: uint8 [n, d/8], a numpy array or a torch tensor."""
        self._add_device(_dev_u8(codes, self.code_size, self.device, "add"))

    def search(self, codes, k):
        """(D, I) numpy arrays: D int32 [nq,k] Hamming distances ascending, I int64 row numbers; equal distances rank the lower row
        first; unused slots (2147483647, -1)."""
        return search_numpy(self, codes, k)

    def search_device(self, codes, k):
        """search returning CUDA tensors; no host synchronisation unless `codes` had to be staged."""
        t = _dev_u8(codes, self.code_size, self.device, "search")
        k = _staging.check_k(k, _ffi.IVR_MAX_K)
        nq = t.shape[0]
        _staging.check_nq(nq)
        D, I = _staging.alloc_DI(nq, k, self.device, torch.int32)
        self._call("ivr_bin_index_search", t, nq, k, D, I)
        _staging.sync_if_staged(_staging.is_staged(t, codes), self.device)
        return D, I

    def reconstruct_n(self, start=0, n=None):
        """The stored codes of rows [start, start + n) as numpy uint8 [n, d/8]."""
        return self._codes_device(start, n).cpu().numpy()

    def reset(self):
        self._call("ivr_bin_index_reset")


def IndexBinaryFlat(d):
    """faiss.IndexBinaryFlat(d) drop-in: d is the code length in bits, a multiple of 8."""
    return BinaryFlatIndex(d)


class IndexLSH(CodedIndex):
    """faiss.IndexLSH(d, nbits, rotate_data, train_thresholds) on one GPU: bit j of a row's code is the sign of
    <x, rrot[j]> - thresholds[j] (>= 0 sets the bit), and search ranks the stored codes by Hamming distance to the query's code.

    search(x, k) returns (D float32, I int64): the Hamming distance as a float, ascending, equal distances rank the lower row first,
    unused slots (2147483648.0, -1).  rotate_data=False takes the first nbits coordinates instead of a rotation and needs
    nbits <= d.  train_thresholds=True makes train(x) set thresholds[j] to the median of projection j over x (element n // 2 of the
    sorted column); add() raises RuntimeError until then."""

    def __init__(self, d, nbits, rotate_data=True, train_thresholds=False, seed=5, device=None):
        self.d, self.nbits = int(d), int(nbits)
        if self.d < 1 or self.d > 65536 or self.nbits < 1 or self.nbits > 2048:
            raise ValueError(f"IndexLSH: d={d} outside [1,65536] or nbits={nbits} outside [1,2048]")
        self.rotate_data, self.train_thresholds = bool(rotate_data), bool(train_thresholds)
        if not self.rotate_data and self.nbits > self.d:
            raise ValueError(f"IndexLSH: rotate_data=False needs nbits={self.nbits} <= d={self.d}")
        self.code_size = (self.nbits + 7) // 8
        self.metric_type = METRIC_L2
        self.is_trained = not self.train_thresholds
        self._index = BinaryFlatIndex(8 * self.code_size, device=device)
        self.device = self._index.device
        self._rrot = lsh_rotation(self.d, self.nbits, seed)
        self._thresholds = np.zeros(self.nbits, np.float32)
        self._rot_dev = self._thr_dev = None

    # -- attributes ------------------------------------------------------------------------------
    @property
    def rrot(self):
        """numpy float32 [nbits, d]: row j is the direction of bit j.  Assignable while the index is empty."""
        return self._rrot

    @rrot.setter
    def rrot(self, m):
        self._require_empty("rrot", "rotation")
        m = np.asarray(m)
        if m.shape != (self.nbits, self.d):
            raise ValueError(f"rrot expects [{self.nbits},{self.d}], got {m.shape}")
        self._rrot = np.ascontiguousarray(m, dtype=np.float32)
        self._rot_dev = None

    @property
    def thresholds(self):
        """numpy float32 [nbits]; applied only when train_thresholds is set.  Assignable while the index is empty."""
        return self._thresholds

    @thresholds.setter
    def thresholds(self, t):
        self._require_empty("thresholds", "thresholds")
        t = np.asarray(t)
        if t.shape != (self.nbits,):
            raise ValueError(f"thresholds expects [{self.nbits}], got {t.shape}")
        self._thresholds = np.ascontiguousarray(t, dtype=np.float32)
        self._thr_dev = None

    # -- encoding --------------------------------------------------------------------------------
    def _encode_device(self, t, proj=None, use_thresholds=True):
        """t: contiguous float32 CUDA tensor [n,d] -> codes uint8 CUDA [n,code_size].  proj: float32 CUDA [n,nbits] that receives
        the projections <x, rrot[j]> (before the threshold), or None."""
        n = t.shape[0]
        codes = torch.empty((n, self.code_size), dtype=torch.uint8, device=self.device)
        rot = thr = None
        if self.rotate_data:
            if self._rot_dev is None:
                self._rot_dev = torch.from_numpy(self._rrot).to(self.device)
            rot = self._rot_dev
        if self.train_thresholds and use_thresholds:
            if self._thr_dev is None:
                self._thr_dev = torch.from_numpy(self._thresholds).to(self.device)
            thr = self._thr_dev
        _ffi.call("ivr_sign_encode", _ffi.CTX, t, n, self.d, rot, thr, self.nbits, codes, proj, device=self.device)
        return codes

    def _encode_chunks(self, x, want_proj, use_thresholds=True):
        """(codes, proj) of every chunk of x, from one launch per chunk."""
        def one(t):
            proj = torch.empty((t.shape[0], self.nbits), dtype=torch.float32, device=self.device) if want_proj else None
            return self._encode_device(t, proj, use_thresholds), proj
        return self._per_chunk(x, one)

    def sa_encode_device(self, x, want_proj=False):
        """(codes uint8 CUDA [n,code_size], proj float32 CUDA [n,nbits] or None): proj is the encoder's own float32 projection
        <x, rrot[j]> (before the threshold) of the same launch that produced the codes.  No host synchronisation when x is a
        contiguous float32 CUDA tensor on the index's device."""
        parts = self._encode_chunks(self._rows(x, "sa_encode"), want_proj)
        return cat_chunks([p[0] for p in parts]), cat_chunks([p[1] for p in parts]) if want_proj else None

    def sa_encode(self, x):
        """The codes of x, numpy uint8 [n, code_size]."""
        return self.sa_encode_device(x)[0].cpu().numpy()

    def train(self, x):
        """Nothing unless train_thresholds is set; then thresholds[j] = element n // 2 of the sorted projections of x on rrot[j]
        (faiss's median rule), computed from the encoder's own float32 projections."""
        if not self.train_thresholds:
            return
        self._require_empty("train", "thresholds")
        x = self._rows(x, "train")
        n = len(x)
        if n < 1:
            raise ValueError("train: no training rows")
        proj = cat_chunks([p[1] for p in self._encode_chunks(x, True, use_thresholds=False)])
        self._thresholds = torch.sort(proj, dim=0).values[n // 2].contiguous().cpu().numpy()
        self._thr_dev = None
        self.is_trained = True

    # -- FAISS surface ---------------------------------------------------------------------------
    def search_device(self, x, k):
        """search returning CUDA tensors: D float32 Hamming distances ascending, I int64 rows; unused slots (2147483648.0, -1)."""
        self._require_trained("search")
        k = _staging.check_k(k, _ffi.IVR_MAX_K)
        codes = self.sa_encode_device(x)[0]
        D, I = self._index.search_device(codes, k)
        return D.to(torch.float32), I
