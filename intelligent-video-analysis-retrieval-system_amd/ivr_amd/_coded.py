"""What the code-based indexes (IndexLSH, PQIndex, SQIndex, PQFastScanIndex) share: rows are encoded on the device, only their codes
are stored, and a search scans the codes.

A subclass supplies `_encode_device(t, ...)` (contiguous float32 CUDA rows -> uint8 CUDA codes), its trained state (`is_trained` and
the tables behind it, refused while rows are stored: `_require_empty`), `search_device`, and in `_index` a store of code rows with
`ntotal`, `_add_device(codes)`, `_codes_device(start, n)`, `reset()` and `close()`: a `_CodeStore` below (the handle of one of the
library's row stores, csrc/search_coded.h), or a `BinaryFlatIndex`, which takes its adding and reading from it.
`DecodableIndex` adds the decode half for the codes that stand for a row (`sa_decode_device` is the subclass's).
"""
import numpy as np
import torch

from . import _ffi, _staging
from ._faiss import search_numpy

ENCODE_CHUNK = 1 << 18        # rows of a host array staged per encoder launch


class _CodeStore(_ffi.Handle):
    """The code rows of a coded index behind one family of the ABI (`abi`_create, _add, _get_codes, _reset, _ntotal, _destroy):
    uint8 [n, code_size] in, the same bytes out.  The library handle is made by the first call that needs it, `abi`_create(ctx,
    *create_args, &handle), so that an index can be made and refuse untrained use where there is no GPU.  owner: the index class, for
    the message of a closed index."""

    def __init__(self, abi, create_args, code_size, owner, device):
        self._abi, self._create_args, self.code_size, self._owner = abi, create_args, code_size, owner
        self._DESTROY = abi + "_destroy"
        self.device = torch.device("cuda", int(device) if device is not None else
                                   torch.cuda.current_device() if torch.cuda.is_available() else 0)
        self._closed = False

    def _call(self, name, *args):
        if self._h is None:
            if self._closed:
                raise RuntimeError(f"{self._owner}: the index is closed")
            self._open(self._abi + "_create", self.device.index, *self._create_args)
        return super()._call(name, *args)

    def close(self):
        self._closed = True
        super().close()

    @property
    def ntotal(self):
        return 0 if self._h is None else int(_ffi.call(self._abi + "_ntotal", self._h))

    def _add_device(self, codes):
        self._call(self._abi + "_add", codes, codes.shape[0])
        torch.cuda.current_stream(self.device).synchronize()  # `codes` may be a temporary staging copy

    def _codes_device(self, start=0, n=None):
        start = int(start)
        n = self.ntotal - start if n is None else int(n)
        if start < 0 or n < 0 or start + n > self.ntotal:
            raise ValueError(f"reconstruct_n: rows [{start},{start + n}) outside [0,{self.ntotal})")
        out = torch.empty((n, self.code_size), dtype=torch.uint8, device=self.device)
        if n:
            self._call(self._abi + "_get_codes", start, n, out)
        return out

    def reset(self):
        if self._h is not None:
            self._call(self._abi + "_reset")


class CodedIndex:
    """Base of the indexes that store codes of their rows.  Expects d, device, is_trained and _index on the instance."""

    # -- attributes ------------------------------------------------------------------------------
    @property
    def ntotal(self):
        return self._index.ntotal

    @property
    def codes(self):
        """The stored codes, numpy uint8 [ntotal, code_size]."""
        return self._index._codes_device().cpu().numpy()

    def _require_trained(self, what):
        if not self.is_trained:
            raise RuntimeError(f"{what}: the index is not trained")

    def _require_empty(self, what, noun):
        """Refuse to replace the table (`noun`) that the stored rows were encoded with."""
        if self.ntotal:
            raise RuntimeError(f"{what}: the index holds {self.ntotal} rows encoded with the current {noun}")

    # -- encoding --------------------------------------------------------------------------------
    def _rows(self, x, what):
        if isinstance(x, np.ndarray) and x.ndim == 1:
            x = x.reshape(1, -1)
        _staging.check_rows(x, self.d, what)
        return x

    def _chunks(self, x):
        """x as contiguous float32 CUDA tensors: a CUDA tensor whole, a host array in blocks of ENCODE_CHUNK rows."""
        if isinstance(x, torch.Tensor) and x.is_cuda:
            yield _staging.dev_f32(x, self.device)
            return
        for i in range(0, max(len(x), 1), ENCODE_CHUNK):
            yield _staging.dev_f32(x[i:i + ENCODE_CHUNK], self.device)

    def _per_chunk(self, x, fn):
        """[fn(t) for every chunk t of x]; a staged chunk is kept until its kernels have run."""
        out = []
        for t in self._chunks(x):
            out.append(fn(t))
            _staging.sync_if_staged(_staging.is_staged(t, x), self.device)
        return out

    # -- FAISS surface ---------------------------------------------------------------------------
    def add(self, x):
        """Append rows: float32 [n,d], numpy or torch; only their codes are kept.  RuntimeError while untrained."""
        self._require_trained("add")
        x = self._rows(x, "add")
        for t in self._chunks(x):
            if t.shape[0]:
                self._index._add_device(self._encode_device(t))

    def search(self, x, k):
        """(D, I) numpy arrays of search_device(x, k)."""
        return search_numpy(self, x, k)

    def reset(self):
        """Drop the rows; what the index was trained to stays."""
        self._index.reset()

    def close(self):
        x = getattr(self, "_index", None)
        if x is not None:
            x.close()


def cat_chunks(parts):
    return parts[0] if len(parts) == 1 else torch.cat(parts)


class DecodableIndex(CodedIndex):
    """A CodedIndex whose codes stand for a row: sa_decode_device(codes) is the subclass's."""

    def sa_encode_device(self, x):
        """The codes of x as a uint8 CUDA tensor [n, code_size].  No host synchronisation when x is a contiguous float32 CUDA tensor
        on the index's device."""
        self._require_trained("sa_encode")
        return cat_chunks(self._per_chunk(self._rows(x, "sa_encode"), self._encode_device))

    def sa_encode(self, x):
        """The codes of x, numpy uint8 [n, code_size] (the module's encode reference states what a code is)."""
        return self.sa_encode_device(x).cpu().numpy()

    def sa_decode(self, codes):
        """numpy float32 [n,d]: the rows the codes stand for."""
        return self.sa_decode_device(codes).cpu().numpy()

    def reconstruct_n(self, start=0, n=None):
        """The decoded rows [start, start + n) as numpy float32 [n,d]: sa_decode of their stored codes."""
        return self.sa_decode_device(self._index._codes_device(start, n)).cpu().numpy()

    def reconstruct(self, i):
        """The decoded row i, numpy float32 [d]."""
        return self.reconstruct_n(int(i), 1)[0]
