"""GPU suite of the row store the flat coded indexes share (csrc/search_coded.hip CodeRows, behind ivr_bin_index_*, ivr_sq_index_* and
ivr_pqfs_index_*, and the _CodeStore of ivr_amd/_coded.py) and of the two-level top-k their scans share (GroupTopK): one contract,
run over the three stores.

The code sizes take every path of the three pack kernels: 8 bits (one byte of one word), 40 (5 bytes: the byte-wise path), 256 (two
whole words, the vector path) and 520 (65 bytes: 5 words stored as 8) for the binary store, d = 20 (a partial K step), 64 (one whole
step, the vector path) and 100 (two steps, the second ragged) for the SQ store, M = 2 (one dword of one word), 8 (four dwords), 10
(W = 2 with six absent sub-quantisers) and 34 (W = 5) for the PQFS store.  The rows arrive in steps of 1, 62, 1, 1, 191, 1, 300 and
443: the totals 1, 63, 64, 65, 256, 257, 557 and 1,000 end on and beside every 64-row group edge and 256-row block edge, and every
store re-allocates at least three times from its first granule.  The stores hold chosen codes, so everything is compared exactly;
no store lets its packed image be read back, so the round trip through get_codes and a search against pq_scan_ref / sq_scan_ref /
pqfs_scan_ref (and a stable numpy sort of popcounts for the Hamming search) stand in for it.  The refusal texts were recorded from the
entry points as they were before they moved onto CodeRows."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

FLT_MAX = np.finfo(np.float32).max
INT32_MAX = np.iinfo(np.int32).max
STEPS = [1, 62, 1, 1, 191, 1, 300, 443]
N = sum(STEPS)
NQ, K_ALL, K_FEW, FEW = 3, 1100, 400, 70                             # k exceeds the rows both times: padding in every result
CASES = [("bin", 8), ("bin", 40), ("bin", 256), ("bin", 520), ("sq", 20), ("sq", 64), ("sq", 100),
         ("pqfs", 2), ("pqfs", 8), ("pqfs", 10), ("pqfs", 34)]
# (ABI prefix, granule, rows allocated at creation)
ABI = {"bin": ("ivr_bin_index", 256, 256), "sq": ("ivr_sq_index", 64, 0), "pqfs": ("ivr_pqfs_index", 256, 0)}


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def last_error():
    from ivr_amd import _ffi
    return (_ffi.load().ivr_last_error(None) or b"").decode()


class Store:
    """An empty store of `size` (bits of a binary code, d of an SQ code, M of a PQFS code), the chosen rows and one fixed batch of
    queries in the form its scan takes."""

    def __init__(self, kind, size):
        from ivr_amd._coded import _CodeStore
        from ivr_amd.binary import BinaryFlatIndex
        self.kind, self.size = kind, size
        self.abi, self.granule, self.cap = ABI[kind]
        rng = np.random.default_rng(1000 * size + len(kind))
        if kind == "bin":
            self.h, self.code_size = BinaryFlatIndex(size), size // 8
            self.form = (rng.standard_normal((NQ, self.code_size, 256)).astype(np.float32),)       # PQ tables, M = nbits / 8
            self.qcodes = rng.integers(0, 256, (NQ, self.code_size), dtype=np.uint8)
        elif kind == "sq":
            self.h, self.code_size = _CodeStore("ivr_sq_index", (size,), size, "SQIndex", None), size
            self.form = (rng.integers(-16256, 16257, (NQ, size)).astype(np.int16), rng.uniform(1e-6, 2e-6, NQ).astype(np.float32),
                         rng.uniform(0.5, 1.5, NQ).astype(np.float32))
        else:
            self.h, self.code_size = _CodeStore("ivr_pqfs_index", (size,), size // 2, "PQFastScanIndex", None), size // 2
            self.form = (rng.integers(0, 256, (NQ, size, 16), dtype=np.uint8), rng.uniform(1e-3, 2e-3, NQ).astype(np.float32),
                         rng.uniform(-1.0, 1.0, NQ).astype(np.float32))
        self.codes = rng.integers(0, 256, (N, self.code_size), dtype=np.uint8)
        self.other = rng.integers(0, 256, (FEW, self.code_size), dtype=np.uint8)
        self.dev = [torch.from_numpy(a).cuda() for a in self.form]

    def add(self, rows):
        """Append rows; True when the store had to re-allocate (CodeRows::reserve_for_add: to max(rows needed, 1.5 capacity), in
        whole granules, one granule at least)."""
        need = self.h.ntotal + len(rows)
        self.h._add_device(torch.from_numpy(rows).cuda())
        if need <= self.cap:
            return False
        want = max(need, self.cap + self.cap // 2, self.granule)
        self.cap = -(-want // self.granule) * self.granule
        return True

    def abi_ntotal(self):
        return self.h._call(self.abi + "_ntotal")

    def rows(self, start=0, n=None):
        return self.h._codes_device(start, n).cpu().numpy()

    def raw_get(self, start, n, out="alloc"):
        if isinstance(out, str):
            out = torch.empty((max(n, 1), self.code_size), dtype=torch.uint8, device="cuda")
        self.h._call(self.abi + "_get_codes", start, n, out)

    def search(self, codes, k):
        """Every search of the store, checked bit for bit against its reference over the rows given."""
        D, I = (torch.empty((NQ, k), dtype=torch.float32, device="cuda"), torch.empty((NQ, k), dtype=torch.int64, device="cuda"))
        if self.kind == "bin":
            from ivr_amd.pq import pq_scan_ref
            self.h._call("ivr_bin_index_search_pq", self.dev[0], NQ, self.code_size, k, D, I)
            Dr, Ir = pq_scan_ref(*self.form, codes, k)
            Dh, Ih = (a.cpu().numpy() for a in self.h.search_device(self.qcodes, k))
            dist = np.unpackbits(self.qcodes[:, None, :] ^ codes[None, :, :], axis=2).sum(axis=2).astype(np.int64)
            order = np.argsort(dist, axis=1, kind="stable")[:, :k]                  # stable: equal distances, the lower row first
            n = order.shape[1]
            assert np.array_equal(Ih[:, :n], order) and np.array_equal(Dh[:, :n], np.take_along_axis(dist, order, axis=1))
            assert (Ih[:, n:] == -1).all() and (Dh[:, n:] == INT32_MAX).all() and Dh.dtype == np.int32
        elif self.kind == "sq":
            from ivr_amd.sq import sq_scan_ref
            self.h._call("ivr_sq_index_search", *self.dev, NQ, k, D, I)
            Dr, Ir = sq_scan_ref(*self.form, codes, k)
        else:
            from ivr_amd.pqfs import pqfs_scan_ref
            self.h._call("ivr_pqfs_index_search", *self.dev, NQ, k, D, I)
            Dr, Ir = pqfs_scan_ref(*self.form, codes, k)
        D, I = D.cpu().numpy(), I.cpu().numpy()
        assert np.array_equal(I, Ir) and np.array_equal(bits(D), bits(Dr))
        return D, I


@pytest.fixture(params=CASES, ids=lambda c: f"{c[0]}{c[1]}")
def store(request):
    s = Store(*request.param)
    yield s
    s.h.close()


def test_an_empty_store_answers_with_padding(store):
    s = store
    assert s.h.ntotal == 0
    D, I = s.search(s.codes[:0], 5)
    assert (I == -1).all() and (D == -FLT_MAX).all()


def test_ragged_adds_come_back_unchanged_and_a_reset_leaves_nothing_to_find(store):
    s = store
    total, point, grown = 0, 0, 0
    for step in STEPS:
        if s.add(s.codes[total:total + step]):
            point, grown = total, grown + 1                          # the rows in front of `point` were copied into the new block
        total += step
        assert s.h.ntotal == s.abi_ntotal() == total
        assert np.array_equal(s.rows(), s.codes[:total])
        lo, hi = max(0, point - 70), min(total, point + 70)          # a window that straddles the last re-allocation point
        assert np.array_equal(s.rows(lo, hi - lo), s.codes[lo:hi])
    assert total == N == 1000 and grown >= 3
    D, I = s.search(s.codes, K_ALL)
    assert (np.sort(I[:, :N], axis=1) == np.arange(N)).all() and (I[:, N:] == -1).all() and (D[:, N:] == -FLT_MAX).all()
    # the SQ and PQFS stores keep the bytes of the 1,000 rows and mask them by number; the binary store clears its block
    s.h.reset()
    assert s.h.ntotal == s.abi_ntotal() == 0
    s.add(s.other)
    assert s.h.ntotal == FEW and np.array_equal(s.rows(), s.other)
    D, I = s.search(s.other, K_FEW)
    assert (np.sort(I[:, :FEW], axis=1) == np.arange(FEW)).all() and (I[:, FEW:] == -1).all() and (D[:, FEW:] == -FLT_MAX).all()


def test_a_refused_call_says_why_and_leaves_the_store_as_it_was(store):
    from ivr_amd import _ffi
    s, a = store, store.abi
    s.add(s.codes[:100])
    for start, n in ((99, 2), (-1, 1), (0, -1), (101, 0)):           # past ntotal, before 0, a negative count, an empty range outside
        with pytest.raises(ValueError):
            s.raw_get(start, n)
        assert last_error() == f"{a}_get_codes: rows [{start},{start + n}) outside [0,100)"
    with pytest.raises(ValueError):
        s.h._call(a + "_add", torch.from_numpy(s.codes[:1]).cuda(), -1)
    assert last_error() == f"{a}_add: n=-1"
    for call, name in ((lambda: s.h._call(a + "_add", None, 1), "_add"), (lambda: s.raw_get(0, 1, None), "_get_codes"),
                       (lambda: _ffi.call(a + "_add", None, None, 0), "_add"),
                       (lambda: _ffi.call(a + "_get_codes", None, 0, 0, None), "_get_codes")):
        with pytest.raises(ValueError):
            call()
        assert last_error() == f"{a}{name}: NULL argument"
    with pytest.raises(ValueError):
        _ffi.call(a + "_reset", None)
    assert last_error() == f"{a}_reset: NULL index"
    if s.kind == "bin":                                              # the binary index's ntotal and destroy take NULL
        assert _ffi.call(a + "_ntotal", None) == 0
        _ffi.call(a + "_destroy", None)
    else:
        assert _ffi.call(a + "_ntotal", None) == -1 and last_error() == f"{a}_ntotal: NULL index"
        with pytest.raises(ValueError):
            _ffi.call(a + "_destroy", None)
        assert last_error() == f"{a}_destroy: NULL index"
    s.h._call(a + "_add", None, 0)                                   # nothing to add: no codes needed
    s.raw_get(100, 0, None)                                          # nothing to read at the end of the rows: no buffer needed
    assert s.h.ntotal == 100 and np.array_equal(s.rows(), s.codes[:100])
    s.search(s.codes[:100], K_FEW)
