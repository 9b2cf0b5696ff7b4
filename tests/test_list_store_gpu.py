"""GPU suite of the list store the coded inverted-file indexes share (csrc/search_lists.hip ListRows, behind ivr_ivfpq_* and
ivr_ivfsq_* and the _ListStore of ivr_amd/_ivf.py): one contract, run over both stores.

Six lists of 0, 1, 63, 64, 65 and 130 rows are an empty list, one row, one short of a 64-row group, exactly one group, one over and
three groups.  The code sizes take every path of the two pack kernels: M = 5 (bytes), 16 (whole words), 33 (3 words) and 80 (5 words
stored as 8) for the PQ store, d = 20 (a partial K step), 64 (one whole step) and 100 (two steps, the second ragged) for the SQ store.
The stores hold chosen codes and labels, so everything is compared exactly; neither store lets its packed image be read back, so the
round trip through get_codes and a scan of every list against ivfpq_scan_ref / ivfsq_scan_ref stand in for it."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

FLT_MAX = np.finfo(np.float32).max
SIZES = [0, 1, 63, 64, 65, 130]
NLIST = len(SIZES)
OFF = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int64)
N = int(OFF[-1])
SMALL = np.concatenate([[0], np.cumsum([2, 0, 0, 0, 0, 1])]).astype(np.int64)
CASES = [("pq", 5), ("pq", 16), ("pq", 33), ("pq", 80), ("sq", 20), ("sq", 64), ("sq", 100)]
NQ, K = 3, 400                                                       # k exceeds the 323 rows: padding in every result


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


class Store:
    """A trained index of `size`-byte codes over NLIST lists, the chosen content and one fixed batch of queries that name every list."""

    def __init__(self, kind, size):
        from ivr_amd.index import FlatIPIndex
        self.kind, self.size = kind, size
        rng = np.random.default_rng(100 * size + len(kind))
        d = 2 * size if kind == "pq" else size
        quantizer = FlatIPIndex(d)
        quantizer.add(np.eye(NLIST, d, dtype=np.float32))
        if kind == "pq":
            from ivr_amd.ivfpq import IndexIVFPQ
            self.idx = IndexIVFPQ(quantizer, d, NLIST, size)
            self.idx.pq.centroids = np.zeros((size, 256, 2), np.float32)
            self.form = (rng.standard_normal((NQ, size, 256)).astype(np.float32),)
        else:
            from ivr_amd.ivfsq import IndexIVFScalarQuantizer
            self.idx = IndexIVFScalarQuantizer(quantizer, d, NLIST)
            self.idx.sq.trained = np.concatenate([np.zeros(d), np.ones(d)]).astype(np.float32)
            self.form = (rng.integers(-16256, 16257, (NQ, d)).astype(np.int16), rng.uniform(1e-6, 2e-6, NQ).astype(np.float32),
                         rng.uniform(0.5, 1.5, NQ).astype(np.float32))
        assert self.idx.is_trained
        self.abi = self.idx._ABI
        self.codes = rng.integers(0, 256, (N, size), dtype=np.uint8)
        self.ids = rng.permutation(N).astype(np.int64) + 1000         # labels are not positions
        self.coarse = rng.uniform(0.1, 1.0, (NQ, NLIST)).astype(np.float32)
        self.every = np.tile(np.arange(NLIST), (NQ, 1)).astype(np.int64)

    def set(self, codes, ids, off):
        self.idx._set_lists(torch.from_numpy(codes).cuda(), torch.from_numpy(ids).cuda(), off)

    def raw_set(self, codes, ids, off, n):
        """The handle's _set_lists alone: the offsets of the Python object stay as they are."""
        self.idx._lists._call(self.abi + "_set_lists", torch.from_numpy(codes).cuda(), torch.from_numpy(ids).cuda(), off.ctypes.data, n)

    def ntotal(self):
        return self.idx._lists._call(self.abi + "_ntotal")

    def rows(self, start=0, n=None):
        c, i = self.idx._rows_device(start, n)
        return c.cpu().numpy(), i.cpu().numpy()

    def scan(self, codes, ids, off):
        """Every list for every query: (D, I), checked bit for bit against the reference scan over the content given."""
        if self.kind == "pq":
            from ivr_amd.ivfpq import ivfpq_scan_ref
            D, I = self.idx.search_tables_preassigned_device(*self.form, self.coarse, self.every, K)
            Dr, Ir = ivfpq_scan_ref(*self.form, self.coarse, self.every, off, codes, ids, K)
        else:
            from ivr_amd.ivfsq import ivfsq_scan_ref
            D, I = self.idx.search_codes_preassigned_device(*self.form, self.coarse, self.every, K)
            Dr, Ir = ivfsq_scan_ref(*self.form, self.coarse, self.every, off, codes, ids, K)
        D, I = D.cpu().numpy(), I.cpu().numpy()
        assert np.array_equal(I, Ir) and np.array_equal(bits(D), bits(Dr))
        return D, I

    def last_error(self):
        from ivr_amd import _ffi
        return (_ffi.load().ivr_last_error(None) or b"").decode()


@pytest.fixture(params=CASES, ids=lambda c: f"{c[0]}{c[1]}")
def store(request):
    s = Store(*request.param)
    s.set(s.codes, s.ids, OFF)
    yield s
    s.idx.close()


def test_rows_come_back_unchanged_and_new_content_replaces_the_old(store):
    s = store
    assert s.ntotal() == s.idx.ntotal == N == 323 and s.idx.list_sizes().tolist() == SIZES
    codes, ids = s.rows()
    assert np.array_equal(codes, s.codes) and np.array_equal(ids, s.ids)
    codes, ids = s.rows(40, 200)                                     # from inside the list of 63 rows to inside the list of 130
    assert np.array_equal(codes, s.codes[40:240]) and np.array_equal(ids, s.ids[40:240])
    for l in range(NLIST):
        assert np.array_equal(s.idx.list_codes(l), s.codes[OFF[l]:OFF[l + 1]]) and np.array_equal(s.idx.list_ids(l), s.ids[OFF[l]:OFF[l + 1]])
    D, I = s.scan(s.codes, s.ids, OFF)
    assert (np.sort(I[:, :N], axis=1) == np.sort(s.ids)).all() and (I[:, N:] == -1).all() and (D[:, N:] == -FLT_MAX).all()
    # smaller content: two rows in the first list, one in the last
    codes2, ids2 = s.codes[[7, 200, 300]], np.array([5, 6, 7], np.int64)
    s.set(codes2, ids2, SMALL)
    assert s.ntotal() == s.idx.ntotal == 3
    codes, ids = s.rows()
    assert np.array_equal(codes, codes2) and np.array_equal(ids, ids2)
    with pytest.raises(ValueError):
        s.idx._lists._call(s.abi + "_get_codes", 0, 4, torch.empty((4, s.size), dtype=torch.uint8, device="cuda"), None)
    D, I = s.scan(codes2, ids2, SMALL)
    assert (np.sort(I[:, :3], axis=1) == ids2).all() and (I[:, 3:] == -1).all() and (D[:, 3:] == -FLT_MAX).all()


def test_a_refused_call_leaves_the_store_as_it_was(store):
    s = store
    before = s.scan(s.codes, s.ids, OFF)
    descends, late, short = OFF.copy(), OFF.copy(), OFF.copy()
    descends[2], descends[3] = OFF[3], OFF[2]
    late[0] = 1
    short[-1] = N - 1
    for off in (descends, late, short):                              # descends; does not start at 0; does not end at n
        with pytest.raises(ValueError):
            s.raw_set(s.codes[::-1].copy(), s.ids[::-1].copy(), off, N)
        assert s.last_error().startswith(s.abi + "_set_lists:")
        assert s.ntotal() == N
    with pytest.raises(ValueError):                                  # a range past ntotal
        s.idx._lists._call(s.abi + "_get_codes", N - 1, 2, torch.empty((2, s.size), dtype=torch.uint8, device="cuda"), None)
    assert s.last_error().startswith(s.abi + "_get_codes:")
    codes, ids = s.rows()
    assert np.array_equal(codes, s.codes) and np.array_equal(ids, s.ids)
    after = s.scan(s.codes, s.ids, OFF)
    assert np.array_equal(after[1], before[1]) and np.array_equal(bits(after[0]), bits(before[0]))


def test_reset_leaves_nothing_to_find(store):
    s = store
    s.idx.reset()
    assert s.ntotal() == s.idx.ntotal == 0 and s.idx.is_trained
    D, I = s.scan(s.codes[:0], s.ids[:0], np.zeros(NLIST + 1, np.int64))
    assert (I == -1).all() and (D == -FLT_MAX).all()
    with pytest.raises(ValueError):
        s.idx._lists._call(s.abi + "_get_codes", 0, 1, torch.empty((1, s.size), dtype=torch.uint8, device="cuda"), None)
    s.set(s.codes, s.ids, OFF)                                       # and the store takes rows again
    codes, ids = s.rows()
    assert np.array_equal(codes, s.codes) and np.array_equal(ids, s.ids)
