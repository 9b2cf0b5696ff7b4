"""GPU suite: FlatIPIndex.remove_ids (faiss IndexFlat::remove_ids) and reconstruct.

The yardstick is the one of test_filtered_search_gpu.py: a fresh FlatIPIndex built from the surviving rows.  After a removal the index
must hold exactly those rows in order (reconstruct_n bit for bit) and answer every kind of search exactly as the fresh index does: D
compared as uint32, I equal, no tolerances."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DIMS = [512, 768, 100, 20]          # 100 pads to 112 (7 chunks, an odd piece count rounded up), 20 takes the non-vector load path
SIZES = [1000, 4099]                # no multiple of 16, 64 or 256


def _unit(rng, n, d):
    x = rng.standard_normal((n, d)).astype(np.float32)
    return x / np.linalg.norm(x, axis=1, keepdims=True)


_ROWS = {}


def _rows(n, d):
    """Seeded unit-norm rows, computed once per shape; the tests only read them."""
    if (n, d) not in _ROWS:
        _ROWS[(n, d)] = _unit(np.random.default_rng(1000 * d + n), n, d)
    return _ROWS[(n, d)]


def _index(X, env=None, capacity=None):
    from ivr_amd.index import FlatIPIndex
    old = {k: os.environ.get(k) for k in (env or {})}
    os.environ.update(env or {})
    try:
        idx = FlatIPIndex(X.shape[1], capacity=len(X) if capacity is None else capacity)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v
    if len(X):
        idx.add(X)
    return idx


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _mask_of(n, ids):
    ids = np.asarray(ids, np.int64)
    ids = ids[(ids >= 0) & (ids < n)]
    m = np.zeros(n, bool)
    m[ids] = True
    return m


def _random_ids(n, frac, seed):
    """About frac of the rows, with duplicates, negative ids and ids at or above n mixed in, shuffled."""
    rng = np.random.default_rng(seed)
    ids = np.flatnonzero(rng.random(n) < frac)
    ids = np.concatenate([ids, ids[::7], [-1, -17, n, n + 3, 5 * n]])
    rng.shuffle(ids)
    return ids.astype(np.int64)


def _pattern(name, n):
    """(what to pass to remove_ids, mask of the removed rows)"""
    from ivr_amd.index import IDSelectorBatch, IDSelectorBitmap, IDSelectorRange
    if name.startswith("range"):
        lo, hi = {"range_head": (0, 37), "range_mid": (17, 83), "range_mid2": (250, 777), "range_tail": (n - 5, n + 100),
                  "range_single": (123, 124), "range_all": (0, n), "range_beyond": (n + 5, n + 50), "range_leaves_7": (7, n)}[name]
        return IDSelectorRange(lo, hi), _mask_of(n, np.arange(max(lo, 0), min(hi, n)))
    if name == "bitmap_every_other":
        m = np.arange(n) % 2 == 0
        return IDSelectorBitmap(np.packbits(m, bitorder="little")), m
    if name == "batch_random":
        ids = _random_ids(n, 0.3, n)
        return IDSelectorBatch(ids), _mask_of(n, ids)
    if name == "batch_empty":
        return IDSelectorBatch(np.zeros(0, np.int64)), np.zeros(n, bool)
    if name == "batch_leaves_768":                  # an exact multiple of 256 survives
        ids = np.random.default_rng(n + 1).choice(n, n - 768, replace=False)
        return IDSelectorBatch(ids), _mask_of(n, ids)
    if name == "plain_array":
        ids = np.array([5, 64, 65, 66, 300, 999, 16, 15], np.int64)
        return ids, _mask_of(n, ids)
    raise KeyError(name)


PATTERNS = ["range_head", "range_mid", "range_mid2", "range_tail", "range_single", "bitmap_every_other", "batch_random", "range_all",
            "batch_empty", "range_beyond", "range_leaves_7", "batch_leaves_768", "plain_array"]


def _remove_and_check(idx, sel, removed, **kw):
    """remove_ids, then in this order: the return value, ntotal, the surviving rows bit for bit.  Returns the survivors."""
    before = idx.reconstruct_n(0, idx.ntotal)
    n = idx.remove_ids(sel, **kw)
    keep = ~removed
    assert n == int(removed.sum())
    assert idx.ntotal == int(keep.sum())
    after = idx.reconstruct_n(0, idx.ntotal)
    assert after.shape == (int(keep.sum()), idx.d)
    assert np.array_equal(_bits(after), _bits(before[keep]))
    return before[keep]


@pytest.mark.parametrize("name", PATTERNS)
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("d", DIMS)
def test_layout(d, n, name):
    X = _rows(n, d)
    idx = _index(X)
    sel, removed = _pattern(name, n)
    left = _remove_and_check(idx, sel, removed)
    assert np.array_equal(_bits(left), _bits(X[~removed]))
    if name == "range_all":
        assert idx.ntotal == 0
        idx.add(X[:50])                             # a later add works, and lands on rows 0..49
        assert np.array_equal(_bits(idx.reconstruct_n(0, 50)), _bits(X[:50]))
        Q = _unit(np.random.default_rng(3), 4, d)
        _same_search(idx, _index(X[:50]), Q, 10)
    idx.close()


def _same_search(idx, fresh, Q, k, **kw):
    D, I = idx.search(Q, k, **kw)
    Dr, Ir = fresh.search(Q, k, **kw)
    assert np.array_equal(I, Ir), np.nonzero((I != Ir).any(1))[0][:8]
    assert np.array_equal(_bits(D), _bits(Dr))
    return D, I


@pytest.mark.parametrize("chunk", ["256", None])
@pytest.mark.parametrize("name", ["batch_random", "bitmap_every_other"])
def test_many_chunks(name, chunk):
    """IVR_REMOVE_CHUNK_ROWS=256 walks the 4099 rows in steps of 256 source rows (partial first and last destination tiles in each):
    through the bounce buffer while rows move down by less than a chunk, straight to the destination from there on.  The default
    is one chunk.  Both must leave the fresh index."""
    n, d = 4099, 512
    X = _rows(n, d)
    idx = _index(X, {"IVR_REMOVE_CHUNK_ROWS": chunk} if chunk else None)
    sel, removed = _pattern(name, n)
    left = _remove_and_check(idx, sel, removed)
    fresh = _index(left)
    rng = np.random.default_rng(8)
    for nq in (3, 100):
        _same_search(idx, fresh, _unit(rng, nq, d), 10)


def test_more_than_one_prefix_block_and_default_chunk():
    """210,003 rows: the kept-row prefix spans four blocks of 1024 groups, and the default chunk (65536 rows) walks several chunks:
    through the bounce buffer for the random 30 % (no row moves down by a whole chunk), straight to the destination once the first
    70,000 rows are gone (every row moves down by more than a chunk)."""
    from ivr_amd.index import IDSelectorRange
    n, d = 210_003, 20
    X = _rows(n, d)
    idx = _index(X)
    ids = _random_ids(n, 0.3, 4)
    left = _remove_and_check(idx, ids, _mask_of(n, ids))
    left = _remove_and_check(idx, IDSelectorRange(70_001, 70_099), _mask_of(len(left), np.arange(70_001, 70_099)))
    left = _remove_and_check(idx, IDSelectorRange(3, 70_003), _mask_of(len(left), np.arange(3, 70_003)))
    fresh = _index(left)
    rng = np.random.default_rng(9)
    for nq in (3, 100):
        _same_search(idx, fresh, _unit(rng, nq, d), 10)


@pytest.fixture(scope="module")
def removed_and_fresh():
    """4099 x 512 with a random 30 % removed, next to the fresh index of the survivors; 1000 x 512 the same way for k > ntotal."""
    out = {}
    for n in (4099, 1000):
        X = _rows(n, 512)
        idx = _index(X)
        sel, removed = _pattern("batch_random", n)
        assert idx.remove_ids(sel) == removed.sum()
        out[n] = (idx, _index(X[~removed]))
    return out


@pytest.mark.parametrize("nq", [3, 40, 100])        # <= 16 queries, the 64-query chunks, the large-batch bf16 scan
def test_search_after_removal(removed_and_fresh, nq):
    idx, fresh = removed_and_fresh[4099]
    Q = _unit(np.random.default_rng(nq), nq, 512)
    _same_search(idx, fresh, Q, 10)


def test_search_k_beyond_ntotal(removed_and_fresh):
    idx, fresh = removed_and_fresh[1000]
    assert idx.ntotal < 2048
    Q = _unit(np.random.default_rng(5), 3, 512)
    D, I = _same_search(idx, fresh, Q, 2048)
    assert (I[:, idx.ntotal:] == -1).all() and (I[:, :idx.ntotal] >= 0).all()
    assert (D[:, idx.ntotal:] == -np.finfo(np.float32).max).all()


def test_range_search_after_removal(removed_and_fresh):
    idx, fresh = removed_and_fresh[4099]
    Q = _unit(np.random.default_rng(6), 8, 512)
    lims, D, I = idx.range_search(Q, 0.12)          # scores are about N(0, 1/512): 0.12 is 2.7 sigma, a few rows per query
    lr, Dr, Ir = fresh.range_search(Q, 0.12)
    assert 0 < lims[-1] < 40 * len(Q)
    assert np.array_equal(lims, lr) and np.array_equal(I, Ir)
    assert np.array_equal(_bits(D), _bits(Dr))


def test_filtered_search_after_removal(removed_and_fresh):
    from ivr_amd.index import IDSelectorRange, SearchParameters
    idx, fresh = removed_and_fresh[4099]
    Q = _unit(np.random.default_rng(7), 5, 512)
    D, I = _same_search(idx, fresh, Q, 10, params=SearchParameters(sel=IDSelectorRange(1001, 2345)))
    assert ((I >= 1001) & (I < 2345)).all()


def test_bf16_scan_copy_moved():
    """10,000 x 128, k = 1: 157 groups (110 after the removal) against 4 (fast_groups(1) + 1) = 96, so the bf16 candidate scan runs.
    A stale or misplaced scan copy gives wrong ids or verification failures (queries redone by the float32 scan)."""
    n, d = 10_000, 128
    X = _rows(n, d)
    Q = _unit(np.random.default_rng(12), 10, d)
    idx = _index(X)
    ids = _random_ids(n, 0.3, 99)
    removed = _mask_of(n, ids)
    assert idx.remove_ids(ids) == removed.sum()
    fresh = _index(X[~removed])
    Dr, Ir = fresh.search(Q, 1)
    assert fresh.scan_stats() == (True, 0)          # the control: this seed needs no failover on a clean index
    D, I = idx.search(Q, 1)
    assert idx.scan_stats() == (True, 0)
    assert np.array_equal(I, Ir) and np.array_equal(_bits(D), _bits(Dr))
    # the same for the large-batch scan, which reads the scan copy in 256-row blocks
    Q = _unit(np.random.default_rng(13), 100, d)
    Dr, Ir = fresh.search(Q, 1)
    assert fresh.scan_stats() == (True, 0)
    D, I = idx.search(Q, 1)
    assert idx.scan_stats() == (True, 0)
    assert np.array_equal(I, Ir) and np.array_equal(_bits(D), _bits(Dr))


def test_remove_then_add():
    """The zeroed tail and the partly filled last tile take new rows."""
    n, d = 1000, 512
    X = _rows(n, d)
    extra = _unit(np.random.default_rng(21), 50, d)
    idx = _index(X)
    sel, removed = _pattern("batch_random", n)
    left = _remove_and_check(idx, sel, removed)
    idx.add(extra)
    both = np.concatenate([left, extra])
    assert np.array_equal(_bits(idx.reconstruct_n(0, idx.ntotal)), _bits(both))
    fresh = _index(both)
    rng = np.random.default_rng(22)
    for nq in (3, 100):
        _same_search(idx, fresh, _unit(rng, nq, d), 10)


def test_two_removals_in_a_row():
    from ivr_amd.index import IDSelectorRange
    n, d = 4099, 100
    X = _rows(n, d)
    idx = _index(X)
    sel, removed = _pattern("bitmap_every_other", n)
    left = _remove_and_check(idx, sel, removed)
    second = _mask_of(len(left), np.arange(100, 333))
    left = _remove_and_check(idx, IDSelectorRange(100, 333), second)
    _same_search(idx, _index(left), _unit(np.random.default_rng(23), 20, d), 10)


def test_remove_then_write():
    from ivr_amd.index import IDSelectorRange
    n, d = 1000, 512
    X = _rows(n, d)
    idx = _index(X)
    left = _remove_and_check(idx, IDSelectorRange(30, 301), _mask_of(n, np.arange(30, 301))).copy()
    new = _unit(np.random.default_rng(24), 40, d)
    idx.write(20, new)                              # spans rows that stayed (20..29) and rows that moved down
    left[20:60] = new
    assert np.array_equal(_bits(idx.reconstruct_n(0, idx.ntotal)), _bits(left))
    _same_search(idx, _index(left), _unit(np.random.default_rng(25), 6, d), 10)


def test_id_base():
    from ivr_amd.index import IDSelectorRange
    n, d = 1000, 20
    idx = _index(_rows(n, d))
    removed = _mask_of(n, np.arange(10, 20))
    _remove_and_check(idx, IDSelectorRange(1_000_010, 1_000_020), removed, id_base=1_000_000)


def test_reconstruct_one_row():
    X = _rows(1000, 100)
    idx = _index(X)
    for i in (0, 17, 999):
        r = idx.reconstruct(i)
        assert r.shape == (100,) and np.array_equal(_bits(r), _bits(X[i]))
    with pytest.raises(ValueError):
        idx.reconstruct(1000)


def test_errors_leave_the_index_unchanged():
    from ivr_amd import _ffi
    X = _rows(1000, 20)
    idx = _index(X)
    lib = _ffi.load()
    n = C.c_int64(7)
    with torch.cuda.device(idx.device):
        assert lib.ivr_index_remove_ids(idx._h, 0, None, C.byref(n), _ffi.stream_ptr()) == -1              # IVR_ERR_INVALID
        bad = _ffi.IdFilter(0, 10, None, -1)
        assert lib.ivr_index_remove_ids(idx._h, 0, C.byref(bad), C.byref(n), _ffi.stream_ptr()) == -1
    for sel in ("all", None, lambda i: True, np.array([1.5, 2.0]), [1, 2, 3]):
        with pytest.raises(ValueError):
            idx.remove_ids(sel)
    assert idx.ntotal == 1000
    assert np.array_equal(_bits(idx.reconstruct_n(0, 1000)), _bits(X))
