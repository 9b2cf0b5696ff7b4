"""GPU suite: row access by id on the flat index - gather_device / scatter_device, the hash-table path of find(), reconstruct_batch /
update_vectors and search_and_reconstruct.

The yardstick is the one of test_id_map_gpu.py: what the index already does, compared bit for bit (float32 as uint32, no tolerances).
A gather must return the bits of reconstruct_n; a scatter must leave the index indistinguishable from one that received the same rows
through single-row write() calls (tiles, bf16 scan copy, the two scan bounds: seen through reconstruct_n, search, range_search and
scan_stats); the table path of find() must agree with the scan path and with numpy bookkeeping, also after the index changed under a
built table; search_and_reconstruct must return search()'s D and I and the positional rows behind them.

n = 1000 and 4099 are no multiple of 16, 64 or 256, so the last tile is partly filled; d = 512 and 20 take the vector and the padded
non-vector load path.  n = 9001 is the smallest size class at which k = 10 takes the bf16 candidate scan: there a stale scan copy or a
stale bound changes a result, and the final write of that chain reports positions too.  Labels are base + a permutation sample with
base = 3 * 10**12, so that a 32-bit truncation shows."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SIZES = [1000, 4099]
DIMS = [512, 20]
BIG = 3 * 10**12
RADIUS = {512: 0.1, 20: 0.5}          # a few per cent of the rows of a query (scores of unit vectors: sigma = d ** -0.5)


def _unit(rng, n, d):
    x = rng.standard_normal((n, d)).astype(np.float32)
    return x / np.linalg.norm(x, axis=1, keepdims=True)


_ROWS = {}


def _rows(n, d):
    """Seeded unit-norm rows, computed once per shape; the tests only read them."""
    if (n, d) not in _ROWS:
        _ROWS[(n, d)] = _unit(np.random.default_rng(1000 * d + n), n, d)
    return _ROWS[(n, d)]


def _labels(n, base=BIG):
    return (base + np.random.default_rng(n).permutation(10 * n)[:n]).astype(np.int64)


def _index(X, ids=None, env=None, capacity=None):
    """A FlatIPIndex over X (id-mapped when ids is given); env is set around the constructor, which is what reads it."""
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
    if ids is not None:
        idx.add_with_ids(X, ids)
    elif len(X):
        idx.add(X)
    return idx


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device="cuda", dtype=dtype)


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


# -- 1. gather ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mapped", [False, True], ids=["plain", "idmap"])
@pytest.mark.parametrize("n,d", [(n, d) for n in SIZES for d in DIMS])
def test_gather_matches_reconstruct_n(n, d, mapped):
    X = _rows(n, d)
    idx = _index(X, _labels(n) if mapped else None)
    stored = idx.reconstruct_n(0, n)
    rng = np.random.default_rng(n + d)
    rows = np.concatenate([rng.integers(0, n, 300), [0, n - 1, -1, n, 0, n - 1]]).astype(np.int64)     # repeats, both ends, two outside
    rng.shuffle(rows)
    got = idx.gather_device(_dev(rows, torch.int64)).cpu().numpy()
    inside = (rows >= 0) & (rows < n)
    assert inside.sum() == len(rows) - 2
    assert _same_bits(got[inside], stored[rows[inside]])
    assert np.isnan(got[~inside]).all() and got[~inside].shape == (2, d)
    one = idx.gather_device(_dev([n - 1], torch.int64)).cpu().numpy()
    assert _same_bits(one, stored[n - 1:n])
    assert idx.gather_device(torch.empty(0, dtype=torch.int64, device="cuda")).shape == (0, d)


# -- 2. scatter == single writes -----------------------------------------------------------------------------------------------------
def _observe(idx, Q, d):
    """Everything a caller can see of the stored state: the float32 tiles (reconstruct_n), the bf16 scan copy and the two scan
    bounds (search at k = 10, its fallback count, range search)."""
    D, I = idx.search(Q, 10)
    stats = idx.scan_stats()
    lims, Dr, Ir = idx.range_search(Q, RADIUS[d])
    return {"rows": _bits(idx.reconstruct_n(0, idx.ntotal)), "D": _bits(D), "I": I, "stats": np.asarray(stats, np.int64), "lims": lims,
            "Dr": _bits(Dr), "Ir": Ir}


@pytest.mark.parametrize("normalize", [True, False], ids=["normalize", "raw"])
@pytest.mark.parametrize("n,d", [(n, d) for n in SIZES for d in DIMS] + [(9001, 512)])
def test_scatter_equals_single_writes(n, d, normalize):
    X = _rows(n, d)
    rng = np.random.default_rng(3 * n + d)
    m = 37
    # distinct rows: three in the first tile, two in another, the last stored row (its tile is partly filled), the rest anywhere
    fixed = [1, 7, 15, 16 * 5 + 2, 16 * 5 + 9, n - 1]
    rest = rng.permutation(np.setdiff1d(np.arange(n), fixed))[:m - len(fixed)]
    rows = rng.permutation(np.concatenate([fixed, rest])).astype(np.int64)
    assert len(np.unique(rows)) == m
    new = _unit(rng, m, d)
    if not normalize:
        new = new * np.float32(3)                      # norm 3: the norm bound of the bf16 scan must move
    Q = np.concatenate([new[:4] / np.linalg.norm(new[:4], axis=1, keepdims=True), _unit(rng, 12, d)]).astype(np.float32)
    A, B = _index(X), _index(X)
    for i in range(m):
        A.write(int(rows[i]), new[i:i + 1], normalize=normalize)
    B.scatter_device(_dev(rows, torch.int64), _dev(new, torch.float32), normalize=normalize)
    torch.cuda.synchronize()
    a, b = _observe(A, Q, d), _observe(B, Q, d)
    for key in a:
        assert np.array_equal(a[key], b[key]), key
    assert not np.array_equal(a["rows"], _bits(X))                         # the writes did land
    assert np.array_equal(a["I"][:4, 0], rows[:4])                         # and a search finds the new vectors where they went
    # entries outside [0, ntotal) are skipped: nothing changes
    B.scatter_device(_dev([-1, n], torch.int64), _dev(_unit(rng, 2, d) * np.float32(7), torch.float32), normalize=normalize)
    torch.cuda.synchronize()
    c = _observe(B, Q, d)
    for key in a:
        assert np.array_equal(a[key], c[key]), key


# -- 3. table == scan == numpy ----------------------------------------------------------------------------------------------------
def _lowest(ids):
    out = {}
    for r, i in enumerate(ids.tolist()):
        out.setdefault(i, r)
    return out


def _key_sets(ids, dup, rng):
    """Key sets of 1, 5 and 3000 keys: present labels, absent ones, a negative one and the labels that two rows carry."""
    absent = np.setdiff1d(BIG + np.arange(10 * len(ids) + 50), ids)
    big = np.concatenate([rng.choice(ids, 2000), rng.choice(absent, 990), [-1, -5, -BIG], dup, dup, [int(ids[0]), int(ids[-1]), BIG - 1]])
    assert len(big) == 3000
    return [np.asarray([dup[0]], np.int64), np.asarray([ids[3], absent[0], -7, dup[0], dup[1]], np.int64), rng.permutation(big).astype(np.int64)]


@pytest.mark.parametrize("n", SIZES)
def test_find_table_equals_scan_equals_numpy(n):
    d = 20
    rng = np.random.default_rng(n + 5)
    X = _rows(n, d)
    ids = _labels(n)
    ids[n - 3], ids[n // 2] = ids[10], ids[40]                                # two labels stored on two rows each
    dup = np.asarray([ids[10], ids[40]], np.int64)
    T = _index(X, ids, env={"IVR_FIND_TABLE_MIN_KEYS": "0"})                   # always the table
    S = _index(X, ids, env={"IVR_FIND_TABLE_MIN_KEYS": "1000000000"})          # always the scan

    def check(cur, dup):
        low = _lowest(cur)
        for keys in _key_sets(cur, dup, rng):
            want = np.asarray([low.get(int(k), -1) for k in keys], np.int64)
            assert np.array_equal(T.find(keys), want)
            assert np.array_equal(S.find(keys), want)

    check(ids, dup)
    assert T.find(dup)[0] == 10 and T.find(dup)[1] == 40                       # the lower row wins
    # a removal that shifts rows (every third of rows 11 .. 299; both doubled labels stay, the lower row of the second one moves down)
    from ivr_amd.index import IDSelectorBatch
    gone = ids[11:300:3]
    keep = ~np.isin(ids, gone)
    for idx in (T, S):
        assert idx.remove_ids(IDSelectorBatch(gone)) == int((~keep).sum())
    cur = ids[keep]
    check(cur, dup)
    # growth past the capacity (the id table and the rows are re-allocated), with a label that already exists further down
    more = (BIG + 10 * n + 100 + rng.permutation(5 * n)[:n + 77]).astype(np.int64)
    more[5] = cur[-1]
    Xm = _unit(rng, len(more), d)
    for idx in (T, S):
        idx.add_with_ids(Xm, more)
    cur = np.concatenate([cur, more])
    check(cur, np.asarray([cur[len(cur) - len(more) - 1], ids[40]], np.int64))
    # reset, then other labels on other rows
    fresh = (BIG + rng.permutation(4000)[:300]).astype(np.int64)
    fresh[200] = fresh[7]
    for idx in (T, S):
        idx.reset()
        idx.add_with_ids(Xm[:300], fresh)
    check(fresh, np.asarray([fresh[7], fresh[8]], np.int64))
    for idx in (T, S):
        idx.reset()
        idx.add_with_ids(Xm[:0], fresh[:0])
        assert np.array_equal(idx.find(np.asarray([5, -1, BIG], np.int64)), [-1, -1, -1])      # an empty id-mapped index
    P = _index(X[:50])
    with pytest.raises(RuntimeError):
        P.find([3])                                                            # a plain index has no ids


# -- 4. by-id calls --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mapped", [False, True], ids=["plain", "idmap"])
@pytest.mark.parametrize("n,d", [(1000, 512), (4099, 20)])
def test_reconstruct_batch_and_update_vectors(n, d, mapped):
    X = _rows(n, d)
    rng = np.random.default_rng(7 * n + d)
    ids = _labels(n) if mapped else np.arange(n, dtype=np.int64)
    idx = _index(X, ids if mapped else None, env={"IVR_FIND_TABLE_MIN_KEYS": "0"} if d == 20 else None)
    book = X.copy()
    at = rng.choice(n, 200, replace=True)                                     # repeats are fine for a read
    assert _same_bits(idx.reconstruct_batch(ids[at]), book[at])
    rows, R = idx.reconstruct_batch_device(np.concatenate([ids[at[:5]], [ids.max() + 1]]))
    assert np.array_equal(rows.cpu().numpy(), np.concatenate([at[:5], [-1]]))
    assert _same_bits(R.cpu().numpy()[:5], book[at[:5]]) and np.isnan(R.cpu().numpy()[5]).all()
    upd = rng.permutation(n)[:150]
    new = _unit(rng, 150, d) * np.float32(2)
    idx.update_vectors(ids[upd], new)
    book[upd] = new
    assert _same_bits(idx.reconstruct_n(0, n), book)
    if mapped:
        assert np.array_equal(idx.id_map, ids)                                # ids are left alone
    # errors: a missing key writes nothing, duplicates and shapes are refused
    missing = int(ids.max()) + 1
    with pytest.raises(RuntimeError):
        idx.reconstruct_batch([int(ids[0]), missing])
    with pytest.raises(RuntimeError):
        idx.update_vectors(np.asarray([ids[1], missing, ids[2]]), new[:3])
    with pytest.raises(RuntimeError):
        idx.update_vectors(np.asarray([-1]), new[:1])
    with pytest.raises(ValueError):
        idx.update_vectors(np.asarray([ids[1], ids[2], ids[1]]), new[:3])
    with pytest.raises(ValueError):
        idx.update_vectors(ids[:3], new[:2])
    with pytest.raises(ValueError):
        idx.update_vectors(ids[:3], new[:3, :d - 1])
    assert _same_bits(idx.reconstruct_n(0, n), book)
    D, I = idx.search(new[:3], 1)
    assert np.array_equal(I[:, 0], ids[upd[:3]])


# -- 5. search_and_reconstruct -----------------------------------------------------------------------------------------------------
def _check_sar(idx, Q, k, pos_of, params=None):
    D, I, R = idx.search_and_reconstruct(Q, k, params=params)
    Ds, Is = idx.search(Q, k, params=params)
    assert np.array_equal(_bits(D), _bits(Ds)) and np.array_equal(I, Is)
    stored = idx.reconstruct_n(0, idx.ntotal)
    used = I >= 0
    assert R.shape == (len(Q), k, idx.d)
    assert np.array_equal(_bits(R[used]), _bits(stored[pos_of(I[used])]))
    assert np.isnan(R[~used]).all()
    return D, I, R


@pytest.mark.parametrize("n,d", [(n, d) for n in SIZES for d in DIMS] + [(9001, 512)])
def test_search_and_reconstruct_plain(n, d):
    from ivr_amd.index import IDSelectorBatch, IDSelectorRange, SearchParameters
    X = _rows(n, d)
    idx = _index(X)
    rng = np.random.default_rng(n - d)
    Q = _unit(rng, 16, d)
    _, I, _ = _check_sar(idx, Q, 10, lambda i: i)
    assert (I >= 0).all()
    # a range that starts inside a 256-row block, and a batch: the positions must be those of the whole index
    _, I, _ = _check_sar(idx, Q, 10, lambda i: i, SearchParameters(sel=IDSelectorRange(n // 2 + 37, n - 5)))
    assert I.min() >= n // 2 + 37 and I.max() < n - 5
    few = rng.permutation(n)[:7]
    _, I, _ = _check_sar(idx, Q[:3], 10, lambda i: i, SearchParameters(sel=IDSelectorBatch(few)))
    assert (I[:, 7:] == -1).all() and np.isin(I[:, :7], few).all()               # three unused slots per query: NaN rows


def test_search_and_reconstruct_k_beyond_ntotal():
    X = _rows(1000, 20)[:5]
    idx = _index(X)
    D, I, R = _check_sar(idx, X[2:4], 9, lambda i: i)
    assert (I[:, 5:] == -1).all() and (I[:, :5] >= 0).all() and I[0, 0] == 2 and I[1, 0] == 3
    assert np.isnan(R[:, 5:]).all() and not np.isnan(R[:, :5]).any()


@pytest.mark.parametrize("n,d", [(1000, 512), (4099, 20), (9001, 512)])
def test_search_and_reconstruct_id_mapped_returns_the_row_that_scored(n, d):
    from ivr_amd.index import IDSelectorBatch, SearchParameters
    X = _rows(n, d)
    ids = _labels(n)
    lo, hi = 20, n - 30
    ids[hi] = ids[lo]                                                          # one label on two rows with different vectors
    idx = _index(X, ids)
    order = np.argsort(ids, kind="stable")

    def pos_of(labels):                                                        # unique labels -> their row
        p = order[np.searchsorted(ids[order], labels)]
        assert np.array_equal(ids[p], labels)
        return p

    Q = np.concatenate([X[hi:hi + 1], _unit(np.random.default_rng(n), 15, d)])
    D, I, R = idx.search_and_reconstruct(Q, 10)
    Ds, Is = idx.search(Q, 10)
    assert np.array_equal(_bits(D), _bits(Ds)) and np.array_equal(I, Is)
    assert I[0, 0] == ids[lo]                                                  # the shared label ...
    assert _same_bits(R[0, 0], X[hi]) and not _same_bits(R[0, 0], X[lo])       # ... with the vector of the HIGHER row, which scored
    assert int(idx.find([int(ids[lo])])[0]) == lo                              # where a lookup of the label would have said `lo`
    single = I != ids[lo]
    assert np.array_equal(_bits(R[single]), _bits(X[pos_of(I[single])]))
    # a selector over stored ids
    allowed = ids[np.random.default_rng(n + 1).permutation(n)[:400]]
    allowed = allowed[allowed != ids[lo]]
    _check_sar(idx, Q[1:], 10, pos_of, SearchParameters(sel=IDSelectorBatch(allowed)))
