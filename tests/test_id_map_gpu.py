"""GPU suite: stable external ids on the flat index (FlatIPIndex.add_with_ids / IndexIDMap2).

The yardstick is the one of test_remove_ids_gpu.py and test_filtered_search_gpu.py: a PLAIN FlatIPIndex over the same rows, compared
bit for bit (D as uint32, I equal, no tolerances).  With P the plain index, M the id-mapped one and ids[r] the label of row r, every
result of M must be the result of P with its row numbers translated through ids, and a selector over stored ids must act like the
positional batch selector of the rows whose labels it allows.

Labels are base + a random sample of [0, 10 n): not monotone, with gaps; base = 3 * 10**12 catches a 32-bit truncation on the path.
n = 1000 and 4099 are no multiple of 16, 64 or 256; d = 512 and 20 take the vector and the non-vector load path.  At these sizes
every search runs the exact float32 scan; n = 9001 (search test only) is the smallest size class at which k = 10 also takes the bf16
candidate scan, so that the final writes of the <= 16-query chain and of the large-batch scan translate labels too."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SIZES = [1000, 4099]
DIMS = [512, 20]
BIG = 3 * 10**12


def _unit(rng, n, d):
    x = rng.standard_normal((n, d)).astype(np.float32)
    return x / np.linalg.norm(x, axis=1, keepdims=True)


_ROWS, _PAIRS = {}, {}


def _rows(n, d):
    """Seeded unit-norm rows, computed once per shape; the tests only read them."""
    if (n, d) not in _ROWS:
        _ROWS[(n, d)] = _unit(np.random.default_rng(1000 * d + n), n, d)
    return _ROWS[(n, d)]


def _queries(nq, d):
    return _unit(np.random.default_rng(7 * d + nq), nq, d)


def _labels(n, base=0):
    return (base + np.random.default_rng(n).permutation(10 * n)[:n]).astype(np.int64)


def _plain(X):
    from ivr_amd.index import FlatIPIndex
    idx = FlatIPIndex(X.shape[1], capacity=len(X))
    if len(X):
        idx.add(X)
    return idx


def _mapped(X, ids, env=None, capacity=None):
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
    idx.add_with_ids(X, ids)
    return idx


def _pair(n, d, base=0):
    """(X, ids, plain index, id-mapped index) of one shape, built once; only the tests that do not change an index use it."""
    if (n, d, base) not in _PAIRS:
        X, ids = _rows(n, d), _labels(n, base)
        _PAIRS[(n, d, base)] = (X, ids, _plain(X), _mapped(X, ids))
    return _PAIRS[(n, d, base)]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _translate(I, ids):
    return np.where(I >= 0, ids[np.maximum(I, 0)], -1)


def _allowed(sel, ids):
    return np.array([sel.is_member(int(i)) for i in ids], bool)


def _selector(name, n, ids, base):
    """The selector shapes of the suite, over the labels base + [0, 10 n)."""
    from ivr_amd.index import IDSelectorBatch, IDSelectorBitmap, IDSelectorRange
    rng = np.random.default_rng(n + 11)
    if name == "range":                             # about a third of the label span
        return IDSelectorRange(base + 3 * n, base + 6 * n + 5)
    if name == "batch":                             # about 30 % of the stored labels, plus labels that are not stored
        absent = np.setdiff1d(base + np.arange(10 * n), ids)
        return IDSelectorBatch(np.concatenate([ids[rng.random(n) < 0.3], absent[:: max(1, len(absent) // 200)], [-5]]))
    if name == "bitmap":                            # over the label span (base 0 only: a faiss bitmap starts at id 0)
        return IDSelectorBitmap(np.packbits(rng.random(10 * n) < 0.4, bitorder="little"))
    if name == "bitmap_lohi":
        return IDSelectorBitmap(np.packbits(rng.random(10 * n) < 0.4, bitorder="little"), lo=2 * n + 3, hi=7 * n)
    if name == "batch_empty":
        return IDSelectorBatch(np.zeros(0, np.int64))
    if name == "trap":                              # ids in [5000, 6000) only: the labels reach far beyond the selector's bitmap
        return IDSelectorBatch(np.arange(5000, 6000, 3))
    if name == "all":
        return IDSelectorRange(0, 1 << 62)
    if name == "nothing":
        return IDSelectorRange(base + 10 * n, base + 10 * n + 100)
    raise KeyError(name)


def _selector_cases():
    for base in (0, BIG):
        for name in ("range", "batch", "bitmap", "bitmap_lohi", "batch_empty", "trap"):
            if base and name.startswith("bitmap"):
                continue
            yield pytest.param(name, base, id=f"{name}-{'big' if base else '0'}")


@pytest.mark.parametrize("n,d", [(n, d) for n in SIZES for d in DIMS] + [(9001, 512)])
def test_search_labels(n, d):
    X, ids, P, M = _pair(n, d)
    assert M.has_ids and not P.has_ids and M.ntotal == n
    assert np.array_equal(M.id_map, ids)
    shapes = [(3, 10), (70, 10), (5, 200)] + ([(2, 1500)] if n == 1000 else [])      # the last one: k > n
    for nq, k in shapes:
        Q = _queries(nq, d)
        Dp, Ip = P.search(Q, k)
        Dm, Im = M.search(Q, k)
        assert np.array_equal(_bits(Dm), _bits(Dp)), (nq, k)
        assert np.array_equal(Im, _translate(Ip, ids)), (nq, k)
        if k > n:
            assert (Im[:, n:] == -1).all() and (Im[:, :n] >= 0).all()


@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("n", SIZES)
def test_range_search_labels(n, d):
    X, ids, P, M = _pair(n, d)
    Q = _queries(9, d)
    S = np.sort(Q.astype(np.float64) @ X.astype(np.float64).T, axis=1)
    some = float(S[:, -20].mean())                   # about 20 hits per query
    lp, Dp, Ip = P.range_search(Q, some)
    per_query = np.diff(lp)
    assert per_query.min() >= 1 and per_query.max() <= 60, per_query
    lm, Dm, Im = M.range_search(Q, some)
    assert np.array_equal(lm, lp) and np.array_equal(_bits(Dm), _bits(Dp)) and np.array_equal(Im, ids[Ip])
    lm, Dm, Im = M.range_search(Q, float(S.max()) + 0.5)
    assert np.array_equal(lm, np.zeros(10, np.int64)) and len(Dm) == 0 and len(Im) == 0


def test_ties_follow_the_row_order():
    n, d = 1000, 512
    X, ids = _rows(n, d).copy(), _labels(n).copy()
    X[700] = X[5]
    ids[5], ids[700] = 900, 3
    ids[(ids == 900) & (np.arange(n) != 5)] = 10 * n + 1      # keep the two labels unique
    ids[(ids == 3) & (np.arange(n) != 700)] = 10 * n + 2
    M = _mapped(X, ids)
    D, I = M.search(X[5:6], 4)
    assert list(I[0, :2]) == [900, 3] and _bits(D)[0, 0] == _bits(D)[0, 1]
    lims, Dr, Ir = M.range_search(X[5:6], 0.999)
    assert list(Ir) == [900, 3]                       # ascending ROW order


@pytest.mark.parametrize("name,base", _selector_cases())
@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("n", SIZES)
def test_selectors_name_stored_ids(n, d, name, base):
    from ivr_amd.index import IDSelectorBatch, SearchParameters
    X, ids, P, M = _pair(n, d, base)
    sel = _selector(name, n, ids, base)
    rows = np.flatnonzero(_allowed(sel, ids))
    if name in ("batch_empty",) or (name == "trap" and base):
        assert len(rows) == 0
    elif name != "trap":
        assert 0 < len(rows) < n
    ref = SearchParameters(sel=IDSelectorBatch(rows))
    got = SearchParameters(sel=sel)
    for nq, k in [(3, 10), (70, 10)]:
        Q = _queries(nq, d)
        Dp, Ip = P.search(Q, k, params=ref)
        Dm, Im = M.search(Q, k, params=got)
        assert np.array_equal(_bits(Dm), _bits(Dp)), (nq, k)
        assert np.array_equal(Im, _translate(Ip, ids)), (nq, k)
    Q = _queries(9, d)
    radius = float(np.sort(Q.astype(np.float64) @ X.astype(np.float64).T, axis=1)[:, -40].mean())
    lp, Dp, Ip = P.range_search(Q, radius, params=ref)
    lm, Dm, Im = M.range_search(Q, radius, params=got)
    assert np.array_equal(lm, lp) and np.array_equal(_bits(Dm), _bits(Dp)) and np.array_equal(Im, ids[Ip])


def _check_removed(M, X, ids, gone, count):
    keep = ~gone
    assert count == int(gone.sum())
    assert M.ntotal == int(keep.sum())
    assert np.array_equal(M.id_map, ids[keep])
    assert np.array_equal(_bits(M.reconstruct_n()), _bits(X[keep]))
    fresh = _mapped(X[keep], ids[keep])
    for nq, k in [(3, 10), (70, 10)]:
        Q = _queries(nq, X.shape[1])
        Df, If = fresh.search(Q, k)
        Dm, Im = M.search(Q, k)
        assert np.array_equal(_bits(Dm), _bits(Df)) and np.array_equal(Im, If), (nq, k)


def _removal_cases():
    for base in (0, BIG):
        for name in ("range", "batch", "bitmap", "bitmap_lohi", "batch_empty", "trap", "all", "nothing"):
            if base and name.startswith("bitmap"):
                continue
            yield pytest.param(name, base, id=f"{name}-{'big' if base else '0'}")


@pytest.mark.parametrize("name,base", _removal_cases())
@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("n", SIZES)
def test_remove_ids_by_stored_id(n, d, name, base):
    X, ids = _rows(n, d), _labels(n, base)
    M = _mapped(X, ids)
    sel = _selector(name, n, ids, base)
    gone = _allowed(sel, ids)
    if name == "all":
        assert gone.all()
    if name == "nothing":
        assert not gone.any()
    _check_removed(M, X, ids, gone, M.remove_ids(sel))
    assert M.has_ids


def test_remove_ids_through_the_bounce_buffer():
    n, d = 4099, 512
    X, ids = _rows(n, d), _labels(n, BIG)
    M = _mapped(X, ids, env={"IVR_REMOVE_CHUNK_ROWS": "64"})
    sel = _selector("batch", n, ids, BIG)
    _check_removed(M, X, ids, _allowed(sel, ids), M.remove_ids(sel))


def test_remove_then_add_with_ids():
    n, d = 1000, 512
    X, ids = _rows(n, d), _labels(n)
    M = _mapped(X, ids)
    arr = ids[100:400:3].copy()                      # an integer array: wrapped in IDSelectorBatch, naming stored ids
    gone = np.isin(ids, arr)
    assert M.remove_ids(arr) == int(gone.sum()) == len(arr)
    X2, ids2 = _rows(4099, d)[:300], 20 * n + np.arange(300, dtype=np.int64)[::-1]
    M.add_with_ids(X2, ids2)
    Xa, ia = np.concatenate([X[~gone], X2]), np.concatenate([ids[~gone], ids2])
    assert np.array_equal(M.id_map, ia) and np.array_equal(_bits(M.reconstruct_n()), _bits(Xa))
    P = _plain(Xa)
    Q = np.concatenate([X[~gone][:2], X2[:2]])
    Dp, Ip = P.search(Q, 10)
    Dm, Im = M.search(Q, 10)
    assert np.array_equal(_bits(Dm), _bits(Dp)) and np.array_equal(Im, _translate(Ip, ia))
    assert set(Im[:, 0]) == {int(ia[0]), int(ia[1]), int(ids2[0]), int(ids2[1])}      # old labels survive, new ones appear
    assert not np.isin(Im, arr).any()


def test_duplicate_ids():
    from ivr_amd.index import IDSelectorBatch, SearchParameters
    n, d = 1000, 20
    X, ids = _rows(n, d), _labels(n).copy()
    ids[640] = ids[33]
    M = _mapped(X, ids)
    dup = int(ids[33])
    assert list(M.find([dup])) == [33]
    D, I = M.search(_queries(3, d), 5, params=SearchParameters(sel=IDSelectorBatch([dup])))
    assert (I[:, :2] == dup).all() and (I[:, 2:] == -1).all()
    lims, Dr, Ir = M.range_search(_queries(3, d), -2.0, params=SearchParameters(sel=IDSelectorBatch([dup])))
    assert list(lims) == [0, 2, 4, 6]
    assert M.remove_ids(np.array([dup])) == 2
    gone = np.zeros(n, bool)
    gone[[33, 640]] = True
    _check_removed(M, X, ids, gone, 2)
    assert list(M.find([dup])) == [-1]


def test_lookup_and_reconstruct():
    n, d = 4099, 512
    X, ids, P, M = _pair(n, d)
    assert list(M.find(ids[[0, n - 1, 77]])) == [0, n - 1, 77]
    absent = int(np.setdiff1d(np.arange(10 * n), ids)[0])
    assert list(M.find([absent, int(ids[5])])) == [-1, 5]
    assert list(M.find(torch.tensor([int(ids[9])]))) == [9]
    assert np.array_equal(_bits(M.reconstruct(int(ids[77]))), _bits(P.reconstruct(77)))
    assert np.array_equal(_bits(M.reconstruct_n(77, 2)), _bits(X[77:79]))          # positional
    with pytest.raises(RuntimeError):
        M.reconstruct(absent)
    Xb, idb, Pb, Mb = _pair(1000, 20, BIG)
    assert list(Mb.find(idb[[999, 3]])) == [999, 3] and list(Mb.find([int(idb[3]) - BIG])) == [-1]


def test_mode_rules():
    from ivr_amd.index import FlatIPIndex, IndexFlatIP, IndexIDMap, IndexIDMap2
    d = 20
    X, ids = _rows(1000, d), _labels(1000)
    M = _mapped(X[:10], ids[:10])
    with pytest.raises((ValueError, RuntimeError)):
        M.add(X[10:20])
    assert M.ntotal == 10
    P = _plain(X[:10])
    with pytest.raises((ValueError, RuntimeError)):
        P.add_with_ids(X[10:20], ids[10:20])
    assert P.ntotal == 10 and not P.has_ids
    E = FlatIPIndex(d)
    for bad in (np.array([1, 2, -1]), np.array([1, 2]), np.array([1.0, 2.0, 3.0]), torch.tensor([0.5, 1.0, 2.0])):
        with pytest.raises(ValueError):
            E.add_with_ids(X[:3], bad)
    assert E.ntotal == 0 and not E.has_ids
    with pytest.raises(ValueError):
        IndexIDMap2(P)
    for wrap in (IndexIDMap, IndexIDMap2):
        W = wrap(IndexFlatIP(d))
        assert W.has_ids and W.ntotal == 0
        with pytest.raises((ValueError, RuntimeError)):
            W.add(X[:5])
        W.add_with_ids(X[:5], torch.from_numpy(ids[:5]))
        assert np.array_equal(W.search(X[:1], 1)[1], ids[:1].reshape(1, 1))
        W.reset()
        assert not W.has_ids and W.ntotal == 0
        W.add(X[:5])                                  # plain again
        assert np.array_equal(W.search(X[:1], 1)[1], [[0]])
    M.reset()
    assert not M.has_ids
    M.add(X[:4])
    assert M.search(X[3:4], 1)[1][0, 0] == 3


def test_id_table_grows_with_the_rows():
    d = 20
    X = np.concatenate([_rows(4099, d), _rows(1000, d), _rows(1000, d)[:1]])       # 5100 rows
    ids = _labels(len(X), BIG)
    M = _mapped(X[:100], ids[:100], capacity=64)
    M.add_with_ids(X[100:], ids[100:])
    assert M.ntotal == 5100 and np.array_equal(M.id_map, ids)
    assert np.array_equal(_bits(M.reconstruct_n()), _bits(X))
    assert list(M.find(ids[[0, 99, 100, 5099]])) == [0, 99, 100, 5099]


def test_filtered_search_is_graph_capturable():
    """A filtered search on an id-mapped index holds no host synchronisation: it captures into a graph, and the replay equals the
    plain launch bit for bit."""
    n, d, k = 4099, 512, 10
    X, ids, P, M = _pair(n, d, BIG)
    sel = _selector("batch", n, ids, BIG)
    dev = M.device
    Q = torch.from_numpy(_queries(5, d)).to(dev)
    De, Ie = M.search_device(Q, k, sel=sel)
    De, Ie = De.clone(), Ie.clone()
    D = torch.zeros((5, k), dtype=torch.float32, device=dev)
    I = torch.zeros((5, k), dtype=torch.int64, device=dev)
    M.reserve_search(5, k)
    s = torch.cuda.Stream(device=dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        M.search_device(Q, k, out=(D, I), sel=sel)
    torch.cuda.current_stream(dev).wait_stream(s)
    torch.cuda.synchronize(dev)
    D.zero_()
    I.zero_()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        M.search_device(Q, k, out=(D, I), sel=sel)
    g.replay()
    torch.cuda.synchronize(dev)
    assert torch.equal(D.view(torch.int32), De.view(torch.int32)) and torch.equal(I, Ie)
    from ivr_amd.index import IDSelectorBatch, SearchParameters
    Dp, Ip = P.search(Q.cpu().numpy(), k, params=SearchParameters(sel=IDSelectorBatch(np.flatnonzero(_allowed(sel, ids)))))
    assert np.array_equal(_bits(D.cpu().numpy()), _bits(Dp)) and np.array_equal(I.cpu().numpy(), _translate(Ip, ids))
