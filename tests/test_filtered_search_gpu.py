"""GPU suite: filtered search (SearchParameters(sel=IDSelector...) on FlatIPIndex.search / range_search).

The reference for every case is this build's own unfiltered search over the sub-index FlatIPIndex(X[allowed]) with its ids mapped back
through `allowed`: D bit for bit, I equal.  A float64 brute force over the same subset checks the ids away from near-ties."""
import os

import numpy as np
import pytest
import torch

from oracle import search_ref as S

pytestmark = pytest.mark.gpu


def _unit(rng, n, d):
    x = rng.standard_normal((n, d)).astype(np.float32)
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def _index(X, env=None):
    from ivr_amd.index import FlatIPIndex
    old = {k: os.environ.get(k) for k in (env or {})}
    os.environ.update(env or {})
    try:
        idx = FlatIPIndex(X.shape[1], capacity=len(X))
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v
    if len(X):
        idx.add(X)
    return idx


def _params(sel):
    from ivr_amd.index import SearchParameters
    return SearchParameters(sel=sel)


def _bitmap_sel(mask):
    from ivr_amd.index import IDSelectorBitmap
    return IDSelectorBitmap(np.packbits(mask, bitorder="little"))


def _reference(X, Q, k, allowed, env=None, id_base=0):
    """(D, I) of the unfiltered search over X[allowed], ids mapped back (id_base + row)."""
    k_sub = k
    D = np.full((len(Q), k), np.float32(-np.finfo(np.float32).max), np.float32)
    I = np.full((len(Q), k), -1, np.int64)
    if len(allowed) == 0:
        return D, I
    sub = _index(X[allowed], env)
    Ds, Is = sub.search(Q, k_sub)
    ok = Is >= 0
    D[ok] = Ds[ok]
    I[ok] = id_base + allowed[Is[ok]]
    sub.close()
    return D, I


def _assert_same(got, want):
    D, I = got
    Dr, Ir = want
    assert np.array_equal(I, Ir), np.nonzero((I != Ir).any(1))[0][:8]
    assert np.array_equal(D.view(np.uint32), Dr.view(np.uint32))


def _check_f64(got, X, Q, allowed, id_base=0):
    """ids against float64 over the allowed rows, where the k-th score is separated from the next by > 1e-6."""
    D, I = got
    k = D.shape[1]
    if len(allowed) == 0:
        assert (I == -1).all()
        return
    Dr, Ir = S.flat_ip_search(X[allowed], Q, min(k, len(allowed)), dtype=np.float64)
    for q in range(len(Q)):
        n = min(k, len(allowed))
        s = np.sort(Q[q].astype(np.float64) @ X[allowed].astype(np.float64).T)[::-1]
        gaps = np.abs(np.diff(s[:n + 1])) if len(s) > n else np.ones(n)
        firm = gaps[:n] > 1e-6 if len(s) > n else np.ones(n, bool)
        if firm.all():
            assert set(I[q, :n]) == set(id_base + allowed[Ir[q, :n]])
        assert (I[q, n:] == -1).all()


def _search(idx, Q, k, sel, id_base=0):
    D, I = idx.search_device(Q, k, id_base=id_base, sel=sel)
    return D.cpu().numpy(), I.cpu().numpy()


@pytest.fixture(scope="module")
def base50k():
    rng = np.random.default_rng(77)
    X = _unit(rng, 50000, 512)
    Q = _unit(rng, 16, 512)
    return X, Q, _index(X)


def test_full_bitmap_equals_plain_search(base50k):
    X, Q, idx = base50k
    sel = _bitmap_sel(np.ones(len(X), bool))
    got = idx.search(Q, 10, params=_params(sel))
    _assert_same(got, idx.search(Q, 10))


@pytest.mark.parametrize("frac", [0.5, 0.01])
def test_random_bitmaps(base50k, frac):
    X, Q, idx = base50k
    rng = np.random.default_rng(int(frac * 1000))
    mask = rng.random(len(X)) < frac
    allowed = np.flatnonzero(mask)
    got = idx.search(Q, 10, params=_params(_bitmap_sel(mask)))
    _assert_same(got, _reference(X, Q, 10, allowed))
    _check_f64(got, X, Q, allowed)


@pytest.mark.parametrize("n_allowed", [20, 5, 0])
def test_sparse_bitmaps(base50k, n_allowed):
    X, Q, idx = base50k
    rng = np.random.default_rng(n_allowed)
    allowed = np.sort(rng.choice(len(X), n_allowed, replace=False))
    mask = np.zeros(len(X), bool)
    mask[allowed] = True
    got = idx.search(Q, 10, params=_params(_bitmap_sel(mask)))
    _assert_same(got, _reference(X, Q, 10, allowed))
    _check_f64(got, X, Q, allowed)


def test_unaligned_range_and_range_and_bitmap(base50k):
    from ivr_amd.index import IDSelectorRange
    X, Q, idx = base50k
    got = idx.search(Q, 10, params=_params(IDSelectorRange(12345, 37891)))
    allowed = np.arange(12345, 37891)
    _assert_same(got, _reference(X, Q, 10, allowed))
    _check_f64(got, X, Q, allowed)
    # range intersected with a bitmap
    rng = np.random.default_rng(5)
    mask = rng.random(len(X)) < 0.3
    from ivr_amd.index import IDSelectorBitmap
    sel = IDSelectorBitmap(np.packbits(mask, bitorder="little"), lo=777, hi=40001)
    allowed = np.flatnonzero(mask[777:40001]) + 777
    got = idx.search(Q, 10, params=_params(sel))
    _assert_same(got, _reference(X, Q, 10, allowed))


def test_batch_duplicates_and_out_of_range(base50k):
    from ivr_amd.index import IDSelectorBatch
    X, Q, idx = base50k
    ids = np.array([49999, 3, 3, 17, 20000, 20001, 20001, 10 ** 7, -5, 4096, 4097, 31337], np.int64)
    got = idx.search(Q, 10, params=_params(IDSelectorBatch(ids)))
    allowed = np.array(sorted({int(i) for i in ids if 0 <= i < len(X)}), np.int64)
    _assert_same(got, _reference(X, Q, 10, allowed))


def test_id_base_not_multiple_of_8(base50k):
    X, Q, idx = base50k
    id_base = 1000003
    rng = np.random.default_rng(9)
    mask = np.zeros(id_base + len(X), bool)
    mask[id_base:] = rng.random(len(X)) < 0.05
    allowed = np.flatnonzero(mask[id_base:])
    got = _search(idx, Q, 10, _bitmap_sel(mask), id_base=id_base)
    _assert_same(got, _reference(X, Q, 10, allowed, id_base=id_base))


def test_duplicate_row_lower_copy_excluded():
    rng = np.random.default_rng(11)
    X = _unit(rng, 20000, 512)
    Q = _unit(rng, 4, 512)
    X[15000] = Q[0]
    X[300] = Q[0]                       # same row at a lower id
    idx = _index(X)
    D, I = idx.search(Q, 5)
    assert I[0, 0] == 300 and I[0, 1] == 15000
    mask = np.ones(len(X), bool)
    mask[300] = False
    got = idx.search(Q, 5, params=_params(_bitmap_sel(mask)))
    assert got[1][0, 0] == 15000
    assert got[0][0, 0].view(np.uint32) == D[0, 1].view(np.uint32)
    _assert_same(got, _reference(X, Q, 5, np.flatnonzero(mask)))


@pytest.mark.parametrize("d", [768, 100])
def test_other_dims(d):
    rng = np.random.default_rng(d)
    X = _unit(rng, 30000, d)
    Q = _unit(rng, 10, d)
    idx = _index(X)
    mask = rng.random(len(X)) < 0.1
    allowed = np.flatnonzero(mask)
    got = idx.search(Q, 10, params=_params(_bitmap_sel(mask)))
    _assert_same(got, _reference(X, Q, 10, allowed))
    _check_f64(got, X, Q, allowed)


def test_float32_scan_only():
    env = {"IVR_SCAN_BF16": "0"}
    rng = np.random.default_rng(3)
    X = _unit(rng, 30000, 512)
    Q = _unit(rng, 10, 512)
    idx = _index(X, env)
    mask = rng.random(len(X)) < 0.02
    allowed = np.flatnonzero(mask)
    got = idx.search(Q, 10, params=_params(_bitmap_sel(mask)))
    _assert_same(got, _reference(X, Q, 10, allowed, env))


@pytest.mark.parametrize("nq,k", [(1, 1), (10, 50), (64, 128), (65, 10), (1000, 10), (1100, 129), (10, 2048), (65, 129)])
def test_shapes(nq, k):
    rng = np.random.default_rng(nq * 7 + k)
    X = _unit(rng, 60000, 512)
    Q = _unit(rng, nq, 512)
    idx = _index(X)
    mask = rng.random(len(X)) < 0.2
    mask[:1000] = False
    allowed = np.flatnonzero(mask)
    got = idx.search(Q, k, params=_params(_bitmap_sel(mask)))
    _assert_same(got, _reference(X, Q, k, allowed))


def test_range_search_filtered(base50k):
    X, Q, idx = base50k
    rng = np.random.default_rng(21)
    mask = rng.random(len(X)) < 0.25
    allowed = np.flatnonzero(mask)
    from ivr_amd.index import IDSelectorBitmap
    sel = IDSelectorBitmap(np.packbits(mask, bitorder="little"), lo=1234, hi=45678)
    allowed = allowed[(allowed >= 1234) & (allowed < 45678)]
    lims, D, I = idx.range_search(Q, 0.12, params=_params(sel))
    sub = _index(X[allowed])
    lr, Dr, Ir = sub.range_search(Q, 0.12)
    assert lims[-1] > 0
    assert np.array_equal(lims, lr)
    assert np.array_equal(I, allowed[Ir])
    assert np.array_equal(D.view(np.uint32), Dr.view(np.uint32))
    # radius -inf: exactly the allowed rows, for every query
    from ivr_amd.index import IDSelectorRange
    lims, D, I = idx.range_search(Q[:3], -np.inf, params=_params(IDSelectorRange(4000, 4100)))
    assert np.array_equal(lims, [0, 100, 200, 300])
    assert np.array_equal(I, np.tile(np.arange(4000, 4100), 3))


@pytest.fixture(scope="module")
def big1m():
    rng = np.random.default_rng(1)
    X = _unit(rng, 1_000_000, 512)
    Q = _unit(rng, 1000, 512)
    return X, Q, _index(X)


@pytest.mark.parametrize("nq", [10, 1000])
def test_1m_rows(big1m, nq):
    from ivr_amd.index import IDSelectorBatch
    X, Q, idx = big1m
    rng = np.random.default_rng(nq)
    ids = np.concatenate([c + np.arange(100) for c in rng.choice(999_900, 10, replace=False)])
    allowed = np.unique(ids)
    got = idx.search(Q[:nq], 10, params=_params(IDSelectorBatch(ids)))
    _assert_same(got, _reference(X, Q[:nq], 10, allowed))
    mask = rng.random(len(X)) < 0.1
    got = idx.search(Q[:nq], 10, params=_params(_bitmap_sel(mask)))
    _assert_same(got, _reference(X, Q[:nq], 10, np.flatnonzero(mask)))


@pytest.mark.parametrize("nq,n_allowed", [(10, 20), (10, 0), (65, 5), (65, 0), (1000, 5), (1000, 0)])
def test_sparse_filters_stay_on_fast_path(big1m, nq, n_allowed):
    """The -inf sentinel: a bitmap over the whole index that allows fewer rows than k (or none) passes the verification of the bf16
    candidate scan, on the <= 64-query scans (nq 10) and on the large-batch scan with its tile pruning (nq 65, 1000)."""
    X, Q, idx = big1m
    rng = np.random.default_rng(nq + n_allowed + 1)
    mask = np.zeros(len(X), bool)
    mask[rng.choice(len(X), n_allowed, replace=False)] = True
    got = idx.search(Q[:nq], 10, params=_params(_bitmap_sel(mask)))
    assert idx.scan_stats() == (True, 0)
    _assert_same(got, _reference(X, Q[:nq], 10, np.flatnonzero(mask)))


def test_range_restriction_reads_less(big1m):
    from ivr_amd import _ffi
    from ivr_amd.index import IDSelectorRange
    X, Q, idx = big1m
    dev = idx.device.index

    def scan_work(sel):
        idx.search(Q[:10], 10)                                # warm
        _ffi.profile_enable(2, dev)
        _ffi.profile_reset(dev)
        if sel is None:
            idx.search(Q[:10], 10)
        else:
            idx.search(Q[:10], 10, params=_params(sel))
        prof = _ffi.profile_read(dev)
        _ffi.profile_enable(0, dev)
        return sum(v["work"] for name, v in prof.items() if "scan" in name)

    full = scan_work(None)
    part = scan_work(IDSelectorRange(500_000, 510_000))
    assert full > 0 and part <= 0.02 * full, (part, full)


def test_bad_selectors_raise():
    from ivr_amd.index import IDSelectorBatch, IDSelectorBitmap, SearchParameters
    rng = np.random.default_rng(0)
    idx = _index(_unit(rng, 1000, 64))
    Q = _unit(rng, 2, 64)
    with pytest.raises(ValueError):
        idx.search(Q, 5, params={"sel": None})
    with pytest.raises(ValueError):
        SearchParameters(sel=lambda i: True)
    with pytest.raises(ValueError):
        IDSelectorBitmap(np.zeros(8, np.int32))
    with pytest.raises(ValueError):
        IDSelectorBatch(np.array([1.5, 2.0]))
    with pytest.raises(ValueError):
        idx.search_device(Q, 5, sel="all")
    with pytest.raises(ValueError):
        idx.range_search(Q, 0.5, params=object())


def test_compat_prefilter(tmp_path):
    from ivr_amd.compat import UnifiedIndex
    rng = np.random.default_rng(42)
    ui = UnifiedIndex()
    n, folders = 6000, 30
    V = _unit(rng, n, 512)
    metas = [{"folder_name": f"video_{i * folders // n:03d}", "image_name": f"{i}.jpg", "vector_index": i} for i in range(n)]
    ui._install(V, metas, str(tmp_path / "x.npz"))
    q = V[4321] + 0.1 * _unit(rng, 1, 512)[0]
    want = "video_007"
    out = ui.search_vectors(q, k=10, filter_func=lambda m: m["folder_name"] == want, prefilter=True)
    assert len(out) == 10
    assert all(r["metadata"]["folder_name"] == want for r in out)
    assert [r["rank"] for r in out] == list(range(10))
    allowed = np.array([i for i, m in enumerate(metas) if m["folder_name"] == want])
    qn = (q / np.linalg.norm(q)).astype(np.float32)[None]
    _, Ir = S.flat_ip_search(V[allowed], qn, 10, dtype=np.float64)
    assert [r["index"] for r in out] == list(allowed[Ir[0]])
    # the default keeps the reference's filter-after-top-k behaviour
    base = ui.search_vectors(q, k=10)
    post = ui.search_vectors(q, k=10, filter_func=lambda m: m["folder_name"] == want)
    assert [r for r in base if r["metadata"]["folder_name"] == want] == post
