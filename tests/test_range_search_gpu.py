"""GPU suite: exact range search (FlatIPIndex.range_search / ivr_index_range_search).

The reference for every case is this build's own top-k search: for each query the range result must equal, bit for bit, the
entries of search(q, 2048) that score > radius, re-ordered by ascending id (radii are chosen so that no query has more than 2048
hits).  A float64 brute force checks the ids away from the radius and the scores to 1e-5."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

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


def _expected(idx, Q, radius, normalize=False, id_base=0):
    """(lims, D, I) from search(q, 2048): the entries > radius of each query, in ascending id order."""
    Dt, It = idx.search_device(Q, 2048, normalize=normalize, id_base=id_base)
    D, I = Dt.cpu().numpy(), It.cpu().numpy()
    lims, Ds, Is = [0], [], []
    for d, i in zip(D, I):
        keep = (d > radius) & (i >= 0)
        assert keep.sum() < 2048, "radius too low for the top-k reference"
        o = np.argsort(i[keep], kind="stable")
        Ds.append(d[keep][o])
        Is.append(i[keep][o])
        lims.append(lims[-1] + int(keep.sum()))
    return np.array(lims, np.int64), np.concatenate(Ds).astype(np.float32), np.concatenate(Is).astype(np.int64)


def _assert_same(got, want):
    lims, D, I = got
    lr, Dr, Ir = want
    assert np.array_equal(lims, lr), (lims[:8], lr[:8])
    assert np.array_equal(I, Ir)
    assert np.array_equal(D.view(np.uint32), Dr.view(np.uint32))       # bit for bit


def _check_f64(got, X, Q, radius):
    lims, D, I = got
    S = Q.astype(np.float64) @ X.astype(np.float64).T
    for q in range(len(Q)):
        ids = I[lims[q]:lims[q + 1]]
        s = S[q]
        firm = np.abs(s - radius) > 1e-5
        ref = np.nonzero((s > radius) & firm)[0]
        assert np.array_equal(ids[firm[ids]], ref)
        assert np.all(np.diff(ids) > 0)
        assert np.abs(D[lims[q]:lims[q + 1]] - s[ids]).max(initial=0) <= 1e-5


@pytest.fixture(scope="module")
def base20k():
    rng = np.random.default_rng(2024)
    X = _unit(rng, 20000, 512)
    Q = _unit(rng, 130, 512)
    return X, Q, _index(X)


@pytest.mark.parametrize("nq", [1, 10, 64, 130])
def test_bit_exact_against_topk_and_float64(base20k, nq):
    X, Q, idx = base20k
    Q = Q[:nq]
    D0, _ = idx.search(Q[:1], 300)
    radius = float(D0[0, 299])
    got = idx.range_search(Q, radius)
    _assert_same(got, _expected(idx, Q, radius))
    _check_f64(got, X, Q, radius)
    assert got[0][-1] >= 299


def test_bound_stress_bf16_and_exact_scan_agree():
    rng = np.random.default_rng(7)
    d, radius = 512, 0.3
    X = _unit(rng, 30000, d)
    Q = _unit(rng, 4, d)
    # 250 rows per query whose exact score lies within +-2e-3 of the radius (wider than the bf16 error bound of ~4e-3 / 2)
    for qi in range(4):
        rows = rng.choice(len(X), 250, replace=False)
        c = radius + rng.uniform(-2e-3, 2e-3, 250)
        u = rng.standard_normal((250, d))
        u -= (u @ Q[qi].astype(np.float64))[:, None] * Q[qi].astype(np.float64)[None, :]
        u /= np.linalg.norm(u, axis=1, keepdims=True)
        X[rows] = (c[:, None] * Q[qi] + np.sqrt(1 - c[:, None] ** 2) * u).astype(np.float32)
    fast = _index(X)
    assert fast.scan_stats()[0]
    got = fast.range_search(Q, radius)
    want = _expected(fast, Q, radius)
    _assert_same(got, want)
    assert np.all(np.diff(got[0]) >= 100)
    exact = _index(X, {"IVR_SCAN_BF16": "0"})
    assert not exact.scan_stats()[0]
    _assert_same(exact.range_search(Q, radius), got)


def test_ntotal_not_a_multiple_and_dense_minus_inf():
    rng = np.random.default_rng(11)
    X = _unit(rng, 100003, 96)
    Q = _unit(rng, 10, 96)
    idx = _index(X)
    D0, _ = idx.search(Q[:1], 500)
    radius = float(D0[0, 499])
    got = idx.range_search(Q, radius)
    _assert_same(got, _expected(idx, Q, radius))
    _check_f64(got, X, Q, radius)
    # every row of every query (dense: every group is a candidate, the output outgrows the first-guess capacity)
    lims, D, I = idx.range_search(Q[:3], -np.inf)
    assert lims.tolist() == [0, 100003, 200006, 300009]
    assert np.array_equal(I, np.tile(np.arange(100003), 3))
    S = (Q[:3].astype(np.float64) @ X.astype(np.float64).T).reshape(-1)
    assert np.abs(D - S).max() < 1e-5


def test_minus_inf_small_index_returns_every_row():
    rng = np.random.default_rng(12)
    X = _unit(rng, 1000, 512)
    Q = _unit(rng, 10, 512)
    idx = _index(X)
    lims, D, I = idx.range_search(Q, -np.inf)
    assert np.array_equal(lims, np.arange(11) * 1000)
    assert np.array_equal(I, np.tile(np.arange(1000), 10))
    Dt, It = idx.search(Q, 1000)
    for q in range(10):
        o = np.argsort(It[q])
        assert np.array_equal(D[q * 1000:(q + 1) * 1000].view(np.uint32), Dt[q][o].view(np.uint32))


def test_no_hits_and_empty_index():
    rng = np.random.default_rng(13)
    X = _unit(rng, 5000, 64)
    Q = _unit(rng, 5, 64)
    lims, D, I = _index(X).range_search(Q, 1.5)
    assert lims.tolist() == [0] * 6 and len(D) == 0 and len(I) == 0
    from ivr_amd.index import FlatIPIndex
    lims, D, I = FlatIPIndex(64).range_search(Q, -np.inf)
    assert lims.tolist() == [0] * 6 and len(D) == 0 and len(I) == 0


def test_duplicates_id_base_and_normalize():
    rng = np.random.default_rng(14)
    X = _unit(rng, 8000, 512)
    X[4321] = X[17]
    X[7999] = X[17]
    Q = rng.standard_normal((3, 512)).astype(np.float32) * 3.0
    Q[0] = X[17] * 5.0
    idx = _index(X)
    lims, D, I, total = idx.range_search_device(Q, 0.2, normalize=True, id_base=1000)
    lims, D, I = lims.cpu().numpy(), D.cpu().numpy(), I.cpu().numpy()
    assert int(total.item()) == lims[-1] == len(D)
    _assert_same((lims, D, I), _expected(idx, Q, 0.2, normalize=True, id_base=1000))
    assert {1017, 5321, 8999} <= set(I[lims[0]:lims[1]].tolist())
    Qn = Q / np.linalg.norm(Q, axis=1, keepdims=True)
    _check_f64((lims, D, I - 1000), X, Qn, 0.2)


def test_capacity_smaller_than_total():
    rng = np.random.default_rng(15)
    X = _unit(rng, 20000, 512)
    Q = _unit(rng, 12, 512)
    idx = _index(X)
    radius = float(idx.search(Q[:1], 200)[0][0, 199])
    full = idx.range_search(Q, radius)
    n = int(full[0][-1])
    cap = n // 3
    lims, D, I, total = idx.range_search_device(Q, radius, cap=cap)
    assert int(total.item()) == n and np.array_equal(lims.cpu().numpy(), full[0])
    assert len(D) == cap and np.array_equal(I.cpu().numpy(), full[2][:cap])
    assert np.array_equal(D.cpu().numpy().view(np.uint32), full[1][:cap].view(np.uint32))
    # the numpy wrapper re-calls with the exact capacity when its first guess is short
    lims2, D2, I2 = idx.range_search(np.repeat(Q, 20, axis=0), -np.inf)
    assert lims2[-1] == 240 * 20000 and np.array_equal(I2[-20000:], np.arange(20000))


def test_invalid_arguments_raise_before_launch():
    from ivr_amd import _ffi
    rng = np.random.default_rng(16)
    idx = _index(_unit(rng, 1000, 64))
    Q = _unit(rng, 2, 64)
    with pytest.raises(ValueError):
        idx.range_search(Q, float("nan"))
    with pytest.raises(ValueError):
        idx.range_search(_unit(rng, 2, 32), 0.1)
    # the C ABI rejects a NaN radius, nq < 1, cap < 0 and NULL pointers itself
    lib = _ffi.load()
    q = torch.from_numpy(Q).cuda()
    lims = torch.zeros(3, dtype=torch.int64, device="cuda")
    D = torch.zeros(4, device="cuda")
    I = torch.zeros(4, dtype=torch.int64, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())
    call = lambda *a: lib.ivr_index_range_search(idx._h, *a, _ffi.stream_ptr())
    assert call(p(q), 2, C.c_float(float("nan")), 0, 0, p(lims), p(D), p(I), 4) == -1
    assert call(p(q), 0, C.c_float(0.1), 0, 0, p(lims), p(D), p(I), 4) == -1
    assert call(p(q), 2, C.c_float(0.1), 0, 0, p(lims), p(D), p(I), -1) == -1
    assert call(p(q), 2, C.c_float(0.1), 0, 0, None, p(D), p(I), 4) == -1
    torch.cuda.synchronize()
    assert lims.cpu().tolist() == [0, 0, 0]


def test_full_size_1m():
    from ivr_amd.index import FlatIPIndex
    g = torch.Generator(device="cuda").manual_seed(99)
    X = torch.randn((1 << 20) - 7, 512, device="cuda", generator=g)
    X /= X.norm(dim=1, keepdim=True)
    Q = torch.randn(10, 512, device="cuda", generator=g)
    Q /= Q.norm(dim=1, keepdim=True)
    idx = FlatIPIndex(512, capacity=X.shape[0])
    idx.add(X)
    del X
    torch.cuda.empty_cache()
    radius = float(idx.search(Q[:1], 300)[0][0, 299])
    got = idx.range_search(Q, radius)
    _assert_same(got, _expected(idx, Q, radius))
    assert np.all(np.diff(got[0]) > 50)


def test_three_shards_merge_like_one_index():
    from ivr_amd.sharded import merge_range, pack_range, shard_bounds
    rng = np.random.default_rng(17)
    X = _unit(rng, 30001, 512)
    Q = _unit(rng, 20, 512)
    whole = _index(X)
    radius = float(whole.search(Q[:1], 400)[0][0, 399])
    want = whole.range_search(Q, radius)
    parts = []
    for lo, hi in shard_bounds(len(X), 3):
        sh = _index(X[lo:hi])
        parts.append(sh.range_search_device(Q, radius, id_base=lo))
    counts = torch.stack([lims[1:] - lims[:-1] for lims, _, _, _ in parts])
    width = int(counts.sum(1).max().item())
    packed = torch.stack([pack_range(D, I, int(lims[-1].item()), width) for lims, D, I, _ in parts])
    lims, D, I = merge_range(counts, packed)
    _assert_same((lims.cpu().numpy(), D.cpu().numpy(), I.cpu().numpy()), want)
