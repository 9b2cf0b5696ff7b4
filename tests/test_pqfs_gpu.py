"""GPU suite of the 4-bit product-quantisation index (ivr_amd/pqfs.py, csrc/search_pqfs.hip): the store, the encoder, the table
builder and quantiser and the in-register scan against the numpy definitions of ivr_amd/pqfs.py, to the bit wherever they say so."""
import numpy as np
import pytest

from ivr_amd import _ffi
from ivr_amd.pqfs import (IndexPQFastScan, pqfs_encode_ref, pqfs_pack_ref, pqfs_quantize_ref, pqfs_scan_ref, pqfs_score_bound,
                          pqfs_tables_ref, pqfs_unpack_ref)

pytestmark = pytest.mark.gpu
F = np.float32
FLT_MAX = np.finfo(np.float32).max
NS = (1, 63, 64, 65, 255, 256, 257, 1000, 1100)  # both sides of a 64-row group and of a 256-row block; 1100: a second unit of 4 blocks
MS = (2, 6, 16, 30, 64, 128, 256)                # one pair, widths that are no whole 16-byte words, the limit
KS = (1, 10, 2048)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same(got, want):
    assert np.array_equal(got[1], want[1])
    assert np.array_equal(_bits(got[0]), _bits(want[0]))


def _pass():
    return int(_ffi.load().ivr_pqfs_pass_queries())


def _index(M, dsub=1):
    """An index of M sub-quantizers that takes codes: any codebook makes it trained."""
    idx = IndexPQFastScan(M * dsub, M)
    idx.centroids = np.zeros((M, 16, dsub), F)
    return idx


def _codes(rng, n, M):
    return rng.integers(0, 256, (n, M // 2)).astype(np.uint8)


def _tables(rng, nq, M):
    """Random 8-bit tables with 0 and 255 in them, scales of both signs of exponent and biases of both signs."""
    U = rng.integers(0, 256, (nq, M, 16)).astype(np.uint8)
    U[:, :, 3] = 255
    U[:, ::2, 12] = 0
    scale = (rng.uniform(0.5, 2.0, nq) * rng.choice([1e-3, 1.0, 50.0], nq)).astype(F)
    bias = (rng.standard_normal(nq) * 100).astype(F)
    return U, scale, bias


def _check_scan(idx, U, scale, bias, codes, P):
    """Every (nq, k) of the issue against one reference: the ranking is a total order, so fewer queries and a smaller k are
    prefixes of the widest result."""
    n = len(codes)
    want = pqfs_scan_ref(U, scale, bias, codes, max(KS))
    for nq in (1, 2, 3, P, P + 1, 2 * P + 1):             # 2 and 3: the narrower passes of a small call; 2 P + 1: four blocks per wave
        for k in KS:
            D, I = idx.search_tables(U[:nq], scale[:nq], bias[:nq], k)
            assert D.shape == (nq, k) and I.dtype == np.int64
            _same((D, I), (want[0][:nq, :k], want[1][:nq, :k]))
            if k > n:
                assert (I[:, n:] == -1).all() and (D[:, n:] == -FLT_MAX).all()


# -- scan and store ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", MS)
def test_scan_equals_the_definition_and_the_store_returns_its_codes(M):
    P = _pass()
    rng = np.random.default_rng(M)
    U, scale, bias = _tables(rng, 2 * P + 1, M)
    for n in NS:
        codes = _codes(rng, n, M)
        idx = _index(M)
        idx.add_codes(codes)
        assert idx.ntotal == n
        got = idx.codes
        assert got.dtype == np.uint8 and got.shape == (n, M // 2) and np.array_equal(got, codes)
        lo = max(0, n - 70)
        assert np.array_equal(idx._index._codes_device(lo, n - lo).cpu().numpy(), codes[lo:])
        _check_scan(idx, U, scale, bias, codes, P)
        idx.close()


@pytest.mark.parametrize("M", (6, 128))
def test_scan_over_a_store_grown_by_ragged_adds(M):
    P = _pass()
    rng = np.random.default_rng(50 + M)
    U, scale, bias = _tables(rng, 2 * P + 1, M)
    codes = _codes(rng, 1000, M)
    idx = _index(M)
    at = 0
    for step in (1, 62, 1, 1, 191, 1, 300, 443):                    # ends on and beside group and block edges; the store grows
        idx.add_codes(codes[at:at + step])
        at += step
        assert idx.ntotal == at and np.array_equal(idx.codes, codes[:at])
    assert at == 1000
    _check_scan(idx, U, scale, bias, codes, P)
    # reset, then add: the block is reused and what it held is not seen
    idx.reset()
    assert idx.ntotal == 0
    D, I = idx.search_tables(U[:3], scale[:3], bias[:3], 4)
    assert (I == -1).all() and (D == -FLT_MAX).all()
    fewer = _codes(rng, 130, M)
    idx.add_codes(fewer)
    assert np.array_equal(idx.codes, fewer)
    _same(idx.search_tables(U, scale, bias, 200), pqfs_scan_ref(U, scale, bias, fewer, 200))
    idx.close()


def test_scan_query_cap_second_chunk_of_one_query():
    """A chunk holds 4096 queries at most: query 4096 of 4097 is a chunk of its own (c0 = 4096).  100 rows of one-byte codes, tables
    supplied through search_tables."""
    rng = np.random.default_rng(21)
    U, scale, bias = _tables(rng, 4097, 2)
    codes = _codes(rng, 100, 2)
    idx = _index(2)
    idx.add_codes(codes)
    _same(idx.search_tables(U, scale, bias, 3), pqfs_scan_ref(U, scale, bias, codes, 3))
    idx.close()


def test_nibble_order_is_faiss():
    M = 6
    idx = _index(M)
    nib = np.array([[1, 2, 3, 4, 5, 6], [15, 0, 0, 15, 7, 8]], np.uint8)
    idx.add_codes(pqfs_pack_ref(nib))
    assert np.array_equal(idx.codes, np.array([[0x21, 0x43, 0x65], [0x0f, 0xf0, 0x87]], np.uint8))
    # table m scores entry j with 16 m + j + 1 for m < 5 and 0 beyond: acc names the nibbles the scan saw
    U = np.zeros((1, M, 16), np.uint8)
    U[0, :5] = (np.arange(5)[:, None] * 16 + np.arange(16)[None] + 1)
    D, I = idx.search_tables(U, np.ones(1, F), np.zeros(1, F), 2)
    acc = [sum(16 * m + int(r[m]) + 1 for m in range(5)) for r in nib]
    assert I.tolist() == [[1, 0]] and D.tolist() == [[float(acc[1]), float(acc[0])]]
    idx.close()


def test_u16_accumulators_do_not_carry():
    """M = 256 with tables of 255 at the codes of some rows and 0 at the others: acc is 65,280 or 0, alternating between
    neighbouring rows, between neighbouring 64-row groups and between the halves of a block."""
    M, n, P = 256, 600, _pass()
    for shift in (0, 6, 7):
        on = ((np.arange(n) >> shift) & 1) == 0
        nib = np.where(on[:, None], 5, 10) * np.ones((1, M), np.int64)
        nib[~on, ::3] = 0                                            # the rows that score 0 differ among themselves
        codes = pqfs_pack_ref(nib)
        U = np.zeros((P + 1, M, 16), np.uint8)
        U[:, :, 5] = 255
        idx = _index(M)
        idx.add_codes(codes)
        want = pqfs_scan_ref(U, np.ones(P + 1, F), np.zeros(P + 1, F), codes, n)
        assert set(np.unique(want[0])) == {0.0, 65280.0}
        assert np.array_equal(want[1][0], np.concatenate([np.flatnonzero(on), np.flatnonzero(~on)]))
        _same(idx.search_tables(U, np.ones(P + 1, F), np.zeros(P + 1, F), n), want)
        idx.close()


def test_ties_rank_by_row():
    M, n = 16, 700
    rng = np.random.default_rng(3)
    nib = rng.integers(0, 16, (n, M))
    nib[100:400] = nib[7]                                            # identical codes
    nib[500:600, 0], nib[500:600, 1] = np.arange(100) % 16, 15 - np.arange(100) % 16       # distinct codes, equal acc below
    nib[500:600, 2:] = nib[8, 2:]
    codes = pqfs_pack_ref(nib)
    U = rng.integers(0, 256, (3, M, 16)).astype(np.uint8)
    U[:, 0], U[:, 1] = np.arange(16) * 3, np.arange(16) * 3          # U[0][c] + U[1][15 - c] = 45 for every c
    idx = _index(M)
    idx.add_codes(codes)
    # scale 1 and a bias of 2^24: neighbouring acc round to one D, the order stays that of the integers
    scale, bias = np.ones(3, F), np.array([0, 2.0 ** 24, -2.0 ** 25], F)
    want = pqfs_scan_ref(U, scale, bias, codes, n)
    assert (np.diff(want[1][0][np.isin(want[1][0], np.arange(100, 400))]) > 0).all()
    assert len(np.unique(want[0][1])) < len(np.unique(want[0][0]))
    _same(idx.search_tables(U, scale, bias, n), want)
    _same(idx.search_tables(U, scale, bias, 10), (want[0][:, :10], want[1][:, :10]))
    idx.close()


# -- encoder -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dsub", (1, 2, 4, 8, 32))
def test_encoder_follows_the_definition(dsub):
    M, n = 6, 1500
    rng = np.random.default_rng(dsub)
    cent = rng.standard_normal((M, 16, dsub)).astype(F)
    cent[2, 11] = cent[2, 4]                                         # identical centroids resolve to the lower j
    x = rng.standard_normal((n, M * dsub)).astype(F)
    x[:40, 2 * dsub:3 * dsub] = cent[2, 11]
    idx = IndexPQFastScan(M * dsub, M)
    idx.centroids = cent
    packed = idx.sa_encode(x)
    assert packed.dtype == np.uint8 and packed.shape == (n, M // 2)
    got = pqfs_unpack_ref(packed).astype(np.int64)
    want, dist = pqfs_encode_ref(x, cent)
    assert (got[:40, 2] == 4).all() and (got[:, 2] != 11).all()
    xs = x.astype(np.float64).reshape(n, M, dsub)
    tol = 2 * (dsub + 3) * 2.0 ** -23 * ((xs ** 2).sum(-1) + (cent.astype(np.float64) ** 2).sum(-1).max(-1)[None])
    chosen = np.take_along_axis(dist, got[:, :, None], axis=2)[:, :, 0]
    assert (chosen <= dist.min(-1) + tol).all()
    gap = np.sort(dist, axis=-1)
    determined = gap[:, :, 1] - gap[:, :, 0] > tol
    determined[:, 2] &= ~np.isin(want[:, 2], (4, 11))
    assert determined.mean() > 0.95 and np.array_equal(got[determined], want[determined])
    # add stores those codes, decode gathers centroid rows
    idx.add(x[:300])
    assert np.array_equal(idx.codes, packed[:300])
    dec = cent[np.arange(M)[None], got[:300]].reshape(300, M * dsub)
    assert np.array_equal(_bits(idx.sa_decode(packed[:300])), _bits(dec))
    assert np.array_equal(_bits(idx.reconstruct_n(10, 50)), _bits(dec[10:60])) and np.array_equal(_bits(idx.reconstruct(299)), _bits(dec[299]))
    idx.close()


# -- tables --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M, dsub", [(2, 1), (6, 5), (30, 4), (64, 8), (256, 2)])
def test_tables_and_quantiser(M, dsub):
    rng = np.random.default_rng(M + dsub)
    d = M * dsub
    cent = (rng.standard_normal((M, 16, dsub)) * rng.choice([0.1, 1.0, 10.0], (M, 1, 1))).astype(F)
    q = rng.standard_normal((40, d)).astype(F)
    q[0] = 0                                                         # span == 0
    q[1] = 0
    q[1, dsub:2 * dsub] = 1                                          # the tables differ in one slice only
    q[2] *= F(1e-3)
    idx = IndexPQFastScan(d, M)
    idx.centroids = cent
    T, U, scale, bias = idx.compute_tables(q, float_tables=True)
    assert T.dtype == F and T.shape == (40, M, 16) and U.dtype == np.uint8 and U.shape == (40, M, 16)
    ref = pqfs_tables_ref(q, cent)
    mag = np.einsum("imt,mjt->imj", np.abs(q.astype(np.float64)).reshape(40, M, dsub), np.abs(cent.astype(np.float64)))
    assert (np.abs(T.astype(np.float64) - ref) <= (dsub + 2) * 2.0 ** -24 * mag).all()
    Ur, sr, br = pqfs_quantize_ref(T)
    assert np.array_equal(U, Ur) and np.array_equal(_bits(scale), _bits(sr)) and np.array_equal(_bits(bias), _bits(br))
    assert not U[0].any() and scale[0] == 0 and bias[0] == 0
    assert U[1].max() == 255 and not np.delete(U[1], 1, axis=0).any()
    U2, s2, b2 = idx.compute_tables(q)                               # without the float tables: the same bytes
    assert np.array_equal(U2, U) and np.array_equal(_bits(s2), _bits(scale)) and np.array_equal(_bits(b2), _bits(bias))
    U3, s3, b3 = (a.cpu().numpy() for a in idx.quantize_tables_device(T))
    assert np.array_equal(U3, U) and np.array_equal(_bits(s3), _bits(scale)) and np.array_equal(_bits(b3), _bits(bias))
    # a zero query scores every row with the bias
    idx.add(rng.standard_normal((70, d)).astype(F))
    D, I = idx.search(q[:1], 70)
    assert I[0].tolist() == list(range(70)) and (D == bias[0]).all()
    idx.close()


def test_quantiser_on_spans_it_gives_up_on_and_on_hand_made_tables():
    M = 6
    idx = _index(M)
    rng = np.random.default_rng(9)
    T = rng.standard_normal((8, M, 16)).astype(F)
    T[0] = F(2e-38) + np.arange(16, dtype=F) * F(1e-38)              # span 1.5e-37: 255 / span overflows
    T[1] = F(-3.5)                                                   # span == 0
    T[2] = np.arange(M, dtype=F)[:, None]
    T[2, 4, 9] += F(0.25)                                            # one slice alone varies
    T[3] = np.round(T[3] * 4) / 4                                    # many exact ties of rint((T - lo) * a)
    T[4] *= F(1e20)
    T[5] *= F(1e-20)
    U, scale, bias = (a.cpu().numpy() for a in idx.quantize_tables_device(T))
    Ur, sr, br = pqfs_quantize_ref(T)
    assert sr[0] == 0 and sr[1] == 0 and not Ur[:2].any() and br[1] == F(-21)
    assert np.array_equal(U, Ur) and np.array_equal(_bits(scale), _bits(sr)) and np.array_equal(_bits(bias), _bits(br))
    idx.close()


# -- scores and the whole path -------------------------------------------------------------------------------------------------
def unit_rows(rng, n, d):
    x = rng.standard_normal((n, d)).astype(F)
    return x / np.linalg.norm(x, axis=1, keepdims=True).astype(F)


@pytest.fixture(scope="module")
def trained():
    """One trained index of 1,500 rows (d = 64, M = 16) with the rows and queries it was made from."""
    rng = np.random.default_rng(21)
    x, q = unit_rows(rng, 1500, 64), unit_rows(rng, 2 * _pass() + 1, 64)
    idx = IndexPQFastScan(64, 16)
    idx.train(x, niter=6)
    idx.add(x)
    yield idx, x, q
    idx.close()


def test_scores_lie_within_the_bound(trained):
    idx, x, q = trained
    T, U, scale, bias = idx.compute_tables(q, float_tables=True)
    D, I = idx.search(q, 50)
    nib = pqfs_unpack_ref(idx.codes).astype(np.int64)
    exact = np.zeros((len(q), idx.ntotal))
    for m in range(idx.M):
        exact += T[:, m, nib[:, m]].astype(np.float64)
    err = np.abs(D.astype(np.float64) - np.take_along_axis(exact, I, axis=1))
    bound = pqfs_score_bound(T)
    print(f"max |D - sum of float tables| / bound = {(err / bound[:, None]).max():.3f}")
    assert (err <= bound[:, None]).all()


def test_search_is_tables_then_scan(trained):
    idx, x, q = trained
    D, I = idx.search_device(q, 10)
    tabs = idx.compute_tables_device(q)
    D2, I2 = idx.search_tables_device(*tabs, 10)
    _same((D.cpu().numpy(), I.cpu().numpy()), (D2.cpu().numpy(), I2.cpu().numpy()))
    _same(idx.search(q, 10), pqfs_scan_ref(*(t.cpu().numpy() for t in tabs), idx.codes, 10))
    assert idx.search(q[0], 3)[1].shape == (1, 3)                    # one vector is one query


def test_training_is_deterministic_and_lowers_the_error(trained):
    idx, x, q = trained
    assert idx.is_trained and idx.centroids.shape == (16, 16, 4) and np.isfinite(idx.centroids).all()
    again = IndexPQFastScan(64, 16)
    again.train(x, niter=6)
    assert np.array_equal(_bits(again.centroids), _bits(idx.centroids))
    raw = IndexPQFastScan(64, 16)
    raw.train(x, niter=0)                                            # the initial codebooks: sampled rows

    def err(i):
        return float(((i.sa_decode(i.sa_encode(x)) - x) ** 2).sum(1).mean())
    e0, e1 = err(raw), err(idx)
    print(f"reconstruction error: {e0:.4f} untrained sample, {e1:.4f} after 6 iterations")
    assert e1 < 0.9 * e0
    nib = pqfs_unpack_ref(idx.sa_encode(x[:100])).astype(np.int64)
    assert np.array_equal(_bits(idx.sa_decode(idx.sa_encode(x[:100]))), _bits(idx.centroids[np.arange(16)[None], nib].reshape(100, 64)))
    with pytest.raises(RuntimeError, match="holds 1500 rows"):
        idx.centroids = idx.centroids
    with pytest.raises(RuntimeError, match="holds 1500 rows"):
        idx.train(x)
    again.close()
    raw.close()


def test_refine_over_a_fast_scan_base_with_every_row_a_candidate():
    from ivr_amd.index import FlatIPIndex
    from ivr_amd.refine import RefineFlatIndex
    rng = np.random.default_rng(13)
    x, q = unit_rows(rng, 600, 64), unit_rows(rng, 7, 64)
    r = RefineFlatIndex(IndexPQFastScan(64, 16))
    assert not r.is_trained
    r.train(x)
    r.add(x)
    r.k_factor = 60                               # k * k_factor = ntotal: the base proposes every row
    D, I = r.search(q, 10)
    flat = FlatIPIndex(64)
    flat.add(x)
    Df, If = flat.search(q, 10)
    assert np.array_equal(I, If) and np.array_equal(D.view(np.uint32), Df.view(np.uint32))
    r.close()
    r.base_index.close()
    flat.close()


def test_refusals_on_the_device():
    idx = IndexPQFastScan(64, 16)
    x = np.zeros((20, 64), F)
    for call in (lambda: idx.add(x), lambda: idx.search(x, 1), lambda: idx.sa_encode(x), lambda: idx.compute_tables(x),
                 lambda: idx.add_codes(np.zeros((1, 8), np.uint8))):
        with pytest.raises(RuntimeError, match="not trained"):
            call()
    idx.centroids = np.random.default_rng(0).standard_normal((16, 16, 4)).astype(F)
    idx.add(np.random.default_rng(1).standard_normal((20, 64)).astype(F))
    with pytest.raises(ValueError):
        idx.search(x[:1], 0)
    with pytest.raises(ValueError):
        idx.search(x[:1], 2049)
    with pytest.raises(ValueError):
        idx.search(np.zeros((1, 63), F), 1)
    with pytest.raises(ValueError):
        idx.search_tables(np.zeros((1, 16, 15), np.uint8), np.ones(1, F), np.zeros(1, F), 1)
    with pytest.raises(ValueError):
        idx.search_tables(np.zeros((2, 16, 16), np.uint8), np.ones(1, F), np.zeros(2, F), 1)
    with pytest.raises(ValueError):
        idx.add_codes(np.zeros((1, 16), np.uint8))
    with pytest.raises(ValueError):
        idx.reconstruct_n(10, 11)
    idx.close()
    with pytest.raises(RuntimeError, match="closed"):
        idx.add(x)
