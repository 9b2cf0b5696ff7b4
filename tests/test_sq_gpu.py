"""GPU suite of the scalar-quantiser index (ivr_amd/sq.py, csrc/search_sq.hip): the encoder, the query preparation and the int8 MFMA
scan against the numpy definitions of ivr_amd/sq.py, to the bit wherever they say so."""
import numpy as np
import pytest

from ivr_amd.sq import (IndexScalarQuantizer, sq_decode_ref, sq_encode_ref, sq_query_ref, sq_scan_ref, sq_score_bound, sq_tables_ref,
                        sq_train_ref)

pytestmark = pytest.mark.gpu
F = np.float32
FLT_MAX = np.finfo(np.float32).max


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same(got, want):
    assert np.array_equal(got[1], want[1])
    assert np.array_equal(_bits(got[0]), _bits(want[0]))


# -- encoder ---------------------------------------------------------------------------------------------------------------------
def _rows(n, d, seed):
    """Rows with columns of zero range, of tiny and of large range; a third of the values lie outside the range the index is
    trained to (it is trained on the first half of every column's spread)."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, d)).astype(F) * rng.choice(np.array([1e-3, 1.0, 300.0], F), d) + rng.standard_normal(d).astype(F)
    x[:, ::5] = x[0, ::5]                                            # zero range
    return x


def _trained(d, seed):
    t = _rows(64, d, seed + 1000)
    t[:, ::5] = _rows(1, d, seed)[0, ::5]                            # the constant columns hold the rows' own constant
    return sq_train_ref(t * F(0.5) + t.mean(axis=0, dtype=np.float64).astype(F) * F(0.5))


@pytest.mark.parametrize("n", [1, 65, 5003])
@pytest.mark.parametrize("d", [1, 7, 64, 96, 512, 1024])
def test_encode_equals_the_definition(d, n):
    x, tr = _rows(n, d, d + n), _trained(d, d + n)
    want = sq_encode_ref(x, tr)
    if d > 1 and n > 1:
        assert (want == 0).any() and (want == 255).any()          # values on both sides of the trained range
    idx = IndexScalarQuantizer(d)
    idx.trained = tr
    got = idx.sa_encode(x)
    assert got.dtype == np.uint8 and np.array_equal(got, want)
    # through add and back: the same bytes; decode and reconstruct_n: the numpy statement
    idx.add(x)
    assert idx.ntotal == n and np.array_equal(idx.codes, want)
    dec = sq_decode_ref(want, tr)
    assert np.array_equal(_bits(idx.sa_decode(want)), _bits(dec))
    assert np.array_equal(_bits(idx.reconstruct_n()), _bits(dec))
    assert np.array_equal(_bits(idx.reconstruct(n - 1)), _bits(dec[n - 1]))
    lo = max(0, n - 20)
    assert np.array_equal(_bits(idx.reconstruct_n(lo, n - lo)), _bits(dec[lo:]))
    idx.close()


def test_train_on_device_and_host_rows():
    import torch
    x = _rows(300, 40, 3)
    idx = IndexScalarQuantizer(40)
    idx.train(x)
    assert idx.is_trained and np.array_equal(_bits(idx.trained), _bits(sq_train_ref(x)))
    idx.add(x)
    with pytest.raises(RuntimeError):
        idx.train(x)
    with pytest.raises(RuntimeError):
        idx.trained = idx.trained
    idx.reset()
    idx.train(torch.from_numpy(x[:100]).cuda())
    assert np.array_equal(_bits(idx.trained), _bits(sq_train_ref(x[:100])))
    idx.close()


# -- query preparation -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nq", [1, 37])
@pytest.mark.parametrize("d", [1, 7, 64, 96, 512, 1024])
def test_query_codes_equal_the_definition(d, nq):
    tr = _trained(d, d)
    q = _rows(nq, d, 7 * d + nq)
    q[nq // 2] = 0                                                   # an all-zero query: t = 0, scale = 1
    if nq > 2:
        q[1] *= F(1e-20)                                             # tiny and huge queries scale alike
        q[2] *= F(1e12)
    idx = IndexScalarQuantizer(d)
    idx.trained = tr
    t, s, b = idx.compute_query_codes(q)
    tw, sw, bw = sq_query_ref(q, tr)
    assert t.dtype == np.int16 and s.dtype == np.float32 and b.dtype == np.float32
    assert np.array_equal(t, tw) and np.array_equal(_bits(s), _bits(sw))
    assert (t[nq // 2] == 0).all() and s[nq // 2] == 1.0 and b[nq // 2] == 0.0
    assert (np.abs(t).max(axis=1)[s != 1.0] == 16256).all()
    _, offset = sq_tables_ref(tr)
    bound = (d + 2) * 2.0 ** -24 * np.abs(q.astype(np.float64) * offset.astype(np.float64)).sum(axis=1)
    err = np.abs(b.astype(np.float64) - bw)
    print(f"bias: largest error / bound = {(err[bound > 0] / bound[bound > 0]).max() if (bound > 0).any() else 0:.3f}")
    assert (err <= bound).all()
    idx.close()


# -- scan ------------------------------------------------------------------------------------------------------------------------
def _index(d, codes, parts=None):
    idx = IndexScalarQuantizer(d)
    idx.trained = np.concatenate([np.zeros(d, F), np.ones(d, F)])
    at = 0
    for n in parts or [len(codes)]:
        idx.add_codes(codes[at:at + n])
        at += n
    assert at == len(codes) == idx.ntotal
    return idx


def _scan_inputs(d, n, nq, seed):
    """Random codes with repeated rows (their scores tie: the lower row must come first), random t over the whole range with the
    extremes present, random scale and bias."""
    rng = np.random.default_rng(seed)
    codes = rng.integers(0, 256, (n, d), dtype=np.uint8)
    if n > 4:
        codes[n // 2:n // 2 + n // 4] = codes[:n // 4]
    t = rng.integers(-16256, 16257, (nq, d)).astype(np.int16)
    t[:, 0] = 16256
    t[nq // 2, :] = -16256
    scale = rng.uniform(1e-6, 1e-3, nq).astype(F)
    bias = rng.standard_normal(nq).astype(F)
    return codes, t, scale, bias


# every value of every axis occurs: d in {64, 96, 512, 1024} (one K step, a padded K, the workload's, the accumulator's limit),
# ntotal in {1, 15, 17, 63, 65, 197, 5003} (tile and group edges, more groups than k), nq in {1, 9, 17, 33, 70, 131} (around the
# MFMA's 16 columns and the 32-query pass), k in {1, 10, ntotal + 3, 2048}
SCAN_CASES = [(64, 1, 1, 1), (64, 15, 9, 10), (96, 17, 17, "n+3"), (96, 63, 33, 2048), (512, 65, 70, 10), (512, 197, 131, "n+3"),
              (1024, 5003, 33, 10), (64, 5003, 131, 2048), (1024, 197, 1, 1), (96, 5003, 70, 10), (1024, 65, 9, 2048),
              (512, 5003, 17, 1)]


@pytest.mark.parametrize("d, n, nq, k", SCAN_CASES)
def test_search_codes_equals_the_definition(d, n, nq, k):
    k = min(n + 3, 2048) if k == "n+3" else k
    codes, t, scale, bias = _scan_inputs(d, n, nq, d + n + nq)
    idx = _index(d, codes)
    got = idx.search_codes(t, scale, bias, k)
    want = sq_scan_ref(t, scale, bias, codes, k)
    assert got[0].dtype == np.float32 and got[1].dtype == np.int64 and got[0].shape == got[1].shape == (nq, k)
    _same(got, want)
    idx.close()


def test_scan_query_cap_second_chunk_of_one_query():
    """A chunk holds 4096 queries at most: query 4096 of 4097 is a chunk of its own (c0 = 4096)."""
    codes, t, scale, bias = _scan_inputs(8, 100, 4097, 21)
    idx = _index(8, codes)
    _same(idx.search_codes(t, scale, bias, 4), sq_scan_ref(t, scale, bias, codes, 4))
    idx.close()


def test_scan_key_budget_rounds_the_chunk_down_to_whole_passes():
    """65,600 rows are 1025 groups, so k = 1000 selects 1000 groups of 64 keys per query and the 2^25 keys of a chunk hold
    2^25 / 64000 = 524 queries, 512 in whole passes of 32: 520 queries are a chunk of 512 and one of 8.  The first 2 and the last 8
    queries equal the numpy scan, and the one call equals the two calls that split the queries where the chunks do, bit for bit.
    A quarter of the rows repeat earlier ones, so equal scores across groups are ranked by the lower row."""
    n, nq, k, cut = 65600, 520, 1000, 512
    codes, t, scale, bias = _scan_inputs(16, n, nq, 22)
    idx = _index(16, codes, [50, n - 50])
    D, I = idx.search_codes(t, scale, bias, k)
    assert D.shape == I.shape == (nq, k)
    for part in (slice(0, 2), slice(cut, nq)):
        _same((D[part], I[part]), sq_scan_ref(t[part], scale[part], bias[part], codes, k))
    a = idx.search_codes(t[:cut], scale[:cut], bias[:cut], k)
    b = idx.search_codes(t[cut:], scale[cut:], bias[cut:], k)
    _same((D, I), (np.concatenate([a[0], b[0]]), np.concatenate([a[1], b[1]])))
    idx.close()


def test_rows_added_in_two_calls_across_tile_and_group_boundaries():
    codes, t, scale, bias = _scan_inputs(96, 13 + 60 + 130, 9, 5)
    idx = _index(96, codes, [13, 60, 130])                           # 13 -> 73 crosses rows 16 and 64, 73 -> 203 grows the allocation
    assert np.array_equal(idx.codes, codes)
    _same(idx.search_codes(t, scale, bias, 20), sq_scan_ref(t, scale, bias, codes, 20))
    idx.close()


def test_identical_rows_rank_by_row_number():
    codes = np.full((197, 64), 77, np.uint8)
    _, t, scale, bias = _scan_inputs(64, 197, 17, 6)
    idx = _index(64, codes)
    D, I = idx.search_codes(t, scale, bias, 100)
    assert (I == np.arange(100)).all()
    _same((D, I), sq_scan_ref(t, scale, bias, codes, 100))
    idx.close()


def test_extreme_accumulator_and_both_halves_at_their_limits():
    rng = np.random.default_rng(8)
    codes = (rng.integers(0, 2, (197, 1024)) * 255).astype(np.uint8)
    codes[0], codes[1] = 0, 255
    t = (rng.integers(0, 2, (33, 1024)) * 2 - 1).astype(np.int16) * 16256
    t[0], t[1] = 16256, -16256                                        # acc = -+ 2,130,706,432 on row 0, +- 16256 * 127 * 1024 on row 1
    scale, bias = np.ones(33, F), np.zeros(33, F)
    idx = _index(1024, codes)
    D, I = idx.search_codes(t, scale, bias, 197)
    _same((D, I), sq_scan_ref(t, scale, bias, codes, 197))
    assert I[0, 0] == 1 and I[0, -1] == 0 and D[0, -1] == F(-2130706432.0) and I[1, 0] == 0 and D[1, 0] == F(2130706432.0)
    idx.close()


@pytest.mark.parametrize("low", [-64, 63])
def test_caller_made_codes_with_one_low_half_everywhere(low):
    rng = np.random.default_rng(9)
    codes = rng.integers(0, 256, (65, 96), dtype=np.uint8)
    t = (rng.integers(-126, 127, (17, 96)) * 128 + low).astype(np.int16)
    scale, bias = np.full(17, 0.25, F), np.full(17, -3.0, F)
    idx = _index(96, codes)
    _same(idx.search_codes(t, scale, bias, 65), sq_scan_ref(t, scale, bias, codes, 65))
    idx.close()


def test_stale_bytes_behind_ntotal_never_win():
    idx = _index(64, np.full((100, 64), 255, np.uint8))
    idx.reset()
    assert idx.ntotal == 0
    D, I = idx.search(np.ones((2, 64), F), 3)
    assert (I == -1).all() and (D == -FLT_MAX).all()
    idx.add_codes(np.zeros((70, 64), np.uint8))
    D, I = idx.search(np.ones((2, 64), F), 80)                        # a positive query: a row of code 255 would beat every stored row
    assert (I[:, :70] == np.arange(70)).all() and (I[:, 70:] == -1).all() and (D[:, 70:] == -FLT_MAX).all()
    assert (D[:, :70] == D[0, 0]).all()
    idx.close()


# -- the whole path on clustered rows ----------------------------------------------------------------------------------------------
def _unit(rng, n, d):
    x = rng.standard_normal((n, d)).astype(np.float32)
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def clustered(n, d, ncent, nq, seed=1234):
    """Unit rows around ncent random unit centres, row = normalize(centre[j] + g / sqrt(d)), and nq queries of the same kind."""
    rng = np.random.default_rng(seed)
    c = _unit(rng, ncent, d)

    def draw(m):
        x = c[rng.integers(0, ncent, m)] + rng.standard_normal((m, d)).astype(np.float32) / np.float32(d ** 0.5)
        return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)
    return draw(n), draw(nq)


_DATA = {}


def _data():
    if not _DATA:
        X, Q = clustered(5003, 64, 64, 200)
        tr = sq_train_ref(X)
        _DATA["x"] = (X, Q, tr, sq_encode_ref(X, tr))
    return _DATA["x"]


def test_search_is_search_codes_of_compute_query_codes():
    import torch
    X, Q, tr, codes = _data()
    idx = IndexScalarQuantizer(64)
    idx.train(X)
    assert np.array_equal(_bits(idx.trained), _bits(tr))
    idx.add(X)
    assert np.array_equal(idx.codes, codes)
    D, I = idx.search(Q, 10)
    t, s, b = idx.compute_query_codes(Q)
    _same(idx.search_codes(t, s, b, 10), (D, I))
    _same(sq_scan_ref(t, s, b, codes, 10), (D, I))
    Dd, Id = idx.search_device(torch.from_numpy(Q).cuda(), 10)
    assert Dd.is_cuda and Id.is_cuda
    _same((Dd.cpu().numpy(), Id.cpu().numpy()), (D, I))
    _same(idx.search(Q[3], 10), (D[3:4], I[3:4]))                     # one vector is one row
    # every reported score within the stated bound of faiss's score <q, decode(code)>
    vmin, vdiff = tr[:64].astype(np.float64), tr[64:].astype(np.float64)
    S = Q.astype(np.float64) @ (vmin + vdiff * (codes.astype(np.float64) + 0.5) / 255.0).T
    err = np.abs(D.astype(np.float64) - np.take_along_axis(S, I, axis=1))
    bound = np.take_along_axis(sq_score_bound(Q, codes, tr, s), I, axis=1)
    print(f"largest |D - <q, decode>| / bound = {(err / bound).max():.3f}")
    assert (err <= bound).all()
    with pytest.raises(ValueError):
        idx.search(Q[:, :63], 10)
    with pytest.raises(ValueError):
        idx.search(Q, 2049)
    with pytest.raises(ValueError):
        idx.search_codes(t.astype(np.int32), s, b, 10)
    with pytest.raises(ValueError):
        idx.search_codes(t, s[:5], b, 10)
    idx.close()


def test_refine_over_scalar_codes():
    from ivr_amd import IndexRefineFlat, IndexRefineSearchParameters
    from ivr_amd.index import FlatIPIndex, IDSelectorBatch, SearchParameters
    X, Q, tr, codes = _data()
    # every row a candidate: the flat search itself, bit for bit
    r = IndexRefineFlat(IndexScalarQuantizer(64))
    assert not r.is_trained
    r.train(X[:197])
    r.add(X[:197])
    flat = FlatIPIndex(64)
    flat.add(X[:197])
    r.k_factor = 20
    _same(r.search(Q, 10), flat.search(Q, 10))
    with pytest.raises(ValueError):
        r.search(Q, 10, params=IndexRefineSearchParameters(base_index_params=SearchParameters()))     # SQIndex takes none
    r.close()
    r.base_index.close()
    flat.close()
    # k_factor = 2: the scores of the ids it names are the flat index's to the bit, in the flat index's order
    r = IndexRefineFlat(IndexScalarQuantizer(64))
    r.train(X)
    r.add(X)
    r.k_factor = 2
    assert r.ntotal == r.base_index.ntotal == 5003
    D, I = r.search(Q, 10)
    labels = r.base_index.search(Q, 20)[1]
    flat = FlatIPIndex(64)
    flat.add(X)
    top = flat.search(Q, 10)[1]
    for i in range(len(Q)):
        Df, If = flat.search(Q[i], 10, params=SearchParameters(sel=IDSelectorBatch(labels[i])))
        assert np.array_equal(If[0], I[i]) and np.array_equal(_bits(Df[0]), _bits(D[i])), i
    recall = np.mean([len(set(a) & set(b)) / 10 for a, b in zip(I.tolist(), top.tolist())])
    print(f"recall@10 of 8-bit codes + re-ranking at k_factor 2: {recall:.4f}")
    r.close()
    r.base_index.close()
    flat.close()
