"""GPU suite of the product-quantisation index (ivr_amd/pq.py PQIndex, csrc/search_pq.hip).

The encoder and the table builder are pinned to float64 references within the float32 rounding bounds stated in pq_encode_ref and
pq_tables_ref; the scan adds table entries only, so D and I must equal pq_scan_ref element for element.  Sizes sit on both sides of a
64-row wave group, of the two-group unit of a wave and of a query group; M covers a half-filled 16-byte word, one, three and four
words; ties, which quantised scores produce in bulk, are forced by repeated codes and few-valued tables."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

FLT_MAX = np.finfo(np.float32).max


def unit_rows(rng, n, d):
    x = rng.standard_normal((n, d)).astype(np.float32)
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def encode_tol(x, C):
    """[n,M]: 2 (dsub + 3) 2^-23 (|x_m|^2 + max_j |C[m,j]|^2), the tolerance of pq_encode_ref."""
    M, _, dsub = C.shape
    xn = (x.astype(np.float64).reshape(len(x), M, dsub) ** 2).sum(-1)
    cn = (C.astype(np.float64) ** 2).sum(-1).max(-1)
    return 2.0 * (dsub + 3) * 2.0 ** -23 * (xn + cn[None])


def with_codebooks(d, M, C):
    from ivr_amd.pq import IndexPQ
    idx = IndexPQ(d, M)
    idx.centroids = C
    assert idx.is_trained
    return idx


# -- encode --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n, d, M", [(2048, 32, 4), (1000, 64, 16), (1, 32, 4), (300, 128, 1), (77, 128, 2)])
def test_encode_meets_the_tolerance_rule(n, d, M):
    """dsub = 8, 4, 128 (codebook read through the caches) and 64 (the widest slice held in registers); n = 1, a multiple of the
    256-row tile and not one."""
    from ivr_amd.pq import pq_encode_ref
    rng = np.random.default_rng(n + d)
    dsub = d // M
    C = rng.standard_normal((M, 256, dsub)).astype(np.float32)
    C[:, 200] = C[:, 7]                  # identical centroids: the lower one must win
    C[0, 31] = C[0, 30]
    x = rng.standard_normal((n, d)).astype(np.float32)
    x[::3, :dsub] = C[0, 31] + 1e-3 * x[::3, :dsub]          # rows whose nearest centroid is a duplicated one
    x[1::3] = C[:, 200].reshape(-1) + 1e-3 * x[1::3]
    idx = with_codebooks(d, M, C)
    codes = idx.sa_encode(x)
    assert codes.dtype == np.uint8 and codes.shape == (n, M)
    ref, dist = pq_encode_ref(x, C)
    got = np.take_along_axis(dist, codes[:, :, None].astype(np.int64), axis=2)[:, :, 0]
    excess = got - dist.min(-1)
    print(f"encode n={n} d={d} M={M}: {np.mean(codes != ref):.4f} of the codes differ from the float64 argmin, "
          f"max excess / tol = {(excess / encode_tol(x, C)).max():.3f}")
    assert (excess <= encode_tol(x, C)).all()
    assert not (codes == 200).any() and not (codes[:, 0] == 31).any()
    assert (codes[1::3] == 7).all() and (codes[::3, 0] == 30).all()
    idx.close()


# -- tables --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nq", [1, 37])
@pytest.mark.parametrize("d, M", [(32, 4), (64, 16), (128, 1)])
def test_tables_within_the_float32_bound(nq, d, M):
    from ivr_amd.pq import pq_tables_ref
    rng = np.random.default_rng(nq + d)
    dsub = d // M
    C = rng.standard_normal((M, 256, dsub)).astype(np.float32)
    q = rng.standard_normal((nq, d)).astype(np.float32)
    idx = with_codebooks(d, M, C)
    T = idx.compute_tables(q)
    assert T.dtype == np.float32 and T.shape == (nq, M, 256)
    ref = pq_tables_ref(q, C)
    mag = np.einsum("imt,mjt->imj", np.abs(q.astype(np.float64)).reshape(nq, M, dsub), np.abs(C.astype(np.float64)))
    err = np.abs(T.astype(np.float64) - ref)
    print(f"tables nq={nq} d={d} M={M}: max err / bound = {(err / ((dsub + 2) * 2.0 ** -24 * mag)).max():.3f}")
    assert (err <= (dsub + 2) * 2.0 ** -24 * mag).all()
    idx.close()


# -- scan ----------------------------------------------------------------------------------------------------------------------
def scan_index(M, codes, split=None):
    """A trained index of M-byte codes holding `codes`, added in two calls when split is given."""
    idx = with_codebooks(2 * M, M, np.zeros((M, 256, 2), np.float32))
    parts = [codes] if split is None else [codes[:split], codes[split:]]
    for p in parts:
        if len(p):
            idx._index.add(p)
    assert idx.ntotal == len(codes)
    assert np.array_equal(idx.codes, codes)
    return idx


def check_scan(idx, T, codes, k):
    from ivr_amd.pq import pq_scan_ref
    D, I = idx.search_tables(T, k)
    assert D.dtype == np.float32 and I.dtype == np.int64 and D.shape == I.shape == (len(T), k)
    Dr, Ir = pq_scan_ref(T, codes, k)
    assert np.array_equal(I, Ir)
    assert np.array_equal(D.view(np.uint32), Dr.view(np.uint32))


@pytest.mark.parametrize("M", [8, 16, 48, 64])
def test_scan_equals_the_reference_bit_for_bit(M):
    """M = 8 / 16 / 48 / 64: a half-filled word, one, three and four words.  37 queries are more than one query group with a ragged
    last one at every M (groups of 8, 8, 2 and 2 queries)."""
    rng = np.random.default_rng(M)
    for n in (1, 63, 65, 64 * 3 + 5, 5003):
        codes = rng.integers(0, 256, (n, M), dtype=np.uint8)
        if n > 100:
            codes[rng.integers(0, n, n // 3)] = codes[5]          # repeated codes: equal scores across groups
        idx = scan_index(M, codes, split=None if n < 65 else 50)  # two add calls that straddle a 64-row boundary
        for nq in (1, 37):
            T = rng.standard_normal((nq, M, 256)).astype(np.float32)
            for k in (1, 10, n + 3) + ((2048,) if n > 2048 else ()):
                if k <= 2048 and (nq == 37 or k <= 10):
                    check_scan(idx, T, codes, k)
        idx.close()


def test_scan_ties():
    rng = np.random.default_rng(11)
    M, n = 16, 700
    one = np.tile(rng.integers(0, 256, (1, M), dtype=np.uint8), (n, 1))
    idx = scan_index(M, one)
    T = rng.standard_normal((3, M, 256)).astype(np.float32)
    D, I = idx.search_tables(T, 100)
    assert (I == np.arange(100)).all()                            # all rows one code: the lowest rows, in order
    check_scan(idx, T, one, 100)
    idx.close()
    codes = rng.integers(0, 256, (n, M), dtype=np.uint8)
    idx = scan_index(M, codes, split=333)
    two = rng.integers(0, 2, (5, M, 256)).astype(np.float32)      # two-valued tables: scores are small integers
    for k in (1, 10, 64, 703):
        check_scan(idx, two, codes, k)
    negz = np.full((2, M, 256), -0.0, np.float32)
    D, I = idx.search_tables(negz, 10)
    assert (I == np.arange(10)).all() and (D == 0).all() and not np.signbit(D).any()
    check_scan(idx, negz, codes, 10)
    mixed = np.where(rng.random((4, M, 256)) < 0.5, np.float32(-0.0), np.float32(0.0)).astype(np.float32)
    check_scan(idx, mixed, codes, 20)
    idx.reset()
    D, I = idx.search_tables(two, 3)                              # an empty index: unused slots only
    assert (I == -1).all() and (D == -FLT_MAX).all()
    idx.close()


def test_scan_query_cap_second_chunk_of_one_query():
    """A chunk holds 4096 queries at most: query 4096 of 4097 is a chunk of its own (c0 = 4096).  100 rows of 2-byte codes, the
    tables of real queries."""
    rng = np.random.default_rng(21)
    idx = with_codebooks(4, 2, rng.standard_normal((2, 256, 2)).astype(np.float32))
    codes = rng.integers(0, 256, (100, 2), dtype=np.uint8)
    idx._index.add(codes)
    T = idx.compute_tables(rng.standard_normal((4097, 4)).astype(np.float32))
    check_scan(idx, T, codes, 4)
    idx.close()


def test_scan_key_budget_second_chunk_of_eight_queries():
    """65,600 rows are 1025 groups, so k = 1024 selects 1024 groups of 64 keys per query and the 2^25 keys of a chunk hold
    2^25 / (1024 * 64) = 512 queries: 520 queries are a chunk of 512 and one of 8.  The first 2 and the last 8 queries equal the
    numpy scan, and the one call equals the two calls that split the queries where the chunks do, bit for bit.  2-byte codes over
    65,600 rows repeat, so equal scores across groups are ranked by the lower row throughout."""
    from ivr_amd.pq import pq_scan_ref
    rng = np.random.default_rng(22)
    n, nq, k, cut = 65600, 520, 1024, 512
    codes = rng.integers(0, 256, (n, 2), dtype=np.uint8)
    idx = scan_index(2, codes, split=50)
    T = rng.standard_normal((nq, 2, 256)).astype(np.float32)
    D, I = idx.search_tables(T, k)
    assert D.shape == I.shape == (nq, k)
    for part in (slice(0, 2), slice(cut, nq)):
        Dr, Ir = pq_scan_ref(T[part], codes, k)
        assert np.array_equal(I[part], Ir)
        assert np.array_equal(D[part].view(np.uint32), Dr.view(np.uint32))
    Da, Ia = idx.search_tables(T[:cut], k)
    Db, Ib = idx.search_tables(T[cut:], k)
    assert np.array_equal(I, np.concatenate([Ia, Ib]))
    assert np.array_equal(D.view(np.uint32), np.concatenate([Da, Db]).view(np.uint32))
    idx.close()


def test_search_is_the_scan_of_its_own_tables():
    from ivr_amd.pq import IndexPQ
    rng = np.random.default_rng(12)
    x = unit_rows(rng, 1500, 64)
    idx = IndexPQ(64, 16)
    idx.train(x, niter=2)
    idx.add(x[:700])
    idx.add(x[700:])
    q = unit_rows(rng, 9, 64)
    D, I = idx.search(q, 10)
    T = idx.compute_tables(q)
    D2, I2 = idx.search_tables(T, 10)
    assert np.array_equal(I, I2) and np.array_equal(D.view(np.uint32), D2.view(np.uint32))
    check_scan(idx, T, idx.codes, 10)
    Dt, It = idx.search_device(torch.from_numpy(q).cuda(), 10)
    assert np.array_equal(It.cpu().numpy(), I) and np.array_equal(Dt.cpu().numpy(), D)
    with pytest.raises(ValueError):
        idx.search_tables(T[:, :8], 10)
    with pytest.raises(ValueError):
        idx.search(q, 0)
    idx.close()


# -- train ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def train_rows():
    return unit_rows(np.random.default_rng(2024), 2048, 32)


def trained(x, niter, **kw):
    from ivr_amd.pq import IndexPQ
    idx = IndexPQ(32, 4)
    idx.train(x, niter=niter, **kw)
    return idx


def quant_error(idx, x):
    c = idx.sa_encode(x).astype(np.int64)
    rec = idx.centroids.astype(np.float64)[np.arange(idx.M)[None], c].reshape(len(x), idx.d)
    return ((x.astype(np.float64) - rec) ** 2).sum(1).mean()


def test_train_initial_codebooks_and_determinism(train_rows):
    from ivr_amd.ivf import kmeans_sample
    x = train_rows
    a = trained(x, 0)
    first = x[kmeans_sample(len(x), 256, 256, 1234)[:256]]
    assert np.array_equal(a.centroids, first.reshape(256, 4, 8).transpose(1, 0, 2))
    b, c = trained(x, 3), trained(x, 3)
    assert np.array_equal(b.centroids.view(np.uint32), c.centroids.view(np.uint32))
    assert not np.array_equal(trained(x, 3, seed=7).centroids, b.centroids)
    for i in (a, b, c):
        i.close()
    with pytest.raises(ValueError):
        trained(x[:255], 1)


def test_train_one_iteration_is_the_mean_of_the_assigned_slices(train_rows):
    """Every centroid after one iteration = the float64 mean of the slices the float64 argmin assigns to it under the initial
    codebook, per coordinate within (cnt + 2) 2^-24 sum |x_t| / cnt.  A centroid touched by an assignment the encoder's tolerance
    leaves open (it wins or could win a row whose two best distances lie within tol) is skipped; at most 2 % may be."""
    from ivr_amd.ivf import kmeans_sample
    from ivr_amd.pq import pq_encode_ref
    x = train_rows
    xs = x[kmeans_sample(len(x), 256, 256, 1234)]
    C0 = xs[:256].reshape(256, 4, 8).transpose(1, 0, 2)
    ref, dist = pq_encode_ref(xs, C0)
    open_ = dist <= (dist.min(-1) + encode_tol(xs, C0))[:, :, None]           # [n,M,256]: j could be chosen for (row, slice)
    unsure = open_.sum(-1) > 1
    skip = np.zeros((4, 256), bool)
    for i, m in zip(*np.nonzero(unsure)):
        skip[m, open_[i, m]] = True
    print(f"train: {unsure.sum()} ambiguous assignments, {skip.sum()} of {skip.size} centroids skipped")
    assert skip.mean() <= 0.02
    idx = trained(x, 1)
    got = idx.centroids.astype(np.float64)
    checked = 0
    for m in range(4):
        sl = xs[:, 8 * m:8 * m + 8].astype(np.float64)
        for j in np.flatnonzero(~skip[m]):
            rows = sl[ref[:, m] == j]
            cnt = len(rows)
            assert cnt >= 1                       # a centroid is a data point: it keeps at least that one
            bound = (cnt + 2) * 2.0 ** -24 * np.abs(rows).sum(0) / cnt
            assert (np.abs(got[m, j] - rows.mean(0)) <= bound).all(), (m, j)
            checked += 1
    assert checked >= 0.98 * 1024
    idx.close()


def test_training_lowers_the_quantisation_error(train_rows):
    a, b = trained(train_rows, 0), trained(train_rows, 10)
    e0, e10 = quant_error(a, train_rows), quant_error(b, train_rows)
    print(f"mean float64 quantisation error: {e0:.4f} at niter=0, {e10:.4f} at niter=10")
    assert e10 < e0
    a.close()
    b.close()


def test_untrained_index_and_assigned_codebooks(train_rows):
    from ivr_amd.pq import IndexPQ
    idx = IndexPQ(32, 4)
    assert not idx.is_trained and idx.ntotal == 0 and idx.code_size == 4 and idx.dsub == 8
    with pytest.raises(RuntimeError):
        idx.add(train_rows[:10])
    with pytest.raises(RuntimeError):
        idx.search(train_rows[:1], 1)
    with pytest.raises(ValueError):
        idx.centroids = np.zeros((4, 256, 7), np.float32)
    C = np.random.default_rng(1).standard_normal((4, 256, 8)).astype(np.float32)
    idx.centroids = C
    assert idx.is_trained and np.array_equal(idx.centroids, C)
    idx.add(train_rows[:10])
    with pytest.raises(RuntimeError):
        idx.centroids = C                         # rows are encoded with the current codebooks
    with pytest.raises(RuntimeError):
        idx.train(train_rows)
    idx.close()


# -- round trips -----------------------------------------------------------------------------------------------------------------
def test_round_trips_and_reset(train_rows):
    x = train_rows[:777]
    idx = trained(train_rows, 1)
    C = idx.centroids.copy()
    codes = idx.sa_encode(x)
    dec = idx.sa_decode(codes)
    want = C[np.arange(4)[None], codes.astype(np.int64)].reshape(len(x), 32)
    assert dec.dtype == np.float32 and np.array_equal(dec.view(np.uint32), want.view(np.uint32))
    idx.add(x)
    assert idx.ntotal == 777 and np.array_equal(idx.codes, codes)
    assert np.array_equal(idx.reconstruct_n(), idx.sa_decode(idx.codes))
    assert np.array_equal(idx.reconstruct_n(100, 50), want[100:150]) and np.array_equal(idx.reconstruct(776), want[776])
    idx.reset()
    assert idx.ntotal == 0 and idx.is_trained and np.array_equal(idx.centroids, C)
    idx.add(x[:5])
    assert np.array_equal(idx.codes, codes[:5])
    idx.close()


# -- refine ----------------------------------------------------------------------------------------------------------------------
def test_refine_over_a_pq_base_with_every_row_a_candidate():
    from ivr_amd.index import FlatIPIndex, SearchParameters
    from ivr_amd.pq import IndexPQ
    from ivr_amd.refine import IndexRefineSearchParameters, RefineFlatIndex
    rng = np.random.default_rng(13)
    x, q = unit_rows(rng, 600, 64), unit_rows(rng, 7, 64)
    r = RefineFlatIndex(IndexPQ(64, 16))
    assert not r.is_trained
    r.train(x)
    r.add(x)
    r.k_factor = 60                               # k * k_factor = ntotal: the base proposes every row
    D, I = r.search(q, 10)
    flat = FlatIPIndex(64)
    flat.add(x)
    Df, If = flat.search(q, 10)
    assert np.array_equal(I, If) and np.array_equal(D.view(np.uint32), Df.view(np.uint32))
    with pytest.raises(ValueError):
        r.search(q, 10, params=IndexRefineSearchParameters(base_index_params=SearchParameters()))
    with pytest.raises(ValueError):
        RefineFlatIndex(object())
    r.close()
    r.base_index.close()
    flat.close()
