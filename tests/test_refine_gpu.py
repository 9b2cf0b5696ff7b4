"""GPU suite of the re-ranking index: ivr_index_rescore through FlatIPIndex.rescore_device / compute_distance_subset, and
RefineFlatIndex (faiss IndexRefineFlat) on top of it.

The yardstick is the existing flat index, never the new code: a score must carry the bits FlatIPIndex.search reports for the same
(query, row) (float32 compared as uint32, no tolerances), a selection must equal refine_order_ref over those scores and, where a
candidate list names no row twice, the flat search restricted to the list by IDSelectorBatch.

d = 24 has a padded last chunk and a chunk loop shorter than any unrolled batch (2 chunks), d = 64 is exactly one batch of four,
d = 100 a batch of four plus a tail of three, d = 512 and 768 two and three batches of sixteen, and d = 344 (not among the shapes
the feature was specified with) takes all three loops in one row: sixteen, four and two chunks, the last one padded.  kc = 15 / 16 / 17 and 64 / 65 sit
around one and four full waves of 16 candidates, 2048 is the largest list and needs repeats over 1000 rows; 70 queries end in a
partly filled 16-query tile and leave the last workgroup of the scoring pass partly filled."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

FLT_MAX = np.finfo(np.float32).max
NTOTAL, NQ = 1000, 70
DIMS = [24, 64, 100, 344, 512, 768]
KCS = [1, 15, 16, 17, 64, 65, 2048]
BIG = 3 * 10**12


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _unit(rng, n, d):
    x = rng.standard_normal((n, d)).astype(np.float32)
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


_CTX = {}


def _ctx(d, ids=False):
    """Per (d, id-mapped): the index, the queries and S [NQ, NTOTAL] = the score the index's own search reports for every (query,
    row) pair (k = ntotal returns them all).  Made once, only read afterwards."""
    from ivr_amd.index import FlatIPIndex
    if (d, ids) not in _CTX:
        rng = np.random.default_rng(7000 + d)
        X, Q = _unit(rng, NTOTAL, d), _unit(rng, NQ, d)
        idx = FlatIPIndex(d)
        labels = None
        if ids:
            labels = (BIG + np.random.default_rng(d).permutation(10 * NTOTAL)[:NTOTAL]).astype(np.int64)
            idx.add_with_ids(X, labels)
        else:
            idx.add(X)
        D, I = idx.search(Q, NTOTAL)
        if ids:
            order = np.argsort(labels)
            I = order[np.searchsorted(labels[order], I)]
        assert (np.sort(I, axis=1) == np.arange(NTOTAL)).all()
        S = np.empty((NQ, NTOTAL), np.float32)
        np.put_along_axis(S, I, D, axis=1)
        _CTX[(d, ids)] = (idx, X, Q, S, labels)
    return _CTX[(d, ids)]


def _table(d, kc):
    """Candidate rows [NQ, kc]: no row twice in a list while the index has enough rows, random with repeats beyond."""
    rng = np.random.default_rng(100 * d + kc)
    if kc <= NTOTAL:
        return np.stack([rng.permutation(NTOTAL)[:kc] for _ in range(NQ)]).astype(np.int64)
    return rng.integers(0, NTOTAL, (NQ, kc)).astype(np.int64)


# -- scores ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kc", KCS)
@pytest.mark.parametrize("d", DIMS)
def test_scores_carry_the_bits_of_the_flat_search(d, kc):
    idx, X, Q, S, _ = _ctx(d)
    cand = _table(d, kc)
    got = idx.compute_distance_subset(Q, cand)
    assert got.dtype == np.float32 and got.shape == (NQ, kc)
    assert np.array_equal(_bits(got), _bits(np.take_along_axis(S, cand, axis=1)))


@pytest.mark.parametrize("kc", KCS)
@pytest.mark.parametrize("d", DIMS)
def test_scores_on_an_id_mapped_index_go_by_stored_id(d, kc):
    idx, X, Q, S, labels = _ctx(d, ids=True)
    cand = _table(d, kc)
    lab = labels[cand]
    lab[0, 0] = BIG - 1                       # an id that is not stored
    want = np.take_along_axis(S, cand, axis=1)
    want[0, 0] = -FLT_MAX
    assert np.array_equal(_bits(idx.compute_distance_subset(Q, lab)), _bits(want))
    # rescore_device stays positional on an id-mapped index
    got = idx.rescore_device(_dev(Q), _dev(cand))[0].cpu().numpy()
    assert np.array_equal(_bits(got), _bits(np.take_along_axis(S, cand, axis=1)))


# -- selection ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kc", KCS)
@pytest.mark.parametrize("d", DIMS)
def test_selection_equals_the_definition_and_the_restricted_flat_search(d, kc):
    from ivr_amd.index import IDSelectorBatch, SearchParameters
    from ivr_amd.refine import refine_order_ref
    idx, X, Q, S, _ = _ctx(d)
    cand = _table(d, kc)
    Qd, cd = _dev(Q), _dev(cand)
    for k in sorted({1, min(10, kc), kc}):
        D, I, D_all = (t.cpu().numpy() for t in idx.rescore_device(Qd, cd, k, want_all=True))
        assert np.array_equal(_bits(D_all), _bits(np.take_along_axis(S, cand, axis=1)))
        Dr, Ir = refine_order_ref(D_all, cand, k, NTOTAL)
        assert np.array_equal(I, Ir) and np.array_equal(_bits(D), _bits(Dr)), (d, kc, k)
        D2, I2 = (t.cpu().numpy() for t in idx.rescore_device(Qd, cd, k))          # without D_all: the same selection
        assert np.array_equal(I2, I) and np.array_equal(_bits(D2), _bits(D))
        if kc <= NTOTAL:                                                           # no row twice in a list
            for i in range(NQ):
                Df, If = idx.search(Q[i], k, params=SearchParameters(sel=IDSelectorBatch(cand[i])))
                assert np.array_equal(If[0], I[i]) and np.array_equal(_bits(Df[0]), _bits(D[i])), (d, kc, k, i)


def test_selection_on_an_id_mapped_index_reports_positions():
    from ivr_amd.index import IDSelectorBatch, SearchParameters
    idx, X, Q, S, labels = _ctx(100, ids=True)
    cand = _table(100, 65)
    D, I = (t.cpu().numpy() for t in idx.rescore_device(_dev(Q), _dev(cand), 10))
    for i in range(NQ):
        Df, If = idx.search(Q[i], 10, params=SearchParameters(sel=IDSelectorBatch(labels[cand[i]])))
        assert np.array_equal(If[0], labels[I[i]]) and np.array_equal(_bits(Df[0]), _bits(D[i]))


# -- edges -------------------------------------------------------------------------------------------------------------------------
def _small(ntotal, d=40, nq=17, seed=0):
    from ivr_amd.index import FlatIPIndex
    rng = np.random.default_rng(seed + ntotal)
    X, Q = _unit(rng, ntotal, d), _unit(rng, nq, d)
    idx = FlatIPIndex(d)
    if ntotal:
        idx.add(X)
    S = np.full((nq, max(ntotal, 1)), -FLT_MAX, np.float32)
    if ntotal:
        D, I = idx.search(Q, ntotal)
        np.put_along_axis(S, I, D, axis=1)
    return idx, X, Q, S


def _expect(S, cand, ntotal):
    ok = (cand >= 0) & (cand < ntotal)
    return np.where(ok, np.take_along_axis(S, np.where(ok, cand, 0), axis=1), -FLT_MAX).astype(np.float32)


@pytest.mark.parametrize("nq", [1, 17])
@pytest.mark.parametrize("ntotal", [0, 1, 16, 17, 37])
def test_small_indexes_absent_entries_and_repeats(ntotal, nq):
    from ivr_amd.refine import refine_order_ref
    idx, X, Q, S = _small(ntotal)
    Q, S = Q[:nq], S[:nq]
    # every stored row in descending order; rows 0, 15, 16, 31 and ntotal - 1 again where they exist; row 0 three times in all;
    # -1, entries below -1, at ntotal and far above it mixed in
    rows = list(range(ntotal - 1, -1, -1)) + [r for r in sorted({0, 15, 16, 31, ntotal - 1}) if 0 <= r < ntotal] + [0]
    one = np.array([-1, ntotal] + rows[:3] + [-2, ntotal + 5] + rows[3:] + [-7, 2**40, -2**40, 2**31 + 3, 2**32], np.int64)
    cand = np.stack([np.roll(one, i) for i in range(nq)])
    kc = cand.shape[1]
    want_all = _expect(S, cand, ntotal)
    assert np.array_equal(_bits(idx.compute_distance_subset(Q, cand)), _bits(want_all))
    for k in sorted({1, min(5, kc), kc}):
        D, I, D_all = (t.cpu().numpy() for t in idx.rescore_device(_dev(Q), _dev(cand), k, want_all=True))
        assert np.array_equal(_bits(D_all), _bits(want_all))
        Dr, Ir = refine_order_ref(want_all, cand, k, ntotal)
        assert np.array_equal(I, Ir) and np.array_equal(_bits(D), _bits(Dr)), (ntotal, nq, k)
        present = int(((cand[0] >= 0) & (cand[0] < ntotal)).sum())
        assert (I[:, min(present, k):] == -1).all() and (D[:, min(present, k):] == -FLT_MAX).all()
    if ntotal:                                                                    # row 0 is named three times
        D, I = (t.cpu().numpy() for t in idx.rescore_device(_dev(Q), _dev(cand), kc))
        assert ((I == 0).sum(axis=1) == 3).all()
        for i in range(nq):                                                       # the three mentions sit in adjacent slots
            at = np.flatnonzero(I[i] == 0)
            assert at[-1] - at[0] == 2 and len(set(_bits(D[i, at]).tolist())) == 1


def test_a_table_of_only_minus_one():
    idx, X, Q, S = _small(37)
    cand = np.full((17, 20), -1, np.int64)
    D, I, D_all = (t.cpu().numpy() for t in idx.rescore_device(_dev(Q), _dev(cand), 20, want_all=True))
    assert (D_all == -FLT_MAX).all() and (D == -FLT_MAX).all() and (I == -1).all()
    assert (idx.compute_distance_subset(Q, cand) == -FLT_MAX).all()


def test_duplicate_stored_rows_rank_the_lower_row_first_whatever_the_order_given():
    from ivr_amd.index import FlatIPIndex, IDSelectorBatch, SearchParameters
    from ivr_amd.refine import refine_order_ref
    rng = np.random.default_rng(11)
    X, Q = _unit(rng, 300, 72), _unit(rng, 17, 72)
    dup = [3, 20, 21, 150, 299]
    X[dup] = X[3]
    Q[0] = X[3]                                       # the duplicates lead query 0's list
    idx = FlatIPIndex(72)
    idx.add(X)
    one = np.array([299, 150, 7, 21, 20, 250, 3, 100], np.int64)      # the duplicates in descending order
    cand = np.stack([one] * 17)
    D, I, D_all = (t.cpu().numpy() for t in idx.rescore_device(_dev(Q), _dev(cand), 8, want_all=True))
    assert I[0, :5].tolist() == dup and len(set(_bits(D[0, :5]).tolist())) == 1
    Dr, Ir = refine_order_ref(D_all, cand, 8, 300)
    assert np.array_equal(I, Ir) and np.array_equal(_bits(D), _bits(Dr))
    for i in range(17):
        Df, If = idx.search(Q[i], 8, params=SearchParameters(sel=IDSelectorBatch(one)))
        assert np.array_equal(If[0], I[i]) and np.array_equal(_bits(Df[0]), _bits(D[i]))
        at = np.flatnonzero(np.isin(I[i], dup))
        assert at[-1] - at[0] == 4 and I[i, at].tolist() == dup   # bit-equal scores: adjacent, the lower row first


def test_normalize_equals_pre_normalised_queries():
    from ivr_amd.index import FlatIPIndex
    idx, X, Q, S, _ = _ctx(100)
    raw = (Q * np.linspace(0.5, 9.0, NQ, dtype=np.float32)[:, None]).astype(np.float32)
    cand = _table(100, 65)
    D, I, D_all = (t.cpu().numpy() for t in idx.rescore_device(_dev(raw), _dev(cand), 10, normalize=True, want_all=True))
    # the flat search's own scores for the raw queries normalised on the way
    Df, If = (t.cpu().numpy() for t in idx.search_device(raw, NTOTAL, normalize=True))
    Sn = np.empty((NQ, NTOTAL), np.float32)
    np.put_along_axis(Sn, If, Df, axis=1)
    assert np.array_equal(_bits(D_all), _bits(np.take_along_axis(Sn, cand, axis=1)))
    # queries normalised beforehand by the index's own row normalisation
    tmp = FlatIPIndex(100)
    tmp.add(raw, normalize=True)
    Qn = tmp.reconstruct_n()
    tmp.close()
    D2, I2, D_all2 = (t.cpu().numpy() for t in idx.rescore_device(_dev(Qn), _dev(cand), 10, want_all=True))
    assert np.array_equal(_bits(D_all2), _bits(D_all)) and np.array_equal(I2, I) and np.array_equal(_bits(D2), _bits(D))


def test_argument_errors():
    idx, X, Q, S, _ = _ctx(24)
    Qd, cd = _dev(Q), _dev(_table(24, 16))
    with pytest.raises(ValueError):
        idx.rescore_device(Qd, cd, 17)                                   # k > kc
    with pytest.raises(ValueError):
        idx.rescore_device(Qd, cd, 0)
    with pytest.raises(ValueError):
        idx.rescore_device(Qd, cd[:10], 1)                               # one list per query
    with pytest.raises(ValueError):
        idx.rescore_device(Qd, cd.to(torch.int32), 1)
    with pytest.raises(ValueError):
        idx.rescore_device(Qd, cd.cpu(), 1)
    with pytest.raises(ValueError):
        idx.rescore_device(Qd, _dev(np.zeros((NQ, 2049), np.int64)), 1)  # kc > IVR_MAX_K
    with pytest.raises(ValueError):
        idx.rescore_device(Qd, cd.t().contiguous().t(), 1)               # not contiguous
    with pytest.raises(ValueError):
        idx.compute_distance_subset(Q, np.zeros((NQ, 4), np.float32))
    with pytest.raises(ValueError):
        idx.compute_distance_subset(Q, np.zeros((3, 4), np.int64))
    # the C entry point itself: every check comes before the first launch and before any pointer is read
    D_all = torch.empty((NQ, 16), dtype=torch.float32, device="cuda")
    D, I = torch.empty((NQ, 4), dtype=torch.float32, device="cuda"), torch.empty((NQ, 4), dtype=torch.int64, device="cuda")
    for args, text in (((Qd, NQ, cd, 16, 4, False, None, None, None), "no output"),
                       ((Qd, NQ, cd, 16, 4, False, None, D, None), "go together"),
                       ((Qd, NQ, cd, 16, 4, False, None, None, I), "go together"),
                       ((Qd, NQ, cd, 0, 4, False, D_all, None, None), "kc=0"),
                       ((Qd, NQ, cd, 2049, 4, False, D_all, None, None), "kc=2049"),
                       ((Qd, 0, cd, 16, 4, False, D_all, None, None), "nq=0"),
                       ((Qd, 1 << 20, cd, 2048, 4, False, D_all, None, None), r"2\^31"),
                       ((Qd, NQ, cd, 16, 17, False, None, D, I), "k=17"),
                       ((Qd, NQ, cd, 16, 0, False, None, D, I), "k=0")):
        with pytest.raises(ValueError, match=text):
            idx._call("ivr_index_rescore", *args)
    idx._call("ivr_index_rescore", Qd, NQ, cd, 16, 0, False, D_all, None, None)   # k is not read without D / I
    torch.cuda.synchronize()


# -- the class ---------------------------------------------------------------------------------------------------------------------
def _clustered(n, d, ncent, nq, seed=1234):
    """Unit rows around ncent random unit centres, row = normalize(centre[j] + g / sqrt(d)), and nq queries of the same kind."""
    rng = np.random.default_rng(seed)
    c = _unit(rng, ncent, d)

    def draw(m):
        x = c[rng.integers(0, ncent, m)] + rng.standard_normal((m, d)).astype(np.float32) / np.float32(d ** 0.5)
        return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)
    return draw(n), draw(nq)


_CLUSTERED = {}


def _data():
    if not _CLUSTERED:
        _CLUSTERED["x"] = _clustered(4096, 64, 64, 64)
    return _CLUSTERED["x"]


def _flat(X):
    from ivr_amd.index import FlatIPIndex
    f = FlatIPIndex(X.shape[1])
    f.add(X)
    return f


def _same(a, b):
    assert np.array_equal(a[1], b[1])
    assert np.array_equal(_bits(a[0]), _bits(b[0]))


def test_lsh_base_returns_the_exact_order_of_its_candidates():
    from ivr_amd import IndexLSH, IndexRefineFlat
    from ivr_amd.index import IDSelectorBatch, METRIC_INNER_PRODUCT, SearchParameters
    X, Q = _data()
    r = IndexRefineFlat(IndexLSH(64, 64))
    assert r.ntotal == 0 and r.d == 64 and r.is_trained and r.k_factor == 1.0 and r.metric_type == METRIC_INNER_PRODUCT
    assert r.refine_index.d == 64 and r.refine_index.device == r.base_index.device and not r.refine_index.has_ids
    r.add(X)
    r.k_factor = 20
    assert r.ntotal == r.base_index.ntotal == r.refine_index.ntotal == 4096
    D, I = r.search(Q, 10)
    assert D.dtype == np.float32 and I.dtype == np.int64 and D.shape == I.shape == (64, 10)
    labels = r.base_index.search(Q, 200)[1]
    flat = _flat(X)
    top = flat.search(Q, 10)[1]
    for i in range(len(Q)):
        Df, If = flat.search(Q[i], 10, params=SearchParameters(sel=IDSelectorBatch(labels[i])))
        assert np.array_equal(If[0], I[i]) and np.array_equal(_bits(Df[0]), _bits(D[i])), i
        assert set(top[i]) & set(I[i]) == set(top[i]) & set(labels[i])
    # the same through the parameters object, k_factor overriding the attribute
    from ivr_amd import IndexRefineSearchParameters
    r.k_factor = 1
    _same(r.search(Q, 10, params=IndexRefineSearchParameters(k_factor=20)), (D, I))
    Dd, Id = r.search_device(_dev(Q), 10, k_factor=20)
    assert Dd.is_cuda and Id.is_cuda
    _same((Dd.cpu().numpy(), Id.cpu().numpy()), (D, I))
    with pytest.raises(ValueError):
        r.search(Q, 10, params=IndexRefineSearchParameters(base_index_params=SearchParameters()))     # IndexLSH takes none
    with pytest.raises(ValueError):
        r.search(Q, 10, params=IndexRefineSearchParameters(sel=IDSelectorBatch([1, 2])))
    with pytest.raises(ValueError):
        r.search(Q, 10, params=SearchParameters())
    r.close()
    flat.close()


def test_flat_base():
    from ivr_amd import IndexRefineFlat, IndexRefineSearchParameters
    from ivr_amd.index import FlatIPIndex, IDSelectorRange, SearchParameters
    X, Q = _data()
    r = IndexRefineFlat(FlatIPIndex(64))
    r.add(X)
    flat = _flat(X)
    want = flat.search(Q, 10)
    _same(r.search(Q, 10), want)                              # k_factor = 1: the base's own result
    _same(r.search(Q, 10), r.base_index.search(Q, 10))
    r.k_factor = 3
    _same(r.search(Q, 10), want)
    p = SearchParameters(sel=IDSelectorRange(100, 900))
    _same(r.search(Q, 10, params=IndexRefineSearchParameters(base_index_params=p)), flat.search(Q, 10, params=p))
    with pytest.raises(ValueError):
        r.search(Q, 10, params=IndexRefineSearchParameters(base_index_params=object()))
    r.close()
    flat.close()


def test_ivf_base_and_its_parameters():
    from ivr_amd import IndexRefineFlat, IndexRefineSearchParameters, IVFFlatIndex, SearchParametersIVF
    X, Q = _data()
    r = IndexRefineFlat(IVFFlatIndex(64, 16))
    assert not r.is_trained
    r.train(X)
    assert r.is_trained
    r.add(X)
    r.base_index.nprobe = 2
    _same(r.search(Q, 10), r.base_index.search(Q, 10))        # k_factor = 1: the base's own result, bit for bit
    flat = _flat(X)
    every = IndexRefineSearchParameters(base_index_params=SearchParametersIVF(nprobe=16))
    _same(r.search(Q, 10, params=every), flat.search(Q, 10))  # nprobe = nlist reaches the base: the exact result
    r.k_factor = 4
    _same(r.search(Q, 10, params=every), flat.search(Q, 10))
    r.close()
    flat.close()


def test_graph_base_and_its_parameters():
    from ivr_amd import GraphFlatIndex, IndexRefineFlat, IndexRefineSearchParameters, SearchParametersHNSW
    X, Q = _data()
    r = IndexRefineFlat(GraphFlatIndex(64, M=8))
    r.add(X)
    _same(r.search(Q, 10), r.base_index.search(Q, 10))
    hp = SearchParametersHNSW(efSearch=96)
    _same(r.search(Q, 10, params=IndexRefineSearchParameters(base_index_params=hp)), r.base_index.search(Q, 10, params=hp))
    with pytest.raises(ValueError):
        r.search(Q, 10, params=IndexRefineSearchParameters(k_factor=100))      # 1000 labels: the graph's own limit (256)
    r.close()


def test_lifecycle_and_errors():
    from ivr_amd import IndexLSH, IndexRefineFlat, IndexRefineSearchParameters, RefineFlatIndex
    from ivr_amd.index import FlatIPIndex
    X, Q = _data()
    base = FlatIPIndex(64)
    r = IndexRefineFlat(base)
    assert isinstance(r, RefineFlatIndex) and r.base_index is base
    r.add(X[:1000])
    r.add(X[1000:])
    assert r.ntotal == 4096
    whole = IndexRefineFlat(FlatIPIndex(64))
    whole.add(X)
    r.k_factor = whole.k_factor = 5
    _same(r.search(Q, 10), whole.search(Q, 10))
    keys = np.array([4095, 0, 17, 1000, 999])
    assert np.array_equal(_bits(r.reconstruct_batch(keys)), _bits(X[keys]))
    assert np.array_equal(_bits(r.reconstruct(1000)), _bits(X[1000]))
    assert np.array_equal(_bits(r.reconstruct_n(998, 4)), _bits(X[998:1002]))
    with pytest.raises(RuntimeError):
        r.reconstruct_batch(np.array([4096]))
    with pytest.raises(ValueError):
        r.search(Q, 10, params=IndexRefineSearchParameters(k_factor=205))      # 2050 labels > IVR_MAX_K
    r.k_factor = 204.8
    assert r.search(Q, 10)[1].shape == (64, 10)                                # int(10 * 204.8) = 2048 is allowed
    with pytest.raises(ValueError):
        r.k_factor = 0.5
    with pytest.raises(ValueError):
        IndexRefineFlat(base)                                 # a base that holds rows
    with pytest.raises(ValueError):
        IndexRefineFlat(whole)                                # not one of the base classes
    base.add(X[:3])                                           # behind the wrapper's back: labels and rows no longer agree
    with pytest.raises(RuntimeError):
        r.add(X[:3])
    r.reset()
    assert r.ntotal == base.ntotal == r.refine_index.ntotal == 0
    D, I = r.search(Q[:3], 5)
    assert (I == -1).all() and (D == -FLT_MAX).all()
    r.k_factor = 2
    r.add(X[:100])
    _same(r.search(Q, 10), _flat(X[:100]).search(Q, 10))
    mapped = FlatIPIndex(64)
    mapped.add_with_ids(np.zeros((0, 64), np.float32), np.zeros(0, np.int64))
    with pytest.raises(ValueError):
        IndexRefineFlat(mapped)                               # an id-mapped flat base
    lsh = IndexRefineFlat(IndexLSH(64, 64, train_thresholds=True))
    assert not lsh.is_trained
    with pytest.raises(RuntimeError):
        lsh.add(X)                                            # the base refuses: nothing reaches refine_index
    assert lsh.ntotal == 0
    lsh.train(X)
    lsh.add(X)
    assert lsh.is_trained and lsh.ntotal == 4096
    for x in (r, whole, lsh):
        x.close()
