"""GPU suite of the inverted-file index (ivr_amd/ivf.py, csrc/search_ivf.hip).

The yardstick is the flat index: a row's score must be the float32 inner product FlatIPIndex.search computes, to the bit (float32
compared as uint32), and the rows a query sees are exactly those of the lists it probes.  The expected result of a list scan is
therefore flat.search with an IDSelectorBatch over the labels of the probed lists.

List sizes are controlled without trusting the code under test: the quantizer is pre-filled with the unit axis vectors e_0 .. e_12 and
row i is normalize(e_l + 0.3 g / sqrt(d)), g standard normal, so that its dominant coordinate (about 0.96 against noise of 0.03) decides
its list.  SIZES makes runs start at non-multiples of 16, end inside a tile, cross a 256-row boundary and be empty.  Queries are random
unit vectors: scores are continuous, exact ties practically absent; where two neighbouring scores of a result are nevertheless
bit-equal, that run of labels is compared as a set.  Labels are 3 * 10**12 + a permutation sample, so that a 32-bit truncation shows."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SIZES = [0, 1, 15, 16, 17, 63, 64, 65, 255, 257, 1000, 0, 3]
NLIST = len(SIZES)
N = sum(SIZES)
BIG = 3 * 10**12
DIMS = [64, 100, 512, 768]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _unit64(x):
    x = np.asarray(x, np.float64)
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def _axis_quantizer(d, nlist=NLIST):
    from ivr_amd.index import FlatIPIndex
    q = FlatIPIndex(d)
    q.add(np.eye(nlist, d, dtype=np.float32))
    return q


class _Setup:
    """Rows, labels and lists for dimension d, an IVF index over them (two add_with_ids calls) and the flat index of the same rows."""

    def __init__(self, d, build=True):
        rng = np.random.default_rng(7000 + d)
        self.d = d
        self.lists = np.repeat(np.arange(NLIST), SIZES)[rng.permutation(N)]
        self.X = _unit64(np.eye(NLIST, d)[self.lists] + 0.3 * rng.standard_normal((N, d)) / np.sqrt(d)).astype(np.float32)
        # the construction itself: the dominant coordinate is the list, by a wide margin
        c = self.X.astype(np.float64)[:, :NLIST]
        assert np.array_equal(c.argmax(1), self.lists) and (np.sort(c, 1)[:, -1] - np.sort(c, 1)[:, -2]).min() > 0.5
        self.labels = (BIG + rng.permutation(10 * N)[:N]).astype(np.int64)
        self.queries = _unit64(rng.standard_normal((70, d))).astype(np.float32)
        order = np.argsort(self.labels)
        self._sorted, self._order = self.labels[order], order
        if build:
            self.ivf, self.flat = self.make_ivf(), self.make_flat()

    def make_ivf(self, split=N // 2 + 3):
        from ivr_amd.ivf import IndexIVFFlat
        ivf = IndexIVFFlat(_axis_quantizer(self.d), self.d, NLIST)
        ivf.train(self.X)                     # the quantizer holds its centroids: this only sets is_trained
        ivf.add_with_ids(self.X[:split], self.labels[:split])
        ivf.add_with_ids(self.X[split:], self.labels[split:])
        return ivf

    def make_flat(self):
        from ivr_amd.index import FlatIPIndex
        flat = FlatIPIndex(self.d)
        flat.add_with_ids(self.X, self.labels)
        return flat

    def rows_of(self, labels):
        return self._order[np.searchsorted(self._sorted, labels)]


_SETUPS = {}


def _setup(d):
    if d not in _SETUPS:
        _SETUPS[d] = _Setup(d)
    return _SETUPS[d]


def _expected(flat, lists, labels, Q, k, assign):
    """flat.search restricted, per query, to the labels of the lists its assign row names (queries with the same set share a call)."""
    from ivr_amd.index import IDSelectorBatch, SearchParameters
    D = np.empty((len(Q), k), np.float32)
    I = np.empty((len(Q), k), np.int64)
    groups = {}
    for i, row in enumerate(assign):
        groups.setdefault(tuple(sorted({int(l) for l in row if l >= 0})), []).append(i)
    for key, qi in groups.items():
        ids = np.concatenate([labels[lists == l] for l in key] + [np.zeros(0, np.int64)])
        D[qi], I[qi] = flat.search(Q[qi], k, params=SearchParameters(sel=IDSelectorBatch(ids)))
    return D, I


def _assert_same(D, I, De, Ie, what):
    """D bit-equal; I equal, where a run of bit-equal neighbouring scores is compared as a set of labels."""
    assert D.dtype == np.float32 and I.dtype == np.int64 and D.shape == De.shape and I.shape == Ie.shape, what
    assert np.array_equal(_bits(D), _bits(De)), f"{what}: scores differ in {(_bits(D) != _bits(De)).sum()} slots"
    if np.array_equal(I, Ie):
        return
    for q in np.flatnonzero((I != Ie).any(1)):
        b = _bits(D[q])
        starts = np.flatnonzero(np.concatenate([[True], b[1:] != b[:-1]]))
        for a, e in zip(starts, list(starts[1:]) + [len(b)]):
            assert sorted(I[q, a:e]) == sorted(Ie[q, a:e]), f"{what}: query {q} slots {a}..{e}: {I[q, a:e]} != {Ie[q, a:e]}"


def _assign_cases(nq):
    i = np.arange(nq)
    return {
        "hand": np.stack([(5 * i) % NLIST, (7 * i + 3) % NLIST, np.full(nq, 10)], 1),       # differs per query, repeats a list now and then
        "single": (i % NLIST)[:, None],                                                       # every list on its own, the empty ones too
        "empty": np.tile([0, 11], (nq, 1)),
        "all": np.tile(np.arange(NLIST)[::-1], (nq, 1)),                                      # descending: the order must not matter
        "minus1": np.tile([-1, 4, -1, 9], (nq, 1)),
        "twice": np.tile([10, 2, 10], (nq, 1)),
    }


def _check_scan(S, ivf, flat, lists, labels, nq, k):
    Q = S.queries[:nq]
    X64, Q64 = S.X.astype(np.float64), Q.astype(np.float64)
    dp = -(-S.d // 16) * 16
    sizes = np.bincount(lists, minlength=NLIST)
    for name, assign in _assign_cases(nq).items():
        what = f"d={S.d} nq={nq} k={k} {name}"
        D, I = ivf.search_preassigned(Q, k, assign.astype(np.int64))
        De, Ie = _expected(flat, lists, labels, Q, k, assign)
        _assert_same(D, I, De, Ie, what)
        # -1 padding exactly where k exceeds the probed rows
        probed = np.array([sum(sizes[l] for l in {int(l) for l in row if l >= 0}) for row in assign])
        assert np.array_equal((I == -1).sum(1), np.maximum(0, k - probed)), what
        assert ((I == -1) == (np.arange(k)[None, :] >= np.minimum(k, probed)[:, None])).all(), what
        # and the scores against float64 brute force: the index's own acc_eps for unit-norm operands
        ok = I >= 0
        qn, _ = np.nonzero(ok)
        ref = (X64[S.rows_of(I[ok])] * Q64[qn]).sum(1)
        assert np.abs(D[ok].astype(np.float64) - ref).max(initial=0.0) <= dp * 1.2e-7, what
        assert (np.diff(D, axis=1) <= 0).all(), what


# -- 1. the list scan against the flat index, bit for bit -----------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 10, 300])
@pytest.mark.parametrize("nq", [1, 17, 70])
@pytest.mark.parametrize("d", DIMS)
def test_list_scan_matches_filtered_flat_search(d, nq, k):
    S = _setup(d)
    _check_scan(S, S.ivf, S.flat, S.lists, S.labels, nq, k)


def test_several_chunks_give_the_bits_of_one(monkeypatch):
    """A chunk of queries is bounded by its key slots (IVR_IVF_CHUNK_SLOTS, read when the storage of the index is made).  A query
    that names three lists holds at most the rows of the three longest, so one slot more than three such stretches is chunks of 3
    queries: 40 queries are 13 chunks and a ragged last one, every chunk but the first starting inside a 16-query tile of the staged
    queries.  The chunked call equals the unchunked one, and both the filtered flat search."""
    from ivr_amd.index import FlatIPIndex
    from ivr_amd.ivf import IndexIVFFlat
    d, nq, p = 24, 40, 3
    sizes = [5, 64, 0, 130, 17, 300, 1, 33]
    nlist, n = len(sizes), sum(sizes)
    rng = np.random.default_rng(7024)
    lists = np.repeat(np.arange(nlist), sizes)[rng.permutation(n)]
    X = _unit64(np.eye(nlist, d)[lists] + 0.3 * rng.standard_normal((n, d)) / np.sqrt(d)).astype(np.float32)
    assert np.array_equal(X[:, :nlist].argmax(1), lists)
    labels = (BIG + rng.permutation(10 * n)[:n]).astype(np.int64)
    Q = _unit64(rng.standard_normal((nq, d))).astype(np.float32)
    i = np.arange(nq)
    assign = np.stack([(5 * i) % nlist, (3 * i + 1) % nlist, np.where(i % 7 == 0, -1, 5)], 1).astype(np.int64)
    flat = FlatIPIndex(d)
    flat.add_with_ids(X, labels)

    def scan():
        ivf = IndexIVFFlat(_axis_quantizer(d, nlist), d, nlist)
        ivf.train(X)
        ivf.add_with_ids(X, labels)
        assert ivf.list_sizes().tolist() == sizes
        out = [ivf.search_preassigned(Q, k, assign) for k in (10, 500)]
        ivf.close()
        return out

    whole = scan()
    monkeypatch.setenv("IVR_IVF_CHUNK_SLOTS", str(3 * sum(sorted(sizes)[-p:]) + 1))
    chunked = scan()
    for k, (D, I), (Dw, Iw) in zip((10, 500), chunked, whole):
        assert np.array_equal(_bits(D), _bits(Dw)) and np.array_equal(I, Iw), k
        De, Ie = _expected(flat, lists, labels, Q, k, assign)
        _assert_same(D, I, De, Ie, f"chunked k={k}")
        _assert_same(Dw, Iw, De, Ie, f"whole k={k}")
    flat.close()


# -- 2. search = coarse search + list scan --------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [64, 768])
def test_search_is_coarse_search_plus_list_scan(d):
    from ivr_amd.ivf import SearchParametersIVF
    S = _setup(d)
    ivf, Q, k = S.ivf, S.queries[:33], 10
    try:
        for nprobe in (1, 3, NLIST, NLIST + 5):
            ivf.nprobe = nprobe
            D, I = ivf.search(Q, k)
            A = ivf.quantizer.search(Q, min(nprobe, NLIST))[1]
            D2, I2 = ivf.search_preassigned(Q, k, A)
            assert np.array_equal(_bits(D), _bits(D2)) and np.array_equal(I, I2), nprobe
            if nprobe >= NLIST:
                Df, If = S.flat.search(Q, k)
                _assert_same(D, I, Df, If, f"nprobe={nprobe} against the flat search")
        ivf.nprobe = 1
        D1, I1 = ivf.search(Q, k)
        Dp, Ip = ivf.search(Q, k, params=SearchParametersIVF(nprobe=NLIST))
        _assert_same(Dp, Ip, *S.flat.search(Q, k), "SearchParametersIVF(nprobe=nlist)")
        assert ivf.nprobe == 1                                  # for that call only
        D1b, I1b = ivf.search(Q, k)
        assert np.array_equal(_bits(D1), _bits(D1b)) and np.array_equal(I1, I1b)
        assert not np.array_equal(I1, Ip)                       # one list of at most 1000 rows is not the whole index
        # the device variant returns the same, as CUDA tensors
        Dd, Id = ivf.search_device(torch.from_numpy(Q).cuda(), k, nprobe=3)
        ivf.nprobe = 3
        D3, I3 = ivf.search(Q, k)
        assert Dd.is_cuda and Id.is_cuda and np.array_equal(_bits(Dd.cpu().numpy()), _bits(D3)) and np.array_equal(Id.cpu().numpy(), I3)
    finally:
        ivf.nprobe = 1


# -- 3. assignment ----------------------------------------------------------------------------------------------------------------
def test_assignment_invariants():
    from ivr_amd.ivf import IndexIVFFlat
    S = _setup(100)
    ivf = S.ivf
    assert ivf.ntotal == N and ivf.is_trained and ivf.nlist == NLIST and ivf.d == 100 and ivf.metric_type == 0
    sizes = ivf.list_sizes()
    assert sizes.dtype == np.int64 and sizes.tolist() == SIZES
    for l in range(NLIST):
        assert np.array_equal(ivf.list_ids(l), S.labels[S.lists == l]), l          # stored order = the order rows were added in
    cent = ivf.centroids
    assert np.array_equal(cent, ivf.quantizer.reconstruct_n()) and np.array_equal(cent, np.eye(NLIST, 100, dtype=np.float32))
    got = ivf.assign(S.X)
    assert got.dtype == np.int64 and np.array_equal(got, (S.X.astype(np.float64) @ cent.astype(np.float64).T).argmax(1))
    assert np.array_equal(got, S.lists)
    # a plain add labels rows 0 .. n-1 in call order
    plain = IndexIVFFlat(_axis_quantizer(100), 100, NLIST)
    plain.train(S.X)
    plain.add(S.X[:700])
    plain.add(S.X[700:])
    assert plain.ntotal == N
    for l in range(NLIST):
        assert np.array_equal(plain.list_ids(l), np.flatnonzero(S.lists == l)), l
    D, I = plain.search_preassigned(S.X[5:6], 1, np.array([[S.lists[5]]]))
    assert I[0, 0] == 5                                                              # a stored row finds itself under its row number
    plain.close()


# -- 4. the tie rule --------------------------------------------------------------------------------------------------------------
def test_equal_scores_rank_lower_list_then_earlier_row():
    from ivr_amd.ivf import IndexIVFFlat
    d = 64
    quant = _axis_quantizer(d)
    ivf = IndexIVFFlat(quant, d, NLIST)
    ivf.train(None)
    e = np.eye(NLIST, d, dtype=np.float32)
    v = e[2:3]
    rng = np.random.default_rng(4)
    # filler rows around e_2, e_5, e_2, e_2, e_7; the third is added while centroid 5 is 2 e_2, which attracts it like v (1.9 against 0.96)
    filler = _unit64(e[[2, 5, 2, 2, 7]] + 0.3 * rng.standard_normal((5, d)) / np.sqrt(d)).astype(np.float32)
    ivf.add_with_ids(np.concatenate([filler[:2], v]), [100, 101, 7])                  # label 7 -> list 2
    quant.write(5, 2 * v)                                                             # for one add, list 5 attracts v
    ivf.add_with_ids(np.concatenate([v, filler[2:3]]), [3, 102])                      # labels 3 and 102 -> list 5
    quant.write(5, e[5:6])
    ivf.add_with_ids(np.concatenate([filler[3:], v]), [103, 104, 9])                  # label 9 -> list 2, added later
    assert ivf.list_ids(2).tolist() == [100, 7, 103, 9] and ivf.list_ids(5).tolist() == [101, 3, 102] and ivf.list_ids(7).tolist() == [104]
    for assign in ([[2, 5]], [[5, 2]], [[7, 5, 2, -1]], [[5, 2, 5]]):
        D, I = ivf.search_preassigned(v, 3, np.array(assign))
        assert I.tolist() == [[7, 9, 3]], assign
        assert _bits(D).tolist() == [[_bits(np.float32(1.0)).item()] * 3], assign
    ivf.close()


# -- 5. maintenance ---------------------------------------------------------------------------------------------------------------
def test_remove_reconstruct_reset():
    S = _Setup(64, build=False)
    ivf, flat = S.make_ivf(), S.make_flat()
    rng = np.random.default_rng(55)
    in10, in8 = S.labels[S.lists == 10], S.labels[S.lists == 8]
    gone = np.concatenate([S.labels[S.lists == 4], rng.permutation(in10)[:500], rng.permutation(in8)[:100], [BIG - 5]])   # one label nobody holds
    # the rows come back with the bits they were added with, by label
    R = ivf.reconstruct_batch(S.labels[::7])
    assert np.array_equal(_bits(R), _bits(S.X[::7])) and np.array_equal(_bits(ivf.reconstruct(S.labels[11])), _bits(S.X[11]))
    with pytest.raises(RuntimeError):
        ivf.reconstruct(BIG - 5)
    assert ivf.remove_ids(gone) == len(gone) - 1 == flat.remove_ids(gone)
    keep = ~np.isin(S.labels, gone)
    lists, labels = S.lists[keep], S.labels[keep]
    want = np.array(SIZES)
    want[[4, 10, 8]] = [0, 500, 155]
    assert ivf.ntotal == keep.sum() and ivf.list_sizes().tolist() == want.tolist()
    for l in range(NLIST):
        assert np.array_equal(ivf.list_ids(l), labels[lists == l]), l               # survivors keep label, list and order
    D, I = ivf.search_preassigned(S.queries[:9], 2048, np.tile(np.arange(NLIST), (9, 1)))
    assert not np.isin(I, gone).any() and ((I >= 0).sum(1) == keep.sum()).all()
    _check_scan(S, ivf, flat, lists, labels, 17, 10)
    assert ivf.remove_ids(gone) == 0
    # reset keeps the trained quantizer; a fresh add works
    ivf.reset()
    assert ivf.ntotal == 0 and ivf.is_trained and ivf.quantizer.ntotal == NLIST and ivf.list_sizes().tolist() == [0] * NLIST
    D, I = ivf.search_preassigned(S.queries[:2], 3, np.array([[1, 2], [3, 4]]))
    assert (I == -1).all()
    ivf.add(S.X[:300])
    assert ivf.ntotal == 300 and ivf.list_sizes().tolist() == np.bincount(S.lists[:300], minlength=NLIST).tolist()
    ivf.nprobe = NLIST
    D, I = ivf.search(S.X[:300], 1)
    assert np.array_equal(I[:, 0], np.arange(300))
    ivf.close()
    flat.close()


# -- 6. training ------------------------------------------------------------------------------------------------------------------
T_N, T_D, T_NLIST = 4096, 64, 16


def _train_rows():
    rng = np.random.default_rng(606)
    centres = _unit64(rng.standard_normal((T_NLIST, T_D)))
    return _unit64(centres[rng.integers(0, T_NLIST, T_N)] + 0.3 * rng.standard_normal((T_N, T_D)) / np.sqrt(T_D)).astype(np.float32)


def _trained(X, **kw):
    from ivr_amd.ivf import IVFFlatIndex
    ivf = IVFFlatIndex(T_D, T_NLIST)
    assert not ivf.is_trained and ivf.quantizer.ntotal == 0
    ivf.train(X, **kw)
    assert ivf.is_trained and ivf.quantizer.ntotal == T_NLIST
    return ivf


def _objective(X, cent):
    return (X.astype(np.float64) @ cent.astype(np.float64).T).max(1).mean()


def test_training_is_reproducible_spherical_and_improves():
    from ivr_amd.index import FlatIPIndex
    X = _train_rows()
    a, b, c = _trained(X), _trained(X), _trained(X, seed=99)
    ca, cb, cc = a.centroids, b.centroids, c.centroids
    assert ca.shape == (T_NLIST, T_D) and np.array_equal(_bits(ca), _bits(cb))
    assert not np.array_equal(_bits(ca), _bits(cc))
    for cent in (ca, cc):
        assert np.isfinite(cent).all() and np.abs(np.linalg.norm(cent.astype(np.float64), axis=1) - 1).max() <= 1e-6
    # both steps of spherical k-means are non-decreasing in the mean best-centroid score
    c0 = _trained(X, niter=0)
    from ivr_amd.ivf import kmeans_sample
    init = _unit64(X[kmeans_sample(T_N, T_NLIST)[:T_NLIST]])
    assert np.abs(c0.centroids - init).max() <= 1e-6            # niter = 0: the (normalised) initial centroids
    o0, o10 = _objective(X, c0.centroids), _objective(X, ca)
    print(f"mean best-centroid score: niter=0 {o0:.6f}, niter=10 {o10:.6f}")
    assert o10 >= o0
    # plain means (faiss's default) are means: inside the unit ball, not on it
    p = _trained(X, spherical=False)
    nrm = np.linalg.norm(p.centroids.astype(np.float64), axis=1)
    assert np.isfinite(p.centroids).all() and (nrm < 1 - 1e-3).all()
    # nprobe = nlist sees every row: recall@10 against the flat index is 1.0
    a.add(X)
    flat = FlatIPIndex(T_D)
    flat.add(X)
    Q = X[::41]
    a.nprobe = T_NLIST
    D, I = a.search(Q, 10)
    Df, If = flat.search(Q, 10)
    recall = np.mean([len(set(I[i]) & set(If[i])) / 10 for i in range(len(Q))])
    assert recall == 1.0
    assert np.array_equal(_bits(D), _bits(Df))
    assert a.list_sizes().sum() == T_N and np.array_equal(np.bincount(a.assign(X), minlength=T_NLIST), a.list_sizes())
    for x in (a, b, c, c0, p, flat):
        x.close()


def test_training_repairs_an_empty_cluster():
    from ivr_amd.ivf import kmeans_sample
    X = _train_rows()
    first = kmeans_sample(T_N, T_NLIST, 256, 1234)[:T_NLIST]
    X[first[1]] = X[first[0]]                      # two identical initial centroids: ties go to the lower one, the other stays empty
    X[first[7]] = X[first[0]]
    ivf = _trained(X)
    cent = ivf.centroids
    assert cent.shape == (T_NLIST, T_D) and np.isfinite(cent).all()
    assert np.abs(np.linalg.norm(cent.astype(np.float64), axis=1) - 1).max() <= 1e-6
    assert len(np.unique(_bits(cent), axis=0)) == T_NLIST       # the repaired clusters moved apart
    ivf.close()


# -- 7. errors, before any launch -------------------------------------------------------------------------------------------------
def test_errors():
    from ivr_amd import _ffi
    from ivr_amd.index import FlatIPIndex, IDSelectorRange, IndexIDMap2
    from ivr_amd.ivf import METRIC_L2, IndexIVFFlat, IVFFlatIndex, SearchParametersIVF
    d = 64
    x = _unit64(np.random.default_rng(1).standard_normal((40, d))).astype(np.float32)
    fresh = IVFFlatIndex(d, 8)
    with pytest.raises(RuntimeError):
        fresh.add(x)
    with pytest.raises(RuntimeError):
        fresh.add_with_ids(x, np.arange(40))
    with pytest.raises(ValueError):
        fresh.train(x[:7])
    with pytest.raises(ValueError):
        fresh.train(x[:, :32])
    small = FlatIPIndex(d)
    small.add(x[:3])
    with pytest.raises(ValueError):
        IndexIVFFlat(small, d, 8)
    with pytest.raises(ValueError):
        IndexIVFFlat(IndexIDMap2(FlatIPIndex(d)), d, 8)
    with pytest.raises(ValueError):
        IndexIVFFlat(FlatIPIndex(d), d, 8, METRIC_L2)
    with pytest.raises(ValueError):
        IndexIVFFlat(FlatIPIndex(32), d, 8)
    with pytest.raises(ValueError):
        IndexIVFFlat("quantizer", d, 8)
    ivf = IndexIVFFlat(_axis_quantizer(d, 8), d, 8)
    ivf.train(x)
    ivf.add(x)
    ok = np.zeros((2, 3), np.int64)
    for bad in (8, -2):
        a = ok.copy()
        a[1, 2] = bad
        with pytest.raises(ValueError):
            ivf.search_preassigned(x[:2], 5, a)
        with pytest.raises(ValueError):
            ivf.search_preassigned(x[:2], 5, torch.from_numpy(a).cuda())
    with pytest.raises(ValueError):
        ivf.search_preassigned(x[:3], 5, ok)                     # two assign rows for three queries
    with pytest.raises(ValueError):
        ivf.search_preassigned(x[:2], 5, ok.astype(np.float32))
    with pytest.raises(ValueError, match="not supported on IVFFlatIndex"):
        ivf.search(x[:2], 5, params=SearchParametersIVF(sel=IDSelectorRange(0, 10)))
    for k in (0, _ffi.IVR_MAX_K + 1):
        with pytest.raises(ValueError):
            ivf.search(x[:2], k)
        with pytest.raises(ValueError):
            ivf.search_preassigned(x[:2], k, ok)
    with pytest.raises(ValueError):
        ivf.search(x[:2, :32], 5)
    with pytest.raises(ValueError):
        ivf.add(x[:, :32])
    with pytest.raises(ValueError):
        ivf.add_with_ids(x[:2], [1, -1])
    with pytest.raises(ValueError):
        ivf.add_with_ids(x[:2], [1])
    with pytest.raises(ValueError):
        ivf.nprobe = 0
    assert ivf.ntotal == 40                                      # nothing of the above changed the index
    D, I = ivf.search_preassigned(x[:2], 5, ok)
    assert D.shape == (2, 5) and I.dtype == np.int64
    for i in (fresh, ivf, small):
        i.close()
