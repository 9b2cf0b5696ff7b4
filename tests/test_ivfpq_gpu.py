"""GPU suite of the inverted-file index over product-quantised codes (ivr_amd/ivfpq.py IVFPQIndex, csrc/search_ivfpq.hip).

The scan adds a coarse score and table entries only, so D and I of search_tables_preassigned_device must equal ivfpq_scan_ref element
for element; the lists go into the store as chosen codes, so no tolerance enters.  The stored codes are the encoder's output on the
float32 residuals, the same kernel on the same bits, so they are compared exactly too.  Seven lists of 0, 1, 63, 64, 65, 300 and 17
rows sit on both sides of a 64-row wave group; M covers a partly filled 16-byte word and every word count the store has; ties are
forced by repeated codes across lists and few-valued tables."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

FLT_MAX = np.finfo(np.float32).max
SIZES = [0, 1, 63, 64, 65, 300, 17]
NLIST = len(SIZES)
NROWS = sum(SIZES)


def unit_rows(rng, n, d):
    x = rng.standard_normal((n, d)).astype(np.float32)
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def make_index(d, nlist, M, centroids, C=None, by_residual=True):
    """An IVFPQIndex over the given coarse centroids, with the codebooks C assigned when given."""
    from ivr_amd.index import FlatIPIndex
    from ivr_amd.ivfpq import IndexIVFPQ
    quantizer = FlatIPIndex(d)
    quantizer.add(centroids)
    idx = IndexIVFPQ(quantizer, d, nlist, M)
    idx.by_residual = by_residual
    if C is not None:
        idx.pq.centroids = C
        assert idx.is_trained
    return idx


def scan_index(M, codes, ids, off, rng):
    """A trained index of M-byte codes whose lists hold exactly `codes` / `ids` as delimited by `off`."""
    idx = make_index(2 * M, len(off) - 1, M, unit_rows(rng, len(off) - 1, 2 * M), np.zeros((M, 256, 2), np.float32))
    idx._set_lists(torch.from_numpy(codes).cuda(), torch.from_numpy(ids).cuda(), np.asarray(off, np.int64))
    assert idx.ntotal == len(codes) and idx.list_sizes().tolist() == np.diff(off).tolist()
    got_codes, got_ids = idx._rows_device()                        # the unpack kernel at this M's word count
    assert np.array_equal(got_codes.cpu().numpy(), codes) and np.array_equal(got_ids.cpu().numpy(), ids)
    return idx


def check_scan(idx, T, coarse, assign, codes, ids, off, k):
    from ivr_amd.ivfpq import ivfpq_scan_ref
    D, I = idx.search_tables_preassigned_device(T, coarse, assign, k)
    D, I = D.cpu().numpy(), I.cpu().numpy()
    assert D.dtype == np.float32 and I.dtype == np.int64 and D.shape == I.shape == (len(T), k)
    Dr, Ir = ivfpq_scan_ref(T, np.zeros(assign.shape, np.float32) if coarse is None else coarse, assign, off, codes, ids, k)
    assert np.array_equal(I, Ir)
    assert np.array_equal(bits(D), bits(Dr))
    return D, I


def lists_with_ties(rng, M):
    off = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int64)
    codes = rng.integers(0, 256, (NROWS, M), dtype=np.uint8)
    codes[rng.integers(0, NROWS, NROWS // 3)] = codes[70]          # one code repeated across every list: equal scores between lists
    ids = rng.permutation(NROWS).astype(np.int64) + 1000            # labels are not positions
    return codes, ids, off


def assign_rows(rng, nq, p):
    """Probe rows with -1 entries and a list named twice (p >= 3); row 0 of p = nlist names every list once."""
    a = rng.integers(0, NLIST, (nq, p)).astype(np.int64)
    if p >= 3:
        a[::2, 1] = -1
        a[1::2, 2] = a[1::2, 0]
    if p == NLIST:
        a[0] = rng.permutation(NLIST)
    return a


# -- scan ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [2, 16, 24, 48, 64, 128])
def test_scan_equals_the_reference_bit_for_bit(M):
    """M = 2 / 16 / 24 / 48 / 64 / 128: a partly filled word and 1, 2, 3, 4 and 8 words.  37 and 5 queries are more than one
    workgroup of the probe kernel with a ragged last one; k = 510 / 513 are at and above the rows a query probes when it names every
    list."""
    rng = np.random.default_rng(M)
    codes, ids, off = lists_with_ties(rng, M)
    idx = scan_index(M, codes, ids, off, rng)
    for nq in (1, 5, 37):
        T = rng.standard_normal((nq, M, 256)).astype(np.float32)
        two = rng.integers(0, 2, (nq, M, 256)).astype(np.float32)   # two-valued tables: scores are small integers, tied in bulk
        for p in (1, 3, NLIST):
            a = assign_rows(rng, nq, p)
            coarse = rng.standard_normal((nq, p)).astype(np.float32)
            for k in (1, 10) + ((NROWS, NROWS + 3) if p == NLIST else ()):
                check_scan(idx, T, coarse, a, codes, ids, off, k)
            check_scan(idx, two, rng.integers(0, 2, (nq, p)).astype(np.float32), a, codes, ids, off, 50)
            check_scan(idx, two, None, a, codes, ids, off, 50)
    idx.close()


def test_scan_ties_pads_and_the_coarse_score():
    rng = np.random.default_rng(7)
    M = 16
    off = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int64)
    one = np.tile(rng.integers(0, 256, (1, M), dtype=np.uint8), (NROWS, 1))       # every row one code: every score equal
    ids = np.arange(NROWS, dtype=np.int64)
    idx = scan_index(M, one, ids, off, rng)
    T = rng.standard_normal((2, M, 256)).astype(np.float32)
    every = np.tile(np.arange(NLIST)[::-1], (2, 1)).astype(np.int64)             # named in descending order: the order must not matter
    D, I = check_scan(idx, T, None, every, one, ids, off, NROWS + 5)
    assert (I[:, :NROWS] == np.arange(NROWS)).all()                # the lower list first, inside a list the earlier row
    assert (I[:, NROWS:] == -1).all() and (D[:, NROWS:] == -FLT_MAX).all()
    # a nonzero coarse score changes the order between lists: list 6 (17 rows) in front of list 5 (300 rows) in front of the rest
    coarse = np.zeros((2, NLIST), np.float32)
    coarse[:, 0], coarse[:, 1] = 2.0, 1.0                          # entries 0 and 1 name lists 6 and 5
    D, I = check_scan(idx, T, coarse, every, one, ids, off, 400)
    assert (I[:, :17] == np.arange(off[6], off[7])).all() and (I[:, 17:317] == np.arange(off[5], off[6])).all()
    assert (I[:, 317:400] == np.arange(83)).all()
    # only the empty list, only -1: nothing but padding
    for a in ([[0]], [[-1]]):
        D, I = check_scan(idx, T[:1], None, np.array(a, np.int64), one, ids, off, 3)
        assert (I == -1).all() and (D == -FLT_MAX).all()
    negz = np.full((1, M, 256), -0.0, np.float32)
    D, I = check_scan(idx, negz, np.full((1, 2), -0.0, np.float32), np.array([[2, 1]], np.int64), one, ids, off, 10)
    assert (I == np.arange(10)).all() and (D == 0).all() and not np.signbit(D).any()
    with pytest.raises(ValueError):
        idx.search_tables_preassigned_device(T, None, np.full((2, 1), NLIST, np.int64), 1)      # a list that does not exist
    with pytest.raises(ValueError):
        idx.search_tables_preassigned_device(T[:, :8], None, every, 1)
    idx.reset()
    D, I = check_scan(idx, T, None, every, one[:0], ids[:0], np.zeros(NLIST + 1, np.int64), 3)   # an empty index
    assert (I == -1).all() and idx.ntotal == 0
    idx.close()


def test_scan_crosses_the_query_groupings(monkeypatch):
    """The probe kernel takes ivr_ivfpq_probe_queries() queries per workgroup and the scan one; a chunk of queries is bounded by its
    key slots (IVR_IVFPQ_CHUNK_SLOTS, read when the index is made).  With p = 3 a query may probe 5 + 2 + 1 groups = 512 slots, so
    1600 slots are chunks of 3 queries: 2 workgroups of the probe kernel + 3 queries are chunks of 3 with a ragged last one, and
    the chunked call equals the unchunked one."""
    from ivr_amd import _ffi
    rng = np.random.default_rng(8)
    M = 24
    codes, ids, off = lists_with_ties(rng, M)
    nq = 2 * _ffi.load().ivr_ivfpq_probe_queries() + 3
    T = rng.standard_normal((nq, M, 256)).astype(np.float32)
    a = assign_rows(rng, nq, 3)
    coarse = rng.standard_normal((nq, 3)).astype(np.float32)
    whole = scan_index(M, codes, ids, off, rng)
    Dw, Iw = check_scan(whole, T, coarse, a, codes, ids, off, 20)
    whole.close()
    monkeypatch.setenv("IVR_IVFPQ_CHUNK_SLOTS", "1600")
    idx = scan_index(M, codes, ids, off, rng)
    D, I = check_scan(idx, T, coarse, a, codes, ids, off, 20)
    assert np.array_equal(I, Iw) and np.array_equal(bits(D), bits(Dw))
    idx.close()


def scan_shape(max_groups, nq, share=128):
    """(workgroups per query, groups per workgroup, groups per wave) of ivfpq_scan_kernel for a chunk of nq queries that may probe
    max_groups groups each: the grid ivr_ivfpq_search chooses (csrc/search_ivfpq.hip), 8 waves per workgroup."""
    from ivr_amd import _ffi
    cu = _ffi.device_info()["cu_count"]
    gx = max(1, min(-(-max_groups // 8), max(-(-max_groups // share), -(-2 * cu // nq))))
    per_wg = -(-max_groups // gx)
    return gx, per_wg, -(-per_wg // 8)


def walk_rows(rng, nq, nlist):
    """Probe rows of nlist + 3 entries: every list once, one list twice more, one -1, shuffled.  Sorted, a row starts with the -1 and
    holds the duplicates and the empty lists between the lists a wave walks across."""
    a = np.empty((nq, nlist + 3), np.int64)
    for i in range(nq):
        dup = rng.integers(0, nlist)
        a[i] = rng.permutation(np.concatenate([np.arange(nlist), [dup, dup, -1]]))
    return a


@pytest.mark.parametrize("sizes, nq_of", [
    (SIZES, lambda cu: 2 * cu + 3),                          # enough queries to fill the device: one workgroup per query, 11 groups
    ([0, 9000, 1, 6000, 700, 65, 0], lambda cu: 40),         # 249 groups per query: several workgroups per query, 3 groups per wave
])
def test_scan_waves_that_walk_across_lists(sizes, nq_of):
    """A wave of the scan takes a contiguous run of a query's groups and walks forward over the probe entries.  Here a run is 2 or
    3 groups (asserted from the grid the library chooses), so it crosses list boundaries, duplicates of a list, empty lists in the
    middle and at the end of the row, and starts inside a list of several groups.  M = 2 keeps the numpy reference small."""
    from ivr_amd import _ffi
    rng = np.random.default_rng(len(sizes) + sum(sizes))
    M, nlist, n = 2, len(sizes), sum(sizes)
    nq = nq_of(_ffi.device_info()["cu_count"])
    groups = sum(-(-s // 64) for s in sizes)
    gx, per_wg, per_wave = scan_shape(groups, nq)
    print(f"walk: {groups} groups per query, nq = {nq}: {gx} workgroups per query, {per_wg} groups each, {per_wave} per wave")
    assert per_wave >= 2
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    codes = rng.integers(0, 256, (n, M), dtype=np.uint8)
    codes[rng.integers(0, n, n // 3)] = codes[0]                # equal scores across lists
    ids = rng.permutation(n).astype(np.int64)
    idx = scan_index(M, codes, ids, off, rng)
    a = walk_rows(rng, nq, nlist)
    T = rng.standard_normal((nq, M, 256)).astype(np.float32)
    coarse = rng.standard_normal(a.shape).astype(np.float32)
    for k in (10, 700):
        check_scan(idx, T, coarse, a, codes, ids, off, k)
    check_scan(idx, rng.integers(0, 2, T.shape).astype(np.float32), None, a, codes, ids, off, 100)
    # three probed lists of the row only: the run of a wave ends inside the row
    check_scan(idx, T, coarse[:, :5], a[:, :5], codes, ids, off, 10)
    idx.close()


# -- lists: pack, unpack, encode -----------------------------------------------------------------------------------------------
def rows_for_lists(rng, sizes, d):
    """Coarse centroids (the first len(sizes) unit vectors) and rows that fall into list l sizes[l] times, shuffled."""
    cent = np.eye(len(sizes), d, dtype=np.float32)
    lists = rng.permutation(np.repeat(np.arange(len(sizes)), sizes))
    x = cent[lists] + np.float32(0.05) * rng.standard_normal((len(lists), d)).astype(np.float32)
    return cent, x.astype(np.float32), lists


@pytest.mark.parametrize("M, by_residual", [(4, True), (24, True), (24, False), (48, True), (64, True), (128, True)])
def test_lists_after_add_hold_the_encoder_codes_of_the_residuals(M, by_residual):
    """The lists of 0, 1, 63, 64, 65, 300 and 17 rows, added in two calls: list_codes / list_ids are the rows of each list in the
    order they were added, their codes pq.sa_encode of the numpy float32 residual (of the row itself without by_residual), exactly,
    and the whole store is the numpy layout's round trip."""
    from ivr_amd.ivfpq import ivfpq_pack_ref, ivfpq_unpack_ref
    rng = np.random.default_rng(M)
    d = 2 * M
    cent, x, lists = rows_for_lists(rng, SIZES, d)
    idx = make_index(d, NLIST, M, cent, rng.standard_normal((M, 256, 2)).astype(np.float32) * np.float32(0.05), by_residual)
    assert np.array_equal(idx.assign(x), lists) and np.array_equal(idx.centroids, cent)
    cut = 200
    idx.add(x[:cut])
    assert idx.ntotal == cut and idx.list_sizes().tolist() == np.bincount(lists[:cut], minlength=NLIST).tolist()
    idx.add(x[cut:])
    assert idx.ntotal == NROWS and idx.list_sizes().tolist() == SIZES
    want = idx.pq.sa_encode(x - cent[lists] if by_residual else x)
    allc, alli = [], []
    for l in range(NLIST):
        rows = np.flatnonzero(lists == l)                          # ascending: the order of adding
        assert np.array_equal(idx.list_ids(l), rows)
        assert np.array_equal(idx.list_codes(l), want[rows])
        assert idx.list_codes(l).shape == (SIZES[l], M) and idx.list_codes(l).dtype == np.uint8
        allc.append(want[rows])
        alli.append(rows)
    codes, ids = idx._rows_device()
    off = np.concatenate([[0], np.cumsum(SIZES)])
    assert np.array_equal(codes.cpu().numpy(), ivfpq_unpack_ref(ivfpq_pack_ref(np.concatenate(allc), off), off, M))
    assert np.array_equal(ids.cpu().numpy(), np.concatenate(alli))
    with pytest.raises(ValueError):
        idx.list_codes(NLIST)
    with pytest.raises(RuntimeError):
        idx.pq.centroids = idx.pq.centroids                        # rows are encoded with the current codebooks
    with pytest.raises(RuntimeError):
        idx.by_residual = not by_residual
    idx.reset()
    assert idx.ntotal == 0 and idx.is_trained and idx.list_sizes().tolist() == [0] * NLIST
    idx.add_with_ids(x[:70], np.arange(70) + 5)
    assert sorted(np.concatenate([idx.list_ids(l) for l in range(NLIST)]).tolist()) == list(range(5, 75))
    idx.close()


# -- the shared layer ----------------------------------------------------------------------------------------------------------
def test_an_index_holds_no_row_store_but_its_own():
    """A constructed IVFPQIndex reaches, through its instance attributes, no IVFFlatIndex and no FlatIPIndex other than its quantizer:
    the coarse side is the shared layer's, not a second index with an empty row store."""
    from ivr_amd.index import FlatIPIndex
    from ivr_amd.ivf import IVFFlatIndex
    from ivr_amd.ivfpq import IVFPQIndex
    idx = IVFPQIndex(32, 4, 4)
    seen, stack, found = set(), [idx], []
    while stack:
        o = stack.pop()
        if id(o) in seen:
            continue
        seen.add(id(o))
        if isinstance(o, (IVFFlatIndex, FlatIPIndex)):
            found.append(o)
        if isinstance(o, dict):
            stack.extend(o.values())
        elif isinstance(o, (list, tuple, set)):
            stack.extend(o)
        elif type(o).__module__.startswith("ivr_amd"):
            stack.extend(vars(o).values())
    assert len(found) == 1 and found[0] is idx.quantizer
    idx.close()
    idx.close()                                                    # harmless


@pytest.mark.parametrize("spherical, by_residual, repair", [(True, True, False), (False, False, False), (True, False, True), (False, True, True)])
def test_training_is_the_coarse_training_then_the_pq_training(monkeypatch, spherical, by_residual, repair):
    """IVFPQIndex.train leaves the quantizer with the bits IVFFlatIndex.train gives on the same rows and arguments, and the codebooks
    with the bits PQIndex.train gives on the float32 residuals x - centroids[assign(x)] (on x without by_residual).  repair: two
    sampled rows are equal, so an initial centroid and (same permutation, same rows or residuals) an initial codebook entry of every
    slice start empty and both trainings go through the repair of empty clusters, which the test watches being called."""
    from ivr_amd import _kmeans
    from ivr_amd.ivf import IVFFlatIndex, kmeans_sample
    from ivr_amd.ivfpq import IVFPQIndex
    from ivr_amd.pq import PQIndex
    n, d, nlist, M = 2048, 32, 8, 4
    x = unit_rows(np.random.default_rng(77), n, d)
    if repair:
        first = kmeans_sample(n, nlist)[:nlist]
        x[first[1]] = x[first[0]]
    split, repaired = _kmeans.split_empty_clusters, []              # the shapes of the centroid sets that had an empty cluster
    monkeypatch.setattr(_kmeans, "split_empty_clusters", lambda c, n: repaired.append(c.shape) or split(c, n))
    idx = IVFPQIndex(d, nlist, M)
    idx.by_residual = by_residual
    idx.train(x, spherical=spherical)
    if repair:
        assert (nlist, d) in repaired and (256, d // M) in repaired
    del repaired[:]
    flat = IVFFlatIndex(d, nlist)
    flat.train(x, spherical=spherical)
    assert ((nlist, d) in repaired) == repair
    cent = flat.centroids
    assert np.isfinite(cent).all() and np.array_equal(bits(idx.centroids), bits(cent))
    pq = PQIndex(d, M)
    del repaired[:]
    pq.train(x - cent[idx.assign(x)] if by_residual else x)
    assert not repair or (256, d // M) in repaired
    assert np.isfinite(pq.centroids).all() and np.array_equal(bits(idx.pq.centroids), bits(pq.centroids))
    for i in (idx, flat, pq):
        i.close()


# -- end to end ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def trained_rows():
    rng = np.random.default_rng(2025)
    return unit_rows(rng, 1500, 32), unit_rows(rng, 9, 32)


def trained_index(x, by_residual=True, nlist=NLIST, M=16):
    from ivr_amd.index import FlatIPIndex
    from ivr_amd.ivfpq import IndexIVFPQ
    idx = IndexIVFPQ(FlatIPIndex(x.shape[1]), x.shape[1], nlist, M)
    idx.by_residual = by_residual
    assert not idx.is_trained
    idx.train(x, niter=2)
    assert idx.is_trained and idx.quantizer.ntotal == nlist
    return idx


def test_untrained_index_parameters_and_selectors(trained_rows):
    from ivr_amd.index import FlatIPIndex, IDSelectorRange, SearchParameters
    from ivr_amd.ivf import SearchParametersIVF
    from ivr_amd.ivfpq import IndexIVFPQ
    x, q = trained_rows
    idx = IndexIVFPQ(FlatIPIndex(32), 32, NLIST, 16)
    assert (idx.nlist, idx.M, idx.code_size, idx.nprobe, idx.by_residual, idx.ntotal) == (NLIST, 16, 16, 1, True, 0)
    with pytest.raises(RuntimeError):
        idx.add(x[:10])
    with pytest.raises(RuntimeError):
        idx.search(q, 1)
    with pytest.raises(ValueError):
        idx.nprobe = 0
    idx.close()
    idx = trained_index(x)
    with pytest.raises(RuntimeError):
        idx.by_residual = False                                    # trained on residuals
    idx.add(x)
    idx.nprobe = 3
    D3, I3 = idx.search(q, 10)
    idx.nprobe = 1
    D1, I1 = idx.search(q, 10)
    D, I = idx.search(q, 10, params=SearchParametersIVF(nprobe=3))  # overrides the attribute for this call
    assert np.array_equal(I, I3) and np.array_equal(bits(D), bits(D3)) and not np.array_equal(I1, I3)
    Dt, It = idx.search_device(torch.from_numpy(q).cuda(), 10, nprobe=3)
    assert np.array_equal(It.cpu().numpy(), I3) and np.array_equal(bits(Dt.cpu().numpy()), bits(D3))
    with pytest.raises(ValueError, match="not supported on IVFPQIndex"):
        idx.search(q, 10, params=SearchParametersIVF(nprobe=2, sel=IDSelectorRange(0, 5)))
    with pytest.raises(ValueError):
        idx.search(q, 10, params=SearchParameters())
    with pytest.raises(ValueError):
        idx.search(q, 0)
    with pytest.raises(ValueError):
        idx.add_with_ids(x[:2], np.array([3, -1]))
    idx.close()


def test_search_is_search_preassigned_with_the_quantizers_own_lists(trained_rows):
    from ivr_amd.ivf import SearchParametersIVF
    from ivr_amd.ivfpq import ivfpq_scan_ref
    x, q = trained_rows
    idx = trained_index(x)
    idx.add(x[:800])
    idx.add(x[800:])
    off = np.concatenate([[0], np.cumsum(idx.list_sizes())])
    codes, ids = (t.cpu().numpy() for t in idx._rows_device())
    for nprobe in (1, 3):
        Dc, Ic = idx.quantizer.search(q, nprobe)
        D, I = idx.search(q, 10, params=SearchParametersIVF(nprobe=nprobe))
        for coarse_dis in (Dc, None):                              # omitted: the same bits, computed for exactly the named lists
            Dp, Ip = idx.search_preassigned(q, 10, Ic, coarse_dis)
            assert np.array_equal(I, Ip) and np.array_equal(bits(D), bits(Dp))
        Dr, Ir = ivfpq_scan_ref(idx.compute_tables_device(q).cpu().numpy(), Dc, Ic, off, codes, ids, 10)
        assert np.array_equal(I, Ir) and np.array_equal(bits(D), bits(Dr))
    # nprobe >= nlist: no coarse search, every list with the scores compute_distance_subset gives
    every = np.tile(np.arange(NLIST), (len(q), 1))
    D, I = idx.search_device(q, 10, nprobe=NLIST + 5)
    Dp, Ip = idx.search_preassigned(q, 10, every, idx.quantizer.compute_distance_subset(q, every))
    assert np.array_equal(I.cpu().numpy(), Ip) and np.array_equal(bits(D.cpu().numpy()), bits(Dp))
    with pytest.raises(ValueError):
        idx.search_preassigned(q, 10, every[:, :0])
    with pytest.raises(ValueError):
        idx.search_preassigned(q, 10, every + 1)
    idx.close()


def test_without_residuals_every_list_gives_the_scores_of_the_pq_index(trained_rows):
    """by_residual = False and nprobe = nlist: D is PQIndex.search's D over the same rows and codebooks bit for bit; I names rows
    whose recomputed scores are D (equal scores are ordered by list here and by row there)."""
    from ivr_amd.pq import IndexPQ
    x, q = trained_rows
    idx = trained_index(x, by_residual=False)
    idx.add(x)
    pq = IndexPQ(32, 16)
    pq.centroids = idx.pq.centroids
    pq.add(x)
    idx.nprobe = NLIST
    D, I = idx.search(q, 25)
    Dp, _ = pq.search(q, 25)
    assert np.array_equal(bits(D), bits(Dp))
    T, codes = idx.compute_tables_device(q).cpu().numpy(), pq.codes
    S = T[:, 0, codes[:, 0]].copy()
    for m in range(1, 16):
        S = S + T[:, m, codes[:, m]]
    assert sorted(I[0].tolist()) == sorted(set(I[0].tolist())) and I.min() >= 0
    assert np.array_equal(bits(np.take_along_axis(S, I, axis=1) + np.float32(0.0)), bits(D))
    idx.close()
    pq.close()


def test_reconstruction(trained_rows):
    x, _ = trained_rows
    for by_residual in (True, False):
        idx = trained_index(x, by_residual=by_residual)
        labels = np.arange(300, dtype=np.int64) * 3 + 7
        labels[10] = labels[200]                                   # a duplicate label: the lowest stored position answers
        idx.add_with_ids(x[:300], labels)
        lists = idx.assign(x[:300])
        codes = idx.pq.sa_encode(x[:300] - idx.centroids[lists] if by_residual else x[:300])
        dec = idx.pq.sa_decode(codes)
        want = idx.centroids[lists] + dec if by_residual else dec
        ask = np.array([labels[299], labels[0], labels[57], labels[0]])
        got = idx.reconstruct_batch(ask)
        assert got.dtype == np.float32 and np.array_equal(bits(got), bits(want[[299, 0, 57, 0]]))
        assert np.array_equal(bits(idx.reconstruct(int(labels[57]))), bits(want[57]))
        # rows 10 and 200 share a label: the one in the lower list, or the earlier one inside a list, is stored first
        first = 10 if lists[10] <= lists[200] else 200
        assert np.array_equal(bits(idx.reconstruct(int(labels[200]))), bits(want[first]))
        for call in (lambda: idx.reconstruct(8), lambda: idx.reconstruct_batch([7, 8])):
            with pytest.raises(RuntimeError, match="not in the index"):
                call()
        assert idx.reconstruct_batch(np.zeros(0, np.int64)).shape == (0, 32)
        idx.close()


# -- refine --------------------------------------------------------------------------------------------------------------------
def test_refine_over_an_ivfpq_base_with_every_row_a_candidate():
    from ivr_amd.index import FlatIPIndex
    from ivr_amd.ivf import SearchParametersIVF
    from ivr_amd.ivfpq import IndexIVFPQ
    from ivr_amd.refine import IndexRefineFlat, IndexRefineSearchParameters
    rng = np.random.default_rng(14)
    x, q = unit_rows(rng, 500, 32), unit_rows(rng, 7, 32)
    r = IndexRefineFlat(IndexIVFPQ(FlatIPIndex(32), 32, NLIST, 16))
    assert not r.is_trained
    r.train(x)
    r.add(x)
    assert r.is_trained and r.ntotal == r.base_index.ntotal == 500
    params = IndexRefineSearchParameters(k_factor=50, base_index_params=SearchParametersIVF(nprobe=NLIST))     # 10 * 50 = ntotal
    D, I = r.search(q, 10, params=params)
    flat = FlatIPIndex(32)
    flat.add(x)
    Df, If = flat.search(q, 10)
    assert np.array_equal(I, If) and np.array_equal(bits(D), bits(Df))
    r.base_index.nprobe = NLIST
    r.k_factor = 50
    D, I = r.search(q, 10)
    assert np.array_equal(I, If) and np.array_equal(bits(D), bits(Df))
    r.close()
    r.base_index.close()
    flat.close()
