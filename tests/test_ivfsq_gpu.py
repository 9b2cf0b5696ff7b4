"""GPU suite of the inverted-file index over scalar-quantiser codes (ivr_amd/ivfsq.py IVFSQIndex, csrc/search_ivfsq.hip).

The scan is an exact integer sum followed by four individually rounded float32 steps, so D and I of search_codes_preassigned_device
must equal ivfsq_scan_ref element for element; the lists go into the store as chosen codes, so no tolerance enters.  The stored codes
are the encoder's output on the float32 residuals, the same kernel on the same bits, so they are compared exactly too.  Twelve lists
of 0, 1, 15, 16, 17, 63, 64, 65, 0, 300, 700 and 5 rows sit on both sides of a 16-row MFMA tile, of a 64-row group and of the 256-row
split of a workgroup; 1, 16, 17 and 40 queries that all probe a list are one, two and three 16-query pair tiles, some partly filled.
Every quantizer is filled with chosen centroids; only the training test runs k-means."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

FLT_MAX = np.finfo(np.float32).max
SIZES = [0, 1, 15, 16, 17, 63, 64, 65, 0, 300, 700, 5]
NLIST = len(SIZES)
NROWS = sum(SIZES)
OFF = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int64)


def unit_rows(rng, n, d):
    x = rng.standard_normal((n, d)).astype(np.float32)
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def make_index(d, nlist, centroids, trained=None, by_residual=True):
    """An IVFSQIndex over the given coarse centroids, with the min / max table assigned when given."""
    from ivr_amd.index import FlatIPIndex
    from ivr_amd.ivfsq import IndexIVFScalarQuantizer
    quantizer = FlatIPIndex(d)
    quantizer.add(centroids)
    idx = IndexIVFScalarQuantizer(quantizer, d, nlist, by_residual=by_residual)
    assert idx.by_residual == by_residual and not idx.is_trained
    if trained is not None:
        idx.sq.trained = trained
        assert idx.is_trained
    return idx


def scan_index(d, codes, ids, off, rng):
    """A trained index of d-byte codes whose lists hold exactly `codes` / `ids` as delimited by `off`."""
    nlist = len(off) - 1
    idx = make_index(d, nlist, unit_rows(rng, nlist, d), np.concatenate([np.zeros(d), np.ones(d)]).astype(np.float32))
    idx._set_lists(torch.from_numpy(codes).cuda(), torch.from_numpy(ids).cuda(), np.asarray(off, np.int64))
    assert idx.ntotal == len(codes) and idx.list_sizes().tolist() == np.diff(off).tolist()
    got_codes, got_ids = idx._rows_device()                        # the pack and unpack kernels at this d
    assert np.array_equal(got_codes.cpu().numpy(), codes) and np.array_equal(got_ids.cpu().numpy(), ids)
    return idx


def check_scan(idx, form, coarse, assign, codes, ids, off, k):
    from ivr_amd.ivfsq import ivfsq_scan_ref
    t, scale, bias = form
    D, I = idx.search_codes_preassigned_device(t, scale, bias, coarse, assign, k)
    D, I = D.cpu().numpy(), I.cpu().numpy()
    assert D.dtype == np.float32 and I.dtype == np.int64 and D.shape == I.shape == (len(t), k)
    Dr, Ir = ivfsq_scan_ref(t, scale, bias, coarse, assign, off, codes, ids, k)
    assert np.array_equal(I, Ir)
    assert np.array_equal(bits(D), bits(Dr))
    return D, I


def random_lists(rng, d):
    codes = rng.integers(0, 256, (NROWS, d), dtype=np.uint8)
    codes[rng.integers(0, NROWS, NROWS // 4)] = codes[70]          # one code repeated across the lists: equal acc between lists
    ids = rng.permutation(NROWS).astype(np.int64) + 1000            # labels are not positions
    return codes, ids


def random_form(rng, nq, d):
    """Random t in +-16256 and random positive scale and bias; the scale puts float32(acc) * scale near the bias."""
    t = rng.integers(-16256, 16257, (nq, d)).astype(np.int16)
    scale = (rng.uniform(0.5, 1.5, nq) / (16256.0 * 74.0 * np.sqrt(d))).astype(np.float32)
    return t, scale, rng.uniform(0.5, 1.5, nq).astype(np.float32)


def assign_rows(rng, nq, p):
    """p = 12: every query names every list, in an order of its own.  p = 3: three lists with -1 entries and a list named twice.
    p = 1: one list."""
    if p == NLIST:
        return np.stack([rng.permutation(NLIST) for _ in range(nq)]).astype(np.int64)
    a = rng.integers(0, NLIST, (nq, p)).astype(np.int64)
    if p >= 3:
        a[::2, 1] = -1
        a[1::2, 2] = a[1::2, 0]                                     # named twice, with two different coarse scores
        a[0, 0], a[-1, 0] = 10, 9                                   # the lists of 700 and 300 rows are probed whatever nq is
    return a


def holes(rng, a):
    """Rows that name every list -> the same with a -1 and a list named twice in every second row."""
    a = a.copy()
    a[::2, 3] = -1
    a[::2, 7] = a[::2, 1]
    return a


def scan_cases(rng, d, nqs=(1, 16, 17, 40)):
    for nq in nqs:
        form = random_form(rng, nq, d)
        for p in (1, 3, NLIST):
            a = assign_rows(rng, nq, p)
            coarse = rng.uniform(0.1, 1.0, (nq, p)).astype(np.float32)
            for k in (1, 10, 2048):                                 # 2048 exceeds the 1246 stored rows: padding
                yield form, coarse, a, k
            yield form, None, a, 10
            if p == NLIST:
                yield form, coarse, holes(rng, a), 10


# -- scan ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [16, 100, 512, 1024])
def test_scan_equals_the_reference_bit_for_bit(d):
    """d = 16: one K step that is mostly padding; 100: a K that is a multiple of neither 16 nor 64; 512: the unrolled K loop alone;
    1024: the limit of the int32 accumulator and 32 KiB of staged queries."""
    rng = np.random.default_rng(d)
    codes, ids = random_lists(rng, d)
    idx = scan_index(d, codes, ids, OFF, rng)
    for form, coarse, a, k in scan_cases(rng, d):
        check_scan(idx, form, coarse, a, codes, ids, OFF, k)
    idx.close()


def test_scan_is_exact_at_the_int32_limit():
    """d = 1024, rows of all-0 and all-255 codes against t = +-16256 throughout: |acc| reaches 16256 * 128 * 1024 = 127 * 2^24, and
    128 acc_h alone passes 2^31 on the way (sq_combine wraps).  scale = 1 and bias = 0 report float32(acc) itself."""
    d = 1024
    rng = np.random.default_rng(1)
    codes = np.zeros((6, d), np.uint8)
    codes[1] = codes[4] = 255
    codes[2, ::2] = 255
    codes[5] = rng.integers(0, 256, d)
    ids = np.arange(6, dtype=np.int64)
    off = np.array([0, 3, 6], np.int64)
    idx = scan_index(d, codes, ids, off, rng)
    t = np.stack([np.full(d, 16256), np.full(d, -16256), np.where(np.arange(d) % 2, 16256, -16256)]).astype(np.int16)
    one, zero = np.ones(3, np.float32), np.zeros(3, np.float32)
    a = np.tile(np.array([[1, 0]], np.int64), (3, 1))
    D, I = check_scan(idx, (t, one, zero), None, a, codes, ids, off, 6)
    acc = t.astype(np.int64) @ (codes.astype(np.int64) - 128).T
    assert acc.min() == -16256 * 128 * 1024 and acc.max() == 16256 * 128 * 1024
    for i in range(3):
        assert np.array_equal(D[i].astype(np.int64), acc[i, I[i]])  # 127 * 2^24 and the others here are float32 values
    assert D[0, -1] == np.float32(-2130706432.0) and D[1, 0] == np.float32(2130706432.0)
    check_scan(idx, (t, np.full(3, 2.0 ** -20, np.float32), one), np.full((3, 2), 0.5, np.float32), a, codes, ids, off, 4)
    idx.close()


def test_ties_rank_the_lower_list_then_the_earlier_row():
    """One code row stored in two lists and twice in one list, equal coarse scores: whatever order assign names the lists in."""
    d = 100
    rng = np.random.default_rng(3)
    sizes = [4, 70, 20]
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    codes = rng.integers(0, 200, (94, d), dtype=np.uint8)
    same = [1, 3, 4 + 66, 74]                                       # list 0 twice, list 1 in its second group, list 2 first
    codes[same] = 255                                               # against t > 0 the best acc there is
    ids = rng.permutation(94).astype(np.int64)
    idx = scan_index(d, codes, ids, off, rng)
    t = rng.integers(1, 16257, (3, d)).astype(np.int16)
    scale, bias = np.full(3, 1e-7, np.float32), rng.uniform(0.5, 1.5, 3).astype(np.float32)
    for order in ([0, 1, 2], [2, 1, 0], [1, 2, 0]):
        a = np.tile(np.array([order], np.int64), (3, 1))
        D, I = check_scan(idx, (t, scale, bias), np.full((3, 3), 0.5, np.float32), a, codes, ids, off, 10)
        assert (I[:, :4] == ids[same]).all() and (D[:, :4] == D[:, :1]).all() and (D[:, 4] < D[:, 0]).all()
    # a better coarse score for list 2 puts its copy in front
    coarse = np.tile(np.array([[0.5, 0.5, 0.75]], np.float32), (3, 1))
    D, I = check_scan(idx, (t, scale, bias), coarse, np.tile(np.arange(3), (3, 1)), codes, ids, off, 10)
    assert (I[:, 0] == ids[74]).all()
    idx.close()


@pytest.mark.parametrize("bias", [2.0 ** 30, -2.0 ** 30])
def test_distinct_acc_that_round_to_one_score_rank_by_position(bias):
    """|float32(acc) * scale| <= 16256 * 128 * 16 * 9e-7 = 29.97 is below half an ulp on either side of 2^30 (64 above it, 32 below):
    every D is the bias, and the rows come out in stored order although their acc differ."""
    d = 16
    rng = np.random.default_rng(4)
    codes, ids = random_lists(rng, d)
    idx = scan_index(d, codes, ids, OFF, rng)
    t = rng.integers(-16256, 16257, (2, d)).astype(np.int16)
    acc = t.astype(np.int64) @ (codes.astype(np.int64) - 128).T
    assert len(np.unique(acc[0])) > NROWS // 2
    form = (t, np.full(2, 9e-7, np.float32), np.full(2, bias, np.float32))
    a = np.stack([np.arange(NLIST)[::-1], np.random.default_rng(5).permutation(NLIST)]).astype(np.int64)
    D, I = check_scan(idx, form, np.zeros((2, NLIST), np.float32), a, codes, ids, OFF, NROWS + 2)
    assert (D[:, :NROWS] == np.float32(bias)).all() and (I[:, :NROWS] == ids).all() and (I[:, NROWS:] == -1).all()
    idx.close()


def test_several_chunks_give_the_bits_of_one(monkeypatch):
    """A chunk of queries is bounded by its key slots (IVR_IVFSQ_CHUNK_SLOTS, read when the index is made).  A query that names every
    list holds 1246 slots and one that names three at most 700 + 300 + 65, so 4000 slots are chunks of 3 queries: 40 queries are 13
    chunks and a ragged last one, and the chunked call equals the unchunked one."""
    d = 100
    rng = np.random.default_rng(6)
    codes, ids = random_lists(rng, d)
    cases = list(scan_cases(rng, d, nqs=(40,)))
    whole = scan_index(d, codes, ids, OFF, rng)
    want = [check_scan(whole, form, coarse, a, codes, ids, OFF, k) for form, coarse, a, k in cases]
    whole.close()
    monkeypatch.setenv("IVR_IVFSQ_CHUNK_SLOTS", "4000")
    idx = scan_index(d, codes, ids, OFF, rng)
    for (form, coarse, a, k), (Dw, Iw) in zip(cases, want):
        D, I = check_scan(idx, form, coarse, a, codes, ids, OFF, k)
        assert np.array_equal(I, Iw) and np.array_equal(bits(D), bits(Dw))
    idx.close()


def test_scan_argument_checks_and_the_empty_index():
    d = 16
    rng = np.random.default_rng(7)
    codes, ids = random_lists(rng, d)
    idx = scan_index(d, codes, ids, OFF, rng)
    form = random_form(rng, 2, d)
    every = np.tile(np.arange(NLIST), (2, 1)).astype(np.int64)
    for a in ([[0]], [[-1]], [[8, -1, 0]]):                         # only empty lists, only -1: nothing but padding
        D, I = check_scan(idx, tuple(f[:1] for f in form), None, np.array(a, np.int64), codes, ids, OFF, 3)
        assert (I == -1).all() and (D == -FLT_MAX).all()
    with pytest.raises(ValueError):
        idx.search_codes_preassigned_device(*form, None, np.full((2, 1), NLIST, np.int64), 1)    # a list that does not exist
    with pytest.raises(ValueError):
        idx.search_codes_preassigned_device(form[0][:, :8], form[1], form[2], None, every, 1)
    with pytest.raises(ValueError):
        idx.search_codes_preassigned_device(form[0], form[1][:1], form[2], None, every, 1)
    with pytest.raises(ValueError):
        idx.search_codes_preassigned_device(*form, np.zeros((2, 3), np.float32), every, 1)
    idx.reset()
    D, I = check_scan(idx, form, None, every, codes[:0], ids[:0], np.zeros(NLIST + 1, np.int64), 3)     # an empty index
    assert (I == -1).all() and idx.ntotal == 0 and idx.is_trained
    idx.close()
    idx.close()                                                    # harmless


# -- lists: pack, unpack, encode -----------------------------------------------------------------------------------------------
def rows_for_lists(rng, sizes, d):
    """Coarse centroids (the first len(sizes) unit vectors) and rows that fall into list l sizes[l] times, shuffled."""
    cent = np.eye(len(sizes), d, dtype=np.float32)
    lists = rng.permutation(np.repeat(np.arange(len(sizes)), sizes))
    x = cent[lists] + np.float32(0.05) * rng.standard_normal((len(lists), d)).astype(np.float32)
    return cent, x.astype(np.float32), lists


@pytest.mark.parametrize("d, by_residual", [(16, True), (100, True), (100, False), (1024, True)])
def test_lists_after_add_hold_the_encoder_codes_of_the_residuals(d, by_residual):
    """The twelve lists, added in two calls: list_codes / list_ids are the rows of each list in the order they were added, their
    codes sq_encode_ref of the numpy float32 residual (of the row itself without by_residual), exactly, and the whole store is the
    numpy layout's round trip.  reset drops the rows and keeps the training."""
    from ivr_amd.ivfsq import ivfsq_pack_ref, ivfsq_unpack_ref
    from ivr_amd.sq import sq_encode_ref, sq_train_ref
    rng = np.random.default_rng(d)
    cent, x, lists = rows_for_lists(rng, SIZES, d)
    coded = x - cent[lists] if by_residual else x
    trained = sq_train_ref(coded[::2])                              # half of the rows: the others clamp here and there
    idx = make_index(d, NLIST, cent, trained, by_residual)
    assert np.array_equal(idx.assign(x), lists) and np.array_equal(idx.centroids, cent)
    assert (idx.code_size, idx.d, idx.nlist, idx.nprobe) == (d, d, NLIST, 1)
    cut = 500
    idx.add(x[:cut])
    assert idx.ntotal == cut and idx.list_sizes().tolist() == np.bincount(lists[:cut], minlength=NLIST).tolist()
    idx.add(x[cut:])
    assert idx.ntotal == NROWS and idx.list_sizes().tolist() == SIZES and idx.sq.ntotal == 0
    want = sq_encode_ref(coded, trained)
    assert np.array_equal(idx.sq.sa_encode(coded), want)
    allc, alli = [], []
    for l in range(NLIST):
        rows = np.flatnonzero(lists == l)                          # ascending: the order of adding, the first call's rows first
        assert np.array_equal(idx.list_ids(l), rows)
        got = idx.list_codes(l)
        assert got.shape == (SIZES[l], d) and got.dtype == np.uint8 and np.array_equal(got, want[rows])
        allc.append(want[rows])
        alli.append(rows)
    codes, ids = idx._rows_device()
    assert np.array_equal(codes.cpu().numpy(), ivfsq_unpack_ref(ivfsq_pack_ref(np.concatenate(allc), OFF), OFF, d))
    assert np.array_equal(ids.cpu().numpy(), np.concatenate(alli))
    with pytest.raises(ValueError):
        idx.list_codes(NLIST)
    with pytest.raises(RuntimeError):
        idx.sq.trained = trained                                   # rows are encoded with the current table
    with pytest.raises(RuntimeError):
        idx.by_residual = not by_residual
    idx.reset()
    assert idx.ntotal == 0 and idx.is_trained and idx.list_sizes().tolist() == [0] * NLIST
    assert np.array_equal(bits(idx.sq.trained), bits(trained))
    idx.add_with_ids(x[:70], np.arange(70) + 5)
    assert sorted(np.concatenate([idx.list_ids(l) for l in range(NLIST)]).tolist()) == list(range(5, 75))
    idx.close()


# -- training ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spherical, by_residual", [(True, True), (False, False)])
def test_training_is_the_coarse_training_then_the_table_of_the_residuals(spherical, by_residual):
    from ivr_amd.ivf import IVFFlatIndex
    from ivr_amd.ivfsq import IVFSQIndex
    from ivr_amd.sq import sq_train_ref
    n, d, nlist = 2048, 32, 8
    x = unit_rows(np.random.default_rng(77), n, d)
    idx = IVFSQIndex(d, nlist)
    idx.by_residual = by_residual
    with pytest.raises(RuntimeError):
        idx.add(x[:10])
    with pytest.raises(RuntimeError):
        idx.search(x[:2], 1)
    idx.train(x, niter=3, seed=99, max_points_per_centroid=128, spherical=spherical)
    assert idx.is_trained and idx.quantizer.ntotal == nlist
    flat = IVFFlatIndex(d, nlist)
    flat.train(x, niter=3, seed=99, max_points_per_centroid=128, spherical=spherical)
    cent = flat.centroids
    assert np.isfinite(cent).all() and np.array_equal(bits(idx.centroids), bits(cent))
    want = sq_train_ref(x - cent[idx.assign(x)] if by_residual else x)
    assert np.array_equal(bits(idx.sq.trained), bits(want))
    with pytest.raises(RuntimeError):
        idx.by_residual = not by_residual                          # trained on what is coded
    idx.add(x[:100])
    with pytest.raises(RuntimeError):
        idx.train(x)
    for i in (idx, flat):
        i.close()


def test_a_filled_quantizer_is_taken_as_it_is():
    from ivr_amd.sq import sq_train_ref
    rng = np.random.default_rng(78)
    d, nlist = 40, 5
    cent, x = unit_rows(rng, nlist, d), unit_rows(rng, 600, d)
    idx = make_index(d, nlist, cent)
    assert not idx.is_trained
    idx.train(x)
    assert idx.is_trained and np.array_equal(bits(idx.centroids), bits(cent))
    assert np.array_equal(bits(idx.sq.trained), bits(sq_train_ref(x - cent[idx.assign(x)])))
    idx.close()


# -- end to end ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rows():
    rng = np.random.default_rng(2025)
    return unit_rows(rng, NLIST, 48), unit_rows(rng, 1500, 48), unit_rows(rng, 9, 48)


def filled_index(cent, x, by_residual=True):
    idx = make_index(x.shape[1], len(cent), cent, by_residual=by_residual)
    idx.train(x)                                                   # the table only: the quantizer is filled
    return idx


def test_parameters_and_selectors(rows):
    from ivr_amd.index import IDSelectorRange, SearchParameters
    from ivr_amd.ivf import SearchParametersIVF
    cent, x, q = rows
    idx = filled_index(cent, x)
    assert (idx.nlist, idx.code_size, idx.nprobe, idx.by_residual, idx.ntotal) == (NLIST, 48, 1, True, 0)
    with pytest.raises(ValueError):
        idx.nprobe = 0
    idx.add(x)
    idx.nprobe = 3
    D3, I3 = idx.search(q, 10)
    idx.nprobe = 1
    D1, I1 = idx.search(q, 10)
    D, I = idx.search(q, 10, params=SearchParametersIVF(nprobe=3))  # overrides the attribute for this call
    assert np.array_equal(I, I3) and np.array_equal(bits(D), bits(D3)) and not np.array_equal(I1, I3)
    Dt, It = idx.search_device(torch.from_numpy(q).cuda(), 10, nprobe=3)
    assert np.array_equal(It.cpu().numpy(), I3) and np.array_equal(bits(Dt.cpu().numpy()), bits(D3))
    with pytest.raises(ValueError, match="not supported on IVFSQIndex"):
        idx.search(q, 10, params=SearchParametersIVF(nprobe=2, sel=IDSelectorRange(0, 5)))
    with pytest.raises(ValueError):
        idx.search(q, 10, params=SearchParameters())
    with pytest.raises(ValueError):
        idx.search(q, 0)
    with pytest.raises(ValueError):
        idx.add_with_ids(x[:2], np.array([3, -1]))
    idx.close()


def test_search_is_search_preassigned_with_the_quantizers_own_lists(rows):
    from ivr_amd.ivf import SearchParametersIVF
    from ivr_amd.ivfsq import ivfsq_scan_ref
    from ivr_amd.sq import sq_query_ref
    cent, x, q = rows
    idx = filled_index(cent, x)
    idx.add(x[:800])
    idx.add(x[800:])
    off = np.concatenate([[0], np.cumsum(idx.list_sizes())])
    codes, ids = (t.cpu().numpy() for t in idx._rows_device())
    t, scale, bias = (a.cpu().numpy() for a in idx.compute_query_codes_device(q))
    tr, sr, _ = sq_query_ref(q, idx.sq.trained)
    assert np.array_equal(t, tr) and np.array_equal(bits(scale), bits(sr))
    for nprobe in (1, 3):
        Dc, Ic = idx.quantizer.search(q, nprobe)
        D, I = idx.search(q, 10, params=SearchParametersIVF(nprobe=nprobe))
        for coarse_dis in (Dc, None):                              # omitted: the same bits, computed for exactly the named lists
            Dp, Ip = idx.search_preassigned(q, 10, Ic, coarse_dis)
            assert np.array_equal(I, Ip) and np.array_equal(bits(D), bits(Dp))
        Dr, Ir = ivfsq_scan_ref(t, scale, bias, Dc, Ic, off, codes, ids, 10)
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


def test_without_residuals_every_list_gives_the_scores_of_the_sq_index(rows):
    """by_residual = False, the same table and nprobe = nlist: D equals SQIndex.search's D as float32 values for every query (D is a
    monotone function of acc, so the top-k multisets agree whatever the tie order; I is pinned by the scan tests)."""
    from ivr_amd.sq import IndexScalarQuantizer
    cent, x, q = rows
    idx = filled_index(cent, x, by_residual=False)
    idx.add(x)
    sq = IndexScalarQuantizer(48)
    sq.trained = idx.sq.trained
    sq.add(x)
    idx.nprobe = NLIST
    for k in (1, 25, 300):
        D, I = idx.search(q, k)
        Ds, _ = sq.search(q, k)
        assert np.array_equal(D, Ds)
        assert I.min() >= 0 and all(len(set(row.tolist())) == k for row in I)
    idx.close()
    sq.close()


def test_scores_lie_within_the_stated_bound_of_the_float64_score(rows):
    """Trained rows with by_residual: every returned D against <q, c_l + decode(code)> in float64, decode from the float32 vmin and
    vdiff.  Each figure is printed before it is asserted."""
    from ivr_amd.ivfsq import ivfsq_score_bound
    from ivr_amd.sq import sq_encode_ref
    cent, x, q = rows
    idx = filled_index(cent, x)
    idx.add(x)                                                      # label = row of x
    lists = idx.assign(x)
    trained = idx.sq.trained
    codes = sq_encode_ref(x - cent[lists], trained)
    d = x.shape[1]
    vmin, vdiff = trained[:d].astype(np.float64), trained[d:].astype(np.float64)
    dec = vmin + vdiff * ((codes.astype(np.float64) + 0.5) / 255.0)
    truth = q.astype(np.float64) @ (cent[lists].astype(np.float64) + dec).T
    scale = idx.compute_query_codes_device(q)[1].cpu().numpy()
    for nprobe in (2, NLIST):
        D, I = idx.search_device(q, 50, nprobe=nprobe)
        D, I = D.cpu().numpy(), I.cpu().numpy()
        assert I.min() >= 0
        full = np.zeros(truth.shape, np.float32)
        np.put_along_axis(full, I, D, axis=1)
        bound = np.take_along_axis(ivfsq_score_bound(q, codes, trained, scale, cent[lists], full), I, axis=1)
        err = np.abs(D.astype(np.float64) - np.take_along_axis(truth, I, axis=1))
        print(f"nprobe {nprobe}: largest error {err.max():.3e}, smallest bound {bound.min():.3e}, largest error / bound {(err / bound).max():.3f}")
        assert (err <= bound).all()
    idx.close()


def test_reconstruction(rows):
    from ivr_amd.sq import sq_decode_ref, sq_encode_ref
    cent, x, _ = rows
    for by_residual in (True, False):
        idx = filled_index(cent, x, by_residual=by_residual)
        labels = np.arange(300, dtype=np.int64) * 3 + 7
        labels[10] = labels[200]                                   # a duplicate label: the lowest stored position answers
        idx.add_with_ids(x[:300], labels)
        lists = idx.assign(x[:300])
        codes = sq_encode_ref(x[:300] - cent[lists] if by_residual else x[:300], idx.sq.trained)
        dec = sq_decode_ref(codes, idx.sq.trained)
        want = cent[lists] + dec if by_residual else dec
        ask = np.array([labels[299], labels[0], labels[57], labels[0]])
        got = idx.reconstruct_batch(ask)
        assert got.dtype == np.float32 and np.array_equal(bits(got), bits(want[[299, 0, 57, 0]]))
        assert np.array_equal(bits(idx.reconstruct(int(labels[57]))), bits(want[57]))
        first = 10 if lists[10] <= lists[200] else 200             # the lower list, or the earlier one inside a list, is stored first
        assert np.array_equal(bits(idx.reconstruct(int(labels[200]))), bits(want[first]))
        for call in (lambda: idx.reconstruct(8), lambda: idx.reconstruct_batch([7, 8])):
            with pytest.raises(RuntimeError, match="not in the index"):
                call()
        assert idx.reconstruct_batch(np.zeros(0, np.int64)).shape == (0, 48)
        idx.close()


# -- refine --------------------------------------------------------------------------------------------------------------------
def test_refine_over_an_ivfsq_base_with_every_row_a_candidate():
    from ivr_amd.index import FlatIPIndex
    from ivr_amd.ivf import SearchParametersIVF
    from ivr_amd.refine import IndexRefineFlat, IndexRefineSearchParameters
    rng = np.random.default_rng(14)
    x, q = unit_rows(rng, 500, 32), unit_rows(rng, 7, 32)
    r = IndexRefineFlat(make_index(32, NLIST, unit_rows(rng, NLIST, 32)))
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
    with pytest.raises(ValueError):
        r.search(q, 10, params=IndexRefineSearchParameters(base_index_params=object()))
    r.close()
    r.base_index.close()
    flat.close()
