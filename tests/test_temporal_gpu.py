"""GPU suite of the clip search (ivr_amd/temporal.py, csrc/search_seq.hip, csrc/search_range_keys.h): both calls against the numpy
definitions (sequence_search_ref / sequence_range_ref) fed with the frame scores FlatIPIndex.rescore_device reports, element for
element and with the scores compared as bit patterns; then TemporalAnalyzer.find_similar_sequences against the float64 restatement
of the reference's loops."""
import numpy as np
import pytest
import torch

from ivr_amd import temporal
from ivr_amd.index import FlatIPIndex
from temporal_cases import MARGIN, reference_find

pytestmark = pytest.mark.gpu

LENGTHS = (1, 2, 5, 16, 17, 64)
KS = (1, 10, 2048)            # 2048 is more than any stretch here holds: padding
NFRAMES = 65                  # the longest T below: L + 1 for L = 64


def frame_scores(index, q, normalize=False):
    """S float32 [T,N]: the score of every (frame, stored row) from rescore_device, in column blocks of at most 2048 rows."""
    T, N = len(q), index.ntotal
    qd = torch.from_numpy(q).to(index.device)
    S = np.empty((T, N), np.float32)
    for c0 in range(0, N, 2048):
        c1 = min(N, c0 + 2048)
        cand = torch.arange(c0, c1, dtype=torch.int64, device=index.device).repeat(T, 1).contiguous()
        S[:, c0:c1] = index.rescore_device(qd, cand, normalize=normalize)[0].cpu().numpy()
    return S


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def check_topk(index, q, S, L, k, seg=None, ids=None, normalize=False):
    D, I = temporal.sequence_search(index, q, L, k, seg_off=seg, normalize=normalize)
    Dr, Ir = temporal.sequence_search_ref(S, L, k, seg, ids)
    assert D.dtype == np.float32 and I.dtype == np.int64 and D.shape == Dr.shape
    assert np.array_equal(I, Ir), f"top-k labels differ (L={L}, k={k})"
    assert np.array_equal(bits(D), bits(Dr)), f"top-k score bits differ (L={L}, k={k})"


def check_range(index, q, S, L, threshold, seg=None, ids=None, normalize=False):
    lims, D, I = temporal.sequence_range_search(index, q, L, threshold, seg_off=seg, normalize=normalize)
    lr, Dr, Ir = temporal.sequence_range_ref(S, L, threshold, seg.cpu().numpy() if isinstance(seg, torch.Tensor) else seg, ids)
    assert lims.dtype == np.int64 and np.array_equal(lims, lr), f"lims differ (L={L})"
    assert np.array_equal(I, Ir), f"range labels differ (L={L})"
    assert np.array_equal(bits(D), bits(Dr)), f"range score bits differ (L={L})"
    return lims


def make(d, N, seed, nframes=NFRAMES, period=None):
    rng = np.random.default_rng([seed, d, N])
    X = rng.standard_normal((N, d)).astype(np.float32)
    if period:
        X = X[np.arange(N) % period].copy()           # duplicate rows: equal window scores, ranked by start row
    q = rng.standard_normal((nframes, d)).astype(np.float32)
    index = FlatIPIndex(d)
    index.add(X)
    return index, X, q


def median_threshold(S, L):
    W, _ = temporal.sequence_scores_ref(S, L)
    return float(np.median(W)) if W.size else 0.0


@pytest.mark.parametrize("N", [4, 15, 16, 17, 63, 64, 65, 255, 256, 257, 700])
@pytest.mark.parametrize("d", [20, 512])
def test_every_shape_matches_the_definition(d, N):
    index, X, q = make(d, N, 1)
    S_all = frame_scores(index, q)
    for L in LENGTHS:
        for T in sorted({L, L + 1} | {t for t in (16, 17, 40) if t >= L}):
            S = S_all[:T]
            for k in KS:
                check_topk(index, q[:T], S, L, k)
            lims = check_range(index, q[:T], S, L, median_threshold(S, L))      # an attained score when the count is odd
            if N >= L:
                assert 0 < lims[-1] <= (T - L + 1) * (N - L + 1)
            else:
                assert not lims.any()                                              # fewer rows than L: no candidate at all


@pytest.mark.parametrize("L", [1, 2, 5])
def test_segments(L):
    # boundaries at 15 / 16 / 17 and 64 / 65, an empty segment [17, 17), segments shorter than 5 ([15, 16), [16, 17), [17, 19)), row 0
    # in front of the first offset and rows 90 .. 99 past the last
    seg = np.array([1, 15, 16, 17, 17, 19, 64, 65, 90], np.int64)
    index, X, q = make(20, 100, 2, nframes=17)
    S = frame_scores(index, q)
    for k in (1, 10, 2048):
        check_topk(index, q, S, L, k, seg)
    lims = check_range(index, q, S, L, -np.inf, seg)
    _, ok = temporal.sequence_scores_ref(S, L, seg)
    assert lims[-1] == (17 - L + 1) * ok.sum() and 0 < ok.sum() < len(ok)
    check_range(index, q, S, L, median_threshold(S, L), torch.from_numpy(seg).to(index.device))      # offsets already on the device
    # one segment over everything is the call without segments
    D0, I0 = temporal.sequence_search(index, q, L, 10)
    D1, I1 = temporal.sequence_search(index, q, L, 10, seg_off=np.array([0, 100]))
    assert np.array_equal(I0, I1) and np.array_equal(bits(D0), bits(D1))


def test_id_mapped_index_reports_stored_ids():
    rng = np.random.default_rng(3)
    X = rng.standard_normal((257, 20)).astype(np.float32)
    q = rng.standard_normal((17, 20)).astype(np.float32)
    ids = rng.permutation(257).astype(np.int64) + 1000
    index = FlatIPIndex(20)
    index.add_with_ids(X, ids)
    S = frame_scores(index, q)
    for L in (1, 5):
        check_topk(index, q, S, L, 10, ids=ids)
        check_topk(index, q, S, L, 2048, ids=ids)
        check_range(index, q, S, L, median_threshold(S, L), ids=ids)


def test_equal_scores_rank_the_lower_start_row():
    index, X, q = make(20, 257, 4, nframes=17, period=7)
    S = frame_scores(index, q)
    for L in (1, 5):
        W, _ = temporal.sequence_scores_ref(S, L)
        assert np.array_equal(bits(W[:, 0]), bits(W[:, 7]))        # the duplicates do tie, to the bit
        for k in (1, 10, 2048):
            check_topk(index, q, S, L, k)
        D, I = temporal.sequence_search(index, q, L, 10)
        tied = bits(D[:, :-1]) == bits(D[:, 1:])
        assert tied.any() and (I[:, :-1][tied] < I[:, 1:][tied]).all()


def test_threshold_on_an_attained_score_keeps_it():
    index, X, q = make(20, 65, 5, nframes=17)
    S = frame_scores(index, q, normalize=True)
    for L in (2, 5):
        W, _ = temporal.sequence_scores_ref(S, L)
        thr = float(np.sort(W.reshape(-1))[-5])                    # the fifth best window score overall
        lims = check_range(index, q, S, L, thr, normalize=True)
        assert lims[-1] == (W >= np.float32(thr)).sum() >= 5
        lims, D, I = temporal.sequence_range_search(index, q, L, thr, normalize=True)
        assert (bits(D) == bits(np.float32(thr))).any()              # >= keeps the score that equals the threshold
        up = float(np.nextafter(np.float32(thr), np.float32(np.inf)))
        assert temporal.sequence_range_search(index, q, L, up, normalize=True)[0][-1] < lims[-1]
    with pytest.raises(ValueError, match="NaN"):
        index._call("ivr_index_range_search_sequences", torch.from_numpy(q).to(index.device), 17, 2, None, 0, float("nan"), False,
                    torch.zeros(17, dtype=torch.int64, device=index.device), torch.zeros(1, device=index.device),
                    torch.zeros(1, dtype=torch.int64, device=index.device), 0)


def test_cap_below_the_total_counts_everything_and_writes_no_further():
    index, X, q = make(20, 700, 6, nframes=17)
    L = 5
    S = frame_scores(index, q)
    thr = median_threshold(S, L)
    lr, Dr, Ir = temporal.sequence_range_ref(S, L, thr)
    total = int(lr[-1])
    cap = total // 3
    assert cap > 0
    dev = index.device
    lims = torch.empty(17 - L + 2, dtype=torch.int64, device=dev)
    D = torch.full((total,), -7.0, dtype=torch.float32, device=dev)
    I = torch.full((total,), -7, dtype=torch.int64, device=dev)
    index._call("ivr_index_range_search_sequences", torch.from_numpy(q).to(dev), 17, L, None, 0, thr, False, lims, D, I, cap)
    assert np.array_equal(lims.cpu().numpy(), lr)
    assert np.array_equal(I[:cap].cpu().numpy(), Ir[:cap]) and np.array_equal(bits(D[:cap].cpu().numpy()), bits(Dr[:cap]))
    assert (I[cap:] == -7).all() and (D[cap:] == -7.0).all()
    ld, Dd, Id, tot = temporal.sequence_range_search_device(index, q, L, thr, cap=cap)
    assert int(tot.item()) == total and len(Dd) == cap and np.array_equal(Id.cpu().numpy(), Ir[:cap])


@pytest.mark.parametrize("N,T,slots_windows", [(700, 44, 7), (20000, 12, 3)])
def test_chunked_call_has_the_bits_of_the_unchunked_one(monkeypatch, N, T, slots_windows):
    # 700 rows: 40 windows in chunks of 7 (the last holds 5); 20000 rows: stretches of several 4096-key blocks, a select that re-reads
    # its keys, score workgroups side by side, 8 windows in chunks of 3
    L = 5
    whole, X, q = make(20, N, 7, nframes=T)
    monkeypatch.setenv("IVR_SEQ_CHUNK_SLOTS", str((N - L + 1) * slots_windows + 100))
    chunked = FlatIPIndex(20)                                       # the variable is read when the index is created
    chunked.add(X)
    monkeypatch.delenv("IVR_SEQ_CHUNK_SLOTS")
    assert (T - L + 1) % slots_windows != 0
    S = frame_scores(whole, q)
    thr = median_threshold(S, L)
    seg = np.array([3, N // 2, N - 2], np.int64)
    for index in (whole, chunked):
        check_topk(index, q, S, L, 10)
        check_topk(index, q, S, L, 10, seg)
        check_range(index, q, S, L, thr)
        check_range(index, q, S, L, thr, seg)
    a = temporal.sequence_range_search(whole, q, L, thr)
    b = temporal.sequence_range_search(chunked, q, L, thr)
    assert all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(a, b))


def test_find_similar_sequences_matches_the_reference():
    """The reference's (start, order) list, and every score within (d + L + 8) * 2^-24 of the float64 one: the standard bound of a
    length-d float32 dot product of unit rows plus L additions and a division.  Measured on an MI355X: 18 results, largest
    |score - float64 score| 6.1e-08 against the bound 2.0e-06 (the test prints both)."""
    d, L, threshold = 20, 5, 0.8
    rng = np.random.default_rng(17)
    target = rng.standard_normal((30, d))
    database = rng.standard_normal((30, d))
    database[4:24] = target[7:27] + 0.12 * rng.standard_normal((20, d))          # a noisy copy of twenty target frames
    unit = lambda x: (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)      # noqa: E731
    target, database = unit(target), unit(database)
    means = []
    want = reference_find(target.astype(np.float64), database.astype(np.float64), L, threshold, means)
    assert all(abs(v - threshold) > MARGIN for v in means), "seed puts a window mean within 1e-4 of the threshold"
    kept = sorted(v for _, v in want)
    assert all(b - a > 1e-5 for a, b in zip(kept, kept[1:])), "seed puts two kept window means within 1e-5 of each other"
    assert 0 < len(want) < len(means)
    got = temporal.TemporalAnalyzer().find_similar_sequences(target, database, L, threshold)
    assert all(isinstance(s, int) and isinstance(w, float) for s, w in got)
    worst = max(abs(a - b) for (_, a), (_, b) in zip(got, want)) if len(got) == len(want) else float("nan")
    bound = (d + L + 8) * 2.0 ** -24
    print(f"find_similar_sequences: {len(got)} results, largest |score - float64| = {worst:.3e}, bound {bound:.3e}")
    assert [s for s, _ in got] == [s for s, _ in want]
    assert worst <= bound
    assert temporal.TemporalAnalyzer().find_similar_sequences(target[:4], database, L, threshold) == []
