"""GPU suite of the event search (ivr_amd/temporal.py, csrc/search_events.hip): both calls against the numpy definitions
(event_search_ref / event_best_per_segment_ref) fed with the frame scores FlatIPIndex.rescore_device reports.  Every comparison is
exact: the paths element for element, the scores as bit patterns.  R below is the row tile of the step kernel (kEvRows)."""
import numpy as np
import pytest
import torch

from event_cases import SEGMENTS_100, make_chains, make_rows
from ivr_amd import temporal
from ivr_amd.index import FlatIPIndex

pytestmark = pytest.mark.gpu

R = 1024
FLT_MAX = np.finfo(np.float32).max
GAPS = [(1, 1), (2, 1), (2, 2), (63, 1), (63, 30), (63, 63), (64, 1), (64, 33), (64, 64), (65, 1), (65, 2), (65, 65),
        (R - 1, 1), (R - 1, 500), (R - 1, R - 1), (R, 1), (R, 7), (R, R), (R + 1, 1), (R + 1, R), (R + 1, R + 1),
        (4096, 1), (4096, 2000), (4096, 4096)]                 # (max_gap, min_gap)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def frame_scores(index, x, normalize=False):
    """S float32 [B,m,N]: the score of every (event, stored row) from rescore_device, in column blocks of at most 2048 rows."""
    B, m, d = x.shape
    N = index.ntotal
    qd = torch.from_numpy(x.reshape(B * m, d)).to(index.device)
    S = np.empty((B * m, N), np.float32)
    for c0 in range(0, N, 2048):
        c1 = min(N, c0 + 2048)
        cand = torch.arange(c0, c1, dtype=torch.int64, device=index.device).repeat(B * m, 1).contiguous()
        S[:, c0:c1] = index.rescore_device(qd, cand, normalize=normalize)[0].cpu().numpy()
    return S.reshape(B, m, N)


def host(seg):
    return seg.cpu().numpy() if isinstance(seg, torch.Tensor) else seg


def check_topk(index, x, S, k, max_gap, min_gap=1, seg=None, ids=None):
    D, I = temporal.event_search(index, x, k, max_gap, min_gap, seg_off=seg)
    Dr, Ir = temporal.event_search_ref(S, k, min_gap, max_gap, host(seg), ids)
    assert D.dtype == np.float32 and I.dtype == np.int64 and D.shape == Dr.shape and I.shape == Ir.shape
    what = f"(k={k}, gaps {min_gap}..{max_gap}, m={x.shape[1]})"
    assert np.array_equal(I, Ir), f"top-k paths differ {what}"
    assert np.array_equal(bits(D), bits(Dr)), f"top-k score bits differ {what}"
    return D, I


def check_best(index, x, S, max_gap, min_gap=1, seg=None, ids=None):
    D, I = temporal.event_best_per_segment(index, x, max_gap, min_gap, seg_off=seg)
    Dr, Ir = temporal.event_best_per_segment_ref(S, min_gap, max_gap, host(seg), ids)
    assert D.dtype == np.float32 and I.dtype == np.int64 and D.shape == Dr.shape and I.shape == Ir.shape
    what = f"(gaps {min_gap}..{max_gap}, m={x.shape[1]})"
    assert np.array_equal(I, Ir), f"best-per-segment paths differ {what}"
    assert np.array_equal(bits(D), bits(Dr)), f"best-per-segment score bits differ {what}"
    return D, I


def make(d, N, seed, B, m, period=None):
    X = make_rows(d, N, seed, period)
    index = FlatIPIndex(d)
    index.add(X)
    x = make_chains(d, B, m, seed)
    return index, X, x


@pytest.mark.parametrize("N", [1, 2, 15, 16, 17, 63, 64, 65, R - 1, R, R + 1, 2 * R + 3])
def test_every_size_and_gap_matches_the_definition(N):
    index, X, x = make(20, N, 1, 1, 3)
    S = frame_scores(index, x)
    found = 0
    for max_gap, min_gap in GAPS:
        D, I = check_topk(index, x, S, 10, max_gap, min_gap)
        found += int((I[:, :, 0] >= 0).sum())
        if N <= 2 * min_gap:                                       # three events span 2 min_gap + 1 rows at least
            assert (I == -1).all() and (D == -FLT_MAX).all()
        check_best(index, x, S, max_gap, min_gap)
    assert (found > 0) == (N >= 3)
    two = x[:, :2].copy()
    for max_gap, min_gap in GAPS[::3]:
        check_topk(index, two, S[:, :2], 2048, max_gap, min_gap)       # more slots than end rows at every size but the largest: padding


@pytest.mark.parametrize("d", [20, 512])
def test_chain_counts_lengths_and_k(d):
    index, X, x = make(d, R + 1, 2, 17, 8)
    S = frame_scores(index, x)
    # (m, B, k, max_gap, min_gap): every m, B and k of the grid at least twice
    for m, B, k, max_gap, min_gap in [(1, 3, 10, 64, 1), (1, 17, 2048, 5, 5), (2, 17, 1, 64, 1), (2, 1, 2048, R, 3), (3, 17, 10, 65, 2),
                                      (3, 3, 1, 4096, 1), (8, 3, 2048, 64, 1), (8, 1, 10, 200, 100), (8, 3, 1, 4096, 146)]:
        xs = x[:B, :m].copy()
        D, I = check_topk(index, xs, S[:B, :m], k, max_gap, min_gap)
        assert (I[:, 0] >= 0).all()
        check_best(index, xs, S[:B, :m], max_gap, min_gap)
    # 8 events at least 147 rows apart do not fit 1025 rows
    D, I = check_topk(index, x[:1].copy(), S[:1], 10, 4096, 147)
    assert (I == -1).all()


def test_segments():
    index, X, x = make(20, 100, 3, 3, 3)
    S = frame_scores(index, x)
    seg_dev = torch.from_numpy(SEGMENTS_100).to(index.device)
    with_chain = without = 0
    for m in (1, 2, 3):
        xs = x[:, :m].copy()
        for max_gap, min_gap in [(1, 1), (5, 1), (30, 2), (4096, 1)]:
            for k in (1, 10, 2048):
                check_topk(index, xs, S[:, :m], k, max_gap, min_gap, SEGMENTS_100)
            check_topk(index, xs, S[:, :m], 10, max_gap, min_gap, seg_dev)          # offsets already on the device
            D, I = check_best(index, xs, S[:, :m], max_gap, min_gap, SEGMENTS_100)
            Dd, Id = check_best(index, xs, S[:, :m], max_gap, min_gap, seg_dev)
            assert np.array_equal(I, Id) and np.array_equal(bits(D), bits(Dd))
            assert D.shape == (3, 8)
            with_chain += int((I[:, :, 0] >= 0).sum())
            without += int((I[:, :, 0] < 0).sum())
            if m == 3:
                assert (I[:, [1, 2, 3], 0] == -1).all() and (D[:, [1, 2, 3]] == -FLT_MAX).all()     # one row, one row, no row
    assert with_chain > 0 and without > 0
    # one segment over everything is the call without segments
    D0, I0 = temporal.event_search(index, x, 10, 5)
    D1, I1 = temporal.event_search(index, x, 10, 5, seg_off=np.array([0, 100]))
    assert np.array_equal(I0, I1) and np.array_equal(bits(D0), bits(D1))
    D0, I0 = temporal.event_best_per_segment(index, x, 5)
    D1, I1 = temporal.event_best_per_segment(index, x, 5, seg_off=np.array([0, 100]))
    assert D0.shape == (3, 1) and np.array_equal(I0, I1) and np.array_equal(bits(D0), bits(D1))


def test_segments_across_row_tiles():
    # segment boundaries on both sides of the tile boundary at R and windows that reach across it
    seg = np.array([3, 500, R - 1, R, R + 2, 1900, 2 * R + 1], np.int64)
    index, X, x = make(20, 2 * R + 3, 4, 3, 3)
    S = frame_scores(index, x)
    for max_gap, min_gap in [(2, 1), (64, 1), (700, 5), (R, R), (4096, 1)]:
        check_topk(index, x, S, 10, max_gap, min_gap, seg)
        check_best(index, x, S, max_gap, min_gap, seg)


def test_equal_scores_rank_the_lower_row():
    index, X, x = make(20, 257, 5, 3, 3, period=7)
    S = frame_scores(index, x)
    assert np.array_equal(bits(S[:, :, 0]), bits(S[:, :, 7]))        # the duplicates do tie, to the bit
    for max_gap, min_gap in [(20, 1), (7, 7), (64, 3)]:
        for k in (1, 10, 2048):
            check_topk(index, x, S, k, max_gap, min_gap)
        check_best(index, x, S, max_gap, min_gap)
        D, I = temporal.event_search(index, x, 10, max_gap, min_gap)
        tied = bits(D[:, :-1]) == bits(D[:, 1:])
        assert tied.any() and (I[:, :-1, 2][tied] < I[:, 1:, 2][tied]).all()
        # equal predecessors: with windows longer than the period the best predecessor score occurs more than once in a window
        if max_gap - min_gap >= 7:
            C, P, ok = temporal.event_scores_ref(S[0], min_gap, max_gap)
            r = 200
            win = np.arange(r - max_gap, r - min_gap + 1)
            assert (bits(C[0, win]) == bits(C[0, P[1, r]])).sum() > 1 and P[1, r] == win[bits(C[0, win]) == bits(C[0, P[1, r]])][0]


def test_id_mapped_index_reports_stored_ids_along_the_path():
    rng = np.random.default_rng(6)
    X = make_rows(20, 257, 6)
    ids = rng.permutation(257).astype(np.int64) + 1000
    index = FlatIPIndex(20)
    index.add_with_ids(X, ids)
    x = make_chains(20, 3, 3, 6)
    S = frame_scores(index, x)
    for k in (10, 2048):
        D, I = check_topk(index, x, S, k, 30, 2, ids=ids)
    assert (I[:, :10] >= 1000).all()
    check_best(index, x, S, 30, 2, np.array([0, 100, 101, 257]), ids=ids)


def test_one_event_is_the_flat_search():
    index, X, x = make(20, R + 1, 7, 17, 1)
    D, I = temporal.event_search(index, x, 10, 64)
    Ds, Is = index.search(x[:, 0].copy(), 10)
    assert np.array_equal(I[:, :, 0], Is) and np.array_equal(bits(D), bits(np.asarray(Ds, np.float32)))


def test_adjacent_rows_are_the_clip_search_window():
    index, X, x = make(20, 300, 8, 3, 5)
    S = frame_scores(index, x)
    D, I = temporal.event_search(index, x, 2048, 1, 1)
    for b in range(3):
        W, ok = temporal.sequence_scores_ref(S[b], 5)
        W = W[0] + np.float32(0.0)                                  # window 0 of the chain's five frames against every start
        order = np.lexsort((np.arange(len(W)), -W.astype(np.float64)))
        assert len(W) == 296 and (I[b, 296:] == -1).all()
        assert np.array_equal(I[b, :296], order[:, None] + np.arange(5)[None, :])
        assert np.array_equal(bits(D[b, :296]), bits(W[order]))


def test_chunked_call_has_the_bits_of_the_unchunked_one(monkeypatch):
    # 17 chains of 3 events in chunks of 5 (the last holds 2): chunks start at frames 15, 30, 45, inside a 16-frame tile
    N, B, m = 700, 17, 3
    whole, X, x = make(20, N, 9, B, m)
    monkeypatch.setenv("IVR_SEQ_CHUNK_SLOTS", str(N * 5 + 100))
    chunked = FlatIPIndex(20)                                       # the variable is read when the index is created
    chunked.add(X)
    monkeypatch.delenv("IVR_SEQ_CHUNK_SLOTS")
    S = frame_scores(whole, x)
    seg = np.array([3, N // 2, N - 2], np.int64)
    out = []
    for index in (whole, chunked):
        out.append(check_topk(index, x, S, 10, 64, 2) + check_topk(index, x, S, 10, 64, 2, seg)
                   + check_best(index, x, S, 64, 2) + check_best(index, x, S, 64, 2, seg))
    assert all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(*out))


def test_empty_index():
    index = FlatIPIndex(20)
    x = make_chains(20, 3, 3, 10)
    D, I = temporal.event_search(index, x, 10, 5)
    assert D.shape == (3, 10) and I.shape == (3, 10, 3) and (D == -FLT_MAX).all() and (I == -1).all()
    D, I = temporal.event_best_per_segment(index, x, 5, seg_off=np.array([0, 4, 9]))
    assert D.shape == (3, 2) and I.shape == (3, 2, 3) and (D == -FLT_MAX).all() and (I == -1).all()
    D, I = temporal.event_best_per_segment(index, x, 5)
    assert D.shape == (3, 1) and (D == -FLT_MAX).all() and (I == -1).all()


def test_side_stream_and_repeat_calls_agree():
    index, X, x = make(20, 700, 11, 3, 3)
    xd = torch.from_numpy(x).to(index.device)
    seg = torch.tensor([0, 300, 700], dtype=torch.int64, device=index.device)
    first = [t.clone() for t in temporal.event_search_device(index, xd, 10, 64, 1, seg)]
    again = temporal.event_search_device(index, xd, 10, 64, 1, seg)
    side = torch.cuda.Stream(device=index.device)
    side.wait_stream(torch.cuda.current_stream(index.device))
    with torch.cuda.stream(side):
        other = temporal.event_search_device(index, xd, 10, 64, 1, seg)
        best = temporal.event_best_per_segment_device(index, xd, 64, 1, seg)
    side.synchronize()
    for a, b, c in zip(first, again, other):
        assert torch.equal(a, b) and torch.equal(a, c)
    S = frame_scores(index, x)
    Dr, Ir = temporal.event_best_per_segment_ref(S, 1, 64, seg.cpu().numpy())
    assert np.array_equal(best[1].cpu().numpy(), Ir) and np.array_equal(bits(best[0].cpu().numpy()), bits(Dr))


def test_library_rejects_arguments_outside_the_ranges():
    index, X, x = make(20, 50, 12, 2, 3)
    dev = index.device
    q = torch.from_numpy(x.reshape(6, 20)).to(dev)
    D = torch.zeros((2, 4), dtype=torch.float32, device=dev)
    I = torch.zeros((2, 4, 3), dtype=torch.int64, device=dev)
    seg = torch.tensor([0, 50], dtype=torch.int64, device=dev)

    def top(B=2, m=3, min_gap=1, max_gap=4, seg=None, nseg=0, k=4, q=q, D=D, I=I):
        index._call("ivr_index_search_events", q, B, m, min_gap, max_gap, seg, nseg, k, False, D, I)

    def best(B=2, m=3, min_gap=1, max_gap=4, seg=None, nseg=0, q=q, D=D, I=I):
        index._call("ivr_index_best_events_per_segment", q, B, m, min_gap, max_gap, seg, nseg, False, D, I)

    for call in (top, best):
        call()                                                     # the arguments in range pass
        for bad, text in [(dict(m=0), "m=0"), (dict(m=9), "m=9"), (dict(B=0), "B=0"), (dict(min_gap=0), "gaps"),
                          (dict(min_gap=5), "gaps"), (dict(max_gap=4097), "gaps"), (dict(seg=seg, nseg=0), "nseg=0"),
                          (dict(q=None), "NULL"), (dict(D=None), "NULL"), (dict(I=None), "NULL")]:
            with pytest.raises(ValueError, match=text):
                call(**bad)
    for k in (0, 2049):
        with pytest.raises(ValueError, match=f"k={k}"):
            top(k=k)
    with pytest.raises(ValueError, match="k=0"):
        temporal.event_search(index, x, 0, 4)
    with pytest.raises(ValueError, match="gaps"):
        temporal.event_best_per_segment(index, x, 4097)


def test_find_event_sequences_finds_the_planted_chain():
    rng = np.random.default_rng(13)
    d = 64
    events = rng.standard_normal((3, d)).astype(np.float32)
    database = rng.standard_normal((400, d)).astype(np.float32)
    planted = (120, 131, 170)
    for j, r in enumerate(planted):
        database[r] = events[j] + 0.1 * rng.standard_normal(d).astype(np.float32)
    got = temporal.TemporalAnalyzer().find_event_sequences(events, database, max_gap=50, min_gap=2, k=10)
    assert len(got) == 10 and all(isinstance(p, tuple) and len(p) == 3 and isinstance(w, float) for p, w in got)
    assert got[0][0] == planted and got[0][1] > 0.9 and all(a[1] >= b[1] for a, b in zip(got, got[1:]))
    assert all(2 <= b - a <= 50 for p, _ in got for a, b in zip(p, p[1:]))
    # a gap bound the planted chain does not meet: it is not reported
    assert all(p != planted for p, _ in temporal.TemporalAnalyzer().find_event_sequences(events, database, max_gap=30, k=10))
