"""CPU suite of the event search (ivr_amd/temporal.py): the numpy definition (event_scores_ref and the two result forms) against a full
enumeration of the admissible chains, the tie rules, and the argument checks that need no device.  No compute call reaches a device
and the library is not loaded."""
import numpy as np
import pytest
import torch

from event_cases import SEGMENTS_SMALL, admissible, chain_sum, enumerate_chains, ordered, small_cases
from ivr_amd import _ffi, temporal
from ivr_amd.index import FlatIPIndex

FLT_MAX = np.finfo(np.float32).max


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def paths_of(P, ends):
    m = P.shape[0]
    out = []
    for r in ends:
        path = [int(r)]
        for j in range(m - 1, 0, -1):
            path.append(int(P[j, path[-1]]))
        out.append(path[::-1])
    return out


def test_definition_equals_the_enumeration_of_every_admissible_chain():
    ties = with_segments = absent = 0
    for S, min_gap, max_gap, seg in small_cases():
        m, N = S.shape
        C, P, ok = temporal.event_scores_ref(S, min_gap, max_gap, seg)
        best, any_chain = enumerate_chains(S, min_gap, max_gap, seg)
        assert np.array_equal(ok[m - 1], any_chain)
        assert np.array_equal(bits(C[m - 1][any_chain]), bits(best[any_chain]))
        ends = np.flatnonzero(any_chain)
        for r, path in zip(ends, paths_of(P, ends)):
            assert path[-1] == r and admissible(path, N, seg, min_gap, max_gap)
            assert bits(chain_sum(S, path)) == bits(C[m - 1, r])
            for j in range(1, m):                                   # every prefix of a reported path is the reported best of its own end
                assert ok[j - 1, path[j - 1]] and bits(chain_sum(S, path[:j])) == bits(C[j - 1, path[j - 1]])
        for j in range(1, m):                                       # equal predecessors inside a window do occur
            for r in np.flatnonzero(ok[j]):
                a, b = max(r - max_gap, 0), r - min_gap
                win = [p for p in range(a, b + 1) if ok[j - 1, p] and admissible([p, r], N, seg, min_gap, max_gap)]
                top = max(ordered(C[j - 1, p]) for p in win)
                same = [p for p in win if ordered(C[j - 1, p]) == top]
                ties += len(same) > 1
                assert P[j, r] == same[0]                            # the LOWER row
        with_segments += seg is not None
        absent += int((~any_chain).sum())
    assert ties > 50 and with_segments > 100 and absent > 100


def test_tie_rules_are_pinned():
    # two equal predecessors (rows 0 and 1): the lower one; two equal chain scores (end rows 2 and 3): the lower end row first
    S = np.array([[1.0, 1.0, 0.0, 0.0], [0.0, 0.0, 2.0, 2.0]], np.float32)
    C, P, ok = temporal.event_scores_ref(S, 1, 3)
    assert P[1].tolist() == [-1, 0, 0, 0] and ok[1].tolist() == [False, True, True, True]
    D, I = temporal.event_search_ref(S, 3, 1, 3)
    assert I[0].tolist() == [[0, 2], [0, 3], [0, 1]] and D[0].tolist() == [1.5, 1.5, 0.5]
    # -0.0 ties with +0.0, and the lower row wins whichever sign it carries
    S = np.array([[0.0, -0.0, -0.0, 0.0], [0.0, 0.0, 1.0, 1.0]], np.float32)
    assert temporal.event_scores_ref(S, 1, 1)[1][1].tolist() == [-1, 0, 1, 2]
    assert temporal.event_scores_ref(S, 1, 2)[1][1].tolist() == [-1, 0, 0, 1]
    # min_gap = 2 skips the neighbour; the window is cut at the segment start
    S = np.array([[5.0, 1.0, 9.0, 0.0, 0.0], [0.0, 0.0, 0.0, 0.0, 1.0]], np.float32)
    assert temporal.event_scores_ref(S, 2, 4)[1][1].tolist() == [-1, -1, 0, 0, 2]
    assert temporal.event_scores_ref(S, 2, 4, np.array([1, 5]))[1][1].tolist() == [-1, -1, -1, 1, 2]
    # best per segment: one entry per segment, (-FLT_MAX, -1) where no chain fits
    D, I = temporal.event_best_per_segment_ref(S, 2, 4, np.array([0, 2, 5]))
    assert D.shape == (1, 2) and I.shape == (1, 2, 2)
    assert D[0, 0] == -FLT_MAX and I[0, 0].tolist() == [-1, -1] and I[0, 1].tolist() == [2, 4] and D[0, 1] == 5.0
    # labels of an id-mapped index along the whole path
    ids = np.arange(5) * 10 + 7
    assert temporal.event_search_ref(S, 1, 2, 4, ids=ids)[1][0, 0].tolist() == [27, 47]


def test_one_event_is_a_plain_descending_sort():
    rng = np.random.default_rng(5)
    S = (rng.integers(-6, 7, size=(1, 40)) / 2.0).astype(np.float32)
    D, I = temporal.event_search_ref(S, 50, 1, 1)
    order = sorted(range(40), key=lambda r: (-float(S[0, r]), r))
    assert I[0, :40, 0].tolist() == order and I[0, 40:].tolist() == [[-1]] * 10
    assert np.array_equal(bits(D[0, :40]), bits(S[0, order] + np.float32(0.0))) and (D[0, 40:] == -FLT_MAX).all()
    assert len(set(S[0].tolist())) < 40                          # ties occur


def test_results_follow_the_scores_on_the_segmented_case():
    rng = np.random.default_rng(9)
    S = (rng.integers(-4, 5, size=(3, 3, 14)) / 2.0).astype(np.float32)
    D, I = temporal.event_search_ref(S, 20, 1, 3, SEGMENTS_SMALL)
    Db, Ib = temporal.event_best_per_segment_ref(S, 1, 3, SEGMENTS_SMALL)
    assert D.shape == (3, 20) and I.shape == (3, 20, 3) and Db.shape == (3, 4) and Ib.shape == (3, 4, 3)
    for b in range(3):
        best, ok = enumerate_chains(S[b], 1, 3, SEGMENTS_SMALL)
        n = int(ok.sum())
        ends = I[b, :n, 2]
        assert sorted(ends.tolist()) == np.flatnonzero(ok).tolist() and (I[b, n:] == -1).all()
        W = (best / np.float32(3)).astype(np.float32) + np.float32(0.0)
        assert np.array_equal(bits(D[b, :n]), bits(W[ends]))
        keys = [(-int(ordered(W[r])), int(r)) for r in ends]
        assert keys == sorted(keys)
        for s in range(4):
            inside = [r for r in ends if SEGMENTS_SMALL[s] <= r < SEGMENTS_SMALL[s + 1]]
            if inside:
                assert Ib[b, s, 2] == inside[0] and bits(Db[b, s]) == bits(W[inside[0]])
            else:
                assert Db[b, s] == -FLT_MAX and (Ib[b, s] == -1).all()
        assert (Db[b, 0] == -FLT_MAX) and (Db[b, 2] == -FLT_MAX) and Db[b, 1] > -FLT_MAX       # empty, shorter than m, long enough


def test_argument_checks_name_the_offending_values():
    assert _ffi.IVR_EVENT_MAX_LEN == 8 == temporal.EVENT_MAX_LEN and _ffi.IVR_EVENT_MAX_GAP == 4096 == temporal.EVENT_MAX_GAP
    S = np.zeros((2, 5), np.float32)
    with pytest.raises(ValueError, match=r"\[m,N\]"):
        temporal.event_scores_ref(np.zeros((9, 5), np.float32), 1, 1)
    with pytest.raises(ValueError, match=r"gaps \[0,1\]"):
        temporal.event_scores_ref(S, 0, 1)
    with pytest.raises(ValueError, match=r"gaps \[3,2\]"):
        temporal.event_scores_ref(S, 3, 2)
    with pytest.raises(ValueError, match=r"gaps \[1,4097\]"):
        temporal.event_scores_ref(S, 1, 4097)
    with pytest.raises(ValueError, match="integer"):
        temporal.event_scores_ref(S, 1, 2.0)
    index = FlatIPIndex.__new__(FlatIPIndex)             # no handle: every check below fails before the library is called
    index.d, index.device = 8, torch.device("cpu")
    x = np.zeros((2, 3, 8), np.float32)
    for call in (lambda *a, **k: temporal.event_search_device(a[0], a[1], 5, *a[2:], **k), temporal.event_best_per_segment_device):
        with pytest.raises(ValueError, match="FlatIPIndex"):
            call(object(), x, 4)
        with pytest.raises(ValueError, match=r"\[B,m,8\]"):
            call(index, x[:, :, :7], 4)
        with pytest.raises(ValueError, match=r"\[B,m,8\]"):
            call(index, x[0, 0], 4)
        with pytest.raises(ValueError, match=r"m=9 events outside \[1,8\]"):
            call(index, np.zeros((1, 9, 8), np.float32), 4)
        with pytest.raises(ValueError, match="no chains"):
            call(index, np.zeros((0, 3, 8), np.float32), 4)
        with pytest.raises(ValueError, match=r"gaps \[1,0\]"):
            call(index, x, 0)
        with pytest.raises(ValueError, match=r"gaps \[5,4\]"):
            call(index, x, 4, min_gap=5)
        with pytest.raises(ValueError, match=r"gaps \[1,4097\]"):
            call(index, x, 4097)
        with pytest.raises(ValueError, match="ascend"):
            call(index, x, 4, seg_off=np.array([0, 5, 3]))
    with pytest.raises(ValueError, match=r"k=0 outside"):
        temporal.event_search_device(index, x, 0, 4)
    with pytest.raises(ValueError, match=r"k=2049 outside"):
        temporal.event_search_device(index, x, 2049, 4)
    ta = temporal.TemporalAnalyzer()
    with pytest.raises(ValueError):
        ta.find_event_sequences([[1.0]], np.zeros((4, 1), np.float32), 3)
    with pytest.raises(ValueError):
        ta.find_event_sequences(np.zeros(4, np.float32), np.zeros((4, 1), np.float32), 3)
    assert ta.find_event_sequences(np.zeros((0, 3), np.float32), np.zeros((4, 3), np.float32), 3) == []


def test_lazy_package_exports_resolve():
    import ivr_amd
    for name in ("event_search", "event_search_device", "event_best_per_segment", "event_best_per_segment_device", "event_scores_ref",
                 "event_search_ref", "event_best_per_segment_ref"):
        assert name in ivr_amd.__all__
        assert getattr(ivr_amd, name) is getattr(temporal, name)
