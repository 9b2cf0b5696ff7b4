"""GPU suite of the moment search (ivr_amd/moments.py, csrc/search_moments.hip): both calls against the numpy definitions
(moment_search_ref / moment_range_search_ref) fed with the frame scores FlatIPIndex.rescore_device reports.  Every comparison is
exact: rows and counts element for element, the scores as bit patterns.  B below is the block of the run passes
(ivr_moment_block_rows)."""
import numpy as np
import pytest
import torch

from event_cases import make_rows
from group_cases import layouts
from moment_cases import FLT_MAX, pattern_rows
from ivr_amd import moments
from ivr_amd.index import FlatIPIndex

pytestmark = pytest.mark.gpu

B = 4096                                                           # checked against the library below: the ids are fixed at collection
NEG_INF = float("-inf")


def block():
    assert moments.moment_block_rows() == B, "the cases are written for a block of 4096 rows"
    return B


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def make_queries(d, nq, seed):
    return np.random.default_rng([seed, d, nq]).standard_normal((nq, d)).astype(np.float32)


def frame_scores(index, x, normalize=False):
    """S float32 [nq,N]: the score of every (query, stored row) from rescore_device, in column blocks of at most 2048 rows."""
    nq, N = x.shape[0], index.ntotal
    qd = torch.from_numpy(x).to(index.device)
    S = np.empty((nq, N), np.float32)
    for c0 in range(0, N, 2048):
        c1 = min(N, c0 + 2048)
        cand = torch.arange(c0, c1, dtype=torch.int64, device=index.device).repeat(nq, 1).contiguous()
        S[:, c0:c1] = index.rescore_device(qd, cand, normalize=normalize)[0].cpu().numpy()
    return S


def host(seg):
    return seg.cpu().numpy() if isinstance(seg, torch.Tensor) else seg


def assert_same(got, want, what):
    assert len(got) == len(want)
    for name, a, b in zip(("lims", "D", "I", "Lo", "Hi", "Cnt")[6 - len(got):], got, want):
        assert a.dtype == b.dtype and a.shape == b.shape, f"{name}: {a.dtype}{a.shape} against {b.dtype}{b.shape} {what}"
        same = np.array_equal(bits(a), bits(b)) if a.dtype == np.float32 else np.array_equal(a, b)
        assert same, f"{name} differs {what}"


def check_range(index, x, S, thr, gap, seg=None, ids=None, normalize=False):
    got = moments.moment_range_search(index, x, thr, gap, seg_off=seg, normalize=normalize)
    assert_same(got, moments.moment_range_search_ref(S, thr, gap, host(seg), ids), f"(range, N={S.shape[1]}, thr={thr}, gap={gap})")
    return got


def check_topk(index, x, S, k, thr, gap, min_count=1, rank="peak", seg=None, ids=None, normalize=False):
    got = moments.moment_search(index, x, k, thr, gap, min_count, rank, seg_off=seg, normalize=normalize)
    want = moments.moment_search_ref(S, k, thr, gap, min_count, rank, host(seg), ids)
    assert_same(got, want, f"(top-k, N={S.shape[1]}, k={k}, thr={thr}, gap={gap}, min_count={min_count}, rank={rank})")
    return got


def check_all(index, x, S, thr, gap, seg=None, k=10, **kw):
    out = check_range(index, x, S, thr, gap, seg, **kw)
    check_topk(index, x, S, k, thr, gap, 1, "peak", seg, **kw)
    check_topk(index, x, S, k, thr, gap, 1, "count", seg, **kw)
    return out


def make(d, N, seed, nq, period=None):
    X = make_rows(d, N, seed, period)
    index = FlatIPIndex(d)
    index.add(X)
    return index, X, make_queries(d, nq, seed)


@pytest.mark.parametrize("N", [1, 15, 16, 17, 63, 64, 65, 1023, 1024, 1025, B - 1, B, B + 1, 2 * B + 3])
def test_every_size_and_layout_matches_the_definition(N):
    index, X, x = make(20, N, 1, 2)
    S = frame_scores(index, x)
    thr = float(np.sort(S[0])[int(0.6 * N)])                      # an actual score: equality occurs, about 40 % of the rows are hot
    found = 0
    for i, (name, seg) in enumerate(layouts(N, block()).items()):
        lims = check_all(index, x, S, thr, (0, 1, 3)[i % 3], seg, k=(10, 2048)[i % 2])[0]
        found += int(lims[-1])
    assert found > 0


def pattern_index(N, g):
    """The prescribed hot patterns at N = 3 B + 5, one per query column; hot = 1 (column 6: 1 and 2), cold = 0, threshold 0.5."""
    C = np.zeros((N, 9), np.float32)
    C[:, 1] = 1                                                    # 0: none hot; 1: all hot
    C[::2, 2] = 1                                                  # 2: alternating hot / cold
    C[[B - 1, B], 3] = 1                                           # 3: hot only at B - 1 and B
    C[[B - 1 - g, B], 4] = 1                                       # 4: g cold rows between two hot ones across the block boundary
    C[[5, 2 * B + 7], 5] = 1                                       # 5: a whole cold block between two hot rows
    C[:, 6] = 1
    C[[2 * B + 50, 100, B + 9], 6] = 2                             # 6: one moment over all three blocks, equal peaks in different blocks
    C[[15, 16, 1023, 1024], 7] = 1                                 # 7: hot pairs across a tile and across a 1024-row boundary
    C[[0, N - 1], 8] = 1                                           # 8: the first and the last row
    X, x = pattern_rows(C)
    index = FlatIPIndex(20)
    index.add(X)
    S = frame_scores(index, x)
    assert np.array_equal(bits(S), bits(C.T))                      # the scores are the prescribed values, to the bit
    return index, x, S


SEGS = {"none": None,
        "at_B": np.array([0, B, 3 * B + 5], np.int64),                                 # a boundary exactly at B, between two hot rows
        "tile": np.array([0, 8, 8, B + 1, 3 * B + 5], np.int64),                       # a boundary inside a tile, and an empty segment
        "ends": np.array([3, 2 * B, 3 * B + 1], np.int64)}                             # hot rows in front of the first and behind the last offset


@pytest.mark.parametrize("layout", list(SEGS))
def test_prescribed_patterns_across_the_block_boundaries(layout):
    N, g = 3 * block() + 5, 3
    index, x, S = pattern_index(N, g)
    seg = SEGS[layout]
    count = {}
    for gap in (0, 1, g - 1, g, 2 * B, 2 * B + 1):
        lims, D, I, Lo, Hi, Cnt = check_all(index, x, S, 0.5, gap, seg)
        count[gap] = np.diff(lims)
        col = lambda j: list(zip(Lo[lims[j]:lims[j + 1]], Hi[lims[j]:lims[j + 1]], Cnt[lims[j]:lims[j + 1]], I[lims[j]:lims[j + 1]]))  # noqa: E731
        if layout == "none" and gap == 0:
            assert col(1) == [(0, N - 1, N, 0)] and col(6) == [(0, N - 1, N, 100)] and col(3) == [(B - 1, B, 2, B - 1)]
            assert col(7) == [(15, 16, 2, 15), (1023, 1024, 2, 1023)]
        if layout == "at_B" and gap == 0:
            assert col(3) == [(B - 1, B - 1, 1, B - 1), (B, B, 1, B)] and col(1) == [(0, B - 1, B, 0), (B, N - 1, N - B, B)]
            assert col(6) == [(0, B - 1, B, 100), (B, N - 1, N - B, B + 9)]
        if layout == "tile" and gap == 0:
            assert col(1) == [(0, 7, 8, 0), (8, B, B - 7, 8), (B + 1, N - 1, N - B - 1, B + 1)]
        if layout == "ends" and gap == 0:
            assert col(1) == [(3, 2 * B - 1, 2 * B - 3, 3), (2 * B, 3 * B, B + 1, 2 * B)] and col(8) == []
    nseg_hot = {"none": 1, "at_B": 2, "tile": 3, "ends": 2}[layout]
    assert (count[0][0], count[2 * B + 1][0]) == (0, 0)                                # none hot
    if layout == "none":
        assert count[0][2] == (N + 1) // 2                                             # the greatest moment count
        assert (count[g][4], count[g - 1][4]) == (1, 2)
        assert (count[2 * B + 1][5], count[2 * B][5]) == (1, 2)
    assert count[1][2] == nseg_hot                                                     # alternating with max_gap 1: one moment per segment


@pytest.mark.parametrize("d", [20, 512])
@pytest.mark.parametrize("normalize", [False, True])
def test_query_counts_dimensions_and_normalisation(d, normalize):
    N = 1100
    index, X, xall = make(d, N, 2, 65, period=7)                   # duplicate rows: equal scores inside every moment
    Sall = frame_scores(index, xall, normalize)
    thr = float(np.sort(Sall[0])[N // 2])                          # an actual score: equality occurs in query 0, half of whose rows are hot
    seg = np.array([3, 40, 40, 41, 300, 1024, 1030, 1098], np.int64)
    for nq in (1, 16, 17, 65):
        x, S = xall[:nq].copy(), Sall[:nq]
        lims = check_all(index, x, S, thr, 1, seg, normalize=normalize)[0]
        check_all(index, x, S, thr, 0, normalize=normalize)
        assert lims[1] > 0
    if normalize:
        assert np.abs(Sall[:1]).max() < np.abs(frame_scores(index, xall[:1])).max()   # the query was scaled down to unit length


def test_k_and_min_count():
    N = 2 * block() + 3
    index, X, x = make(20, N, 3, 3)
    S = frame_scores(index, x)
    thr = float(np.sort(S[1])[int(0.7 * N)])
    top = int(moments.moments_ref(S, thr, 2)[0][:, 2].max())
    for k in (1, 10, 2048):
        for min_count in (1, 2, top + 1):
            for rank in ("peak", "count"):
                D, I, Lo, Hi, Cnt = check_topk(index, x, S, k, thr, 2, min_count, rank)
                assert (Cnt[I >= 0] >= min_count).all()
    D, I, Lo, Hi, Cnt = moments.moment_search(index, x[:1], 5, thr, 2, top + 1)
    assert (D == -FLT_MAX).all() and (I == -1).all() and (Lo == -1).all() and (Hi == -1).all() and (Cnt == 0).all()      # all padding


def test_cap_counts_everything_and_writes_below_it():
    N = block() + 300
    index, X, x = make(20, N, 4, 5)
    S = frame_scores(index, x)
    thr = float(np.sort(S[0])[N // 2])
    want = moments.moment_range_search_ref(S, thr, 1)
    total = int(want[0][-1])
    assert total > 40
    xd = torch.from_numpy(x).to(index.device)
    exact = moments.moment_range_search_device(index, xd, thr, 1)                      # cap=None: a counting pass, then the exact one
    assert int(exact[6].item()) == total and all(len(t) == total for t in exact[1:6])
    assert_same([t.cpu().numpy() for t in exact[:6]], want, "(cap=None)")
    none = moments.moment_range_search_device(index, xd, thr, 1, cap=0)
    assert np.array_equal(none[0].cpu().numpy(), want[0]) and all(len(t) == 0 for t in none[1:6])
    # a cap below the total: everything is counted, the entries below the cap are written, the slots beyond are left as they were
    cap = total // 2
    lims = torch.zeros(6, dtype=torch.int64, device=index.device)
    D = torch.full((total,), -7.0, dtype=torch.float32, device=index.device)
    I, Lo, Hi, Cnt = (torch.full((total,), -7, dtype=torch.int64, device=index.device) for _ in range(4))
    index._call("ivr_index_range_search_moments", xd, 5, None, 0, thr, 1, False, lims, D, I, Lo, Hi, Cnt, cap)
    got = [t.cpu().numpy() for t in (lims, D, I, Lo, Hi, Cnt)]
    assert np.array_equal(got[0], want[0])
    for a, b in zip(got[1:], want[1:]):
        assert np.array_equal(a[:cap].view(np.uint8), b[:cap].view(np.uint8)) and (a[cap:] == -7).all()


def test_chunked_call_has_the_bits_of_the_unchunked_one(monkeypatch):
    # 65 queries in chunks of 16: 140 slots hold no query's 700 scores, so a chunk is the one 16-query tile it holds at least
    N = 700
    whole, X, x = make(20, N, 5, 65, period=7)
    monkeypatch.setenv("IVR_SEQ_CHUNK_SLOTS", "140")
    chunked = FlatIPIndex(20)                                       # the variable is read when the index is created
    chunked.add(X)
    monkeypatch.delenv("IVR_SEQ_CHUNK_SLOTS")
    S = frame_scores(whole, x)
    thr = float(np.sort(S.reshape(-1))[S.size // 2])               # an actual score, the median of all: equality occurs
    seg = np.array([3, 50, 51, 51, 300, 301, 640, 641, 698], np.int64)
    out = []
    for index in (whole, chunked):
        out.append(check_range(index, x, S, thr, 1, seg) + check_topk(index, x, S, 10, thr, 1, 2, "count", seg)
                   + check_topk(index, x, S, 3, thr, 0, 1, "peak"))
    assert all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(*out))
    assert (np.diff(out[0][0]) > 0).sum() > 16                     # queries of more than one chunk have moments


def test_id_mapped_index_labels_the_peak_by_id_and_the_bounds_by_row():
    rng = np.random.default_rng(6)
    N = 300
    X = make_rows(20, N, 6)
    ids = rng.permutation(N).astype(np.int64) + 1000
    index = FlatIPIndex(20)
    index.add_with_ids(X, ids)
    x = make_queries(20, 3, 6)
    S = frame_scores(index, x)
    thr = float(np.sort(S[0])[N // 2])
    seg = np.array([0, 100, 101, 290], np.int64)
    lims, D, I, Lo, Hi, Cnt = check_all(index, x, S, thr, 1, seg, ids=ids)
    assert len(I) and (I >= 1000).all() and (Lo < N).all() and (Hi < N).all() and (Lo <= Hi).all()


def test_side_stream_and_repeat_calls_agree():
    N = 2 * block() + 3
    index, X, x = make(20, N, 7, 17)
    xd = torch.from_numpy(x).to(index.device)
    seg = torch.tensor([0, 300, 700, N], dtype=torch.int64, device=index.device)
    S = frame_scores(index, x)
    thr = float(np.sort(S[0])[N // 2])
    total = int(moments.moment_range_search_ref(S, thr, 1, seg.cpu().numpy())[0][-1])
    first = [t.clone() for t in moments.moment_search_device(index, xd, 20, thr, 1, seg_off=seg)]
    first += [t.clone() for t in moments.moment_range_search_device(index, xd, thr, 1, seg, cap=total)[:6]]
    again = moments.moment_search_device(index, xd, 20, thr, 1, seg_off=seg) + moments.moment_range_search_device(index, xd, thr, 1, seg, cap=total)[:6]
    side = torch.cuda.Stream(device=index.device)
    side.wait_stream(torch.cuda.current_stream(index.device))
    with torch.cuda.stream(side):
        other = moments.moment_search_device(index, xd, 20, thr, 1, seg_off=seg) + moments.moment_range_search_device(index, xd, thr, 1, seg, cap=total)[:6]
    side.synchronize()
    for a, b, c in zip(first, again, other):
        assert torch.equal(a, b) and torch.equal(a, c)
    assert_same([t.cpu().numpy() for t in first[:5]], moments.moment_search_ref(S, 20, thr, 1, seg_off=seg.cpu().numpy()), "(side stream)")
    assert_same([t.cpu().numpy() for t in first[5:]], moments.moment_range_search_ref(S, thr, 1, seg.cpu().numpy()), "(side stream)")


def test_identities_with_the_flat_search():
    N = 2 * block() + 3
    index, X, x = make(20, N, 8, 17)
    Ds, Is = index.search(x, 1)
    # every row hot, no gap to bridge, no segments: one moment over the whole index, whose peak is the best row
    D, I, Lo, Hi, Cnt = moments.moment_search(index, x, 1, NEG_INF, 0)
    assert (Lo == 0).all() and (Hi == N - 1).all() and (Cnt == N).all()
    assert np.array_equal(I, Is) and np.array_equal(bits(D), bits(np.asarray(Ds, np.float32)))
    lims, D, I, Lo, Hi, Cnt = moments.moment_range_search(index, x, NEG_INF, 0)
    assert lims.tolist() == list(range(18)) and np.array_equal(I, Is[:, 0]) and (Cnt == N).all()
    # a threshold above every score: padding only, lims of zeros
    D, I, Lo, Hi, Cnt = moments.moment_search(index, x, 4, float("inf"), 1)
    assert (D == -FLT_MAX).all() and (I == -1).all() and (Lo == -1).all() and (Hi == -1).all() and (Cnt == 0).all()
    lims, D, I, Lo, Hi, Cnt = moments.moment_range_search(index, x, 1e30, 1)
    assert (lims == 0).all() and len(D) == len(I) == len(Lo) == len(Hi) == len(Cnt) == 0


def test_library_rejects_arguments_outside_the_ranges_and_an_empty_index_is_unused_slots():
    index, X, x = make(20, 50, 9, 2)
    dev = index.device
    q = torch.from_numpy(x).to(dev)
    D = torch.zeros((2, 4), dtype=torch.float32, device=dev)
    I, Lo, Hi, Cnt = (torch.zeros((2, 4), dtype=torch.int64, device=dev) for _ in range(4))
    lims = torch.zeros(3, dtype=torch.int64, device=dev)
    seg = torch.tensor([0, 50], dtype=torch.int64, device=dev)

    def topk(nq=2, seg=None, nseg=0, thr=0.0, gap=1, min_count=1, rank=0, k=4, q=q, D=D):
        index._call("ivr_index_search_moments", q, nq, seg, nseg, thr, gap, min_count, rank, k, False, D, I, Lo, Hi, Cnt)

    def rng(nq=2, seg=None, nseg=0, thr=0.0, gap=1, lims=lims, cap=8):
        index._call("ivr_index_range_search_moments", q, nq, seg, nseg, thr, gap, False, lims, D, I, Lo, Hi, Cnt, cap)

    topk()                                                         # the arguments in range pass
    rng()
    for bad, text in [(dict(nq=0), "nq=0"), (dict(seg=seg, nseg=0), "nseg=0"), (dict(thr=float("nan")), "NaN"), (dict(gap=-1), "max_gap=-1"),
                      (dict(min_count=0), "min_count=0"), (dict(rank=5), "rank=5"), (dict(k=0), "k=0"), (dict(k=2049), "k=2049"),
                      (dict(q=None), "NULL"), (dict(D=None), "NULL")]:
        with pytest.raises(ValueError, match=text):
            topk(**bad)
    for bad, text in [(dict(nq=0), "nq=0"), (dict(seg=seg, nseg=0), "nseg=0"), (dict(gap=-2), "max_gap=-2"), (dict(lims=None), "NULL"),
                      (dict(cap=-1), "cap=-1")]:
        with pytest.raises(ValueError, match=text):
            rng(**bad)
    empty = FlatIPIndex(20)
    D, I, Lo, Hi, Cnt = moments.moment_search(empty, x, 3, 0.0, seg_off=np.array([0, 4, 9]))
    assert D.shape == (2, 3) and (D == -FLT_MAX).all() and (I == -1).all() and (Lo == -1).all() and (Hi == -1).all() and (Cnt == 0).all()
    out = moments.moment_range_search(empty, x, 0.0)
    assert out[0].tolist() == [0, 0, 0] and all(len(o) == 0 for o in out[1:])


def test_retriever_returns_the_moments_of_a_query():
    from ivr_amd.compat import FAISSRetriever, KeyframeMetadata
    rng = np.random.default_rng(10)
    d, per = 32, 8
    folders = ["L01_V001", "L01_V002", "L02_V001"]
    feats = rng.standard_normal((len(folders) * per, d)).astype(np.float32)
    query = rng.standard_normal(d).astype(np.float32)
    for r, noise in [(6, 0.3), (7, 0.2), (8, 0.1), (10, 0.25), (20, 0.05)]:       # a shot that runs across the end of folder 0, and one frame
        feats[r] = query + noise * rng.standard_normal(d).astype(np.float32)
    metas = [KeyframeMetadata(folder_name=folders[i // per], image_name=f"{i % per:03d}.jpg", frame_id=i % per, file_path=f"/k/{i}.jpg",
                              clip_features=feats[i] / np.linalg.norm(feats[i])) for i in range(len(feats))]
    r = FAISSRetriever()
    r.build_index(feats, metas)
    res = r.search_moments(query, k=5, threshold=0.6, max_gap=1)
    spans = [(m.metadata.folder_name, m.metadata.image_name, [c.metadata.image_name for c in m.temporal_context]) for m in res]
    assert spans == [("L02_V001", "004.jpg", ["004.jpg", "004.jpg"]), ("L01_V002", "000.jpg", ["000.jpg", "002.jpg"]),
                     ("L01_V001", "007.jpg", ["006.jpg", "007.jpg"])]
    assert [m.rank for m in res] == [1, 2, 3] and all(c.similarity_score == 0.0 and c.rank == 0 for m in res for c in m.temporal_context)
    flat = r.search(query, k=1)[0]
    assert res[0].metadata.get_unique_key() == flat.metadata.get_unique_key() and res[0].similarity_score == flat.similarity_score
    assert [m.metadata.image_name for m in r.search_moments(query, k=5, threshold=0.6, max_gap=1, min_count=2)] == ["000.jpg", "007.jpg"]
