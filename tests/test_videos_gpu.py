"""GPU suite of the video search (ivr_amd/videos.py, csrc/search_videos.hip): both calls against the numpy definitions
(video_scores_ref / video_search_ref) fed with the frame scores FlatIPIndex.rescore_device reports.  Every comparison is exact: V and
D as bit patterns, Vseg element for element."""
import numpy as np
import pytest
import torch

from event_cases import make_rows
from group_cases import layouts
from ivr_amd import grouping, videos
from ivr_amd.index import FlatIPIndex
from video_cases import FLT_MAX, MODES, SET_SIZES, SIZES, make_members, set_offsets

pytestmark = pytest.mark.gpu

PIECE = 2048            # stored rows of one workgroup of the score pass: the layouts put boundaries around it


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def frame_scores(index, x, normalize=False):
    """S float32 [members,N]: the score of every (member, stored row) from rescore_device, in column blocks of at most 2048 rows."""
    nq, N = x.shape[0], index.ntotal
    qd = torch.from_numpy(x).to(index.device)
    S = np.empty((nq, N), np.float32)
    for c0 in range(0, N, 2048):
        c1 = min(N, c0 + 2048)
        cand = torch.arange(c0, c1, dtype=torch.int64, device=index.device).repeat(nq, 1).contiguous()
        S[:, c0:c1] = index.rescore_device(qd, cand, normalize=normalize)[0].cpu().numpy()
    return S


def make(d, N, seed, period=None):
    X = make_rows(d, N, seed, period)
    index = FlatIPIndex(d)
    index.add(X)
    return index, X


def check(index, x, S, seg, sets, k=10, exclude=None, normalize=False, modes=MODES):
    """Both calls in every mode against the definition; returns {mode: (V, Vseg, D)}."""
    sums = videos.video_sums_ref(S, seg, sets)
    out = {}
    for mode in modes:
        what = f"(N={S.shape[1]}, members={S.shape[0]}, mode={mode}, k={k})"
        V = videos.video_scores(index, x, seg, sets, mode, normalize=normalize)
        Vr = videos.video_scores_ref(S, seg, sets, mode, sums)
        assert V.dtype == np.float32 and V.shape == Vr.shape
        assert np.array_equal(bits(V), bits(Vr)), f"score bits differ {what}: {int((bits(V) != bits(Vr)).sum())} of {V.size}"
        Vseg, D = videos.video_search(index, x, k, seg, sets, mode, exclude, normalize=normalize)
        Vs, Dr = videos.video_search_ref(S, k, seg, sets, mode, exclude, sums)
        assert Vseg.dtype == np.int64 and D.dtype == np.float32 and Vseg.shape == Vs.shape and D.shape == Dr.shape
        assert np.array_equal(Vseg, Vs), f"videos differ {what}"
        assert np.array_equal(bits(D), bits(Dr)), f"ranked score bits differ {what}"
        out[mode] = (V, Vseg, D)
    return out


@pytest.mark.parametrize("N", SIZES)
def test_every_size_and_layout_matches_the_definition(N):
    index, X = make(20, N, 1)
    sets = set_offsets([1, 17, 65, 15])                              # one column, two tiles, two blocks, one short tile
    x = make_members(20, int(sets[-1]), 1)
    S = frame_scores(index, x)
    for name, seg in layouts(N, PIECE).items():
        out = check(index, x, S, seg, sets, k=10)
        ranked = out["symmetric"][1]
        assert ranked[0, 0] >= 0 or name in ("marks", "inside")      # only the layouts that leave rows outside can be without a video
        if name in ("none", "one"):
            assert (ranked[:, 1:] == -1).all()                       # k above the number of videos: unused slots


@pytest.mark.parametrize("d", [20, 512])
@pytest.mark.parametrize("m", SET_SIZES)
def test_every_set_size_in_both_dimensions_with_normalisation_and_exclusion(d, m):
    N = 1100
    index, X = make(d, N, 2)
    sets = set_offsets([m, 2, 33, m])                                # the size under test twice, at two alignments of the packed members
    x = make_members(d, int(sets[-1]), 2)
    seg = np.array([3, 40, 40, 41, 300, 1024, 1030, 1098], np.int64)
    exclude = np.array([3, 0, -1, 6], np.int64)
    for normalize in (False, True):
        S = frame_scores(index, x, normalize)
        out = check(index, x, S, seg, sets, k=5, exclude=exclude, normalize=normalize)
        check(index, x, S, None, sets, k=1, normalize=normalize, modes=("symmetric",))
        for mode in MODES:
            Vseg = out[mode][1]
            assert 3 not in Vseg[0] and 0 not in Vseg[1] and 6 not in Vseg[3] and (Vseg[2] >= 0).all()
    # one set without set_off
    one = x[:m].copy()
    check(index, one, frame_scores(index, one), seg, None, k=7)


def test_the_largest_set_and_a_long_video():
    # 4096 members in one set: 64 blocks maximise into one line of row maxima; one video longer than a piece of the score pass
    N = 2 * PIECE + 3
    index, X = make(20, N, 3)
    x = make_members(20, videos.VIDEO_MAX_MEMBERS, 3)
    S = frame_scores(index, x)
    seg = np.array([0, 5, PIECE + 700, N], np.int64)
    check(index, x, S, seg, None, k=3)
    with pytest.raises(ValueError, match="4097 members > 4096"):
        videos.video_scores(index, make_members(20, 4097, 3), seg)


def test_equal_scores_rank_the_lower_video():
    index, X = make(20, 257, 4, period=7)
    x = X[[0, 1, 2, 3, 4, 5, 6, 0, 1, 2, 9, 3]].copy()              # members that are stored rows, some of them twice
    sets = set_offsets([7, 3, 2])
    S = frame_scores(index, x)
    assert np.array_equal(bits(S[:, 0]), bits(S[:, 7])) and np.array_equal(bits(S[0]), bits(S[7]))      # the duplicates do tie, to the bit
    seg = np.array([0, 16, 33, 64, 64, 130, 257], np.int64)          # every non-empty video holds each of the seven distinct rows
    out = check(index, x, S, seg, sets, k=6)
    V, Vseg, D = out["forward"]
    assert (bits(V[:, [0, 1, 2, 4, 5]]) == bits(V[:, :1])).all()     # every member finds the same best match in every video
    assert (Vseg == np.array([0, 1, 2, 4, 5, -1])).all() and (D[:, 5] == -FLT_MAX).all()
    check(index, x, S, np.arange(258, dtype=np.int64), sets, k=2048)           # every row a video: the duplicates tie in every mode


def test_chunked_call_has_the_bits_of_the_unchunked_one(monkeypatch):
    N = 700
    X = make_rows(20, N, 5)
    whole = FlatIPIndex(20)
    whole.add(X)
    sets = set_offsets([5, 20, 70, 3, 16])
    x = make_members(20, int(sets[-1]), 5)
    S = frame_scores(whole, x)
    seg = np.array([3, 50, 51, 51, 300, 301, 640, 641, 698], np.int64)
    ref = check(whole, x, S, seg, sets, k=4)
    # 704 row slots per set: a budget of 3000 holds four sets (two chunks), one of 800 a single set (five chunks)
    for slots in ("3000", "800"):
        monkeypatch.setenv("IVR_SEQ_CHUNK_SLOTS", slots)
        chunked = FlatIPIndex(20)                                    # the variable is read when the index is created
        chunked.add(X)
        monkeypatch.delenv("IVR_SEQ_CHUNK_SLOTS")
        out = check(chunked, x, S, seg, sets, k=4)
        for mode in MODES:
            assert all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(ref[mode], out[mode]))


def test_side_stream_and_repeat_calls_agree():
    N = 2 * PIECE + 3
    index, X = make(20, N, 6)
    sets = set_offsets([70, 9, 16])
    x = make_members(20, int(sets[-1]), 6)
    xd = torch.from_numpy(x).to(index.device)
    seg = torch.tensor([0, 300, 700, N], dtype=torch.int64, device=index.device)
    first = [t.clone() for t in videos.video_search_device(index, xd, 3, seg, sets)] + [videos.video_scores_device(index, xd, seg, sets).clone()]
    again = list(videos.video_search_device(index, xd, 3, seg, sets)) + [videos.video_scores_device(index, xd, seg, sets)]
    side = torch.cuda.Stream(device=index.device)
    side.wait_stream(torch.cuda.current_stream(index.device))
    with torch.cuda.stream(side):
        other = list(videos.video_search_device(index, xd, 3, seg, sets)) + [videos.video_scores_device(index, xd, seg, sets)]
    side.synchronize()
    for a, b, c in zip(first, again, other):
        assert torch.equal(a, b) and torch.equal(a, c)
    S = frame_scores(index, x)
    Vs, Dr = videos.video_search_ref(S, 3, seg.cpu().numpy(), sets)
    assert np.array_equal(first[0].cpu().numpy(), Vs) and np.array_equal(bits(first[1].cpu().numpy()), bits(Dr))
    assert np.array_equal(bits(first[2].cpu().numpy()), bits(videos.video_scores_ref(S, seg.cpu().numpy(), sets)))


def test_related_videos_is_the_search_of_every_video_without_itself(monkeypatch):
    rng = np.random.default_rng(7)
    lengths = rng.integers(5, 71, size=40)
    lengths[[3, 17]] = 0                                             # two videos without rows
    seg = set_offsets(lengths)
    N = int(seg[-1])
    index, X = make(20, N, 7, period=301)                            # some frames of late videos repeat frames of early ones
    S = frame_scores(index, index.reconstruct_n(0, N))
    full = np.flatnonzero(lengths > 0)
    sets = set_offsets(lengths[full])
    for mode in ("symmetric", "forward"):
        Vs, Dr = videos.video_search_ref(S, 5, seg, sets, mode, exclude=full)
        want_seg = np.full((40, 5), -1, np.int64)
        want_D = np.full((40, 5), -FLT_MAX, np.float32)
        want_seg[full], want_D[full] = Vs, Dr
        Vseg, D = videos.related_videos(index, seg, 5, mode)
        assert np.array_equal(Vseg, want_seg) and np.array_equal(bits(D), bits(want_D))
        assert not (Vseg == np.arange(40)[:, None]).any()            # never the video itself
    monkeypatch.setattr(videos, "RELATED_CHUNK_ROWS", 300)           # several calls, each with a few videos
    Vseg, D = videos.related_videos(index, torch.from_numpy(seg).to(index.device), 5, "symmetric", videos=[39, 3, 0, 20])
    Vs, Dr = videos.video_search_ref(S, 5, seg, sets, "symmetric", exclude=full)
    at = {int(j): i for i, j in enumerate(full)}
    for line, j in enumerate([39, 3, 0, 20]):
        if j == 3:
            assert (Vseg[line] == -1).all() and (D[line] == -FLT_MAX).all()
        else:
            assert np.array_equal(Vseg[line], Vs[at[j]]) and np.array_equal(bits(D[line]), bits(Dr[at[j]]))


def test_one_member_forward_is_best_per_segment_within_the_fixed_point():
    N = 1500
    index, X = make(20, N, 8)
    x = make_members(20, 9, 8) * np.float32(2.0 ** -10)             # scores around 2^-8: their float32 grid is finer than 2^-24
    seg = np.array([2, 2, 90, 91, 600, 600, 1024, 1400, 1499], np.int64)
    Db, Ib = grouping.best_per_segment(index, x, seg)
    V = videos.video_scores(index, x, seg, np.arange(10, dtype=np.int64), "forward")
    assert V.shape == Db.shape
    assert np.array_equal(V == -FLT_MAX, Ib < 0)                     # the empty videos
    used = Ib >= 0
    # float32(fix(s) / 2^24) against s: the fixed point rounds by at most 2^-25, and a multiple of 2^-24 below 1 is a float32 (from
    # 0.5 on s 2^24 is an integer and the round trip exact), so the conversion back adds nothing
    bound = 2.0 ** -25
    assert (np.abs(V[used].astype(np.float64) - Db[used].astype(np.float64)) <= bound).all()
    assert not np.array_equal(bits(V[used]), bits(Db[used]))         # within the bound, and not to the bit


def test_library_rejects_bad_sets_and_an_empty_index_is_unused_slots():
    index, X = make(20, 50, 9)
    dev = index.device
    q = torch.from_numpy(make_members(20, 6, 9)).to(dev)
    V = torch.zeros((3, 1), dtype=torch.float32, device=dev)

    def scores(off, nq=6):
        t = torch.tensor(off, dtype=torch.int64, device=dev)
        index._call("ivr_index_video_scores", q, nq, t, len(off) - 1, None, 0, 2, False, V)

    scores([0, 1, 4, 6])                                             # the arguments in range pass
    scores([1, 2, 3, 5])                                             # members in front of the first set and behind the last are skipped
    for off, text in [([0, 2, 2, 6], "set 1 is empty"), ([0, 5, 3, 6], r"set_off\[1\]=5 > set_off\[2\]=3"), ([0, 2, 4, 7], "outside the 6 members"),
                      ([-1, 2, 4, 6], "outside the 6 members")]:
        with pytest.raises(ValueError, match=text):
            scores(off)
    empty = FlatIPIndex(20)
    x = make_members(20, 6, 9)
    Ve = videos.video_scores(empty, x, np.array([0, 4, 9]), np.array([0, 2, 6]))
    assert Ve.shape == (2, 2) and (Ve == -FLT_MAX).all()
    Vseg, D = videos.video_search(empty, x, 3, np.array([0, 4, 9]), np.array([0, 2, 6]))
    assert Vseg.shape == (2, 3) and (Vseg == -1).all() and (D == -FLT_MAX).all()
    Vseg, D = videos.video_search(empty, x, 2)
    assert Vseg.shape == (1, 2) and (Vseg == -1).all() and (D == -FLT_MAX).all()


def test_retriever_searches_by_video_and_lists_related_videos_by_folder():
    from ivr_amd.compat import FAISSRetriever, KeyframeMetadata
    rng = np.random.default_rng(10)
    d, per = 32, 6
    folders = ["L01_V001", "L01_V002", "L02_V001", "L03_V007"]
    feats = rng.standard_normal((len(folders) * per, d)).astype(np.float32)
    feats[18:24] = feats[6:12][::-1] + 0.05 * rng.standard_normal((per, d)).astype(np.float32)       # folder 3 is folder 1 played backwards
    metas = [KeyframeMetadata(folder_name=folders[i // per], image_name=f"{i % per:03d}.jpg", frame_id=i % per, file_path=f"/k/{i}.jpg",
                              clip_features=feats[i] / np.linalg.norm(feats[i])) for i in range(len(feats))]
    r = FAISSRetriever()
    r.build_index(feats, metas)
    clip = feats[6:12][[4, 1, 3]] + 0.02 * rng.standard_normal((3, d)).astype(np.float32)            # three frames of folder 1, out of order
    hits = r.search_by_video(clip, k=3)
    assert [name for name, _ in hits[:2]] == ["L01_V002", "L03_V007"] and len(hits) == 3
    assert all(isinstance(name, str) and isinstance(score, float) for name, score in hits)
    assert all(a[1] >= b[1] for a, b in zip(hits, hits[1:]))
    assert r.search_by_video(clip, k=10, mode="forward")[0][0] == "L01_V002"
    related = r.related_videos(k=2)
    assert sorted(related) == sorted(folders)
    assert related["L01_V002"][0][0] == "L03_V007" and related["L03_V007"][0][0] == "L01_V002"
    assert all(name != own and len(lst) == 2 for own, lst in related.items() for name, _ in lst)
    with pytest.raises(ValueError, match="mode must be"):
        r.search_by_video(clip, mode="max")
