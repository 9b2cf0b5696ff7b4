"""GPU suite of the grouped search (ivr_amd/grouping.py, csrc/search_groups.hip): both calls against the numpy definitions
(group_search_ref / best_per_segment_ref) fed with the frame scores FlatIPIndex.rescore_device reports.  Every comparison is exact:
the segments and the rows element for element, the scores as bit patterns.  P below is the piece of the rows pass
(ivr_group_piece_rows)."""
import numpy as np
import pytest
import torch

from event_cases import make_rows
from group_cases import FLT_MAX, SIZES, layouts
from ivr_amd import grouping
from ivr_amd.index import FlatIPIndex

pytestmark = pytest.mark.gpu

P = None


def piece():
    global P
    if P is None:
        P = grouping.group_piece_rows()
    return P


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


def check_groups(index, x, S, G, g, seg=None, ids=None, normalize=False):
    Gseg, D, I = grouping.group_search(index, x, G, g, seg_off=seg, normalize=normalize)
    Gr, Dr, Ir = grouping.group_search_ref(S, G, g, host(seg), ids)
    assert Gseg.dtype == np.int64 and D.dtype == np.float32 and I.dtype == np.int64
    assert Gseg.shape == Gr.shape and D.shape == Dr.shape and I.shape == Ir.shape
    what = f"(N={S.shape[1]}, G={G}, g={g})"
    assert np.array_equal(Gseg, Gr), f"segments differ {what}"
    assert np.array_equal(I, Ir), f"rows differ {what}"
    assert np.array_equal(bits(D), bits(Dr)), f"score bits differ {what}"
    return Gseg, D, I


def check_best(index, x, S, seg=None, ids=None, normalize=False):
    D, I = grouping.best_per_segment(index, x, seg, normalize=normalize)
    Dr, Ir = grouping.best_per_segment_ref(S, host(seg), ids)
    assert D.dtype == np.float32 and I.dtype == np.int64 and D.shape == Dr.shape and I.shape == Ir.shape
    assert np.array_equal(I, Ir), f"best rows differ (N={S.shape[1]})"
    assert np.array_equal(bits(D), bits(Dr)), f"best score bits differ (N={S.shape[1]})"
    return D, I


def make(d, N, seed, nq, period=None):
    X = make_rows(d, N, seed, period)
    index = FlatIPIndex(d)
    index.add(X)
    return index, X, make_queries(d, nq, seed)


def size_cases():
    p = 2048                                                       # checked against the library below: the ids are fixed at collection
    return [1, 15, 16, 17, 63, 64, 65, 1023, 1024, 1025, p - 1, p, p + 1, 2 * p + 3]


@pytest.mark.parametrize("N", size_cases())
def test_every_size_layout_and_group_shape_matches_the_definition(N):
    assert piece() == 2048, "size_cases() is written for a piece of 2048 rows"
    index, X, x = make(20, N, 1, 1)
    S = frame_scores(index, x)
    for name, seg in layouts(N, piece()).items():
        for G, g in SIZES:
            Gseg, D, I = check_groups(index, x, S, G, g, seg)
            assert Gseg[0, 0] >= 0 or name in ("marks", "inside")      # only the layouts that leave rows outside can be without a group
        check_best(index, x, S, seg)


@pytest.mark.parametrize("d", [20, 512])
@pytest.mark.parametrize("normalize", [False, True])
def test_query_counts_dimensions_and_normalisation(d, normalize):
    N = 1100
    index, X, xall = make(d, N, 2, 65)
    Sall = frame_scores(index, xall, normalize)
    seg = np.array([3, 40, 40, 41, 300, 1024, 1030, 1098], np.int64)
    for nq in (1, 16, 17, 65):
        x, S = xall[:nq].copy(), Sall[:nq]
        check_groups(index, x, S, 10, 3, seg, normalize=normalize)
        check_groups(index, x, S, 4, 64, seg, normalize=normalize)
        check_groups(index, x, S, 10, 1, normalize=normalize)
        check_best(index, x, S, seg, normalize=normalize)
    if normalize:
        assert np.abs(Sall[:1]).max() < np.abs(frame_scores(index, xall[:1])).max()   # the query was scaled down to unit length


def test_equal_scores_rank_the_lower_row_and_the_lower_segment():
    index, X, x = make(20, 257, 3, 3, period=7)
    S = frame_scores(index, x)
    assert np.array_equal(bits(S[:, 0]), bits(S[:, 7]))            # the duplicates do tie, to the bit
    seg = np.array([0, 16, 33, 64, 64, 130, 257], np.int64)        # every non-empty segment holds each of the seven distinct rows
    for G, g in [(1, 1), (5, 1), (5, 3), (5, 64), (2048, 1)]:
        check_groups(index, x, S, G, g, seg)
        check_groups(index, x, S, G, g)
    check_best(index, x, S, seg)
    Gseg, D, I = grouping.group_search(index, x, 5, 20, seg_off=seg)
    assert (Gseg == np.array([0, 1, 2, 4, 5])).all()               # all best scores are equal: the lower segment first
    assert (bits(D[:, :, 0]) == bits(D[:, :1, 0])).all()
    tied = (bits(D[:, :, :-1]) == bits(D[:, :, 1:])) & (I[:, :, 1:] >= 0)     # the unused slots of the 16-row segment tie too
    assert tied.any() and (I[:, :, :-1][tied] < I[:, :, 1:][tied]).all()


def test_id_mapped_index_labels_rows_by_id_and_groups_by_segment_number():
    rng = np.random.default_rng(4)
    N = 300
    X = make_rows(20, N, 4)
    ids = rng.permutation(N).astype(np.int64) + 1000
    index = FlatIPIndex(20)
    index.add_with_ids(X, ids)
    x = make_queries(20, 3, 4)
    S = frame_scores(index, x)
    seg = np.array([0, 100, 101, 290], np.int64)
    for G, g in [(3, 1), (3, 5), (2, 64)]:
        Gseg, D, I = check_groups(index, x, S, G, g, seg, ids=ids)
        assert (I[I >= 0] >= 1000).all() and set(Gseg.reshape(-1).tolist()) <= {0, 1, 2}
    check_best(index, x, S, seg, ids=ids)


@pytest.mark.parametrize("k", [10, 64])
def test_identities_with_the_flat_search(k):
    N = 2 * piece() + 3
    index, X, x = make(20, N, 5, 17)
    Ds, Is = index.search(x, k)
    Ds = np.asarray(Ds, np.float32)
    # one segment, one group of k rows
    Gseg, D, I = grouping.group_search(index, x, 1, k)
    assert (Gseg == 0).all() and np.array_equal(I[:, 0], Is) and np.array_equal(bits(D[:, 0]), bits(Ds))
    # every row its own segment, k groups of one row
    Gseg, D, I = grouping.group_search(index, x, k, 1, seg_off=np.arange(N + 1))
    assert np.array_equal(I[:, :, 0], Is) and np.array_equal(Gseg, Is) and np.array_equal(bits(D[:, :, 0]), bits(Ds))


def test_best_per_segment_is_the_first_column_of_the_grouped_search():
    N = 1500
    index, X, x = make(20, N, 6, 17)
    S = frame_scores(index, x)
    seg = np.array([2, 2, 90, 91, 600, 600, 1024, 1400, 1499], np.int64)
    nseg = len(seg) - 1
    Db, Ib = check_best(index, x, S, seg)
    Gseg, D, I = check_groups(index, x, S, nseg, 1, seg)
    for q in range(17):
        used = Gseg[q] >= 0
        order = np.argsort(Gseg[q][used])
        assert Gseg[q][used][order].tolist() == np.flatnonzero(Ib[q] >= 0).tolist()
        assert np.array_equal(I[q, used, 0][order], Ib[q][Ib[q] >= 0])
        assert np.array_equal(bits(D[q, used, 0][order]), bits(Db[q][Ib[q] >= 0]))
    assert (Ib[:, [0, 4]] == -1).all() and (Db[:, [0, 4]] == -FLT_MAX).all()        # the empty segments
    # without seg_off: one column, the best row of the index
    D1, I1 = check_best(index, x, S)
    assert D1.shape == (17, 1) and np.array_equal(I1[:, 0], index.search(x, 1)[1][:, 0])


def test_chunked_call_has_the_bits_of_the_unchunked_one(monkeypatch):
    # 65 queries in chunks of 16: 8 segment keys per query and 140 slots leave room for 17, taken in whole 16-query tiles
    N = 700
    whole, X, x = make(20, N, 7, 65)
    monkeypatch.setenv("IVR_SEQ_CHUNK_SLOTS", "140")
    chunked = FlatIPIndex(20)                                       # the variable is read when the index is created
    chunked.add(X)
    monkeypatch.delenv("IVR_SEQ_CHUNK_SLOTS")
    S = frame_scores(whole, x)
    seg = np.array([3, 50, 51, 51, 300, 301, 640, 641, 698], np.int64)
    out = []
    for index in (whole, chunked):
        out.append(check_groups(index, x, S, 10, 3, seg) + check_groups(index, x, S, 3, 1, seg) + check_best(index, x, S, seg))
    assert all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(*out))


def test_side_stream_and_repeat_calls_agree():
    index, X, x = make(20, 2 * piece() + 3, 8, 17)
    xd = torch.from_numpy(x).to(index.device)
    seg = torch.tensor([0, 300, 700, 2 * piece() + 3], dtype=torch.int64, device=index.device)
    first = [t.clone() for t in grouping.group_search_device(index, xd, 3, 20, seg)]
    again = grouping.group_search_device(index, xd, 3, 20, seg)
    side = torch.cuda.Stream(device=index.device)
    side.wait_stream(torch.cuda.current_stream(index.device))
    with torch.cuda.stream(side):
        other = grouping.group_search_device(index, xd, 3, 20, seg)
        best = grouping.best_per_segment_device(index, xd, seg)
    side.synchronize()
    for a, b, c in zip(first, again, other):
        assert torch.equal(a, b) and torch.equal(a, c)
    S = frame_scores(index, x)
    Dr, Ir = grouping.best_per_segment_ref(S, seg.cpu().numpy())
    assert np.array_equal(best[1].cpu().numpy(), Ir) and np.array_equal(bits(best[0].cpu().numpy()), bits(Dr))
    Gr, Dg, Ig = grouping.group_search_ref(S, 3, 20, seg.cpu().numpy())
    assert np.array_equal(first[0].cpu().numpy(), Gr) and np.array_equal(first[2].cpu().numpy(), Ig)
    assert np.array_equal(bits(first[1].cpu().numpy()), bits(Dg))


def test_library_rejects_arguments_outside_the_ranges_and_an_empty_index_is_unused_slots():
    index, X, x = make(20, 50, 9, 2)
    dev = index.device
    q = torch.from_numpy(x).to(dev)
    Gseg = torch.zeros((2, 4), dtype=torch.int64, device=dev)
    D = torch.zeros((2, 4, 2), dtype=torch.float32, device=dev)
    I = torch.zeros((2, 4, 2), dtype=torch.int64, device=dev)
    seg = torch.tensor([0, 50], dtype=torch.int64, device=dev)

    def groups(nq=2, seg=None, nseg=0, G=4, g=2, q=q, Gseg=Gseg, D=D, I=I):
        index._call("ivr_index_search_groups", q, nq, seg, nseg, G, g, False, Gseg, D, I)

    def best(nq=2, seg=None, nseg=0, q=q, D=D, I=I):
        index._call("ivr_index_best_per_segment", q, nq, seg, nseg, False, D, I)

    groups()                                                       # the arguments in range pass
    best()
    for bad, text in [(dict(G=0), "G=0"), (dict(g=0), "g=0"), (dict(g=65), "g=65"), (dict(G=33, g=64), "G \\* g = 2112"),
                      (dict(seg=seg, nseg=0), "nseg=0"), (dict(nq=0), "nq=0"), (dict(q=None), "NULL"), (dict(Gseg=None), "NULL"),
                      (dict(D=None), "NULL"), (dict(I=None), "NULL")]:
        with pytest.raises(ValueError, match=text):
            groups(**bad)
    for bad, text in [(dict(seg=seg, nseg=0), "nseg=0"), (dict(nq=0), "nq=0"), (dict(D=None), "NULL")]:
        with pytest.raises(ValueError, match=text):
            best(**bad)
    with pytest.raises(ValueError, match="group_size=65"):
        grouping.group_search(index, x, 1, 65)
    empty = FlatIPIndex(20)
    Gs, Dd, Ii = grouping.group_search(empty, x, 3, 2, seg_off=np.array([0, 4, 9]))
    assert Gs.shape == (2, 3) and Dd.shape == (2, 3, 2) and (Gs == -1).all() and (Dd == -FLT_MAX).all() and (Ii == -1).all()
    Dd, Ii = grouping.best_per_segment(empty, x, np.array([0, 4, 9]))
    assert Dd.shape == (2, 2) and (Dd == -FLT_MAX).all() and (Ii == -1).all()
    Dd, Ii = grouping.best_per_segment(empty, x, None)
    assert Dd.shape == (2, 1) and (Dd == -FLT_MAX).all() and (Ii == -1).all()


def test_retriever_groups_the_hits_by_folder():
    from ivr_amd.compat import FAISSRetriever, KeyframeMetadata
    rng = np.random.default_rng(10)
    d, per = 32, 6
    folders = ["L01_V001", "L01_V002", "L02_V001", "L03_V007"]
    feats = rng.standard_normal((len(folders) * per, d)).astype(np.float32)
    query = rng.standard_normal(d).astype(np.float32)
    feats[13] = query + 0.05 * rng.standard_normal(d).astype(np.float32)      # folder 2 holds the best frame ...
    feats[14] = query + 0.3 * rng.standard_normal(d).astype(np.float32)       # ... and the runner-up
    feats[3] = query + 0.6 * rng.standard_normal(d).astype(np.float32)        # folder 0 comes second
    metas = [KeyframeMetadata(folder_name=folders[i // per], image_name=f"{i % per:03d}.jpg", frame_id=i % per, file_path=f"/k/{i}.jpg",
                              clip_features=feats[i] / np.linalg.norm(feats[i])) for i in range(len(feats))]
    r = FAISSRetriever()
    r.build_index(feats, metas)
    groups = r.search_grouped(query, n_groups=3, group_size=2)
    assert len(groups) == 3 and all(len(grp) == 2 for grp in groups)
    assert [grp[0].metadata.folder_name for grp in groups[:2]] == ["L02_V001", "L01_V001"]
    assert [res.metadata.image_name for res in groups[0]] == ["001.jpg", "002.jpg"] and [res.rank for res in groups[0]] == [1, 2]
    assert all(len({res.metadata.folder_name for res in grp}) == 1 for grp in groups)
    assert len({grp[0].metadata.folder_name for grp in groups}) == 3
    flat = r.search(query, k=1)[0]
    assert groups[0][0].metadata.get_unique_key() == flat.metadata.get_unique_key()
    assert groups[0][0].similarity_score == flat.similarity_score
    assert all(a.similarity_score >= b.similarity_score for grp in groups for a, b in zip(grp, grp[1:]))
    # folders whose rows are not contiguous cannot be segments
    metas[1].folder_name, metas[1].image_name = "L03_V007", "900.jpg"
    r2 = FAISSRetriever()
    r2.build_index(feats, metas)
    with pytest.raises(ValueError, match="not contiguous"):
        r2.search_grouped(query)
