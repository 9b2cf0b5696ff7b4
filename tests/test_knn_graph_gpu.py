"""GPU suite of the neighbour graph (ivr_amd/neighbors.py, csrc/knn.hip): D (to the bit), I and count of ivr_index_knn_graph for exact
equality with the numpy definition knn_graph_ref fed with the scores FlatIPIndex.rescore_device reports for the stored rows as
queries, both orders of every pair; then the flat search as a second witness, and similarity_graphs / build_similarity_relationships
against the float64 reference folder by folder."""
import functools

import numpy as np
import pytest
import torch

from cluster_cases import DS, NS, SEGMENTS, drifting_chains
from ivr_amd import _ffi, neighbors
from ivr_amd.index import FlatIPIndex
from knn_cases import THRESHOLD, TOP, clear_rows, cosines64
from oracle import search_ref

pytestmark = pytest.mark.gpu

KMAX = _ffi.IVR_KNN_MAX_K
LOWEST = np.float32(-np.finfo(np.float32).max)


def self_scores(index):
    """S float32 [N,N]: the score of every (stored row as the query, stored row) from rescore_device, in column blocks of at most
    2048 rows (the helper of test_cluster_gpu.py): S[j, i] and S[i, j] are scored separately, each with its own query."""
    N = index.ntotal
    qd = torch.from_numpy(index.reconstruct_n()).to(index.device)
    S = np.empty((N, N), np.float32)
    for c0 in range(0, N, 2048):
        c1 = min(N, c0 + 2048)
        cand = torch.arange(c0, c1, dtype=torch.int64, device=index.device).repeat(N, 1).contiguous()
        S[:, c0:c1] = index.rescore_device(qd, cand)[0].cpu().numpy()
    return S


def build(X, ids=None):
    index = FlatIPIndex(X.shape[1])
    if ids is None:
        index.add(X)
    else:
        index.add_with_ids(X, ids)
    return index


@functools.lru_cache(maxsize=None)
def case(N, d):
    """(index, X, S) of the drifting chains of one shape: built and scored once, shared by the tests below and left unchanged."""
    X = drifting_chains(N, d)
    index = build(X)
    return index, X, self_scores(index)


def same(got, want, what=""):
    for g, w, name in zip(got, want, ("D", "I", "count")):
        assert g.dtype == w.dtype and g.shape == w.shape, f"{what} {name}: {g.dtype} {g.shape}, expected {w.dtype} {w.shape}"
        a, b = (g.view(np.uint32), w.view(np.uint32)) if name == "D" else (g, w)
        assert np.array_equal(a, b), f"{what} {name} differ in rows {np.unique(np.nonzero(a != b)[0])[:10]}"


def check(index, S, k, seg=None, threshold=None):
    got = neighbors.knn_graph(index, k, seg, threshold)
    want = neighbors.knn_graph_ref(S, k, seg.cpu().numpy() if isinstance(seg, torch.Tensor) else seg, threshold)
    same(got, want, f"k={k} threshold={threshold}")
    return want


@pytest.mark.parametrize("k", [1, 10, KMAX])
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("d", DS)
def test_every_shape_matches_the_definition(d, N, k):
    index, X, S = case(N, d)
    D, I, count = check(index, S, k)
    assert (count == min(k, N - 1)).all()
    if k > N - 1:
        assert (I[:, N - 1:] == -1).all() and (D[:, N - 1:] == LOWEST).all()
    assert (I[:, 0] != np.arange(N)).all()


def test_the_limits_are_the_librarys():
    assert neighbors.knn_max_k() == KMAX


@pytest.mark.parametrize("d", DS)
def test_threshold_is_strict(d):
    index, X, S = case(700, d)
    D0, I0, count0 = check(index, S, TOP)
    D7, I7, count7 = check(index, S, TOP, None, THRESHOLD)
    assert (D7[I7 >= 0] > np.float32(THRESHOLD)).all()
    some = int(((count7 > 0) & (count7 < TOP)).sum())
    print(f"d={d}: {some} rows with 0 < count < {TOP} at threshold {THRESHOLD}")
    assert some > 0
    # an attained score: the third best of a row whose second, third and fourth best differ
    j = int(np.flatnonzero((D0[:, 1] > D0[:, 2]) & (D0[:, 2] > D0[:, 3]))[0])
    hit, i = float(D0[j, 2]), int(I0[j, 2])
    assert S[j, i] == np.float32(hit)
    Dh, Ih, counth = check(index, S, TOP, None, hit)
    assert counth[j] == 2 and i not in Ih[j].tolist()                      # the pair at the threshold is out: the test is >
    below = float(np.nextafter(np.float32(hit), np.float32(-np.inf)))
    Db, Ib, countb = check(index, S, TOP, None, below)
    assert countb[j] >= 3 and Ib[j, 2] == i and countb.sum() > counth.sum()


def segment_rows():
    X = drifting_chains(100, 20, seed=2, lengths=(6, 25)).copy()
    X[0] = X[1]                          # row 0 lies in front of the first offset
    X[15] = X[16] = X[17] = X[14]        # identical rows in [1,15), [15,16), [16,17) and [17,19): the best neighbour lies across a boundary
    X[64] = X[63]                        # [19,64) | [64,65)
    X[90] = X[89]                        # [65,90) | past the last offset
    return X


@pytest.mark.parametrize("threshold", [None, THRESHOLD])
def test_segments(threshold):
    index = build(segment_rows())
    S = self_scores(index)
    D, I, count = check(index, S, TOP, SEGMENTS, threshold)
    check(index, S, TOP, torch.from_numpy(SEGMENTS).to(index.device), threshold)         # offsets already on the device
    for s in range(len(SEGMENTS) - 1):
        lo, hi = int(SEGMENTS[s]), int(SEGMENTS[s + 1])
        part = I[lo:hi]
        assert ((part == -1) | ((part >= lo) & (part < hi))).all()                       # no neighbour crosses a boundary
    alone = [0, 15, 16, 64] + list(range(90, 100))
    assert (count[alone] == 0).all() and not np.isin(I, alone).any()
    if threshold is None:
        assert (count[1:15] == TOP).all() and (count[17:19] == 1).all()
        free = neighbors.knn_graph(index, TOP)[1]
        assert free[14, 0] == 15 and free[63, 0] == 64 and free[0, 0] == 1              # they are neighbours without segments
    # one segment over everything is the call without segments
    same(neighbors.knn_graph(index, TOP, np.array([0, 100]), threshold), neighbors.knn_graph(index, TOP, None, threshold))
    check(index, S, KMAX, SEGMENTS, threshold)


@functools.lru_cache(maxsize=None)
def pieces_case():
    N = 2 * _ffi.call("ivr_knn_piece_rows") + 1
    index = build(drifting_chains(N, 20))
    return index, self_scores(index)


@pytest.mark.parametrize("segments", ["one", "two"])
def test_a_walk_of_several_pieces(segments):
    """2 piece_rows + 1 rows: a walk of three pieces as one segment; as two unequal segments the second walk starts inside the first
    segment's last tile and spans two pieces.  The smallest shape at which the merge across pieces can go wrong."""
    index, S = pieces_case()
    N = index.ntotal
    seg = None if segments == "one" else np.array([0, N // 4 + 5, N], np.int64)
    D, I, count = check(index, S, TOP, seg)
    assert (count == TOP).all()
    if seg is not None:
        assert (I[:seg[1]] < seg[1]).all() and (I[seg[1]:] >= seg[1]).all()


@pytest.mark.parametrize("k", [10, KMAX])
def test_identical_rows_give_the_lowest_other_rows(k):
    index = build(np.repeat(drifting_chains(1, 20), 257, axis=0))
    D, I, count = check(index, self_scores(index), k)
    for j in (0, 1, k - 1, k, k + 1, 256):
        assert I[j].tolist() == [i for i in range(k + 1) if i != j][:k]
    assert (D == D[0, 0]).all() and (count == k).all()


def test_repeated_calls_and_a_second_stream_give_the_same_output():
    index, X, S = case(700, 20)
    seg = torch.tensor([0, 300, 700], dtype=torch.int64, device=index.device)
    first = [t.clone() for t in neighbors.knn_graph_device(index, TOP, seg, THRESHOLD)]
    again = neighbors.knn_graph_device(index, TOP, seg, THRESHOLD)
    side = torch.cuda.Stream(device=index.device)
    side.wait_stream(torch.cuda.current_stream(index.device))
    with torch.cuda.stream(side):
        other = neighbors.knn_graph_device(index, TOP, seg, THRESHOLD)
    side.synchronize()
    for a, b, c in zip(first, again, other):
        assert torch.equal(a, b) and torch.equal(a, c)
    assert first[0].dtype == torch.float32 and first[1].dtype == torch.int64 and first[2].dtype == torch.int32
    assert all(t.is_cuda and t.device == index.device for t in first)
    assert first[0].shape == first[1].shape == (700, TOP) and first[2].shape == (700,)
    same([t.cpu().numpy() for t in first], neighbors.knn_graph_ref(S, TOP, seg.cpu().numpy(), THRESHOLD))


def test_id_mapped_index_gives_the_rows_of_a_plain_one():
    index, X, S = case(257, 20)
    mapped = build(X, np.random.default_rng(3).permutation(257).astype(np.int64) + 1000)
    for threshold in (None, THRESHOLD):
        same(neighbors.knn_graph(mapped, TOP, SEGMENTS, threshold), neighbors.knn_graph(index, TOP, SEGMENTS, threshold))
    assert neighbors.knn_graph(mapped, TOP)[1].max() < 257


def test_after_remove_ids_the_graph_is_that_of_the_surviving_rows():
    _, X, _ = case(257, 20)
    gone = np.random.default_rng(4).choice(257, 60, replace=False)
    keep = np.setdiff1d(np.arange(257), gone)
    index = build(X)
    assert index.remove_ids(gone.astype(np.int64)) == 60 and index.ntotal == 197
    fresh = build(np.ascontiguousarray(X[keep]))
    S = self_scores(fresh)
    for threshold in (None, THRESHOLD):
        want = check(fresh, S, TOP, None, threshold)
        same(neighbors.knn_graph(index, TOP, None, threshold), want)


@pytest.mark.parametrize("N,d", [(700, 512), (257, 20), (65, 512)])
def test_the_flat_search_finds_the_same_neighbours(N, d):
    """search_device returns exact float32 scores in the same key order: the list of row j with j taken out (or, where duplicates
    pushed j out of it, without its last entry) is row j of the graph."""
    index, X, S = case(N, d)
    D, I, count = neighbors.knn_graph(index, TOP)
    rows = torch.from_numpy(index.reconstruct_n()).to(index.device)
    Ds, Is = (t.cpu().numpy() for t in index.search_device(rows, TOP + 1))
    for j in range(N):
        keep = Is[j] != j
        if keep.all():
            keep[-1] = False
        assert I[j].tolist() == Is[j][keep].tolist(), f"row {j}"
        assert np.array_equal(D[j].view(np.uint32), Ds[j][keep].view(np.uint32)), f"row {j}"


def test_an_empty_index_and_bad_arguments():
    index = FlatIPIndex(20)
    D, I, count = neighbors.knn_graph(index, TOP)
    assert D.shape == (0, TOP) and I.shape == (0, TOP) and count.shape == (0,)
    assert D.dtype == np.float32 and I.dtype == np.int64 and count.dtype == np.int32
    assert neighbors.similarity_graphs(index, np.array([0, 0]), []) == {}
    with pytest.raises(ValueError, match=r"k=0 outside \[1,64\]"):
        neighbors.knn_graph(index, 0)
    with pytest.raises(ValueError, match=rf"k={KMAX + 1} outside \[1,64\]"):
        neighbors.knn_graph(index, KMAX + 1)
    with pytest.raises(ValueError, match="threshold=nan is NaN"):
        neighbors.knn_graph(index, TOP, None, float("nan"))
    out = [torch.zeros(1, dtype=t, device=index.device) for t in (torch.float32, torch.int64, torch.int32)]
    with pytest.raises(ValueError, match=r"k=0 outside \[1,64\]"):                        # the library's own check
        index._call("ivr_index_knn_graph", 0, None, 0, 0.7, *out)
    with pytest.raises(ValueError, match="NaN"):
        index._call("ivr_index_knn_graph", TOP, None, 0, float("nan"), *out)


def reference_by_folder(X, seg, keys):
    want, clear = {}, np.zeros(len(X), bool)
    for s in range(len(seg) - 1):
        lo, hi = int(seg[s]), int(seg[s + 1])
        want.update(search_ref.similarity_graph(X[lo:hi], keys[lo:hi], TOP, THRESHOLD))
        clear[lo:hi] = clear_rows(cosines64(X[lo:hi]), TOP, THRESHOLD, X.shape[1])
    return want, clear


@pytest.mark.parametrize("N,d,cuts", [(700, 512, (0, 300, 700)), (257, 20, (0, 257))])
def test_similarity_graphs_follow_the_reference_on_clear_rows(N, d, cuts):
    """similarity_graphs (the stored unit rows) and build_similarity_relationships (raw rows of any norm, normalised on the way in)
    against oracle.search_ref.similarity_graph in float64, folder by folder, on every clear row (knn_cases.clear_rows); at least
    75 % of the rows are clear.  A folder of one row is absent from the result, as in the reference."""
    index, X, S = case(N, d)
    seg = np.array(cuts, np.int64)
    keys = [f"frame_{r:04d}" for r in range(N)]
    want, clear = reference_by_folder(X, seg, keys)
    print(f"N={N} d={d}: {int(clear.sum())} of {N} rows clear")
    assert clear.sum() >= 0.75 * N
    got = neighbors.similarity_graphs(index, seg, keys)
    assert sorted(got) == keys
    raw = (X.astype(np.float64) * np.random.default_rng(12).uniform(0.5, 3.0, (N, 1))).astype(np.float32)
    folders = {f"folder{s}": (raw[seg[s]:seg[s + 1]], keys[seg[s]:seg[s + 1]]) for s in range(len(seg) - 1)}
    folders["single"] = (raw[:1], ["lonely"])
    built = neighbors.build_similarity_relationships(folders)
    assert sorted(built) == keys and "lonely" not in built
    want_raw, clear_raw = reference_by_folder(raw, seg, keys)
    short = 0
    for r in range(N):
        if clear[r]:
            assert got[keys[r]] == want[keys[r]], f"row {r}"
            short += 0 < len(want[keys[r]]) < TOP
        if clear_raw[r]:
            assert built[keys[r]] == want_raw[keys[r]], f"row {r} (raw)"
    assert short > 0
    # a one-row segment among the stored rows is absent too
    got1 = neighbors.similarity_graphs(index, np.array([0, 1, N]), keys)
    assert keys[0] not in got1 and len(got1) == N - 1
