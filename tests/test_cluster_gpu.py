"""GPU suite of the frame clustering (ivr_amd/cluster.py, csrc/cluster.hip): labels, core bytes and cluster counts of ivr_index_dbscan
for exact equality with the numpy definition dbscan_ref fed with the scores FlatIPIndex.rescore_device reports for the stored rows as
queries; then the representative step against its numpy restatement and the float64 reference, and cluster_similar_frames against
the reference's lists."""
import functools

import numpy as np
import pytest
import torch

from cluster_cases import (DS, EPS, MIN_SAMPLES, NS, SEGMENTS, border_and_noise, clear_winner, contested_border, distances64,
                           drifting_chains, one_chain, reference_cluster_similar_frames, reference_representative)
from ivr_amd import cluster
from ivr_amd.index import FlatIPIndex
from oracle.reduce_ref import flat_score_bound

pytestmark = pytest.mark.gpu


def self_scores(index):
    """S float32 [N,N]: the score of every (stored row as the query, stored row) from rescore_device, in column blocks of at most
    2048 rows (the frame_scores helper of test_temporal_gpu.py with the reconstructed rows as the frames)."""
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


def check(index, S, eps, min_samples, seg=None):
    got = cluster.dbscan(index, eps, min_samples, seg)
    want = cluster.dbscan_ref(S, eps, min_samples, seg.cpu().numpy() if isinstance(seg, torch.Tensor) else seg)
    for g, w, what in zip(got, want, ("labels", "core", "nclusters")):
        assert g.dtype == w.dtype and g.shape == w.shape, f"{what}: {g.dtype} {g.shape}, expected {w.dtype} {w.shape}"
        assert np.array_equal(g, w), f"{what} differ (eps={eps}, min_samples={min_samples}): rows {np.flatnonzero(g != w)[:10]}"
    return want


def attained_eps(S, near):
    """The float32 distance 1 - S[j, i] of a pair i < j that lies closest to `near`: the `<=` of the edge test decides that pair."""
    j, i = np.tril_indices(len(S), -1)
    dist = np.float32(1) - S[j, i]
    return float(dist[np.argmin(np.abs(dist - np.float32(near)))])


@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("d", DS)
def test_every_shape_matches_the_definition(d, N):
    index, X, S = case(N, d)
    eps_hit = attained_eps(S, 0.03)
    j, i = np.tril_indices(N, -1)
    dist = np.float32(1) - S[j, i]
    below = np.nextafter(np.float32(eps_hit), np.float32(0))
    assert (dist <= np.float32(eps_hit)).sum() > (dist <= below).sum()        # the pair at eps is an edge only because the test is <=
    border = noise = 0
    for eps in (EPS, eps_hit):
        for min_samples in MIN_SAMPLES:
            labels, core, ncl = check(index, S, eps, min_samples)
            b, n = border_and_noise(labels, core)
            border, noise = border + b, noise + n
    assert noise > 0 and (border > 0 or N < 3)           # a border row needs a core row with two neighbours: three rows at least
    if N == 700:
        assert check(index, S, EPS, 2)[2][0] >= 20       # tens of clusters


@pytest.mark.parametrize("min_samples", MIN_SAMPLES)
def test_segments(min_samples):
    X = drifting_chains(100, 20, seed=2, lengths=(6, 25)).copy()
    X[0] = X[1]                          # row 0 lies in front of the first offset
    X[15] = X[16] = X[17] = X[14]        # identical rows in [1,15), [15,16), [16,17) and [17,19): no edge crosses a boundary
    X[64] = X[63]                        # [19,64) | [64,65)
    X[90] = X[89]                        # [65,90) | past the last offset
    index = build(X)
    S = self_scores(index)
    labels, core, ncl = check(index, S, EPS, min_samples, SEGMENTS)
    check(index, S, EPS, min_samples, torch.from_numpy(SEGMENTS).to(index.device))       # offsets already on the device
    assert ncl.shape == (8,)
    assert (labels[[0]] == -1).all() and (labels[90:] == -1).all() and not core[[0]].any() and not core[90:].any()
    if min_samples >= 2:
        assert (labels[[15, 16, 64]] == -1).all()        # a segment of one row never has a neighbour
    if min_samples == 2:
        free = cluster.dbscan(index, EPS, min_samples)[0]
        assert free[15] == free[16] == free[14] >= 0 and free[64] == free[63] >= 0 and free[0] == free[1] >= 0       # they do join without segments
    # numbering restarts in every segment
    for s in range(8):
        part = labels[SEGMENTS[s]:SEGMENTS[s + 1]]
        assert sorted(set(part[part >= 0].tolist())) == list(range(ncl[s]))
    assert (ncl > 0).sum() >= (3 if min_samples <= 3 else 2)
    # one segment over everything is the call without segments
    a = cluster.dbscan(index, EPS, min_samples)
    b = cluster.dbscan(index, EPS, min_samples, np.array([0, 100]))
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("order", ["sorted", "reversed", "permuted"])
def test_one_long_chain_is_one_cluster(order):
    X = one_chain(700, 40)
    p = {"sorted": np.arange(700), "reversed": np.arange(700)[::-1], "permuted": np.random.default_rng(9).permutation(700)}[order]
    index = build(np.ascontiguousarray(X[p]))
    S = self_scores(index)
    j, i = np.tril_indices(700, -1)
    assert ((np.float32(1) - S[j, i]) <= np.float32(EPS)).sum() == 699       # every row reaches its predecessor and successor only
    labels, core, ncl = check(index, S, EPS, 2)
    assert (labels == 0).all() and core.all() and ncl.tolist() == [1]
    labels, core, ncl = check(index, S, EPS, 3)            # the two ends are border rows of the one cluster
    assert (labels == 0).all() and core.sum() == 698 and ncl.tolist() == [1]
    assert (check(index, S, EPS, 4)[0] == -1).all()


def test_identical_rows_are_one_cluster_whatever_the_contention():
    X = np.repeat(drifting_chains(1, 20), 257, axis=0)
    index = build(X)
    S = self_scores(index)
    for min_samples, all_core in ((2, True), (257, True), (258, False)):
        labels, core, ncl = check(index, S, EPS, min_samples)
        assert core.all() == all_core and core.any() == all_core
        assert (labels == (0 if all_core else -1)).all() and ncl.tolist() == [int(all_core)]


def test_contested_border_row_takes_the_lower_root():
    X = contested_border()
    rng = np.random.default_rng(5)
    seen = set()
    for p in [np.arange(9), np.arange(9)[::-1]] + [rng.permutation(9) for _ in range(16)]:
        index = build(np.ascontiguousarray(X[p]))
        labels, core, ncl = check(index, self_scores(index), EPS, 4)
        mid = int(np.flatnonzero(p == 4)[0])
        first = int(np.flatnonzero(core)[0])
        assert core[mid] == 0 and core.sum() == 8 and ncl.tolist() == [2] and labels[mid] == labels[first] == 0
        seen.add(bool(p[first] < 4))
        index.close()
    assert seen == {True, False}


def test_repeated_calls_and_a_second_stream_give_the_same_output():
    index, X, S = case(700, 20)
    seg = torch.tensor([0, 300, 700], dtype=torch.int64, device=index.device)
    first = [t.clone() for t in cluster.dbscan_device(index, EPS, 3, seg)]
    again = cluster.dbscan_device(index, EPS, 3, seg)
    side = torch.cuda.Stream(device=index.device)
    side.wait_stream(torch.cuda.current_stream(index.device))
    with torch.cuda.stream(side):
        other = cluster.dbscan_device(index, EPS, 3, seg)
    side.synchronize()
    for a, b, c in zip(first, again, other):
        assert torch.equal(a, b) and torch.equal(a, c)
    assert first[0].dtype == torch.int32 and first[1].dtype == torch.uint8 and first[2].dtype == torch.int32 and first[0].is_cuda


def test_id_mapped_index_gives_the_labels_of_a_plain_one():
    index, X, S = case(257, 20)
    mapped = build(X, np.random.default_rng(3).permutation(257).astype(np.int64) + 1000)
    for min_samples in (2, 3):
        a = cluster.dbscan(index, EPS, min_samples, SEGMENTS)
        b = cluster.dbscan(mapped, EPS, min_samples, SEGMENTS)
        assert all(np.array_equal(x, y) for x, y in zip(a, b))


def test_after_remove_ids_the_labels_are_those_of_the_surviving_rows():
    _, X, _ = case(257, 20)
    gone = np.random.default_rng(4).choice(257, 60, replace=False)
    keep = np.setdiff1d(np.arange(257), gone)
    index = build(X)
    assert index.remove_ids(gone.astype(np.int64)) == 60 and index.ntotal == 197
    fresh = build(np.ascontiguousarray(X[keep]))
    S = self_scores(fresh)
    for min_samples in (2, 3):
        want = check(fresh, S, EPS, min_samples)
        got = cluster.dbscan(index, EPS, min_samples)
        assert all(np.array_equal(x, y) for x, y in zip(got, want))


def test_an_empty_index_succeeds_and_writes_nothing():
    index = FlatIPIndex(20)
    labels, core, ncl = cluster.dbscan(index, EPS, 2)
    assert labels.shape == (0,) and core.shape == (0,) and ncl.tolist() == [0]
    with pytest.raises(ValueError, match="eps"):
        index._call("ivr_index_dbscan", -1.0, 2, None, 0, torch.zeros(1, dtype=torch.int32, device=index.device),
                    torch.zeros(1, dtype=torch.uint8, device=index.device), torch.zeros(1, dtype=torch.int32, device=index.device))


@pytest.mark.parametrize("N,d", [(700, 20), (700, 512), (257, 512)])
def test_representatives_match_the_restatement_and_the_reference(N, d):
    """select_representatives equals representatives_ref exactly, and the float64 restatement of the reference's mean-then-argmax
    wherever the best two cosines of a cluster differ by more than flat_score_bound.  The inputs are the drifting chains clustered
    with min_samples = 3, so that every cluster has three rows at least (the two rows of a pair tie by symmetry); at least 90 % of
    their clusters are that clear (tests/test_cluster_cpu.py checks the same on the CPU)."""
    index, X, S = case(N, d)
    seg = np.array([0, 100, 100, 257], np.int64) if N == 257 else None          # cluster numbers that restart, an empty segment
    labels, core, ncl = cluster.dbscan_device(index, EPS, 3, seg)
    off, members = cluster.cluster_members(labels, ncl, seg)
    reps = cluster.select_representatives(index, off, members).cpu().numpy()
    off, members = off.cpu().numpy(), members.cpu().numpy()
    assert len(off) - 1 == int(ncl.sum()) >= 3 and len(members) == int((labels >= 0).sum())
    assert np.array_equal(reps, cluster.representatives_ref(index.reconstruct_n(), off, members))
    clear = 0
    for c in range(len(off) - 1):
        m, gaps = members[off[c]:off[c + 1]].tolist(), []
        want = reference_representative(m, X, gaps)
        if clear_winner(gaps[0], d):
            clear += 1
            assert reps[c] == want
    assert clear >= 0.9 * (len(off) - 1), f"{clear} of {len(off) - 1} clusters have a clear winner"


def test_segment_best_cosine_ties_and_empty_runs():
    from ivr_amd import _ffi
    dev = torch.device("cuda", torch.cuda.current_device())
    e = torch.eye(4, device=dev)
    rows = torch.stack([e[1], e[0], e[0], e[2], torch.zeros(4, device=dev), e[0], e[0], e[0], e[0], e[0]]).contiguous()
    off = torch.tensor([0, 3, 3, 5, 10, 12], dtype=torch.int64, device=dev)          # [0,3) [3,3) empty [3,5) [5,10) ties across waves, [10,12) clipped to nothing
    centers = torch.stack([e[0], e[0], e[3], e[0], e[0]]).contiguous()
    best = torch.empty(5, dtype=torch.int64, device=dev)
    score = torch.empty(5, dtype=torch.float32, device=dev)
    _ffi.call("ivr_segment_best_cosine", _ffi.CTX, rows, 10, off, 5, 4, centers, best, score, device=dev)
    lowest = float(-np.finfo(np.float32).max)
    assert best.tolist() == [1, -1, 3, 5, -1] and score.tolist() == [1.0, lowest, 0.0, 1.0, lowest]


def test_cluster_similar_frames_returns_the_reference_lists():
    rng = np.random.default_rng(11)
    X = drifting_chains(65, 512, seed=2).astype(np.float64) * rng.uniform(0.5, 3.0, (65, 1))      # raw embeddings: any norm
    emb = list(X.astype(np.float32))
    D = distances64(np.asarray(emb))
    assert np.abs(D[np.triu_indices(65, 1)] - EPS).min() > flat_score_bound(512, 1.0), "seed puts a distance within the score bound of eps"
    want = reference_cluster_similar_frames(emb)
    assert len(want) >= 3 and sum(len(c) for c in want) == 65
    got = cluster.cluster_similar_frames(emb, list(range(65)))
    assert got == want
    noise = [c for c in want if not (D[np.ix_(c, c)] + np.eye(len(c)) <= EPS).any()][0]              # the list of the -1 label
    assert len(noise) >= 2
    # every list gets a representative, the noise list included
    for c in want:
        gaps = []
        ref = reference_representative(c, np.asarray(emb), gaps)
        rep = cluster.select_representative_frame(c, np.asarray(emb))
        assert rep in c
        if len(c) == 1 or clear_winner(gaps[0], 512):
            assert rep == ref
    assert cluster.cluster_similar_frames(emb[:1]) == [[0]] and cluster.cluster_similar_frames([]) == []
