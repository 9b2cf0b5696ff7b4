"""GPU suite of the diversified search (ivr_amd/diversify.py, csrc/search_diverse.hip): ivr_index_diversify against the numpy
definitions (mmr_ref / suppress_ref) fed with the scores FlatIPIndex.rescore_device reports: R for (query, row) and P for (stored row
as the query, row), the stored rows from reconstruct_batch.  Every comparison is exact: the labels element for element, D and M as
bit patterns."""
import numpy as np
import pytest
import torch

from diverse_cases import (FLT_MAX, bits, ends_early, k_values, lists_of, make_cand, make_queries, row_tie_decides, shot_rows, unit_rows)
from event_cases import make_rows
from ivr_amd import _ffi, diversify
from ivr_amd.index import FlatIPIndex
from ivr_amd.refine import refine_order_ref

pytestmark = pytest.mark.gpu

LAMBDAS = (0.0, 0.3, 0.5, 1.0)
BELOW, ABOVE = -2.0, 2.0                       # thresholds below and above every pair score of unit rows
_cases = {}


def score_table(index, x, normalize=False):
    """float32 [n,N]: the score of every (row of x as the query, stored row) from rescore_device, in blocks of at most 256 queries and
    2048 stored rows."""
    n, N = x.shape[0], index.ntotal
    S = np.empty((n, N), np.float32)
    for q0 in range(0, n, 256):
        qd = torch.from_numpy(np.ascontiguousarray(x[q0:q0 + 256])).to(index.device)
        for c0 in range(0, N, 2048):
            c1 = min(N, c0 + 2048)
            cand = torch.arange(c0, c1, dtype=torch.int64, device=index.device).repeat(len(qd), 1).contiguous()
            S[q0:q0 + 256, c0:c1] = index.rescore_device(qd, cand, normalize=normalize)[0].cpu().numpy()
    return S


def tables(index, x, ids=None, normalize=False):
    """(Rfull [nq,N], Pfull [N,N]): Pfull[i, j] is the score reported for (query = stored row i, row j)."""
    stored = index.reconstruct_batch(np.arange(index.ntotal) if ids is None else ids)
    return score_table(index, x, normalize), score_table(index, stored)


def make(d, N, seed, nq, period=None, unit=True):
    X = unit_rows(d, N, seed, period) if unit else make_rows(d, N, seed, period)
    index = FlatIPIndex(d)
    index.add(X)
    return index, X, make_queries(d, nq, seed)


def shared(d=20, N=300, seed=1, nq=33, period=37):
    """One index of duplicate unit rows with its score tables, built once for the tests that only read it."""
    key = (d, N, seed, nq, period)
    if key not in _cases:
        index, X, x = make(d, N, seed, nq, period)
        _cases[key] = (index, x) + tables(index, x)
    return _cases[key]


def check(index, x, cand, k, mode, param, Rfull, Pfull, ids=None, normalize=False):
    nq = cand.shape[0]
    cd = torch.from_numpy(cand).to(index.device)
    call, ref = (diversify.mmr_rerank, diversify.mmr_ref) if mode == "mmr" else (diversify.suppress_rerank, diversify.suppress_ref)
    D, I, M = call(index, x[:nq], cd, k, param, normalize=normalize)
    R, P = lists_of(Rfull[:nq], Pfull, cand)
    Dr, Ir, Mr = ref(R, P, cand, k, param, index.ntotal, ids)
    assert (D.dtype, I.dtype, M.dtype) == (np.float32, np.int64, np.float32) and D.shape == I.shape == M.shape == (nq, k)
    what = f"({mode} {param}, N={index.ntotal}, nq={nq}, kc={cand.shape[1]}, k={k})"
    assert np.array_equal(I, Ir), f"labels differ {what}"
    assert np.array_equal(bits(D), bits(Dr)), f"score bits differ {what}"
    assert np.array_equal(bits(M), bits(Mr)), f"redundancy bits differ {what}"
    return D, I, M


@pytest.mark.parametrize("kc", [1, 15, 16, 17, 64, 65, 256, 257, 2048])
def test_every_list_length_matches_the_definition(kc):
    # 1 .. 2048 candidates: across the group of 16, the wave, the switch of the block size (512) and the maximum; beyond 300 entries
    # the rows repeat; query 0 holds the three kinds of absent entry
    index, x, Rfull, Pfull = shared()
    nq = 3 if kc <= 257 else 1
    cand = make_cand(nq, kc, 300, 1, absent=True)
    for k in k_values(kc):
        whole = kc == _ffi.IVR_MAX_K and k == kc                   # 2,048 steps on the host: two parameters are enough
        for lam in (0.5,) if whole else LAMBDAS:
            check(index, x, cand, k, "mmr", lam, Rfull, Pfull)
        for thr in (0.95, ABOVE) if whole else (0.95, BELOW, ABOVE):
            D, I, M = check(index, x, cand, k, "suppress", thr, Rfull, Pfull)
            if thr == BELOW:
                assert (I[:, 0] >= 0).all() and (I[:, 1:] == -1).all()


@pytest.mark.parametrize("N", [1, 15, 16, 17, 65, 300])
def test_every_index_size_matches_the_definition(N):
    index, X, x = make(20, N, 2, 17, period=7 if N > 7 else None)
    Rfull, Pfull = tables(index, x)
    for kc in (1, 17, 65):
        cand = make_cand(17, kc, N, 2, absent=True)
        for k in k_values(kc):
            check(index, x, cand, k, "mmr", 0.3, Rfull, Pfull)
            check(index, x, cand, k, "mmr", 1.0, Rfull, Pfull)
            check(index, x, cand, k, "suppress", 0.95, Rfull, Pfull)


@pytest.mark.parametrize("d", [20, 512])
@pytest.mark.parametrize("nq", [1, 17, 33])
def test_dimensions_and_query_counts(d, nq):
    index, x, Rfull, Pfull = shared(d=d)
    cand = make_cand(nq, 65, 300, 3, absent=True)
    for k in (10, 65):
        for lam in LAMBDAS:
            check(index, x, cand, k, "mmr", lam, Rfull, Pfull)
        check(index, x, cand, k, "suppress", 0.95, Rfull, Pfull)


def test_the_cases_are_not_vacuous():
    # per mode a result that is not the relevance order, a step the row tie-break decides, a suppress query that ends early
    index, x, Rfull, Pfull = shared()
    mmr_differs = sup_differs = tie = early = False
    for kc in (17, 64, 257):
        cand = make_cand(3, kc, 300, 1)
        k = min(kc, 10)
        plain = refine_order_ref(lists_of(Rfull[:3], Pfull, cand)[0], cand, k, 300)[1]
        mmr_differs |= not np.array_equal(check(index, x, cand, k, "mmr", 0.3, Rfull, Pfull)[1], plain)
        D, I, M = check(index, x, cand, kc, "suppress", 0.95, Rfull, Pfull)
        sup_differs |= not np.array_equal(I[:, :k], plain)
        early |= ends_early(I)
        D, I, M = check(index, x, cand, k, "mmr", 1.0, Rfull, Pfull)
        tie |= row_tie_decides(I, D)
    assert mmr_differs and sup_differs and tie and early


def test_a_run_of_near_duplicates_gives_one_hit_per_shot():
    X = shot_rows(20, 12, 8, 2)                                     # 12 shots of 8 rows: a unit row + 1e-3 * noise
    index = FlatIPIndex(20)
    index.add(X)
    x = make_queries(20, 3, 2)
    Rfull, Pfull = tables(index, x)
    cand = make_cand(3, 64, 96, 2)
    D, I, M = check(index, x, cand, 64, "suppress", 0.95, Rfull, Pfull)
    assert ends_early(I) and ((I >= 0).sum(axis=1) == 12).all()
    assert all(len({int(r) // 8 for r in row[:12]}) == 12 for row in I)
    D, I, M = check(index, x, cand, 8, "mmr", 0.5, Rfull, Pfull)
    plain = refine_order_ref(lists_of(Rfull, Pfull, cand)[0], cand, 8, 96)[1]
    assert len({int(r) // 8 for r in I[0]}) > len({int(r) // 8 for r in plain[0]})
    assert (M[:, 1:] < 0.95).any() and (M[:, 0] == -FLT_MAX).all()


@pytest.mark.parametrize("k", [1, 10])
def test_lambda_one_through_mmr_search_is_the_flat_search(k):
    index, x, Rfull, Pfull = shared()
    Ds, Is = index.search(x[:17], k)
    for fetch_k in (k, 50, 300, 400):                               # 400 > ntotal: the search pads its labels with -1
        D, I, M = diversify.mmr_search(index, x[:17], k, fetch_k, 1.0)
        assert np.array_equal(I, Is) and np.array_equal(bits(D), bits(np.asarray(Ds, np.float32))), f"fetch_k={fetch_k}"
        D, I, M = diversify.dedup_search(index, x[:17], k, fetch_k, threshold=float("inf"))
        assert np.array_equal(I, Is) and np.array_equal(bits(D), bits(np.asarray(Ds, np.float32))), f"fetch_k={fetch_k}"


def test_search_then_rerank_is_the_definition_over_the_search_labels():
    index, x, Rfull, Pfull = shared()
    cand = index.search(x[:17], 50)[1]
    R, P = lists_of(Rfull[:17], Pfull, cand)
    for got, want in ((diversify.mmr_search(index, x[:17], 10, 50, 0.3), diversify.mmr_ref(R, P, cand, 10, 0.3, 300)),
                      (diversify.dedup_search(index, x[:17], 10, 50), diversify.suppress_ref(R, P, cand, 10, 0.95, 300))):
        assert np.array_equal(got[1], want[1]) and np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(bits(got[2]), bits(want[2]))
    # the default threshold drops the exact duplicates the plain search returns side by side
    plain = index.search(x[:17], 10)[1]
    assert not np.array_equal(diversify.dedup_search(index, x[:17], 10, 50)[1], plain)


def test_absent_entries_and_rows_named_twice():
    index, x, Rfull, Pfull = shared()
    cand = np.array([[5, -1, 5, 300, 42, 2**40, 5 + 37, 9, -7, -1],         # row 5 twice and its duplicate row 42 twice
                     [-1, 300, 2**40, -5, 301, -1, -1, 2**62, -1, -1]], np.int64)     # nothing present
    for k in (1, 4, 10):
        for lam in LAMBDAS:
            D, I, M = check(index, x, cand, k, "mmr", lam, Rfull, Pfull)
            assert (I[1] == -1).all() and (D[1] == -FLT_MAX).all() and (M[1] == -FLT_MAX).all()
        for thr in (0.95, BELOW, ABOVE):
            check(index, x, cand, k, "suppress", thr, Rfull, Pfull)
    D, I, M = check(index, x, cand, 10, "mmr", 1.0, Rfull, Pfull)
    assert sorted(I[0, :5].tolist()) == [5, 5, 9, 42, 42] and (I[0, 5:] == -1).all()
    at = I[0].tolist().index(5)
    assert I[0, at + 1] == 5 and I[0, at + 2] == 42 and I[0, at + 3] == 42     # equal scores: the lower row, then the position
    assert bits(D[0, at]) == bits(D[0, at + 3])
    D, I, M = check(index, x, cand, 10, "suppress", 0.95, Rfull, Pfull)
    assert I[0, 2] == -1 and {int(I[0, 0]), int(I[0, 1])} == {5, 9}              # one of the four mentions survives


def test_m_may_be_null():
    index, x, Rfull, Pfull = shared()
    cand = torch.from_numpy(make_cand(3, 65, 300, 4)).to(index.device)
    xd = torch.from_numpy(x[:3]).to(index.device)
    for mode, param in ((diversify.MMR, 0.5), (diversify.SUPPRESS, 0.95)):
        D = torch.zeros((3, 65), dtype=torch.float32, device=index.device)
        I = torch.zeros((3, 65), dtype=torch.int64, device=index.device)
        index._call("ivr_index_diversify", xd, 3, cand, 65, 65, mode, param, False, D, I, None)
        call = diversify.mmr_rerank_device if mode == diversify.MMR else diversify.suppress_rerank_device
        Dm, Im, Mm = call(index, xd, cand, 65, param)
        assert torch.equal(I, Im) and torch.equal(D.view(torch.int32), Dm.view(torch.int32))


def test_normalised_queries():
    index, X, x = make(20, 300, 5, 17, period=37, unit=False)      # rows of length ~ sqrt(20): pair scores far above 1
    Rfull, Pfull = tables(index, x, normalize=True)
    assert np.abs(Rfull).max() < np.abs(score_table(index, x[:1])).max()      # the queries were scaled down to unit length
    cand = make_cand(17, 65, 300, 5, absent=True)
    for k in (10, 65):
        check(index, x, cand, k, "mmr", 0.3, Rfull, Pfull, normalize=True)
        check(index, x, cand, k, "suppress", 15.0, Rfull, Pfull, normalize=True)
    D, I, M = diversify.mmr_search(index, x, 10, 50, 1.0, normalize=True)
    Ds, Is = index.search_device(torch.from_numpy(x).to(index.device), 10, normalize=True)
    assert np.array_equal(I, Is.cpu().numpy()) and np.array_equal(bits(D), bits(Ds.cpu().numpy()))


def test_id_mapped_index_labels_by_id_and_takes_positions():
    rng = np.random.default_rng(6)
    N = 300
    X = unit_rows(20, N, 6, period=37)
    ids = rng.permutation(N).astype(np.int64) * 3 + 1000
    index = FlatIPIndex(20)
    index.add_with_ids(X, ids)
    x = make_queries(20, 17, 6)
    Rfull, Pfull = tables(index, x, ids=ids)
    cand = make_cand(17, 65, N, 6, absent=True)                     # positions, although the index labels by id
    for k in (10, 65):
        D, I, M = check(index, x, cand, k, "mmr", 0.3, Rfull, Pfull, ids=ids)
        assert (I[I >= 0] >= 1000).all()
        check(index, x, cand, k, "suppress", 0.95, Rfull, Pfull, ids=ids)
    # through the search: its labels are stored ids, turned back into rows on the device
    row_of = {int(v): r for r, v in enumerate(ids)}
    labels = index.search(x, 50)[1]
    rows = np.vectorize(row_of.get)(labels).astype(np.int64)
    R, P = lists_of(Rfull, Pfull, rows)
    D, I, M = diversify.mmr_search(index, x, 10, 50, 0.3)
    Dr, Ir, Mr = diversify.mmr_ref(R, P, rows, 10, 0.3, N, ids)
    assert np.array_equal(I, Ir) and np.array_equal(bits(D), bits(Dr)) and np.array_equal(bits(M), bits(Mr))


def test_an_empty_index_gives_unused_slots_only():
    empty = FlatIPIndex(20)
    x = make_queries(20, 3, 7)
    cand = torch.from_numpy(make_cand(3, 17, 300, 7)).to(empty.device)
    for out in (diversify.mmr_rerank(empty, x, cand, 5, 0.5), diversify.suppress_rerank(empty, x, cand, 17, 0.95),
                diversify.mmr_search(empty, x, 4, 10), diversify.dedup_search(empty, x, 4, 10)):
        D, I, M = out
        assert (I == -1).all() and (D == -FLT_MAX).all() and (M == -FLT_MAX).all()


def test_side_stream_and_repeat_calls_agree():
    index, x, Rfull, Pfull = shared()
    xd = torch.from_numpy(x[:17]).to(index.device)
    cand = torch.from_numpy(make_cand(17, 600, 300, 8)).to(index.device)       # the 1,024-thread block
    first = [t.clone() for t in diversify.mmr_rerank_device(index, xd, cand, 40, 0.3)]
    again = diversify.mmr_rerank_device(index, xd, cand, 40, 0.3)
    side = torch.cuda.Stream(device=index.device)
    side.wait_stream(torch.cuda.current_stream(index.device))
    with torch.cuda.stream(side):
        other = diversify.mmr_rerank_device(index, xd, cand, 40, 0.3)
        searched = diversify.dedup_search_device(index, xd, 10, 50)
    side.synchronize()
    for a, b, c in zip(first, again, other):
        assert torch.equal(a, b) and torch.equal(a, c)
    host = cand.cpu().numpy()
    check(index, x, host, 40, "mmr", 0.3, Rfull, Pfull)
    D, I, M = diversify.dedup_search(index, x[:17], 10, 50)
    assert np.array_equal(searched[1].cpu().numpy(), I) and np.array_equal(bits(searched[0].cpu().numpy()), bits(D))


def test_library_rejects_arguments_outside_the_ranges():
    index, x, Rfull, Pfull = shared()
    dev = index.device
    q = torch.from_numpy(x[:2]).to(dev)
    cand = torch.zeros((2, 4), dtype=torch.int64, device=dev)
    D = torch.zeros((2, 2), dtype=torch.float32, device=dev)
    I = torch.zeros((2, 2), dtype=torch.int64, device=dev)

    def call(nq=2, kc=4, k=2, mode=0, param=0.5, q=q, cand=cand, D=D, I=I):
        index._call("ivr_index_diversify", q, nq, cand, kc, k, mode, param, False, D, I, None)

    call()                                                         # the arguments in range pass
    call(mode=1, param=-3.0)                                       # a threshold is any number
    for bad, text in [(dict(kc=0, k=1), "kc=0"), (dict(kc=2049), "kc=2049"), (dict(k=0), "k=0"), (dict(k=5), "k=5"), (dict(mode=2), "mode=2"),
                      (dict(param=-0.1), "lambda=-0.1"), (dict(param=1.5), "lambda=1.5"), (dict(param=float("nan")), "param=nan"),
                      (dict(nq=0), "nq=0"), (dict(q=None), "NULL"), (dict(cand=None), "NULL"), (dict(D=None), "NULL"), (dict(I=None), "NULL")]:
        with pytest.raises(ValueError, match=text):
            call(**bad)


def test_pair_scores_are_symmetric_to_the_bit_on_this_case():
    # the definition names the direction (the chosen row is the query) and does not rely on this; DESIGN.md records the outcome
    index, x, Rfull, Pfull = shared(d=512)
    differing = int((bits(Pfull) != bits(Pfull.T)).sum())
    print(f"pair scores with P[i,j] != P[j,i] as bit patterns: {differing} of {Pfull.size}")
    assert differing == 0


def test_retriever_returns_the_frames_of_mmr_search():
    from ivr_amd.compat import FAISSRetriever, KeyframeMetadata
    feats = shot_rows(32, 6, 5, 9, noise=1e-2)                     # 6 shots of 5 near-duplicate frames
    query = feats[7] + 0.3 * make_queries(32, 1, 9)[0] / np.sqrt(32.0)
    metas = [KeyframeMetadata(folder_name=f"L01_V{i // 5:03d}", image_name=f"{i % 5:03d}.jpg", frame_id=i % 5, file_path=f"/k/{i}.jpg",
                              clip_features=feats[i]) for i in range(len(feats))]
    r = FAISSRetriever()
    r.build_index(feats, metas)
    results = r.search_diverse(query, k=4, fetch_k=20, lambda_mult=0.3)
    D, I, M = diversify.mmr_search(r.index, r._normalize_and_validate_features(query), 4, 20, 0.3)
    assert [r.metadata_to_id[res.metadata.get_unique_key()] for res in results] == I[0].tolist()
    assert [res.rank for res in results] == [1, 2, 3, 4]
    assert results[0].metadata.get_unique_key() == r.search(query, k=1)[0].metadata.get_unique_key()
    assert len({res.metadata.folder_name for res in results}) > len({res.metadata.folder_name for res in r.search(query, k=4)})
    same = r.search_diverse(query, k=4, fetch_k=20, lambda_mult=1.0)
    assert [res.metadata.get_unique_key() for res in same] == [res.metadata.get_unique_key() for res in r.search(query, k=4)]
    with pytest.raises(ValueError, match="lambda_mult=1.5"):
        r.search_diverse(query, lambda_mult=1.5)
