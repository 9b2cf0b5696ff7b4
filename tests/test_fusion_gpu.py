"""GPU suite of the fused search (ivr_amd/fusion.py, csrc/search_fused.hip): both calls against the numpy definitions
(fused_search_ref / fused_range_search_ref) fed with the member scores FlatIPIndex.rescore_device reports, and against the flat
search.  Every comparison is exact: the rows element for element, the scores as bit patterns."""
import numpy as np
import pytest
import torch

from fusion_cases import COMBINES, FLT_MAX, FOLDS, bits, f32, make_mask, make_members, make_rows, make_weights, pad_pow2
from ivr_amd import _ffi, fusion
from ivr_amd.index import FlatIPIndex

pytestmark = pytest.mark.gpu


def member_scores(index, Q, normalize=False):
    """S float32 [nq,slots,N]: the score of every (member, stored row) from rescore_device, in column blocks of at most 2048 rows."""
    nq, slots, d = Q.shape
    N = index.ntotal
    qd = torch.from_numpy(np.ascontiguousarray(Q.reshape(nq * slots, d))).to(index.device)
    S = np.empty((nq * slots, N), np.float32)
    for c0 in range(0, N, 2048):
        c1 = min(N, c0 + 2048)
        cand = torch.arange(c0, c1, dtype=torch.int64, device=index.device).repeat(nq * slots, 1).contiguous()
        S[:, c0:c1] = index.rescore_device(qd, cand, normalize=normalize)[0].cpu().numpy()
    return S.reshape(nq, slots, N)


def make_index(d, N, seed, period=None, ids=None):
    X = make_rows(d, N, seed, period)
    index = FlatIPIndex(d)
    if ids is None:
        index.add(X)
    else:
        index.add_with_ids(X, ids)
    return index, X


def thresholds(F):
    """A threshold inside the scores (the median of query 0) and one that is a score itself: the >= of the range form."""
    return float(np.median(F[0])), float(F[0, 0] + f32(0.0))


def check(index, S, k, fold, combine, ids=None, normalize=False, ranges=True, **args):
    """fused_search and fused_range_search with **args against the definitions on S (slot order); returns (D, I)."""
    W, R = fusion.fused_tables(**args)
    S = S[:R.shape[0], :R.shape[1]]
    what = f"(N={S.shape[2]}, nq={S.shape[0]}, slots={S.shape[1]}, k={k}, {fold}, {combine})"
    D, I = fusion.fused_search(index, k=k, fold=fold, combine=combine, normalize=normalize, **args)
    Dr, Ir = fusion.fused_search_ref(S, W, R, k, fold, combine, ids)
    assert D.dtype == np.float32 and I.dtype == np.int64 and D.shape == Dr.shape and I.shape == Ir.shape
    assert np.array_equal(I, Ir), f"rows differ {what}"
    assert np.array_equal(bits(D), bits(Dr)), f"score bits differ {what}"
    if ranges:
        F = fusion.fused_scores_ref(S, W, R, fold, combine)
        for thr in thresholds(F):
            lims, Dg, Ig = fusion.fused_range_search(index, threshold=thr, fold=fold, combine=combine, normalize=normalize, **args)
            lr, Dgr, Igr = fusion.fused_range_search_ref(S, W, R, thr, fold, combine, ids)
            assert lims.dtype == np.int64 and np.array_equal(lims, lr), f"lims differ {what}"
            assert np.array_equal(Ig, Igr) and np.array_equal(bits(Dg), bits(Dgr)), f"range results differ {what}"
            assert lims[-1] > 0
    return D, I


@pytest.mark.parametrize("N", [1, 15, 16, 17, 63, 64, 65, 1023, 1024, 1025, 2051])
def test_every_edge_of_the_row_walk(N):
    d, nq = 20, 2
    index, X = make_index(d, N, 1)
    P, Ng = make_members(d, nq, 3, 1), make_members(d, nq, 1, 2)
    S = member_scores(index, np.concatenate([P, Ng], axis=1))
    # k > N wherever IVR_MAX_K allows one; at N = 2051 the largest k there is
    for k in (1, 10, min(N + 5, _ffi.IVR_MAX_K)):
        for fold in FOLDS:
            for combine in COMBINES:
                D, I = check(index, S, k, fold, combine, ranges=k == 10, positives=P, negatives=Ng)
                assert (I[:, min(k, N):] == -1).all() and (D[:, min(k, N):] == -FLT_MAX).all() and (I[:, :min(k, N)] >= 0).all()


@pytest.mark.parametrize("d", [20, 512])
@pytest.mark.parametrize("normalize", [False, True])
def test_every_set_width_and_a_ragged_tile(d, normalize):
    N, nmax = 1100, 65
    index, X = make_index(d, N, 2)
    modes = [(f, c) for f in FOLDS for c in COMBINES]
    seen = set()
    for i, width in enumerate((1, 2, 3, 5, 8, 9, 16)):
        mn = width // 3                                            # 0, 0, 1, 1, 2, 3, 5 negative members
        m = width - mn
        sp = pad_pow2(width)
        seen.add(sp)
        P, Ng = make_members(d, nmax, m, 3), (make_members(d, nmax, mn, 4) if mn else None)
        S = member_scores(index, P if Ng is None else np.concatenate([P, Ng], axis=1), normalize)
        Wp, Wn = make_weights(nmax, m, 5), (make_weights(nmax, mn, 6) if mn else None)
        mask = make_mask(nmax, m, 7)                               # absent slots first, last and in the middle
        for j, nq in enumerate((1, 16 // sp, 16 // sp + 1, nmax)):
            fold, combine = modes[(i + j) % len(modes)]
            args = dict(positives=P[:nq], weights=Wp[:nq], mask=mask[:nq])
            if mn:
                args.update(negatives=Ng[:nq], negative_weights=Wn[:nq])
            check(index, S, 10, fold, combine, normalize=normalize, **args)
        # the list form: set q keeps its first 1 + q % m positive members, the padding is absent
        nq = 16 // sp + 1
        counts = [1 + q % m for q in range(nq)]
        args = dict(positives=[P[q, :c] for q, c in enumerate(counts)], weights=[Wp[q, :c] for q, c in enumerate(counts)])
        if mn:
            args.update(negatives=[Ng[q] for q in range(nq)], negative_weights=[Wn[q] for q in range(nq)])
        W, R = fusion.fused_tables(**args)
        assert R.shape == (nq, max(counts) + mn) and [int((r > 0).sum()) for r in R] == counts
        Sl = np.concatenate([S[:nq, :max(counts)], S[:nq, m:]], axis=1)
        check(index, Sl, 10, *modes[i % len(modes)], normalize=normalize, **args)
    assert seen == {1, 2, 4, 8, 16}


@pytest.mark.parametrize("nq", [1, 17])
def test_singleton_sets_with_weight_one_are_the_flat_search(nq):
    d, N, k = 20, 2051, 10
    index, X = make_index(d, N, 3)
    x = make_members(d, nq, 1, 8)
    Ds, Is = index.search(x[:, 0], k)
    for fold in FOLDS:
        D, I = fusion.fused_search(index, x, k, fold=fold)
        assert np.array_equal(I, Is) and np.array_equal(bits(D), bits(np.asarray(Ds, np.float32)))


def test_explain_holds_the_member_scores_and_folds_back_to_the_result():
    d, N, nq, k = 20, 700, 5, 12
    index, X = make_index(d, N, 4)
    P, Ng = make_members(d, nq, 3, 9), make_members(d, nq, 2, 10)
    mask = make_mask(nq, 3, 11)
    Wp, Wn = make_weights(nq, 3, 12), make_weights(nq, 2, 13)
    args = dict(positives=P, weights=Wp, negatives=Ng, negative_weights=Wn, mask=mask)
    W, R = fusion.fused_tables(**args)
    Q = np.concatenate([P, Ng], axis=1)
    for fold in FOLDS:
        for combine in COMBINES:
            D, I, E = fusion.fused_search(index, k=k, fold=fold, combine=combine, explain=True, **args)
            assert E.shape == (nq, k, 5) and E.dtype == np.float32
            F = fusion.fused_scores_ref(np.ascontiguousarray(E.transpose(0, 2, 1)), W, R, fold, combine)
            assert np.array_equal(bits(F + f32(0.0)), bits(D)), (fold, combine)
            qd = torch.from_numpy(np.ascontiguousarray(Q.reshape(nq * 5, d))).to(index.device)
            cand = torch.from_numpy(I).to(index.device).repeat_interleave(5, dim=0).contiguous()
            Sx = index.rescore_device(qd, cand)[0].cpu().numpy().reshape(nq, 5, k).transpose(0, 2, 1)
            present = np.broadcast_to((R != 0)[:, None, :], E.shape)
            assert np.array_equal(bits(E[present]), bits(Sx[present])) and (E[~present] == -FLT_MAX).all()
    # a result list longer than the index: the unused hits are -FLT_MAX in every slot
    small, _ = make_index(d, 5, 5)
    D, I, E = fusion.fused_search(small, P, 8, explain=True)
    assert (I[:, 5:] == -1).all() and (E[:, 5:] == -FLT_MAX).all() and (E[:, :5] > -FLT_MAX).all()


def test_both_branches_of_veto_and_ties_to_the_lower_row():
    d, N, nq, k = 20, 300, 3, 60
    index, X = make_index(d, N, 6, period=37)                      # rows r and r + 37 are exact duplicates
    P = make_members(d, nq, 2, 14)
    Ng = np.broadcast_to(X[[0, 5]], (nq, 2, d)).copy()              # the originals of two runs of duplicates are the negative examples
    S = member_scores(index, np.concatenate([P, Ng], axis=1))
    W, R = fusion.fused_tables(P, negatives=Ng)
    assert np.array_equal(bits(S[:, :, 0]), bits(S[:, :, 37]))     # the duplicates do tie, to the bit
    T = S * W[:, :, None]
    Pm, Nn = T[:, :2].max(axis=1), T[:, 2:].max(axis=1)
    assert (Pm > Nn).any() and (Pm <= Nn).any()                     # both branches occur among the rows
    for fold in FOLDS:
        D, I = check(index, S, k, fold, "veto", positives=P, negatives=Ng)
        tied = bits(D[:, :-1]) == bits(D[:, 1:])
        assert tied.any() and (I[:, :-1][tied] < I[:, 1:][tied]).all()
        check(index, S, k, fold, "margin", positives=P, negatives=Ng)
    F = fusion.fused_scores_ref(S, W, R, "max", "veto")
    assert (F[:, [0, 37, 5, 42]] < 0).all() and np.array_equal(bits(F[:, 0]), bits(-(S[:, 2, 0] * S[:, 2, 0])))


def test_chunked_call_has_the_bits_of_the_unchunked_one(monkeypatch):
    # 40 fused queries of 4 columns: a stretch is 704 keys, 12 stretches and a bit fit the budget = three query tiles per chunk, four chunks
    d, N, nq = 20, 700, 40
    whole, X = make_index(d, N, 7)
    monkeypatch.setenv("IVR_SEQ_CHUNK_SLOTS", str(704 * 12 + 5))
    chunked = FlatIPIndex(d)                                        # the variable is read when the index is created
    chunked.add(X)
    monkeypatch.delenv("IVR_SEQ_CHUNK_SLOTS")
    P, Ng = make_members(d, nq, 3, 15), make_members(d, nq, 1, 16)
    S = member_scores(whole, np.concatenate([P, Ng], axis=1))
    Wp = make_weights(nq, 3, 17)
    out = []
    for index in (whole, chunked):
        got = []
        for fold, combine in (("max", "margin"), ("sum", "veto"), ("min", "margin")):
            got += list(check(index, S, 10, fold, combine, positives=P, weights=Wp, negatives=Ng))
            F = fusion.fused_scores_ref(S, *fusion.fused_tables(P, Wp, Ng), fold, combine)
            lims, D, I = fusion.fused_range_search(index, P, float(np.median(F)), fold=fold, combine=combine, weights=Wp, negatives=Ng)
            assert lims[0] == 0 and lims[-1] == len(D) and (np.diff(lims)[12:] > 0).sum() > 12     # lims carries across the chunks
            got += [lims, D, I]
        out.append(got)
    assert all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(*out))


def test_id_mapped_index_side_stream_and_repeat_calls():
    rng = np.random.default_rng(8)
    d, N, nq = 20, 1500, 6
    ids = rng.permutation(N).astype(np.int64) * 3 + 1000
    ids[::5] += 2 ** 33                                             # labels beyond 2^32
    index, X = make_index(d, N, 8, ids=ids)
    P, Ng = make_members(d, nq, 2, 18), make_members(d, nq, 1, 19)
    S = member_scores(index, np.concatenate([P, Ng], axis=1))
    D, I = check(index, S, 10, "max", "margin", ids=ids, positives=P, negatives=Ng)
    assert np.isin(I, ids).all() and (I > 2 ** 32).any()
    check(index, S, 10, "sum", "veto", ids=ids, positives=P, negatives=Ng)
    Pd, Nd = torch.from_numpy(P).to(index.device), torch.from_numpy(Ng).to(index.device)
    first = [t.clone() for t in fusion.fused_search_device(index, Pd, 10, negatives=Nd)]
    rfirst = [t.clone() for t in fusion.fused_range_search_device(index, Pd, 0.5, negatives=Nd)]
    again = fusion.fused_search_device(index, Pd, 10, negatives=Nd)
    side = torch.cuda.Stream(device=index.device)
    side.wait_stream(torch.cuda.current_stream(index.device))
    with torch.cuda.stream(side):
        other = fusion.fused_search_device(index, Pd, 10, negatives=Nd)
        rother = fusion.fused_range_search_device(index, Pd, 0.5, negatives=Nd)
    side.synchronize()
    for a, b, c in zip(first, again, other):
        assert torch.equal(a, b) and torch.equal(a, c)
    for a, b in zip(rfirst, rother):
        assert torch.equal(a, b)
    assert np.array_equal(first[1].cpu().numpy(), I) and np.array_equal(bits(first[0].cpu().numpy()), bits(D))
    # explain on an id-mapped index finds the rows behind the labels
    Dx, Ix, E = fusion.fused_search(index, P, 10, negatives=Ng, explain=True)
    row = {int(v): r for r, v in enumerate(ids)}
    rows = np.vectorize(row.get)(Ix)
    assert np.array_equal(bits(E), bits(np.stack([S[q][:, rows[q]].T for q in range(nq)])))


def test_library_rejects_invalid_arguments_and_the_index_stays_usable():
    d = 20
    index, X = make_index(d, 50, 9)
    dev = index.device
    x = make_members(d, 2, 1, 20)[:, 0]
    before = index.search(x, 5)
    q = torch.from_numpy(make_members(d, 2, 4, 21).reshape(8, d)).to(dev)
    w = torch.ones(8, dtype=torch.float32, device=dev)
    role = torch.tensor([1, 1, -1, 0, 1, 0, 0, -1], dtype=torch.int8, device=dev)
    D, I = torch.zeros((2, 3), dtype=torch.float32, device=dev), torch.zeros((2, 3), dtype=torch.int64, device=dev)
    lims = torch.zeros(3, dtype=torch.int64, device=dev)

    def topk(q=q, nq=2, slots=4, w=w, role=role, fold=0, combine=0, k=3, D=D, I=I):
        index._call("ivr_index_search_fused", q, nq, slots, w, role, fold, combine, k, False, D, I)

    def rng_(q=q, nq=2, slots=4, w=w, role=role, fold=0, combine=0, thr=0.0, lims=lims, D=D, I=I, cap=6):
        index._call("ivr_index_range_search_fused", q, nq, slots, w, role, fold, combine, thr, False, lims, D, I, cap)

    topk()                                                         # the arguments in range pass
    rng_()
    nopos = torch.tensor([1, 1, -1, 0, 0, 0, 0, -1], dtype=torch.int8, device=dev)
    winf, wnan = w.clone(), w.clone()
    winf[5], wnan[2] = float("inf"), float("nan")
    badrole = role.clone()
    badrole[1] = 3
    bad = [(dict(slots=3), "slots=3"), (dict(slots=0), "slots=0"), (dict(slots=32), "slots=32"), (dict(role=nopos), "set 1 has no positive member"),
           (dict(w=winf), "not finite"), (dict(w=wnan), "not finite"), (dict(role=badrole), "role=3"), (dict(fold=3), "fold=3"),
           (dict(fold=-1), "fold=-1"), (dict(combine=2), "combine=2"), (dict(nq=0), "nq=0"), (dict(q=None), "NULL"), (dict(w=None), "NULL"),
           (dict(role=None), "NULL"), (dict(D=None), "NULL"), (dict(I=None), "NULL")]
    for kw, text in bad:
        with pytest.raises(ValueError, match=text):
            topk(**kw)
        with pytest.raises(ValueError, match=text):
            rng_(**kw)
    for kw, text in [(dict(k=0), "k=0"), (dict(k=_ffi.IVR_MAX_K + 1), f"k={_ffi.IVR_MAX_K + 1}")]:
        with pytest.raises(ValueError, match=text):
            topk(**kw)
    for kw, text in [(dict(lims=None), "NULL"), (dict(cap=-1), "cap=-1"), (dict(thr=float("nan")), "NaN")]:
        with pytest.raises(ValueError, match=text):
            rng_(**kw)
    # the same through the Python layer, with its own messages
    P = make_members(d, 2, 3, 22)
    for kw, text in [(dict(fold="mean"), "fold='mean'"), (dict(combine="x"), "combine='x'"), (dict(weights=np.full((2, 3), np.nan)), "finite"),
                     (dict(mask=np.zeros((2, 3), bool)), "no positive member"), (dict(k=0), "k=0")]:
        with pytest.raises(ValueError, match=text):
            fusion.fused_search(index, P, **{"k": 3, **kw})
    with pytest.raises(ValueError, match="dimension"):
        fusion.fused_search(index, make_members(d + 1, 2, 3, 22), 3)
    after = index.search(x, 5)
    assert np.array_equal(before[1], after[1]) and np.array_equal(bits(before[0]), bits(after[0]))
    empty = FlatIPIndex(d)
    Dd, Ii = fusion.fused_search(empty, P, 4)
    assert Dd.shape == (2, 4) and (Dd == -FLT_MAX).all() and (Ii == -1).all()
    le, De, Ie = fusion.fused_range_search(empty, P, 0.0)
    assert le.tolist() == [0, 0, 0] and len(De) == 0 and len(Ie) == 0


def test_retriever_fuses_several_query_vectors():
    from ivr_amd.compat import FAISSRetriever, KeyframeMetadata
    rng = np.random.default_rng(10)
    d, n = 32, 40
    feats = rng.standard_normal((n, d)).astype(np.float32)
    qa, qb, qn = (rng.standard_normal(d).astype(np.float32) for _ in range(3))
    feats[7] = qa + 0.05 * rng.standard_normal(d).astype(np.float32)          # answers the first expansion
    feats[21] = qb + 0.05 * rng.standard_normal(d).astype(np.float32)         # answers the second
    feats[30] = qa + qn                                                        # looks like the negative example too
    metas = [KeyframeMetadata(folder_name=f"L01_V{i // 10:03d}", image_name=f"{i % 10:03d}.jpg", frame_id=i % 10, file_path=f"/k/{i}.jpg",
                              clip_features=feats[i] / np.linalg.norm(feats[i])) for i in range(n)]
    r = FAISSRetriever()
    r.build_index(feats, metas)
    # the members as the retriever stages them: its own normalisation of the same vectors, handed to the library as they are
    members = r._normalize_and_validate_features(np.stack([qa, qb]))[None]
    negative = r._normalize_and_validate_features(qn[None])[None]
    low = high = False
    for k, kw, fkw in [(6, dict(), dict()),
                       (6, dict(fold="sum", weights=[0.7, 0.3]), dict(fold="sum", weights=np.array([[0.7, 0.3]], np.float32))),
                       (n, dict(fold="sum", weights=[1.5, 1.5]), dict(fold="sum", weights=np.array([[1.5, 1.5]], np.float32))),
                       (n, dict(fold="min", weights=[1.5, -0.5]), dict(fold="min", weights=np.array([[1.5, -0.5]], np.float32))),
                       (n, dict(negative_features=[qn]), dict(negatives=negative))]:
        res = r.search_fused([qa, qb], k=k, **kw)
        D, I = (t.cpu().numpy() for t in fusion.fused_search_device(r.index, members, k, normalize=False, **fkw))
        assert [x.metadata.frame_id + 10 * int(x.metadata.folder_name[-3:]) for x in res] == I[0].tolist()
        assert [x.rank for x in res] == list(range(1, k + 1))
        assert [x.similarity_score for x in res] == [max(0.0, min(1.0, float(v))) for v in D[0]]     # the clamp of search(), exactly
        assert [x.query_relevance for x in res] == [x.similarity_score for x in res]
        low, high = low or bool((D[0] < 0.0).any()), high or bool((D[0] > 1.0).any())
    assert low and high                                             # both ends of the clamp were exercised
    top = r.search_fused([qa, qb], k=2)
    assert {x.metadata.get_unique_key() for x in top} == {metas[7].get_unique_key(), metas[21].get_unique_key()}
    assert r.search_fused([qa], k=3, negative_features=[qn])[0].metadata.get_unique_key() == metas[7].get_unique_key()
