"""CPU suite of the fused search (ivr_amd/fusion.py): the numpy definition against a brute force written here and in fusion_cases.py
(Python loops, np.float32 scalars, the pairwise tree spelled out), its argument checks, and the two new symbols of the C ABI.  Every
comparison is exact: ids element for element, scores as bit patterns."""
import ctypes
import re

import numpy as np
import pytest

from conftest import ROOT
from fusion_cases import (COMBINES, FLT_MAX, FOLDS, bits, brute_range, brute_scores, brute_topk, f32, small_roles, small_scores, tree_sum)
from ivr_amd import _ffi, fusion

NAMES = ("ivr_index_search_fused", "ivr_index_range_search_fused")


def weights_for(R, seed):
    rng = np.random.default_rng([seed, R.shape[0], R.shape[1]])
    W = (rng.random(R.shape) * 4 - 2).astype(np.float32)
    W[0, 0] = -1.0                                                # a weight of -1 on a positive member
    return W


@pytest.mark.parametrize("slots", [1, 2, 3, 4, 5, 8, 11, 16])
@pytest.mark.parametrize("negatives", [False, True])
@pytest.mark.parametrize("halves", [False, True])
def test_scores_match_the_brute_force(slots, negatives, halves):
    nq, N = 3, 40
    S = small_scores(nq, slots, N, 1, halves)
    R = small_roles(nq, slots, 1, negatives and slots > 1)
    W = weights_for(R, 1)
    if halves:
        assert (bits(S) == 0x80000000).any() and (bits(S) == 0).any()          # -0.0 and +0.0 are among the scores
    for fold in FOLDS:
        for combine in COMBINES:
            F = fusion.fused_scores_ref(S, W, R, fold, combine)
            Fb = brute_scores(S, W, R, fold, combine)
            assert F.dtype == np.float32 and F.shape == (nq, N)
            # the sign of a zero is not part of the definition (-0.0 ranks and is reported as +0.0)
            assert np.array_equal(bits(F + f32(0.0)), bits(Fb + f32(0.0))), (slots, fold, combine)
            for k in (1, 7, N + 3):
                D, I = fusion.fused_search_ref(S, W, R, k, fold, combine)
                Db, Ib = brute_topk(Fb, k)
                assert np.array_equal(I, Ib) and np.array_equal(bits(D), bits(Db))
            thr = float(np.median(Fb))
            lims, D, I = fusion.fused_range_search_ref(S, W, R, thr, fold, combine)
            lb, Db, Ib = brute_range(Fb, thr)
            assert np.array_equal(lims, lb) and np.array_equal(I, Ib) and np.array_equal(bits(D), bits(Db))
            assert lims[-1] > 0 and (D >= f32(thr)).all()


def test_absent_slots_in_the_middle_of_a_set_do_not_move_the_other_members():
    S = small_scores(2, 8, 30, 2)
    R = np.array([[1, 0, 1, -1, 0, 1, 0, 0], [0, 1, 0, 0, -1, 0, 0, 1]], np.int8)
    W = weights_for(R, 2)
    for fold in FOLDS:
        F = fusion.fused_scores_ref(S, W, R, fold, "margin")
        assert np.array_equal(bits(F + f32(0.0)), bits(brute_scores(S, W, R, fold, "margin") + f32(0.0)))
    # the scores and weights of an absent slot are never read: garbage there changes nothing
    S2, W2 = S.copy(), W.copy()
    S2[:, :, :][R == 0] = 1e30
    W2[R == 0] = -7.0
    for fold in FOLDS:
        assert np.array_equal(bits(fusion.fused_scores_ref(S, W, R, fold, "veto")), bits(fusion.fused_scores_ref(S2, W2, R, fold, "veto")))


def test_sum_of_three_is_the_tree_over_four_slots_not_the_ascending_sum():
    # Three members in the slots 0, 1, 2 are the tree over four slots with a +0.0 fourth term, (a + b) + (c + 0).  x + 0.0 is x, so
    # that tree can never differ from the ascending sum of three; what pins the order is the cases below, where it does differ: an
    # absent slot in the middle, (a + 0) + (b + c); four members, (a + b) + (c + e); five members over eight slots
    a, b, c = f32(1.0), f32(2.0 ** -24), f32(2.0 ** -24)
    S = np.array([[[a], [b], [c]]], np.float32)                    # [1,3,1]
    W = np.ones((1, 3), np.float32)
    R = np.ones((1, 3), np.int8)
    tree = tree_sum([a, b, c, f32(0.0)])
    assert bits(fusion.fused_scores_ref(S, W, R, "sum"))[0, 0] == bits(tree)
    assert bits(tree) == bits(f32(f32(a + b) + f32(c + f32(0.0))))
    # slots 0, (absent), 2, 3: the tree adds the two small terms first and they survive; the ascending sum loses both
    S4 = np.array([[[a], [f32(9.0)], [b], [c]]], np.float32)
    R4 = np.array([[1, 0, 1, 1]], np.int8)
    W4 = np.ones((1, 4), np.float32)
    got = fusion.fused_scores_ref(S4, W4, R4, "sum")[0, 0]
    ascending = f32(f32(a + b) + c)
    assert bits(got) == bits(f32(f32(a + f32(0.0)) + f32(b + c)))
    assert bits(got) != bits(ascending), "the inputs must tell the tree from the ascending sum"
    assert got == f32(1.0 + 2.0 ** -23) and ascending == f32(1.0)
    # four members in four slots: (a + b) + (c + e) keeps 2^-23, ((a + b) + c) + e loses every small term
    e = f32(2.0 ** -24)
    S4 = np.array([[[a], [b], [c], [e]]], np.float32)
    got = fusion.fused_scores_ref(S4, W4, np.ones((1, 4), np.int8), "sum")[0, 0]
    assert bits(got) == bits(tree_sum([a, b, c, e])) == bits(f32(1.0 + 2.0 ** -23))
    assert bits(got) != bits(f32(f32(f32(a + b) + c) + e)) and f32(f32(f32(a + b) + c) + e) == f32(1.0)
    # five members: the tree over eight slots, ((a + b) + (c + e)) + ((g + 0) + (0 + 0))
    g = f32(-1.0)
    S5 = np.array([[[a], [b], [c], [e], [g]]], np.float32)
    got = fusion.fused_scores_ref(S5, np.ones((1, 5), np.float32), np.ones((1, 5), np.int8), "sum")[0, 0]
    assert bits(got) == bits(tree_sum([a, b, c, e, g, f32(0.0), f32(0.0), f32(0.0)])) == bits(f32(2.0 ** -23))
    assert f32(f32(f32(f32(a + b) + c) + e) + g) == f32(0.0)


def test_singleton_sets_with_weight_one_are_the_plain_top_k():
    S = small_scores(4, 1, 60, 3, halves=True)
    W = np.ones((4, 1), np.float32)
    R = np.ones((4, 1), np.int8)
    for fold in FOLDS:
        for combine in COMBINES:
            D, I = fusion.fused_search_ref(S, W, R, 9, fold, combine)
            Db, Ib = brute_topk(S[:, 0], 9)
            assert np.array_equal(I, Ib) and np.array_equal(bits(D), bits(Db))


def test_ties_pads_and_the_range_test():
    S = np.zeros((1, 2, 6), np.float32)
    S[0, 0] = [1, 3, 3, -0.0, 0.0, 3]
    S[0, 1] = [1, 3, 3, 0.0, -0.0, 3]
    W = np.ones((1, 2), np.float32)
    R = np.ones((1, 2), np.int8)
    D, I = fusion.fused_search_ref(S, W, R, 8, "min")
    assert I.tolist() == [[1, 2, 5, 0, 3, 4, -1, -1]]              # equal scores: the lower row; -0.0 ties with +0.0
    assert D[0, :6].tolist() == [3, 3, 3, 1, 0, 0] and (bits(D[0, 4:6]) == 0).all() and (D[0, 6:] == -FLT_MAX).all()
    lims, D, I = fusion.fused_range_search_ref(S, W, R, 3.0, "min")
    assert lims.tolist() == [0, 3] and I.tolist() == [1, 2, 5]      # >= : the rows AT the threshold are in
    lims, D, I = fusion.fused_range_search_ref(S, W, R, 0.0, "max")
    assert I.tolist() == [0, 1, 2, 3, 4, 5] and (bits(D[3:5]) == 0).all()
    ids = np.array([50, 40, 2 ** 40, 7, 8, 9], np.int64)
    assert fusion.fused_search_ref(S, W, R, 2, "min", ids=ids)[1].tolist() == [[40, 2 ** 40]]
    assert fusion.fused_range_search_ref(S, W, R, 3.0, "min", ids=ids)[2].tolist() == [40, 2 ** 40, 9]


def test_veto_sinks_a_row_by_the_square_of_its_negative_score():
    S = np.array([[[0.9, 0.2, 0.5], [0.1, 0.8, 0.5]]], np.float32)  # member 0 positive, member 1 negative
    W = np.ones((1, 2), np.float32)
    R = np.array([[1, -1]], np.int8)
    F = fusion.fused_scores_ref(S, W, R, "max", "veto")[0]
    assert bits(F[0]) == bits(f32(0.9)) and bits(F[1]) == bits(-(f32(0.8) * f32(0.8))) and bits(F[2]) == bits(-(f32(0.5) * f32(0.5)))
    F = fusion.fused_scores_ref(S, W, R, "max", "margin")[0]
    assert np.array_equal(bits(F), bits(S[0, 0] - S[0, 1]))


def test_argument_checks():
    S = small_scores(2, 3, 10, 4)
    W = np.ones((2, 3), np.float32)
    R = np.ones((2, 3), np.int8)
    ok = dict(S=S, weights=W, roles=R)
    fusion.fused_scores_ref(**ok)
    for bad, text in [(dict(S=small_scores(2, 17, 10, 4), weights=np.ones((2, 17)), roles=np.ones((2, 17), np.int8)), "17 members"),
                      (dict(roles=np.array([[1, 1, 1], [0, -1, 0]], np.int8)), "set 1 has no positive member"),
                      (dict(weights=np.array([[1, np.inf, 1], [1, 1, 1]], np.float32)), "finite"),
                      (dict(weights=np.array([[1, np.nan, 1], [1, 1, 1]], np.float32)), "finite"),
                      (dict(roles=np.full((2, 3), 2, np.int8)), "roles must be"),
                      (dict(fold="mean"), "fold='mean'"), (dict(combine="minus"), "combine='minus'"),
                      (dict(weights=np.ones((2, 2))), "must both be"), (dict(S=S[:, :2]), "does not match"), (dict(S=S[0]), r"\[nq,slots,N\]")]:
        with pytest.raises(ValueError, match=text):
            fusion.fused_scores_ref(**{**ok, **bad})
    for k in (0, -1, _ffi.IVR_MAX_K + 1):
        with pytest.raises(ValueError, match="k="):
            fusion.fused_search_ref(S, W, R, k)
    with pytest.raises(ValueError, match="NaN"):
        fusion.fused_range_search_ref(S, W, R, float("nan"))
    # the tables of a call, as fused_search builds them
    d = 6
    P = np.zeros((2, 3, d), np.float32)
    Wt, Rt = fusion.fused_tables(P, negatives=np.zeros((2, 2, d), np.float32), negative_weights=[0.5, 2.0])
    assert Rt.tolist() == [[1, 1, 1, -1, -1]] * 2 and Wt.tolist() == [[1, 1, 1, 0.5, 2.0]] * 2 and Rt.dtype == np.int8
    Wt, Rt = fusion.fused_tables([np.zeros((2, d)), np.zeros((3, d))], weights=[[1, 2], [3, 4, 5]], negatives=[np.zeros((0, d)), np.zeros((1, d))])
    assert Rt.tolist() == [[1, 1, 0, 0], [1, 1, 1, -1]] and Wt.tolist() == [[1, 2, 0, 0], [3, 4, 5, 1]]
    Wt, Rt = fusion.fused_tables(P, mask=np.array([[True, False, True], [False, False, True]]))
    assert Rt.tolist() == [[1, 0, 1], [0, 0, 1]] and Wt.tolist() == [[1, 0, 1], [0, 0, 1]]
    for bad, text in [(dict(positives=np.zeros((2, 17, d), np.float32)), "17 members"),
                      (dict(positives=np.zeros((2, 9, d), np.float32), negatives=np.zeros((2, 8, d), np.float32)), "17 members"),
                      (dict(positives=P, mask=np.array([[True, True, True], [False, False, False]])), "set 1 has no positive member"),
                      (dict(positives=P, weights=np.full((2, 3), np.inf)), "finite"),
                      (dict(positives=P, weights=np.ones((2, 4))), "weights"),
                      (dict(positives=P, negatives=np.zeros((3, 1, d), np.float32)), "3 sets for 2"),
                      (dict(positives=P, negative_weights=[1.0]), "without negatives"),
                      (dict(positives=P, mask=np.ones((2, 2), bool)), "mask must be"),
                      (dict(positives=[np.zeros((2, d))], mask=np.ones((1, 2), bool)), "array form"),
                      (dict(positives=np.zeros((2, d), np.float32)), r"\[nq,m,d\]")]:
        with pytest.raises(ValueError, match=text):
            fusion.fused_tables(**bad)


def _header():
    return re.sub(r"/\*.*?\*/", "", open(f"{ROOT}/include/ivr_api.h").read(), flags=re.S)


def test_the_new_symbols_are_declared_bound_and_exported():
    lib = ctypes.CDLL(_ffi.LIB_PATH)
    for name in NAMES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", _header()), f"{name} not declared in ivr_api.h"
        assert name in _ffi.EXPORTS and name in _ffi._STREAM and name not in _ffi._VALUE
        assert hasattr(lib, name), f"{name} declared in ivr_api.h but not exported"
    for fold, v in _ffi.IVR_FUSE_FOLD.items():
        assert re.search(r"#define\s+IVR_FUSE_" + fold.upper() + r"\s+" + str(v) + r"\b", _header())
    for combine, v in _ffi.IVR_FUSE_COMBINE.items():
        assert re.search(r"#define\s+IVR_FUSE_" + combine.upper() + r"\s+" + str(v) + r"\b", _header())
    assert re.search(r"#define\s+IVR_FUSE_MAX_MEMBERS\s+16\b", _header()) and fusion.FUSE_MAX_MEMBERS == 16


def test_lazy_package_exports_resolve():
    import ivr_amd
    for name in ("fused_search", "fused_search_device", "fused_range_search", "fused_range_search_device", "fused_scores_ref",
                 "fused_search_ref", "fused_range_search_ref", "fused_tables"):
        assert getattr(ivr_amd, name) is getattr(fusion, name) and name in ivr_amd.__all__
