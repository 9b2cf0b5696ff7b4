"""CPU suite of the diversified search (ivr_amd/diversify.py, csrc/search_diverse.hip): the numpy definitions mmr_ref / suppress_ref
against a brute force that loops over sets and sorts tuples, their identities with refine_order_ref, the ABI of the new entry point,
the argument checks that need no device, and a check on the host that the cases of the GPU suite hold what they are there for.  No
compute call reaches a device."""
import ctypes
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
from diverse_cases import (FLT_MAX, bits, brute, ends_early, host_scores, k_values, lists_of, make_cand, make_queries, row_tie_decides, same,
                           shot_rows, small_cases, unit_rows)
from ivr_amd import _ffi, diversify
from ivr_amd.index import FlatIPIndex
from ivr_amd.refine import refine_order_ref

NAME = "ivr_index_diversify"
LAMBDAS = (0.0, 0.3, 0.5, 1.0)


# -- the definition against the brute force ------------------------------------------------------------------------------------------
def test_definitions_are_the_brute_force_on_small_cases_with_ties():
    twice = absent = negzero = early = by_row = by_position = 0
    for R, P, cand, ntotal in small_cases():
        kc = cand.shape[1]
        ids = np.arange(ntotal, dtype=np.int64)[::-1] * 3 + 100
        present = (cand >= 0) & (cand < ntotal)
        absent += int((~present).sum())
        twice += sum(len(set(c[p].tolist())) < int(p.sum()) for c, p in zip(cand, present))
        negzero += int((np.signbit(R) & (R == 0)).sum())
        for k in k_values(kc):
            for labels in (None, ids):
                for lam in LAMBDAS:
                    got = diversify.mmr_ref(R, P, cand, k, lam, ntotal, labels)
                    assert same(got, brute(R, P, cand, k, "mmr", lam, ntotal, labels)), f"mmr kc={kc} k={k} lambda={lam}"
                for thr in (-np.inf, -0.5, 0.0, 0.5, np.inf):
                    got = diversify.suppress_ref(R, P, cand, k, thr, ntotal, labels)
                    assert same(got, brute(R, P, cand, k, "suppress", thr, ntotal, labels)), f"suppress kc={kc} k={k} threshold={thr}"
                    early += int(((got[1][:, -1] == -1) & (present.sum(axis=1) >= k)).any())
            D, I, M = diversify.mmr_ref(R, P, cand, k, 1.0, ntotal)
            by_row += int(row_tie_decides(I, D))
            by_position += int(((bits(D[:, 1:]) == bits(D[:, :-1])) & (I[:, 1:] == I[:, :-1]) & (I[:, 1:] >= 0)).any())
    assert min(twice, absent, negzero, early, by_row, by_position) > 0            # the cases do hold what they are there for


def test_hand_made_case():
    #                row 4    2    7    2    9 (absent)
    cand = np.array([[4, 2, 7, 2, 9]], np.int64)
    R = np.array([[0.9, 0.8, 0.8, 0.8, 5.0]], np.float32)
    P = np.zeros((1, 5, 5), np.float32)
    P[0, 0] = [1.0, 0.9, 0.1, 0.9, 0.0]                # row 4 looks like row 2
    P[0, 2] = [0.1, 0.2, 1.0, 0.2, 0.0]
    P[0, 1] = P[0, 3] = [0.9, 1.0, 0.2, 1.0, 0.0]
    # lambda = 1: relevance order, equal scores the lower row first, a row named twice in adjacent slots in the order of cand
    D, I, M = diversify.mmr_ref(R, P, cand, 5, 1.0, ntotal=9)
    assert I.tolist() == [[4, 2, 2, 7, -1]] and np.array_equal(bits(D), bits(np.array([[0.9, 0.8, 0.8, 0.8, -FLT_MAX]], np.float32)))
    assert np.array_equal(bits(M), bits(np.array([[-FLT_MAX, 0.9, 1.0, 0.2, -FLT_MAX]], np.float32)))
    # lambda = 0.5: row 7 overtakes the two mentions of row 2, which resemble what is chosen already
    D, I, M = diversify.mmr_ref(R, P, cand, 3, 0.5, ntotal=9)
    assert I.tolist() == [[4, 7, 2]] and np.array_equal(bits(M), bits(np.array([[-FLT_MAX, 0.1, 0.9]], np.float32)))
    # suppress at 0.85: both mentions of row 2 go with the first choice, and the list ends early
    D, I, M = diversify.suppress_ref(R, P, cand, 4, 0.85, ntotal=9)
    assert I.tolist() == [[4, 7, -1, -1]] and np.array_equal(bits(M), bits(np.array([[-FLT_MAX, 0.1, -FLT_MAX, -FLT_MAX]], np.float32)))
    # the test is >=: a pair score equal to the threshold suppresses
    assert diversify.suppress_ref(R, P, cand, 4, 0.9, ntotal=9)[1].tolist() == [[4, 7, -1, -1]]
    assert diversify.suppress_ref(R, P, cand, 4, np.nextafter(np.float32(0.9), np.float32(1)), ntotal=9)[1].tolist() == [[4, 2, 7, -1]]
    # without ntotal row 9 is present and the most relevant; labels of an id-mapped index
    ids = np.arange(10, dtype=np.int64) + 50
    assert diversify.mmr_ref(R, P, cand, 2, 1.0, ids=ids)[1].tolist() == [[59, 54]]
    # -0.0 ranks as +0.0 (the lower row wins the tie) and is reported as +0.0
    D, I, M = diversify.mmr_ref(np.array([[0.0, -0.0]], np.float32), np.full((1, 2, 2), -0.0, np.float32), np.array([[3, 1]]), 2, 0.5)
    assert I.tolist() == [[1, 3]] and bits(D).tolist() == [[0, 0]] and bits(M)[0, 1] == 0
    # every entry absent: unused slots only
    D, I, M = diversify.suppress_ref(R, P, np.full((1, 5), -1), 2, 0.5)
    assert (I == -1).all() and (D == -FLT_MAX).all() and (M == -FLT_MAX).all()


def test_lambda_one_and_an_infinite_threshold_are_the_relevance_order():
    for R, P, cand, ntotal in small_cases(60, seed=6):
        for k in k_values(cand.shape[1]):
            Dr, Ir = refine_order_ref(R, cand, k, ntotal)
            for D, I, M in (diversify.mmr_ref(R, P, cand, k, 1.0, ntotal), diversify.suppress_ref(R, P, cand, k, np.inf, ntotal)):
                assert np.array_equal(I, Ir) and np.array_equal(bits(D), bits(Dr))


def test_a_threshold_below_every_pair_score_returns_one_result():
    for R, P, cand, ntotal in small_cases(60, seed=7):
        k = cand.shape[1]
        D, I, M = diversify.suppress_ref(R, P, cand, k, -np.inf, ntotal)
        Dr, Ir = refine_order_ref(R, cand, 1, ntotal)
        assert np.array_equal(I[:, :1], Ir) and (I[:, 1:] == -1).all() and (D[:, 1:] == -FLT_MAX).all() and (M == -FLT_MAX).all()


def test_the_cases_of_the_gpu_suite_are_not_vacuous():
    # the rows, queries and lists of test_diverse_gpu.py with scores computed on the host: every condition that suite asserts on the
    # device results holds for the definition already
    X, x = unit_rows(20, 300, 1, period=37), make_queries(20, 3, 1)
    Rfull, Pfull = host_scores(X, x)
    mmr_differs = sup_differs = tie = early = False
    for kc in (17, 64, 257):
        cand = make_cand(3, kc, 300, 1)
        R, P = lists_of(Rfull, Pfull, cand)
        k = min(kc, 10)
        plain = refine_order_ref(R, cand, k, 300)[1]
        mmr_differs |= not np.array_equal(diversify.mmr_ref(R, P, cand, k, 0.3, 300)[1], plain)
        D, I, M = diversify.suppress_ref(R, P, cand, kc, 0.95, 300)
        sup_differs |= not np.array_equal(I[:, :k], plain)
        early |= ends_early(I)
        D, I, M = diversify.mmr_ref(R, P, cand, k, 1.0, 300)
        tie |= row_tie_decides(I, D)
    assert mmr_differs and sup_differs and tie and early
    X = shot_rows(20, 12, 8, 2)
    Rfull, Pfull = host_scores(X, make_queries(20, 3, 2))
    cand = make_cand(3, 64, 96, 2)
    R, P = lists_of(Rfull, Pfull, cand)
    D, I, M = diversify.suppress_ref(R, P, cand, 64, 0.95, 96)
    assert ends_early(I) and ((I >= 0).sum(axis=1) == 12).all()           # one hit per shot
    assert len({int(r) // 8 for r in diversify.mmr_ref(R, P, cand, 8, 0.5, 96)[1][0]}) > len({int(r) // 8 for r in refine_order_ref(R, cand, 8, 96)[1][0]})


# -- ABI and surfaces ------------------------------------------------------------------------------------------------------------------
def _header():
    return re.sub(r"/\*.*?\*/", "", open(f"{ROOT}/include/ivr_api.h").read(), flags=re.S)


def _ctype_of(decl):
    decl = decl.strip()
    if "*" in decl or decl.startswith("ivr_stream"):
        return ctypes.c_void_p
    return {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "float": ctypes.c_float}[decl.split()[0]]


def test_header_binding_and_library_agree():
    m = re.search(r"\bint\s+" + NAME + r"\s*\(([^)]*)\)\s*;", _header())
    assert m, f"{NAME} not declared in ivr_api.h"
    params = [p.strip() for p in m.group(1).split(",")]
    assert [re.sub(r"[\s*]+", " ", p).split()[-1] for p in params] == ["idx", "q", "nq", "cand", "kc", "k", "mode", "param", "normalize_q", "D",
                                                                    "I", "M", "stream"]
    res, args = _ffi._SIGS[NAME]
    assert res is ctypes.c_int and args == [_ctype_of(p) for p in params]
    assert _ffi._STREAM[NAME] == len(params) - 1 and NAME not in _ffi._VALUE
    assert NAME in _ffi.EXPORTS and _ffi.EXPORTS[-1] == NAME                     # appended
    assert hasattr(ctypes.CDLL(_ffi.LIB_PATH), NAME)
    assert re.search(r"#define\s+IVR_DIVERSE_MMR\s+0\b", _header()) and re.search(r"#define\s+IVR_DIVERSE_SUPPRESS\s+1\b", _header())
    assert (_ffi.IVR_DIVERSE_MMR, _ffi.IVR_DIVERSE_SUPPRESS) == (0, 1) == (diversify.MMR, diversify.SUPPRESS)


def test_api_version_is_unchanged_and_the_index_class_grew_no_method():
    assert _ffi.API_VERSION == 11 and _ffi.load().ivr_api_version() == 11
    assert re.search(r"#define\s+IVR_API_VERSION\s+11\b", _header())
    assert not [n for n in dir(FlatIPIndex) if any(w in n.lower() for w in ("mmr", "divers", "suppress"))]


def test_lazy_package_exports_resolve():
    import ivr_amd
    for name in ("mmr_search", "mmr_search_device", "dedup_search", "dedup_search_device", "mmr_rerank", "mmr_rerank_device",
                 "suppress_rerank", "suppress_rerank_device", "mmr_ref", "suppress_ref"):
        assert name in ivr_amd.__all__
        assert getattr(ivr_amd, name) is getattr(diversify, name)


def test_library_rejects_bad_arguments_before_any_device_call():
    lib = _ffi.load()
    one = ctypes.c_void_p(1)                   # never dereferenced: every call below fails its checks first
    K = _ffi.IVR_MAX_K

    def call(idx=one, q=one, nq=1, cand=one, kc=4, k=2, mode=0, param=0.5, D=one, I=one, M=None):
        rc = lib.ivr_index_diversify(idx, q, nq, cand, kc, k, mode, param, 0, D, I, M, None)
        return rc, lib.ivr_last_error(None)

    for bad, text in [(dict(idx=None), b"NULL"), (dict(q=None), b"NULL"), (dict(cand=None), b"NULL"), (dict(D=None), b"NULL"),
                      (dict(I=None), b"NULL"), (dict(nq=0), b"nq=0"), (dict(kc=0, k=1), b"kc=0 outside [1,2048]"),
                      (dict(kc=K + 1), b"kc=2049 outside [1,2048]"), (dict(k=0), b"k=0 outside [1,kc=4]"), (dict(k=5), b"k=5 outside [1,kc=4]"),
                      (dict(nq=1 << 20, kc=K, k=1), b"nq * kc = 2147483648"), (dict(mode=2), b"mode=2"), (dict(mode=-1), b"mode=-1"),
                      (dict(param=-0.1), b"lambda=-0.1 outside [0,1]"), (dict(param=1.5), b"lambda=1.5 outside [0,1]"),
                      (dict(param=float("nan")), b"param=nan"), (dict(mode=1, param=float("nan")), b"param=nan")]:
        rc, err = call(**bad)
        assert rc == -1 and text in err, (bad, err)


def test_argument_checks_name_the_offending_values():
    index = FlatIPIndex.__new__(FlatIPIndex)             # no handle: every check below fails before the library is called
    index.d, index.device = 8, torch.device("cpu")
    x = np.zeros((2, 8), np.float32)
    cand = torch.zeros((2, 4), dtype=torch.int64)
    for call in (diversify.mmr_rerank_device, diversify.suppress_rerank_device):
        with pytest.raises(ValueError, match="FlatIPIndex, got object"):
            call(object(), x, cand, 2, 0.5)
        with pytest.raises(ValueError, match="contiguous int64 CUDA tensor"):
            call(index, x, cand, 2, 0.5)
        with pytest.raises(ValueError, match="Query dimension"):
            call(index, np.zeros((2, 9), np.float32), cand, 2, 0.5)
        with pytest.raises(ValueError, match="is NaN"):
            call(index, x, cand, 2, float("nan"))
        with pytest.raises(ValueError, match="must be a number, got str"):
            call(index, x, cand, 2, "0.5")
    for call in (diversify.mmr_search_device, diversify.dedup_search_device, diversify.mmr_search, diversify.dedup_search):
        with pytest.raises(ValueError, match="FlatIPIndex, got object"):
            call(object(), x, 2, 4)
        with pytest.raises(ValueError, match=r"k=5 outside \[1,fetch_k=4\]"):
            call(index, x, 5, 4)
        with pytest.raises(ValueError, match=r"k=2049 outside \[1,2048\]"):
            call(index, x, 5, 2049)
    for lam in (-0.1, 1.5):
        with pytest.raises(ValueError, match=rf"lambda_mult={lam} outside \[0,1\]"):
            diversify.mmr_rerank_device(index, x, cand, 2, lam)
        with pytest.raises(ValueError, match=rf"lambda_mult={lam} outside \[0,1\]"):
            diversify.mmr_ref(np.zeros((1, 2), np.float32), np.zeros((1, 2, 2), np.float32), np.zeros((1, 2), np.int64), 1, lam)
    R, P, c = np.zeros((1, 3), np.float32), np.zeros((1, 3, 3), np.float32), np.zeros((1, 3), np.int64)
    with pytest.raises(ValueError, match=r"k=4 outside \[1,3\]"):
        diversify.suppress_ref(R, P, c, 4, 0.5)
    with pytest.raises(ValueError, match=r"\[nq,kc,kc\]"):
        diversify.mmr_ref(R, P[:, :2], c, 1, 0.5)
