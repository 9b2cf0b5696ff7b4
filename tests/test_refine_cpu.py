"""CPU suite of the re-ranking index (ivr_amd/refine.py, csrc/search_refine.hip): the ABI of the new entry point, the lazy package
exports, the argument checks that need no device, and refine_order_ref (the definition the ordering pass is pinned to) against a
plain Python sort on hand-made cases.  No compute call reaches a device."""
import ctypes
import re

import numpy as np
import pytest

from conftest import ROOT
from ivr_amd import _ffi

FLT_MAX = float(np.finfo(np.float32).max)


def _header():
    src = open(f"{ROOT}/include/ivr_api.h").read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def _ctype_of(decl):
    decl = decl.strip()
    if "*" in decl or decl.startswith("ivr_stream"):
        return ctypes.c_void_p
    return {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "float": ctypes.c_float}[decl.split()[0]]


def test_header_declares_rescore_with_the_stream_last():
    m = re.search(r"\bint\s+ivr_index_rescore\s*\(([^)]*)\)\s*;", _header())
    assert m, "ivr_index_rescore not declared in ivr_api.h"
    params = [p.strip() for p in m.group(1).split(",")]
    assert len(params) == 11
    assert params[-1].startswith("ivr_stream")
    names = [re.sub(r"[\s*]+", " ", p).split()[-1] for p in params]
    assert names == ["idx", "q", "nq", "cand", "kc", "k", "normalize_q", "D_all", "D", "I", "stream"]


def test_binding_agrees_with_the_header_and_the_library():
    m = re.search(r"\bint\s+ivr_index_rescore\s*\(([^)]*)\)\s*;", _header())
    want = [_ctype_of(p) for p in m.group(1).split(",")]
    res, args = _ffi._SIGS["ivr_index_rescore"]
    assert res is ctypes.c_int and args == want
    assert _ffi._STREAM["ivr_index_rescore"] == len(want) - 1
    assert "ivr_index_rescore" in _ffi.EXPORTS and "ivr_index_rescore" not in _ffi._VALUE
    assert hasattr(ctypes.CDLL(_ffi.LIB_PATH), "ivr_index_rescore")


def test_api_version_is_still_11():
    assert _ffi.API_VERSION == 11
    assert _ffi.load().ivr_api_version() == 11
    assert re.search(r"#define\s+IVR_API_VERSION\s+11\b", _header())


def test_null_index_is_rejected():
    lib = _ffi.load()
    assert lib.ivr_index_rescore(None, None, 1, None, 1, 1, 0, None, None, None, None) == -1
    assert b"NULL" in lib.ivr_last_error(None)


def test_lazy_package_exports_resolve():
    import ivr_amd
    from ivr_amd import refine
    for name in ("RefineFlatIndex", "IndexRefineFlat", "IndexRefineSearchParameters", "refine_order_ref"):
        assert name in ivr_amd.__all__
        assert getattr(ivr_amd, name) is getattr(refine, name)
    with pytest.raises(AttributeError):
        ivr_amd.IndexRefinePQ


def test_search_parameters_and_k_factor_validation():
    from ivr_amd._faiss import typed_params
    from ivr_amd.index import IDSelectorRange, SearchParameters
    from ivr_amd.ivf import SearchParametersIVF
    from ivr_amd.refine import IndexRefineSearchParameters, RefineFlatIndex, _check_k_factor
    p = IndexRefineSearchParameters()
    assert p.k_factor is None and p.base_index_params is None and p.sel is None
    inner = SearchParametersIVF(nprobe=4)
    p = IndexRefineSearchParameters(k_factor=3, base_index_params=inner)
    assert p.k_factor == 3.0 and isinstance(p.k_factor, float) and p.base_index_params is inner
    assert IndexRefineSearchParameters(k_factor=1).k_factor == 1.0
    for bad in (0, 0.99, -2, float("nan")):
        with pytest.raises(ValueError):
            IndexRefineSearchParameters(k_factor=bad)
        with pytest.raises(ValueError):
            _check_k_factor(bad, "test")
    # a selector on the refine level is refused by typed_params, as on the other approximate indexes
    assert typed_params(p, IndexRefineSearchParameters, "RefineFlatIndex") is p
    with pytest.raises(ValueError, match="selectors"):
        typed_params(IndexRefineSearchParameters(sel=IDSelectorRange(0, 4)), IndexRefineSearchParameters, "RefineFlatIndex")
    with pytest.raises(ValueError):
        typed_params(SearchParameters(), IndexRefineSearchParameters, "RefineFlatIndex")
    # the k_factor attribute of the index goes through the same check (no handle is opened for it)
    x = RefineFlatIndex.__new__(RefineFlatIndex)
    x._k_factor = 1.0
    x.k_factor = 2.5
    assert x.k_factor == 2.5
    for bad in (0.5, 0, float("nan")):
        with pytest.raises(ValueError):
            x.k_factor = bad
    assert x.k_factor == 2.5
    with pytest.raises(ValueError):          # anything but one of the four index classes is refused before a device is touched
        RefineFlatIndex(object())


# -- refine_order_ref against a plain Python sort ------------------------------------------------------------------------------------
def _python_order(S, cand, k, ntotal):
    D, I = [], []
    for srow, crow in zip(S, cand):
        present = [(-float(s), int(c)) for s, c in zip(srow, crow) if 0 <= c < ntotal]
        present.sort()
        present = present[:k]
        D.append([-s + 0.0 for s, _ in present] + [-FLT_MAX] * (k - len(present)))
        I.append([c for _, c in present] + [-1] * (k - len(present)))
    return np.array(D, np.float32), np.array(I, np.int64)


def _check(S, cand, k, ntotal):
    from ivr_amd.refine import refine_order_ref
    S, cand = np.asarray(S, np.float32), np.asarray(cand, np.int64)
    D, I = refine_order_ref(S, cand, k, ntotal)
    Dp, Ip = _python_order(S, cand, k, ntotal)
    assert D.dtype == np.float32 and I.dtype == np.int64 and D.shape == I.shape == (len(S), k)
    assert np.array_equal(D.view(np.uint32), Dp.view(np.uint32)), (D, Dp)
    assert np.array_equal(I, Ip), (I, Ip)
    return D, I


def test_order_ties_between_rows_given_in_descending_row_order():
    D, I = _check([[0.5, 0.5, 0.5, 0.75]], [[9, 7, 3, 8]], 4, 10)
    assert I.tolist() == [[8, 3, 7, 9]] and D.tolist() == [[0.75, 0.5, 0.5, 0.5]]
    _check([[0.5, 0.5, 0.5, 0.75]], [[9, 7, 3, 8]], 2, 10)


def test_order_a_row_named_three_times_sits_in_adjacent_slots():
    D, I = _check([[0.25, 1.0, 0.25, 0.5, 0.25]], [[4, 1, 4, 2, 4]], 5, 10)
    assert I.tolist() == [[1, 2, 4, 4, 4]]
    D, I = _check([[0.25, 1.0, 0.25, 0.5, 0.25]], [[4, 1, 4, 2, 4]], 4, 10)
    assert I.tolist() == [[1, 2, 4, 4]]


def test_order_absent_entries_mixed_in():
    # -1, below -1, at ntotal and far above it: their scores (even the best of the list) are ignored
    S = [[9.0, 0.1, 9.0, 0.3, 9.0, 0.2, 9.0]]
    cand = [[-1, 5, 6, 0, -7, 3, 2**40]]
    D, I = _check(S, cand, 5, 6)
    assert I.tolist() == [[0, 3, 5, -1, -1]]
    assert D[0, 3:].tolist() == [-FLT_MAX, -FLT_MAX]
    # without ntotal only negative entries are absent
    from ivr_amd.refine import refine_order_ref
    assert refine_order_ref(np.array(S, np.float32), np.array(cand), 2)[1].tolist() == [[6, 2**40]]


def test_order_all_absent_list_and_k_equal_kc():
    D, I = _check([[1.0, 2.0, 3.0], [1.0, 2.0, 3.0]], [[-1, -1, -1], [2, 0, 1]], 3, 3)
    assert I.tolist() == [[-1, -1, -1], [1, 0, 2]]
    assert D[0].tolist() == [-FLT_MAX] * 3 and D[1].tolist() == [3.0, 2.0, 1.0]


def test_order_k_above_the_present_candidates_and_signed_zero():
    D, I = _check([[-0.0, 0.0, -1.0, 5.0]], [[1, 0, 2, -1]], 4, 3)
    assert I.tolist() == [[0, 1, 2, -1]]                      # -0.0 ties with +0.0: the lower row first
    assert D.view(np.uint32)[0, :2].tolist() == [0, 0]        # and is reported as +0.0
    assert D[0, 3] == -FLT_MAX


def test_order_rejects_bad_arguments():
    from ivr_amd.refine import refine_order_ref
    S = np.zeros((2, 3), np.float32)
    for k in (0, 4):
        with pytest.raises(ValueError):
            refine_order_ref(S, np.zeros((2, 3), np.int64), k)
    with pytest.raises(ValueError):
        refine_order_ref(S, np.zeros((2, 4), np.int64), 1)
