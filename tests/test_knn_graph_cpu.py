"""CPU suite of the neighbour graph (ivr_amd/neighbors.py, csrc/knn.hip): the numpy definition knn_graph_ref against a float64 brute
force on the seeded rows and on hand-made cases, the ABI of the three new entry points and the argument checks that need no device.
No compute call reaches a device."""
import ctypes
import re

import numpy as np
import pytest
import torch

from cluster_cases import drifting_chains
from conftest import ROOT
from ivr_amd import _ffi, neighbors
from ivr_amd.index import FlatIPIndex
from knn_cases import THRESHOLD, TOP, brute_force64, clear_rows, cosines64
from oracle.reduce_ref import flat_score_bound

NEW = ("ivr_knn_max_k", "ivr_knn_piece_rows", "ivr_index_knn_graph")
LOWEST = np.float32(-np.finfo(np.float32).max)


def scores32(X):
    """What the index computes for unit rows, in numpy float32."""
    return (X @ X.T).astype(np.float32)


# -- the definition against float64 --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,d", [(700, 20), (257, 20), (700, 512), (257, 512)])
def test_knn_graph_ref_is_the_float64_brute_force_on_clear_rows(N, d):
    """Top 10 others above 0.7 and top 10 others without a threshold: on every clear row (knn_cases.clear_rows) the float32
    definition names the float64 neighbours in the float64 order, and at least 80 % of the rows are clear."""
    X = drifting_chains(N, d)
    sim, S = cosines64(X), scores32(X)
    assert np.abs(S.astype(np.float64) - sim).max() < flat_score_bound(d, 1.0)
    for threshold in (THRESHOLD, None):
        D, I, count = neighbors.knn_graph_ref(S, TOP, None, threshold)
        assert D.dtype == np.float32 and I.dtype == np.int64 and count.dtype == np.int32
        assert D.shape == I.shape == (N, TOP) and count.shape == (N,)
        want = brute_force64(sim, TOP, threshold)
        clear = clear_rows(sim, TOP, threshold, d)
        print(f"N={N} d={d} threshold={threshold}: {int(clear.sum())} of {N} rows clear")
        assert clear.sum() >= 0.8 * N, f"{int(clear.sum())} of {N} rows are clear"
        for j in np.flatnonzero(clear).tolist():
            assert I[j, :count[j]].tolist() == want[j] and count[j] == len(want[j]), f"row {j}"
            assert (I[j, count[j]:] == -1).all() and (D[j, count[j]:] == LOWEST).all()
            assert np.abs(D[j, :count[j]] - sim[j, want[j]]).max(initial=0) < flat_score_bound(d, 1.0)
        if threshold is not None:
            assert ((count > 0) & (count < TOP)).any() and (count == TOP).any()


def hand_scores():
    S = np.full((6, 6), 9.0, np.float32)                   # the diagonal is larger than anything: never reported
    S[0, 1:] = [0.8, 0.8, 0.95, 0.95, 0.95]                # a tie: the lower row first
    S[1, [0, 2, 3, 4, 5]] = [np.float32(0.7), 0.75, 1, 1, 1]       # a score equal to float32(0.7)
    S[2, [0, 1, 3, 4, 5]] = [0.2, np.nan, 0.5, 0.6, -np.inf]
    S[3, [0, 1, 2, 4, 5]] = [1, 1, 1, 0.71, 1]
    S[4, [0, 1, 2, 3, 5]] = [0.3, 0.1, 0.2, -0.0, 0.25]
    S[5, :5] = [0.9, 0.9, 0.9, 0.9, 0.9]
    return S


def test_hand_made_cases_segments_threshold_ties_and_padding():
    S = hand_scores()
    seg = np.array([0, 3, 3, 5], np.int64)                 # [0,3) [3,3) empty [3,5); row 5 lies past the last offset
    D, I, count = neighbors.knn_graph_ref(S, 2, seg, 0.7)
    assert I.tolist() == [[1, 2], [2, -1], [-1, -1], [4, -1], [-1, -1], [-1, -1]]
    assert count.tolist() == [2, 1, 0, 1, 0, 0]
    want = np.array([[0.8, 0.8], [0.75, LOWEST], [LOWEST, LOWEST], [0.71, LOWEST], [LOWEST, LOWEST], [LOWEST, LOWEST]], np.float32)
    assert np.array_equal(D.view(np.uint32), want.view(np.uint32))
    # just below float32(0.7) the pair (1, 0) comes in; the comparison is made in float32, so the double 0.7 rounds first
    below = float(np.nextafter(np.float32(0.7), np.float32(0)))
    D, I, count = neighbors.knn_graph_ref(S, 2, seg, below)
    assert I[1].tolist() == [2, 0] and count.tolist() == [2, 2, 0, 1, 0, 0]
    # no threshold, no segments, k beyond the row count: NaN is no candidate, -inf is one, -0.0 is reported as +0.0
    D, I, count = neighbors.knn_graph_ref(S, 6)
    assert count.tolist() == [5, 5, 4, 5, 5, 5]
    assert I[0].tolist() == [3, 4, 5, 1, 2, -1] and I[2].tolist() == [4, 3, 0, 5, -1, -1] and I[4].tolist() == [0, 5, 2, 1, 3, -1]
    assert D[2, 3] == -np.inf and D[4, 4].view(np.uint32) == 0 and (D[:, 5] == LOWEST).all()
    # a threshold of -inf given as a number is "none" too, +inf keeps nothing
    assert all(np.array_equal(a, b) for a, b in zip(neighbors.knn_graph_ref(S, 6, None, -np.inf), (D, I, count)))
    assert neighbors.knn_graph_ref(S, 6, None, np.inf)[2].tolist() == [0] * 6
    # one segment over everything is the call without segments; offsets past the rows are clipped
    assert all(np.array_equal(a, b) for a, b in zip(neighbors.knn_graph_ref(S, 6, [0, 6]), (D, I, count)))
    assert all(np.array_equal(a, b) for a, b in zip(neighbors.knn_graph_ref(S, 6, [-2, 9]), (D, I, count)))
    # a segment of one row has no neighbours; row 2's only candidate scores NaN
    assert neighbors.knn_graph_ref(S, 1, [0, 1, 3])[2].tolist() == [0, 1, 0, 0, 0, 0]
    with pytest.raises(ValueError):
        neighbors.knn_graph_ref(np.zeros((2, 3), np.float32), 1)


# -- ABI and surfaces ------------------------------------------------------------------------------------------------------------------
def _header():
    return re.sub(r"/\*.*?\*/", "", open(f"{ROOT}/include/ivr_api.h").read(), flags=re.S)


def _ctype_of(decl):
    decl = decl.strip()
    if "*" in decl or decl.startswith("ivr_stream"):
        return ctypes.c_void_p
    return {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "float": ctypes.c_float}[decl.split()[0]]


@pytest.mark.parametrize("name,names", [
    (NEW[0], []), (NEW[1], []),
    (NEW[2], ["idx", "k", "seg_off", "nseg", "threshold", "D", "I", "count", "stream"])])
def test_header_binding_and_library_agree(name, names):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", _header())
    assert m, f"{name} not declared in ivr_api.h"
    params = [p.strip() for p in m.group(1).split(",") if p.strip() != "void"]
    assert [re.sub(r"[\s*]+", " ", p).split()[-1] for p in params] == names
    res, args = _ffi._SIGS[name]
    assert res is ctypes.c_int and args == [_ctype_of(p) for p in params]
    if names:
        assert _ffi._STREAM[name] == len(params) - 1 and name not in _ffi._VALUE
    else:
        assert name not in _ffi._STREAM and name in _ffi._VALUE
    assert name in _ffi.EXPORTS
    assert hasattr(ctypes.CDLL(_ffi.LIB_PATH), name)


def test_api_version_is_still_11_and_no_class_grew_a_method():
    assert _ffi.API_VERSION == 11 and _ffi.load().ivr_api_version() == 11
    assert re.search(r"#define\s+IVR_API_VERSION\s+11\b", _header())
    assert not [n for n in dir(FlatIPIndex) if "knn" in n.lower() or "neighbo" in n.lower()]


def test_limits_of_the_library():
    assert re.search(r"#define\s+IVR_KNN_MAX_K\s+64\b", _header())
    assert neighbors.knn_max_k() == _ffi.IVR_KNN_MAX_K == 64
    rows = _ffi.call("ivr_knn_piece_rows")
    assert rows >= 64 and rows % 16 == 0


def test_library_rejects_bad_arguments_before_any_device_call():
    lib = _ffi.load()
    assert lib.ivr_index_knn_graph(None, 10, None, 0, 0.7, None, None, None, None) == -1
    assert b"NULL" in lib.ivr_last_error(None)
    fake = ctypes.create_string_buffer(64)                 # stands for the handle and the outputs: a rejected call reads none of them
    p = ctypes.cast(fake, ctypes.c_void_p)
    for k in (0, -3, 65):
        assert lib.ivr_index_knn_graph(p, k, None, 0, 0.7, p, p, p, None) == -1
        assert f"k={k} outside [1,64]".encode() in lib.ivr_last_error(None)
    assert lib.ivr_index_knn_graph(p, 10, None, 0, float("nan"), p, p, p, None) == -1
    assert b"NaN" in lib.ivr_last_error(None)
    assert lib.ivr_index_knn_graph(p, 10, p, 0, 0.7, p, p, p, None) == -1
    assert b"nseg=0" in lib.ivr_last_error(None)


def test_lazy_package_exports_resolve():
    import ivr_amd
    for name in ("knn_graph", "knn_graph_device", "knn_graph_ref", "similarity_graphs", "build_similarity_relationships"):
        assert name in ivr_amd.__all__
        assert getattr(ivr_amd, name) is getattr(neighbors, name)
    assert neighbors.SIMILAR_TOP == 10 and neighbors.SIMILAR_THRESHOLD == 0.7


def test_argument_checks_name_the_offending_values():
    index = FlatIPIndex.__new__(FlatIPIndex)             # no handle: every check below fails before the library is called
    index.d, index.device = 8, torch.device("cpu")
    with pytest.raises(ValueError, match="FlatIPIndex"):
        neighbors.knn_graph_device(object(), 10)
    with pytest.raises(ValueError, match=r"k=0 outside \[1,64\]"):
        neighbors.knn_graph_device(index, 0)
    with pytest.raises(ValueError, match=r"k=65 outside \[1,64\]"):
        neighbors.knn_graph_device(index, 65)
    with pytest.raises(ValueError, match="k must be an integer, got float"):
        neighbors.knn_graph_device(index, 2.0)
    with pytest.raises(ValueError, match="k must be an integer, got bool"):
        neighbors.knn_graph_device(index, True)
    with pytest.raises(ValueError, match=r"threshold=nan is NaN"):
        neighbors.knn_graph_device(index, 10, threshold=float("nan"))
    with pytest.raises(ValueError, match="threshold must be a number, got str"):
        neighbors.knn_graph_device(index, 10, threshold="0.7")
    with pytest.raises(ValueError, match=r"seg_off\[1\]=5 > seg_off\[2\]=3"):
        neighbors.knn_graph_device(index, 10, seg_off=np.array([0, 5, 3]))
    with pytest.raises(ValueError, match="integers"):
        neighbors.knn_graph_device(index, 10, seg_off=np.array([0.0, 5.0]))
    with pytest.raises(ValueError, match=r"\[nseg\+1\]"):
        neighbors.knn_graph_device(index, 10, seg_off=np.array([0]))
    with pytest.raises(ValueError, match=r"k=65 outside"):
        neighbors.knn_graph_ref(np.zeros((2, 2), np.float32), 65)
    # the reference's early return needs no device either: nothing but folders of fewer than two rows
    assert neighbors.build_similarity_relationships({}) == {}
    assert neighbors.build_similarity_relationships({"a": (np.ones((1, 4), np.float32), ["x"])}) == {}
    with pytest.raises(ValueError, match="features"):
        neighbors.build_similarity_relationships({"a": (np.ones((3, 4), np.float32), ["x"])})
