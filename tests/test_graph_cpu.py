"""CPU suite of the graph index (ivr_amd/graph.py, csrc/search_graph.hip): the ABI of the new entry points, the numpy definitions
on hand-made cases, and the quality of the definition itself (so that the GPU tests can be pure equality tests).  No compute call
reaches a device."""
import ctypes
import re

import numpy as np

from conftest import ROOT
from ivr_amd import _ffi
from ivr_amd.graph import graph_build_ref, graph_link_ref, graph_prune_ref, graph_search_ref

NEW = ["ivr_graph_max_ef", "ivr_graph_max_cand", "ivr_graph_create", "ivr_graph_destroy", "ivr_graph_reset", "ivr_graph_ntotal",
       "ivr_graph_set_rows", "ivr_graph_prune", "ivr_graph_set_neighbors", "ivr_graph_search"]


def _header():
    src = open(f"{ROOT}/include/ivr_api.h").read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def test_header_binding_and_library_agree_on_the_new_symbols():
    declared = set(re.findall(r"\b(ivr_[a-z0-9_]+)\s*\(", _header()))
    lib = ctypes.CDLL(_ffi.LIB_PATH)
    for name in NEW:
        assert name in declared, f"{name} not declared in ivr_api.h"
        assert name in _ffi.EXPORTS, f"{name} not bound in _ffi"
        assert hasattr(lib, name), f"{name} not exported by the library"


def test_limits_agree_and_are_large_enough():
    lib = _ffi.load()
    ef = int(re.search(r"#define\s+IVR_GRAPH_MAX_EF\s+(\d+)", _header()).group(1))
    cand = int(re.search(r"#define\s+IVR_GRAPH_MAX_CAND\s+(\d+)", _header()).group(1))
    assert ef == lib.ivr_graph_max_ef() == _ffi.IVR_GRAPH_MAX_EF and ef >= 256
    assert cand == lib.ivr_graph_max_cand() == _ffi.IVR_GRAPH_MAX_CAND and cand >= 64
    assert _ffi.IVR_GRAPH_MAX_DEGREE <= 64


def test_api_version_is_still_11():
    assert _ffi.API_VERSION == 11
    assert _ffi.load().ivr_api_version() == 11
    assert re.search(r"#define\s+IVR_API_VERSION\s+11\b", _header())


def test_null_handles_are_rejected():
    lib = _ffi.load()
    out = ctypes.c_void_p()
    assert lib.ivr_graph_create(None, 64, 16, ctypes.byref(out)) == -1
    assert b"NULL" in lib.ivr_last_error(None)
    assert lib.ivr_graph_reset(None) == -1
    assert b"NULL" in lib.ivr_last_error(None)
    assert lib.ivr_graph_set_rows(None, None, 1, None) == -1
    assert b"NULL" in lib.ivr_last_error(None)
    assert lib.ivr_graph_prune(None, None, 1, 1, None, None, None) == -1
    assert b"NULL" in lib.ivr_last_error(None)
    assert lib.ivr_graph_set_neighbors(None, None, 1, None) == -1
    assert b"NULL" in lib.ivr_last_error(None)
    assert lib.ivr_graph_search(None, None, 1, 1, 1, None, 1, 1, 0, None, None, None, None) == -1
    assert b"NULL" in lib.ivr_last_error(None)
    assert lib.ivr_graph_ntotal(None) == 0
    assert lib.ivr_graph_destroy(None) == 0


# -- the definitions on hand-made cases ------------------------------------------------------------------------------------------
def test_prune_keeps_the_first_and_drops_what_a_kept_one_is_closer_to():
    # base 0 = (2,0): <0,1> = 4, <0,2> = 4, <0,3> = 2.  1 is kept (the first always is); 2: <2,1> = 6 > <0,2> = 4, dropped;
    # 3: <3,1> = -1 <= <0,3> = 2, kept
    x = np.array([[2, 0], [2, 1], [2, 2], [1, -3]], np.float32)
    cand = np.full((4, 3), -1, np.int32)
    cand[0] = [1, 2, 3]
    nbr, sc = graph_prune_ref(x, cand, 3)
    assert nbr.dtype == np.int32 and sc.dtype == np.float32 and nbr.shape == sc.shape == (4, 3)
    assert nbr[0].tolist() == [1, 3, -1] and sc[0].tolist() == [4.0, 2.0, 0.0]
    assert (nbr[1:] == -1).all() and (sc[1:] == 0).all()
    nbr, sc = graph_prune_ref(x, cand, 1)            # stops at M kept
    assert nbr[0].tolist() == [1] and sc[0].tolist() == [4.0]
    cand[0] = [3, 1, 2]                              # whatever comes first is kept
    assert graph_prune_ref(x, cand, 3)[0][0, 0] == 3


def test_link_skips_a_present_row_and_stops_at_R():
    nbr = np.array([[1, 2], [0, -1], [-1, -1], [2, -1]], np.int32)
    sc = np.array([[5, 3], [5, 0], [0, 0], [7, 0]], np.float32)
    g = graph_link_ref(nbr, sc, 3)
    assert g.dtype == np.int32
    # row 0: the offer of 1 (1 -> 0) is skipped, 1 is a forward neighbour already; row 2: offers 3 (score 7) before 0 (score 3)
    assert g.tolist() == [[1, 2, -1], [0, -1, -1], [3, 0, -1], [2, -1, -1]]
    assert graph_link_ref(nbr, sc, 1).tolist() == [[1], [0], [3], [2]]
    # a star: rows 1 .. 6 all point at row 0, equal scores offer the lower row first, a better score goes in front of them
    star = np.full((7, 1), -1, np.int32)
    star[1:] = 0
    ssc = np.zeros((7, 1), np.float32)
    ssc[1:] = 1
    ssc[5] = 2
    assert graph_link_ref(star, ssc, 4)[0].tolist() == [5, 1, 2, 3]


def _two_components():
    x = np.array([[3, 0], [2, 0], [1, 0], [3, 1], [2, 1], [1, 1]], np.float32)
    graph = np.array([[1, -1], [0, 2], [1, -1], [4, -1], [3, 5], [4, -1]], np.int32)
    return x, graph


def test_search_stays_in_the_component_of_its_entry_and_pads():
    x, graph = _two_components()
    q = np.array([[1, 1]], np.float32)
    D, I, nexp = graph_search_ref(x, graph, q, 5, 5, [[2]], 100)
    assert D.dtype == np.float32 and I.dtype == np.int64 and nexp.dtype == np.int32
    assert I.tolist() == [[0, 1, 2, -1, -1]] and nexp.tolist() == [3]
    assert D[0, :3].tolist() == [3.0, 2.0, 1.0] and (D[0, 3:] == -np.finfo(np.float32).max).all()
    D, I, nexp = graph_search_ref(x, graph, q, 2, 5, [[4]], 100)
    assert I.tolist() == [[3, 4]] and D.tolist() == [[4.0, 3.0]] and nexp.tolist() == [3]


def test_search_max_expansions_and_entry_cleaning():
    x, graph = _two_components()
    q = np.array([[1, 0]], np.float32)
    D, I, nexp = graph_search_ref(x, graph, q, 3, 3, [[2]], 1)
    assert nexp.tolist() == [1] and I.tolist() == [[1, 2, -1]]               # 2 was expanded, 1 found, 0 not reached
    a = graph_search_ref(x, graph, q, 3, 3, [[2, 2, -1, 1, 99]], 100)
    b = graph_search_ref(x, graph, q, 3, 3, [[1, 2]], 100)
    for u, v in zip(a, b):
        assert np.array_equal(u, v)
    # ef cuts the entries: with ef = 1 only the best entry survives
    D, I, nexp = graph_search_ref(x, graph, q, 1, 1, [[2, 1]], 100)
    assert I.tolist() == [[0]] and nexp.tolist() == [2]


def test_build_of_one_row_and_of_duplicates():
    assert graph_build_ref(np.ones((1, 4), np.float32), 2, 40).tolist() == [[-1, -1, -1, -1]]
    x = np.array([[1, 0], [1, 0], [0, 1]], np.float32)      # row 1 duplicates row 0: left out by number, so each has the other
    g = graph_build_ref(x, 2, 40)
    assert g.shape == (3, 4) and g[0, 0] == 1 and g[1, 0] == 0


def test_the_definition_reaches_high_recall():
    """recall@10 of graph_search_ref at ef = 64 on 3,000 clustered unit rows, M = 8, efConstruction = 40, 8 entries out of a
    256-row sample: measured 0.998 (499 of 500 hits), mean out-degree 9.5, at most 64 expansions; the bound is 0.95."""
    rng = np.random.RandomState(0)
    cen = rng.randn(30, 32)

    def draw(n):
        v = cen[rng.randint(30, size=n)] + rng.randn(n, 32)
        return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)

    x, q = draw(3000), draw(50)
    graph = graph_build_ref(x, 8, 40)
    assert graph.shape == (3000, 16)
    sample = np.sort(rng.permutation(3000)[:256])
    s = q.astype(np.float64) @ x.astype(np.float64).T
    entries = sample[np.argsort(-s[:, sample], axis=1, kind="stable")[:, :8]]
    D, I, nexp = graph_search_ref(x, graph, q, 10, 64, entries, 8 * 64)
    truth = np.argsort(-s, axis=1, kind="stable")[:, :10]
    hits = sum(len(set(I[i].tolist()) & set(truth[i].tolist())) for i in range(50))
    print(f"recall@10 = {hits / 500:.3f}, mean out-degree = {(graph >= 0).sum(1).mean():.2f}, max expansions = {nexp.max()}")
    assert hits >= 475
    assert nexp.max() <= 64 + 64
