"""GPU suite of the graph index: the prune kernel, the torch link step and the search kernel against the numpy definitions of
ivr_amd/graph.py, element for element.  Wherever results are compared with the definitions the rows and queries are small integers
(randint(-3, 4)): every inner product is then exact in float32 and ties are frequent, so the tie rule is exercised throughout."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from ivr_amd import _ffi
from ivr_amd.graph import (GraphFlatIndex, IndexHNSWFlat, SearchParametersHNSW, entry_sample, graph_build_ref, graph_knn_ref,
                           graph_link_ref, graph_prune_ref, graph_search_ref, link_device)
from ivr_amd.index import FlatIPIndex, IDSelectorRange, normalize_L2

pytestmark = pytest.mark.gpu

MAX_EF, MAX_CAND = _ffi.IVR_GRAPH_MAX_EF, _ffi.IVR_GRAPH_MAX_CAND
N = 1000


def _ints(seed, n, d):
    return np.random.RandomState(seed).randint(-3, 4, size=(n, d)).astype(np.float32)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# -- 1. prune ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _prune_data(d):
    x = _ints(d, 300, d)
    x[280:] = x[:20]                                 # 20 duplicated rows
    return x, graph_knn_ref(x, MAX_CAND)


def _prune_gpu(x, cand, M):
    lib, dev = _ffi.load(), torch.device("cuda", torch.cuda.current_device())
    n, Cn = cand.shape
    h = C.c_void_p()
    _ffi.check(lib.ivr_graph_create(_ffi.context(dev.index), x.shape[1], 8, C.byref(h)), "ivr_graph_create")
    try:
        xt = torch.from_numpy(x).to(dev)
        ct = torch.from_numpy(np.ascontiguousarray(cand, dtype=np.int32)).to(dev)
        nbr = torch.full((n, M), -7, dtype=torch.int32, device=dev)
        sc = torch.full((n, M), -7.0, dtype=torch.float32, device=dev)
        _ffi.check(lib.ivr_graph_set_rows(h, C.c_void_p(xt.data_ptr()), n, _ffi.stream_ptr()), "ivr_graph_set_rows")
        assert lib.ivr_graph_ntotal(h) == n
        _ffi.check(lib.ivr_graph_prune(h, C.c_void_p(ct.data_ptr()), Cn, M, C.c_void_p(nbr.data_ptr()), C.c_void_p(sc.data_ptr()),
                                       _ffi.stream_ptr()), "ivr_graph_prune")
        torch.cuda.synchronize()
        return nbr, sc
    finally:
        lib.ivr_graph_destroy(h)


@pytest.mark.parametrize("M", [4, 32])
@pytest.mark.parametrize("Cn", [1, 15, 40, MAX_CAND])
@pytest.mark.parametrize("d", [16, 100, 512])
def test_prune_kernel_equals_the_definition(d, Cn, M):
    x, cand = _prune_data(d)
    cand = cand[:, :Cn]
    nbr, sc = _prune_gpu(x, cand, M)
    rn, rs = graph_prune_ref(x, cand, M)
    assert np.array_equal(nbr.cpu().numpy(), rn)
    assert np.array_equal(_bits(sc.cpu().numpy()), _bits(rs))
    assert (rn[:, 0] >= 0).all()                     # the first candidate is always kept


def test_prune_kernel_on_lists_that_are_mostly_empty():
    x = _ints(3, 5, 100)
    cand = np.full((5, 40), -1, np.int32)
    cand[:, :4] = graph_knn_ref(x, 4)
    nbr, sc = _prune_gpu(x, cand, 32)
    rn, rs = graph_prune_ref(x, cand, 32)
    assert np.array_equal(nbr.cpu().numpy(), rn) and np.array_equal(_bits(sc.cpu().numpy()), _bits(rs))
    assert (rn[:, 0] >= 0).all() and (rn[:, 4:] == -1).all()


# -- 2. link -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,Cn,M,R", [(16, 40, 4, 8), (100, 40, 32, 64), (16, MAX_CAND, 4, 5), (512, 15, 4, 8)])
def test_link_step_equals_the_definition(d, Cn, M, R):
    x, cand = _prune_data(d)
    nbr, sc = graph_prune_ref(x, cand[:, :Cn], M)
    dev = torch.device("cuda", torch.cuda.current_device())
    got = link_device(torch.from_numpy(nbr).to(dev), torch.from_numpy(sc).to(dev), R).cpu().numpy()
    ref = graph_link_ref(nbr, sc, R)
    assert got.dtype == np.int32 and np.array_equal(got, ref)
    # Only the small R are reached here: the heuristic keeps about ten of 40 candidates, so no row of 300 collects 64 entries.
    # The stop at a large R is covered by test_link_step_on_a_star, where one row receives far more than R offers.
    if R <= 8:
        assert ((ref >= 0).sum(1) == R).any()        # some row was filled up and had to stop at R


def test_link_step_on_a_star():
    n, R = 40, 6
    nbr = np.full((n, 2), -1, np.int32)
    nbr[1:, 0] = 0                                   # every row offers itself to row 0 ...
    nbr[0] = [3, 5]                                  # ... which already holds 3 and 5
    sc = np.zeros((n, 2), np.float32)
    sc[1:, 0] = np.random.RandomState(1).randint(0, 4, n - 1)      # many equal scores
    sc[0] = [2, 1]
    dev = torch.device("cuda", torch.cuda.current_device())
    got = link_device(torch.from_numpy(nbr).to(dev), torch.from_numpy(sc).to(dev), R).cpu().numpy()
    ref = graph_link_ref(nbr, sc, R)
    assert np.array_equal(got, ref)
    assert (ref[0] >= 0).all() and ref[0, :2].tolist() == [3, 5] and len(set(ref[0].tolist())) == R


# -- 3. search -----------------------------------------------------------------------------------------------------------------
M3 = 8


@functools.lru_cache(maxsize=None)
def _search_fixture(d):
    """One index of N integer rows per dimension with its built graph, and the hand-made graphs over the same rows."""
    x = _ints(100 + d, N, d)
    idx = GraphFlatIndex(d, M=M3)
    idx.add(x)
    built = idx.graph()
    r = np.arange(N)
    ring = np.full((N, 2 * M3), -1, np.int32)
    ring[:, :4] = np.stack([(r + 1) % N, (r - 1) % N, (r + 7) % N, (r - 7) % N], 1)
    h = N // 2
    halves = np.full((N, 2 * M3), -1, np.int32)
    lo, base = r % h, (r // h) * h
    halves[:, :4] = np.stack([(lo + 1) % h, (lo - 1) % h, (lo + 7) % h, (lo - 7) % h], 1) + base[:, None]
    loops = built.copy()
    loops[:, 0] = r                                  # self-loops
    loops[:, 1] = loops[:, 2]                        # repeated neighbours
    loops[:, 5] = loops[:, 3]
    graphs = {"built": built, "ring": ring, "halves": halves, "none": np.full((N, 2 * M3), -1, np.int32), "loops": loops}
    return x, idx, graphs


def _entries(seed, nq, ne, hi):
    e = np.random.RandomState(seed).randint(0, hi, size=(nq, ne)).astype(np.int32)
    if ne > 1:
        e[:, 1] = e[:, 0]                            # repeats
        e[::3, 2] = -1                               # and -1
    return e


SEARCH_CASES = [
    # graph, d, ef, k, ne, nq, max_expansions
    ("built", 16, 16, 10, 8, 70, N),
    ("built", 100, 17, 17, 8, 70, N),
    ("built", 512, 64, 10, 8, 70, N),
    ("built", 16, MAX_EF, MAX_EF, 8, 70, N),
    ("built", 100, MAX_EF, 10, 1, 1, N),
    ("built", 16, 1, 1, 1, 70, N),
    ("built", 16, 1, 1, 8, 1, 3),
    ("built", 100, 64, 64, 1, 70, 3),
    ("built", 512, 16, 1, 8, 1, 1),
    ("built", 512, 17, 10, 8, 70, 1),
    ("ring", 16, 64, 10, 8, 70, N),
    ("ring", 100, 17, 1, 1, 1, 3),
    ("ring", 512, 16, 16, 8, 70, N),
    ("halves", 16, 64, 64, 8, 70, N),
    ("halves", 100, 16, 10, 1, 1, N),
    ("none", 16, 16, 10, 8, 70, N),
    ("none", 512, 64, 1, 1, 1, 1),
    ("loops", 100, 16, 10, 8, 70, N),
    ("loops", 16, 17, 17, 8, 1, 3),
    ("loops", 512, 64, 10, 1, 70, N),
]


@pytest.mark.parametrize("graph,d,ef,k,ne,nq,mx", SEARCH_CASES)
def test_search_kernel_equals_the_definition(graph, d, ef, k, ne, nq, mx):
    x, idx, graphs = _search_fixture(d)
    g = graphs[graph]
    idx.set_graph(g)
    q = _ints(7 * ef + nq, nq, d)
    e = _entries(ef + ne, nq, ne, N // 2 if graph == "halves" else N)
    D, I, nexp = idx.search_from(q, k, e, efSearch=ef, max_expansions=mx, return_stats=True)
    Dr, Ir, nr = graph_search_ref(x, g, q, k, ef, e, mx)
    assert I.dtype == np.int64 and D.dtype == np.float32 and nexp.dtype == np.int32
    assert np.array_equal(I, Ir)
    assert np.array_equal(_bits(D), _bits(Dr))
    assert np.array_equal(nexp, nr)
    if graph == "halves":
        assert (I < N // 2).all()
    if graph == "none":
        assert (nexp <= min(ef, ne)).all() and (I[:, min(k, ne):] == -1).all()


def test_search_kernel_on_one_row():
    x = _ints(5, 1, 16)
    idx = GraphFlatIndex(16, M=M3)
    idx.add(x)
    assert idx.graph().tolist() == [[-1] * (2 * M3)]
    q = _ints(6, 3, 16)
    e = np.array([[0, 0, -1, 0, 0, 0, 0, 0]] * 3, np.int32)
    D, I, nexp = idx.search_from(q, 10, e, efSearch=16, max_expansions=1, return_stats=True)
    Dr, Ir, nr = graph_search_ref(x, idx.graph(), q, 10, 16, e, 1)
    assert np.array_equal(I, Ir) and np.array_equal(_bits(D), _bits(Dr)) and np.array_equal(nexp, nr)
    assert (I[:, 0] == 0).all() and (I[:, 1:] == -1).all() and nexp.tolist() == [1, 1, 1]
    idx.close()


# -- 4. full build -------------------------------------------------------------------------------------------------------------
def _entries_by_definition(x, q, n_entry, sample):
    rows = entry_sample(len(x), sample)
    s = q.astype(np.float64) @ x[rows].astype(np.float64).T
    return rows[np.argsort(-s, axis=1, kind="stable")[:, :n_entry]]


def test_full_build_and_search_equal_the_definitions():
    d, M = 24, 6
    x = _ints(11, 1300, d)
    x[990:1000] = x[:10]
    q = _ints(12, 40, d)
    idx = IndexHNSWFlat(d, M)
    idx.hnsw.entry_sample = 256
    assert idx.hnsw.efConstruction == 40 and idx.hnsw.efSearch == 16 and idx.is_trained and idx.metric_type == 0
    for n in (1000, 1300):
        idx.add(x[idx.ntotal:n])
        assert idx.ntotal == n
        g = idx.graph()
        assert g.dtype == np.int32 and g.shape == (n, 2 * M)
        assert np.array_equal(g, graph_build_ref(x[:n], M, 40))
        e = _entries_by_definition(x[:n], q, 8, 256)
        Dr, Ir, _ = graph_search_ref(x[:n], g, q, 10, 16, e, 8 * 16)
        D, I = idx.search(q, 10)
        assert np.array_equal(I, Ir) and np.array_equal(_bits(D), _bits(Dr))
        Dr, Ir, _ = graph_search_ref(x[:n], g, q, 20, 33, e, 8 * 33)
        D, I = idx.search(q, 20, SearchParametersHNSW(efSearch=33))
        assert np.array_equal(I, Ir) and np.array_equal(_bits(D), _bits(Dr))
    assert np.array_equal(idx.reconstruct_n(0, 5), x[:5]) and np.array_equal(idx.reconstruct(1299), x[1299])
    idx.reset()
    assert idx.ntotal == 0 and idx.graph().shape == (0, 2 * M)
    idx.close()


def test_add_with_a_saved_graph_installs_it_without_a_build():
    d, M = 24, 6
    x = _ints(21, 400, d)
    q = _ints(22, 20, d)
    a = GraphFlatIndex(d, M)
    a.add(x)
    g = a.graph()
    b = GraphFlatIndex(d, M)
    bad = g.copy()
    bad[7, 0] = 400
    for wrong in (bad, g[:-1], g.astype(np.float32)):
        with pytest.raises(ValueError):
            b.add(x, graph=wrong)
        assert b.ntotal == 0                         # refused before any row was stored
    b.add(x, graph=g)
    assert b.ntotal == 400 and np.array_equal(b.graph(), g) and "knn" not in b.build_times
    Da, Ia = a.search(q, 10)
    Db, Ib = b.search(q, 10)
    assert np.array_equal(Ia, Ib) and np.array_equal(_bits(Da), _bits(Db))
    a.close()
    b.close()


# -- 5. continuous rows --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [64, 768])
def test_scores_carry_the_bits_of_the_flat_search(d):
    rng = np.random.RandomState(d)
    n = 500
    x = rng.standard_normal((n, d)).astype(np.float32)
    q = rng.standard_normal((30, d)).astype(np.float32)
    flat = FlatIPIndex(d)
    flat.add(x)
    Df, If = flat.search(q, n)
    idx = GraphFlatIndex(d, M=8)
    idx.add(x)
    for ef in (16, 64):
        D, I = idx.search(q, 10, SearchParametersHNSW(efSearch=ef))
        assert (I >= 0).all()
        for i in range(len(q)):
            assert len(set(I[i].tolist())) == 10
            assert (np.diff(D[i]) <= 0).all()
            pos = {int(r): j for j, r in enumerate(If[i])}
            assert np.array_equal(_bits(D[i]), _bits(Df[i, [pos[int(r)] for r in I[i]]]))
    # a connected graph walked to the end with ef = n is the flat search
    n2 = min(250, MAX_EF)
    idx2 = GraphFlatIndex(d, M=8)
    idx2.add(x[:n2])
    g = idx2.graph()
    r = np.arange(n2)
    g[:, -2], g[:, -1] = (r - 1) % n2, (r + 1) % n2
    idx2.set_graph(g)
    flat2 = FlatIPIndex(d)
    flat2.add(x[:n2])
    Df, If = flat2.search(q, n2)
    D, I, nexp = idx2.search_from(q, n2, np.zeros((len(q), 1), np.int32), efSearch=n2, max_expansions=n2, return_stats=True)
    assert (nexp == n2).all()
    assert np.array_equal(_bits(D), _bits(Df))
    for i in range(len(q)):                          # runs of bit-equal scores are compared as sets
        for v in np.unique(_bits(D[i])):
            m = _bits(D[i]) == v
            assert sorted(I[i][m].tolist()) == sorted(If[i][m].tolist())
    for o in (flat, flat2, idx, idx2):
        o.close()


def test_normalize_q_of_the_walk_is_normalize_L2():
    """ivr_graph_search with normalize_q set gives, bit for bit, the walk of queries normalised by normalize_L2 beforehand; so does
    search_device(normalize=True).  A zero query stays zero."""
    d, n = 100, 400
    rng = np.random.RandomState(9)
    x = rng.standard_normal((n, d)).astype(np.float32)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    q = (3.0 * rng.standard_normal((70, d))).astype(np.float32)
    q[5] = 0
    qn = q.copy()
    normalize_L2(qn)
    assert np.allclose(np.linalg.norm(np.delete(qn, 5, 0), axis=1), 1, atol=1e-5) and not qn[5].any()
    idx = GraphFlatIndex(d, M=8)
    idx.add(x)
    e = _entries(4, len(q), 8, n)
    want = idx.search_from(qn, 10, e, efSearch=32, return_stats=True)
    got = idx.search_from(q, 10, e, efSearch=32, return_stats=True, normalize=True)
    plain = idx.search_from(q, 10, e, efSearch=32)
    assert np.array_equal(got[1], want[1]) and np.array_equal(_bits(got[0]), _bits(want[0])) and np.array_equal(got[2], want[2])
    assert not np.array_equal(_bits(plain[0]), _bits(want[0]))       # the flag does something
    dev = torch.device("cuda", torch.cuda.current_device())
    D1, I1 = idx.search_device(torch.from_numpy(q).to(dev), 10, normalize=True)
    D2, I2 = idx.search_device(torch.from_numpy(qn).to(dev), 10)
    assert torch.equal(I1, I2) and torch.equal(D1.view(torch.int32), D2.view(torch.int32))
    idx.close()


# -- 6. refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals_and_the_empty_index():
    with pytest.raises(ValueError):
        IndexHNSWFlat(16, 8, metric=1)
    with pytest.raises(ValueError):
        GraphFlatIndex(16, M=33)                     # degree 66 > 64
    idx = IndexHNSWFlat(16, 4)
    D, I = idx.search(np.zeros((3, 16), np.float32), 5)
    assert (I == -1).all() and (D == -np.finfo(np.float32).max).all() and I.shape == (3, 5)
    with pytest.raises(ValueError):
        idx.hnsw.efConstruction = MAX_CAND + 1
    with pytest.raises(ValueError):
        idx.add(np.zeros((4, 15), np.float32))
    x = _ints(2, 50, 16)
    idx.add(x)
    q = x[:2]
    with pytest.raises(ValueError):
        idx.search(np.zeros((2, 15), np.float32), 5)
    with pytest.raises(ValueError):
        idx.search(q, 0)
    with pytest.raises(ValueError):
        idx.search(q, MAX_EF + 1)
    with pytest.raises(ValueError):
        idx.search(q, 5, SearchParametersHNSW(efSearch=MAX_EF + 1))
    with pytest.raises(ValueError):
        idx.search(q, 5, SearchParametersHNSW(sel=IDSelectorRange(0, 10)))
    g = idx.graph()
    before = g.copy()
    bad = g.copy()
    bad[3, 1] = 50
    with pytest.raises(ValueError):
        idx.set_graph(bad)
    bad[3, 1] = -2
    with pytest.raises(ValueError):
        idx.set_graph(bad)
    with pytest.raises(ValueError):
        idx.set_graph(g[:, :4])
    with pytest.raises(ValueError):
        idx.set_graph(g.astype(np.float32))
    assert np.array_equal(idx.graph(), before)       # nothing was installed
    D, I = idx.search(q, 5)
    assert (I >= 0).all() and (D[:, 0] >= (x[:2] * x[:2]).sum(1)).all()     # the entry sample holds all 50 rows: the best is found
    idx.close()
