"""GPU suite: every index class gives one answer whatever form the queries arrive in - a host array that is staged, a tensor that is
converted or compacted on the way, a CUDA tensor used in place, a single vector - and refuses the other forms with fixed texts.
Public methods only; the shapes are the smallest that take every staging path."""
import re

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

D_, NQ, K = 24, 3, 5
DEV = "cuda:0"
EMPTY = r"^ivr_index_search: ivr_index_search: (NULL argument|nq=0)$"


def _unit(seed, n, d=D_):
    x = np.random.default_rng(seed).standard_normal((n, d)).astype(np.float32)
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def _view(a):
    """A non-contiguous CUDA view holding `a`: odd storage offset, row stride wider than the row."""
    wide = torch.zeros((a.shape[0], 2 * a.shape[1] + 1), dtype=torch.from_numpy(a[:1]).dtype, device=DEV)
    v = wide[:, 1:a.shape[1] + 1]
    v.copy_(torch.from_numpy(a))
    assert not v.is_contiguous()
    return v


def _forms(Q):
    """name -> (queries, rows of Q they hold)."""
    return {
        "numpy_f64": (Q.astype(np.float64), slice(None)),
        "numpy_fortran": (np.asfortranarray(Q), slice(None)),
        "cpu_tensor": (torch.from_numpy(Q.copy()), slice(None)),
        "cpu_tensor_f64": (torch.from_numpy(Q.astype(np.float64)), slice(None)),
        "cuda": (torch.from_numpy(Q).to(DEV), slice(None)),
        "cuda_f64": (torch.from_numpy(Q.astype(np.float64)).to(DEV), slice(None)),
        "cuda_view": (_view(Q), slice(None)),
        "one_numpy": (Q[1].copy(), slice(1, 2)),
    }


def _raises(exc, text):
    return pytest.raises(exc, match="^" + re.escape(text) + "$")


def _same(index, Q, forms, device_too=True, **kw):
    """Every form gives what the numpy float32 (uint8) array of the same rows gives; returns that answer for all of Q."""
    base = index.search(Q, K, **kw)
    assert base[1].dtype == np.int64 and base[1].shape == (len(Q), K) and (base[1] >= 0).all()
    for name, (q, rows) in forms.items():
        Db, Ib = base if rows == slice(None) else index.search(Q[rows], K, **kw)
        D, I = index.search(q, K, **kw)
        assert isinstance(D, np.ndarray) and D.dtype == Db.dtype and I.dtype == np.int64, name
        assert np.array_equal(D, Db) and np.array_equal(I, Ib), name
        if device_too and getattr(q, "ndim", 2) == 2:
            Dd, Id = index.search_device(q, K)
            assert Dd.is_cuda and Id.is_cuda and Id.dtype == torch.int64, name
            assert np.array_equal(Dd.cpu().numpy(), Db) and np.array_equal(Id.cpu().numpy(), Ib), name
    return base


@pytest.fixture(scope="module")
def Q():
    return _unit(11, NQ)


# -- FlatIPIndex -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def flat():
    from ivr_amd.index import FlatIPIndex
    idx = FlatIPIndex(D_)
    idx.add(_unit(1, 200))
    yield idx
    idx.close()


def test_flat_every_query_form(flat, Q):
    from ivr_amd.index import IDSelectorRange, SearchParameters
    forms = _forms(Q)
    forms["list"] = (Q.tolist(), slice(None))                  # search() takes what numpy.asarray takes
    forms["one_list"] = (Q[1].tolist(), slice(1, 2))
    base = _same(flat, Q, {n: f for n, f in forms.items() if "list" not in n})
    assert base[0].dtype == np.float32 and (np.diff(base[0], axis=1) <= 0).all()
    _same(flat, Q, {n: f for n, f in forms.items() if "list" in n}, device_too=False)
    sel = SearchParameters(sel=IDSelectorRange(20, 120))
    fbase = _same(flat, Q, forms, device_too=False, params=sel)
    assert ((fbase[1] >= 20) & (fbase[1] < 120)).all()
    Db, Ib, Rb = flat.search_and_reconstruct(Q, K)
    assert np.array_equal(Db, base[0]) and np.array_equal(Ib, base[1]) and np.array_equal(Rb, flat.reconstruct_n()[Ib])
    for name, (q, rows) in forms.items():
        for got, want in zip(flat.search_and_reconstruct(q, K), flat.search_and_reconstruct(Q[rows], K)):
            assert np.array_equal(got, want), name
        for got, want in zip(flat.range_search(q, 0.3), flat.range_search(Q[rows], 0.3)):
            assert np.array_equal(got, want), name
    # a CUDA tensor that is used in place may be handed over as the output's producer: no copy, same answer
    out = (torch.empty((NQ, K), dtype=torch.float32, device=DEV), torch.empty((NQ, K), dtype=torch.int64, device=DEV))
    Dd, Id = flat.search_device(forms["cuda"][0], K, out=out)
    assert Dd is out[0] and Id is out[1] and np.array_equal(Id.cpu().numpy(), base[1])


def test_flat_refused_forms(flat, Q):
    from ivr_amd.index import IDSelectorRange, SearchParameters
    one = torch.from_numpy(Q[1]).to(DEV)
    with _raises(ValueError, "Query dimension ((24,)) != index dimension (24)"):
        flat.search(one, K)                                     # search() reshapes a numpy vector only
    with _raises(ValueError, "Query dimension ((24,)) != index dimension (24)"):
        flat.search_device(Q[1], K)
    with _raises(ValueError, "Query dimension ((24,)) != index dimension (24)"):
        flat.search_and_reconstruct_device(Q[1], K)
    with _raises(ValueError, "Query dimension ((3, 25)) != index dimension (24)"):
        flat.search(_unit(2, NQ, 25), K)
    with _raises(ValueError, "Query dimension ((3, 25)) != index dimension (24)"):
        flat.range_search(_unit(2, NQ, 25), 0.5)
    with _raises(ValueError, "expected a numpy array or a torch tensor"):
        flat.search_device(Q.tolist(), K)
    for k in (0, 2049):
        with _raises(ValueError, f"k={k} outside [1,2048]"):
            flat.search(Q, k)
        with _raises(ValueError, f"k={k} outside [1,2048]"):
            flat.search_and_reconstruct(Q, k)
    with _raises(ValueError, "range_search: no queries"):
        flat.range_search(np.zeros((0, D_), np.float32), 0.5)
    with pytest.raises(ValueError, match=EMPTY):                # the library's own refusal, under the name of the call
        flat.search(np.zeros((0, D_), np.float32), K)
    # the order of the checks: selector, then dimension, then k
    with _raises(ValueError, "sel must be an IDSelectorRange / IDSelectorBatch / IDSelectorBitmap, got int"):
        flat.search_device(_unit(2, NQ, 25), 0, sel=3)
    with _raises(ValueError, "params must be a SearchParameters, got IDSelectorRange"):
        flat.search(_unit(2, NQ, 25), 0, params=IDSelectorRange(0, 1))
    with _raises(ValueError, "Query dimension ((3, 25)) != index dimension (24)"):
        flat.search(_unit(2, NQ, 25), 0, params=SearchParameters())
    for what, call in (("add", flat.add), ("add_with_ids", lambda x: flat.add_with_ids(x, np.arange(len(x)))),
                       ("update_vectors", lambda x: flat.update_vectors(np.arange(len(x)), x))):
        with _raises(ValueError, f"{what} expects [n,24], got (3, 25)"):
            call(_unit(2, NQ, 25))
    assert flat.ntotal == 200


# -- IVFFlatIndex ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ivf():
    from ivr_amd.ivf import IVFFlatIndex
    X = _unit(3, 300)
    idx = IVFFlatIndex(D_, 4)
    idx.train(X)
    idx.add(X)
    idx.nprobe = 2
    yield idx
    idx.close()


def test_ivf_every_query_form(ivf, Q):
    from ivr_amd.ivf import SearchParametersIVF
    forms = _forms(Q)
    forms["one_cuda"] = (torch.from_numpy(Q[1]).to(DEV), slice(1, 2))           # a 1-D tensor is one query here
    forms["list"] = (Q.tolist(), slice(None))
    assert _same(ivf, Q, forms)[0].dtype == np.float32
    _same(ivf, Q, forms, device_too=False, params=SearchParametersIVF(nprobe=4))
    # search_preassigned: the integer table in every form it is taken in
    assign = np.array([[0, 1], [3, -1], [2, 2]], np.int64)
    pbase = ivf.search_preassigned(Q, K, assign)
    for a in (assign.astype(np.int32), np.asfortranarray(assign), torch.from_numpy(assign), torch.from_numpy(assign).to(DEV),
              torch.from_numpy(assign.astype(np.int16)).to(DEV)):
        for q in (Q, forms["cuda"][0], forms["cuda_view"][0]):
            D, I = ivf.search_preassigned(q, K, a)
            assert np.array_equal(D, pbase[0]) and np.array_equal(I, pbase[1])
    for got, want in zip(ivf.search_preassigned(Q[1], K, assign[1:2]), ivf.search_preassigned(Q[1:2], K, assign[1:2])):
        assert np.array_equal(got, want)


def test_ivf_refused_forms(ivf, Q):
    from ivr_amd.index import IDSelectorRange, SearchParameters
    from ivr_amd.ivf import SearchParametersIVF
    with _raises(ValueError, "Query dimension ((3, 25)) != index dimension (24)"):
        ivf.search(_unit(2, NQ, 25), K)
    with _raises(ValueError, "k=0 outside [1,2048]"):
        ivf.search(Q, 0)
    with pytest.raises(ValueError, match=EMPTY):                # the coarse search refuses first
        ivf.search(np.zeros((0, D_), np.float32), K)
    with _raises(ValueError, "search: no queries"):
        ivf.search(np.zeros((0, D_), np.float32), K, params=SearchParametersIVF(nprobe=4))
    with _raises(ValueError, "params must be a SearchParametersIVF, got SearchParameters"):
        ivf.search(Q, K, params=SearchParameters())
    with _raises(ValueError, "search: ID selectors are not supported on IVFFlatIndex"):
        ivf.search(Q, K, params=SearchParametersIVF(sel=IDSelectorRange(0, 5)))
    with _raises(ValueError, "search_preassigned: assign must be integers, got float32"):
        ivf.search_preassigned(Q, K, np.zeros((NQ, 2), np.float32))
    for bad in (torch.zeros((NQ, 2)), torch.zeros((NQ, 2), dtype=torch.bool), [[0, 1]] * NQ):
        with _raises(ValueError, "search_preassigned: assign must be an integer numpy array or torch tensor"):
            ivf.search_preassigned(Q, K, bad)
    for bad in (np.zeros((NQ + 1, 2), np.int64), np.zeros(NQ, np.int64), np.zeros((NQ, 0), np.int64)):
        with _raises(ValueError, f"search_preassigned: assign must be [3,p] with p >= 1, got {bad.shape}"):
            ivf.search_preassigned(Q, K, bad)
    for bad in (4, -2):
        with _raises(ValueError, "search_preassigned: assign entries must lie in [-1, 4)"):
            ivf.search_preassigned(Q, K, np.array([[0, 1], [bad, 1], [2, 3]]))
    with _raises(ValueError, "add expects [n,24], got (3, 25)"):
        ivf.add(_unit(2, NQ, 25))
    with _raises(ValueError, "add_with_ids expects [n,24], got (24,)"):
        ivf.add_with_ids(Q[0], np.arange(1))
    assert ivf.ntotal == 300


# -- GraphFlatIndex ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def graph():
    from ivr_amd.graph import GraphFlatIndex
    idx = GraphFlatIndex(D_, M=4)
    idx.add(_unit(4, 200))
    yield idx
    idx.close()


def test_graph_every_query_form(graph, Q):
    from ivr_amd.graph import SearchParametersHNSW
    forms = _forms(Q)
    forms["one_cuda"] = (torch.from_numpy(Q[1]).to(DEV), slice(1, 2))
    forms["list"] = (Q.tolist(), slice(None))
    base = _same(graph, Q, forms)
    assert base[0].dtype == np.float32
    _same(graph, Q, forms, device_too=False, params=SearchParametersHNSW(efSearch=40))
    # search_from: entries as numpy of any integer dtype or nested lists; out-of-range entries are skipped
    entries = np.array([[0, 7], [199, -1], [5, 5]], np.int64)
    fbase = graph.search_from(Q, K, entries, return_stats=True)
    assert fbase[2].dtype == np.int32 and fbase[2].shape == (NQ,)
    for e in (entries.astype(np.int32), np.asfortranarray(entries), entries.tolist()):
        for q in (Q, forms["numpy_f64"][0], forms["cuda_view"][0]):
            for got, want in zip(graph.search_from(q, K, e, return_stats=True), fbase):
                assert np.array_equal(got, want)
    D, I = graph.search_from(Q, K, np.concatenate([entries, [[2**40], [-9], [200]]], axis=1))
    assert np.array_equal(D, fbase[0]) and np.array_equal(I, fbase[1])
    # set_graph: the table in every form it is taken in installs the same graph
    table = graph.graph()
    assert table.dtype == np.int32 and table.shape == (200, 8)
    for g in (table.astype(np.int64), torch.from_numpy(table), torch.from_numpy(table).to(DEV), np.asfortranarray(table)):
        graph.set_graph(g)
        assert np.array_equal(graph.graph(), table)
        D, I = graph.search(Q, K)
        assert np.array_equal(D, base[0]) and np.array_equal(I, base[1])


def test_graph_refused_forms(graph, Q):
    from ivr_amd.graph import SearchParametersHNSW
    from ivr_amd.index import IDSelectorRange, SearchParameters
    table = graph.graph()
    with _raises(ValueError, "Query dimension ((3, 25)) != index dimension (24)"):
        graph.search(_unit(2, NQ, 25), K)
    for k in (0, 257):
        with _raises(ValueError, f"k={k} outside [1,256]"):
            graph.search(Q, k)
    with _raises(ValueError, "search: no queries"):
        graph.search(np.zeros((0, D_), np.float32), K)
    with _raises(ValueError, "params must be a SearchParametersHNSW, got SearchParameters"):
        graph.search(Q, K, params=SearchParameters())
    with _raises(ValueError, "search: ID selectors are not supported on GraphFlatIndex"):
        graph.search(Q, K, params=SearchParametersHNSW(sel=IDSelectorRange(0, 5)))
    with _raises(ValueError, "set_graph: the graph must hold integers, got float32"):
        graph.set_graph(table.astype(np.float32))
    for bad in (torch.from_numpy(table).float(), torch.from_numpy(table).bool(), table.tolist()):
        with _raises(ValueError, "set_graph: the graph must be an integer numpy array or torch tensor"):
            graph.set_graph(bad)
    with _raises(ValueError, "set_graph: expected [200,8], got (199, 8)"):
        graph.set_graph(table[:199])
    for bad in (200, -2):
        g = table.copy()
        g[17, 3] = bad
        with _raises(ValueError, "set_graph: entries must lie in [-1, 200)"):
            graph.set_graph(g)
    with _raises(ValueError, "add: expected [203,8], got (200, 8)"):
        graph.add(_unit(5, 3), graph=table)
    for bad in (np.zeros((NQ, 1), np.float32), np.zeros(NQ, np.int64), np.zeros((NQ + 1, 1), np.int64), np.zeros((NQ, 65), np.int64)):
        with _raises(ValueError, "search_from: entries must be integers [3,1..64]"):
            graph.search_from(Q, K, bad)
    with _raises(ValueError, "add expects [n,24], got (3, 25)"):
        graph.add(_unit(2, NQ, 25))
    assert graph.ntotal == 200 and np.array_equal(graph.graph(), table)


# -- BinaryFlatIndex ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def binary():
    from ivr_amd.binary import BinaryFlatIndex
    idx = BinaryFlatIndex(64)
    idx.add(np.random.default_rng(6).integers(0, 256, (300, 8), dtype=np.uint8))
    yield idx
    idx.close()


def test_binary_every_query_form(binary):
    C = np.random.default_rng(7).integers(0, 256, (NQ, 8), dtype=np.uint8)
    forms = {
        "numpy_fortran": (np.asfortranarray(C), slice(None)),
        "cpu_tensor": (torch.from_numpy(C.copy()), slice(None)),
        "cuda": (torch.from_numpy(C).to(DEV), slice(None)),
        "cuda_view": (_view(C), slice(None)),
        "one_numpy": (C[1].copy(), slice(1, 2)),
        "one_cuda": (torch.from_numpy(C[1]).to(DEV), slice(1, 2)),
    }
    base = _same(binary, C, forms)
    assert base[0].dtype == np.int32 and (np.diff(base[0], axis=1) >= 0).all()
    Dd, Id = binary.search_device(forms["one_cuda"][0], K)
    Db, Ib = binary.search(C[1:2], K)
    assert np.array_equal(Dd.cpu().numpy(), Db) and np.array_equal(Id.cpu().numpy(), Ib)
    # add takes the same forms: the stored codes are the same bytes
    from ivr_amd.binary import BinaryFlatIndex
    other = BinaryFlatIndex(64)
    for c, _ in forms.values():
        other.add(c)
    assert np.array_equal(other.reconstruct_n(), np.concatenate([C, C, C, C, C[1:2], C[1:2]]))
    other.close()


def test_binary_refused_forms(binary):
    C = np.random.default_rng(7).integers(0, 256, (NQ, 8), dtype=np.uint8)
    with _raises(ValueError, "search: codes must be uint8, got float32"):
        binary.search(C.astype(np.float32), K)
    with _raises(ValueError, "search: codes must be a uint8 numpy array or torch tensor"):
        binary.search(torch.from_numpy(C).to(torch.int32), K)
    with _raises(ValueError, "search: codes must be a uint8 numpy array or torch tensor"):
        binary.search(C.tolist(), K)
    with _raises(ValueError, "search expects uint8 [n,8], got (3, 9)"):
        binary.search(np.zeros((NQ, 9), np.uint8), K)
    with _raises(ValueError, "search expects uint8 [n,8], got (9,)"):
        binary.search(np.zeros(9, np.uint8), K)
    with _raises(ValueError, "add expects uint8 [n,8], got (3, 9)"):
        binary.add(np.zeros((NQ, 9), np.uint8))
    for k in (0, 2049):
        with _raises(ValueError, f"k={k} outside [1,2048]"):
            binary.search(C, k)
    with _raises(ValueError, "search: no queries"):
        binary.search(np.zeros((0, 8), np.uint8), K)
    assert binary.ntotal == 300


# -- IndexLSH ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lsh():
    from ivr_amd.binary import IndexLSH
    idx = IndexLSH(D_, 32)
    idx.add(_unit(8, 300))
    yield idx
    idx.close()


def test_lsh_every_query_form(lsh, Q):
    forms = _forms(Q)
    base = _same(lsh, Q, forms)
    assert base[0].dtype == np.float32 and (np.diff(base[0], axis=1) >= 0).all()
    codes = lsh.sa_encode(Q)
    assert codes.dtype == np.uint8 and codes.shape == (NQ, 4)
    for name, (q, rows) in forms.items():
        assert np.array_equal(lsh.sa_encode(q), lsh.sa_encode(Q[rows])), name


def test_lsh_refused_forms(lsh, Q):
    with _raises(ValueError, "sa_encode expects [n,24], got (24,)"):
        lsh.search(torch.from_numpy(Q[1]).to(DEV), K)              # only a numpy vector becomes one row
    with _raises(ValueError, "sa_encode expects [n,24], got (3, 25)"):
        lsh.search(_unit(2, NQ, 25), K)
    with _raises(ValueError, "sa_encode expects [n,24], got ()"):
        lsh.search(Q.tolist(), K)
    with _raises(ValueError, "add expects [n,24], got (3, 25)"):
        lsh.add(_unit(2, NQ, 25))
    for k in (0, 2049):
        with _raises(ValueError, f"k={k} outside [1,2048]"):
            lsh.search(Q, k)
    with _raises(ValueError, "search: no queries"):
        lsh.search(np.zeros((0, D_), np.float32), K)
    assert lsh.ntotal == 300
