"""CPU suite: the binding layer of ivr_amd (_ffi.call, _ffi.Handle, _staging, _faiss) against a stub library: how arguments are
marshalled, what a status becomes, which exports carry a stream, and the exact texts of the shared checks."""
import contextlib
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from ivr_amd import _faiss, _ffi, _staging

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ivr_api.h")
CPU = torch.device("cpu")


class StubLib:
    """Stands in for the loaded library: every export records its arguments and returns `rc`."""

    def __init__(self, rc=0):
        self.rc, self.calls = rc, []

    def ivr_last_error(self, ctx):
        return b"boom"

    def __getattr__(self, name):
        if name not in _ffi._SIGS:
            raise AttributeError(name)

        def fn(*args):
            self.calls.append((name, args))
            return self.rc
        return fn


@pytest.fixture
def stub(monkeypatch):
    lib = StubLib()
    monkeypatch.setattr(_ffi, "_lib", lib)
    monkeypatch.setattr(_ffi, "stream_ptr", lambda stream=None: C.c_void_p(0x5EED))
    monkeypatch.setattr(_ffi, "context", lambda device=0: C.c_void_p(0xC000 + device))
    lib.devices = []

    @contextlib.contextmanager
    def device(d):
        lib.devices.append(d)
        yield
    monkeypatch.setattr(torch.cuda, "device", device)
    return lib


def _byref_of(arg, obj):
    return type(arg).__name__ == "CArgObject" and arg._obj is obj


def test_call_marshals_every_slot_kind(stub):
    h, s = C.c_void_p(0x1000), C.c_void_p(0x2000)
    q = torch.zeros((3, 4), dtype=torch.float32)
    D, I = torch.zeros((3, 5)), torch.zeros((3, 5), dtype=torch.int64)
    # c_void_p slots: c_void_p, tensor, None, address; integer slots: int and bool
    assert _ffi.call("ivr_index_search", h, q, 3, 5, True, 7, D, None, s) is None
    name, a = stub.calls[-1]
    assert name == "ivr_index_search" and a[0] is h and a[8] is s
    assert a[1:8] == (q.data_ptr(), 3, 5, True, 7, D.data_ptr(), None)
    _ffi.call("ivr_index_add", h, 0xABC0, np.int64(2), False, s)            # a numpy integer, as ctypes takes one
    assert stub.calls[-1][1][1:4] == (0xABC0, 2, 0) and type(stub.calls[-1][1][2]) is int
    # float slot, POINTER(struct) slot by reference or None
    f = _ffi.IdFilter(1, 9, None, 0)
    lims = torch.zeros(4, dtype=torch.int64)
    _ffi.call("ivr_index_range_search_filtered", h, q, 3, 0.5, False, 0, f, lims, D, I, 10, s)
    a = stub.calls[-1][1]
    assert a[3] == 0.5 and type(a[3]) is float and _byref_of(a[6], f)
    _ffi.call("ivr_index_search_reconstruct", h, q, 3, 5, False, 0, None, D, I, D, s)
    assert stub.calls[-1][1][6] is None
    n, out = C.c_int64(0), C.c_void_p()
    _ffi.call("ivr_index_remove_ids", h, 0, f, n, s)
    assert _byref_of(stub.calls[-1][1][2], f) and _byref_of(stub.calls[-1][1][3], n)
    _ffi.call("ivr_index_create", h, 24, 0, out)
    assert _byref_of(stub.calls[-1][1][3], out)
    # what ctypes takes as it is: a ctypes array in a pointer slot, bytes in a char* slot
    two, mean = (C.c_int * 2)(), _ffi.f3((1, 2, 3))
    _ffi.call("ivr_index_scan_stats", h, two)
    assert stub.calls[-1][1][1] is two
    _ffi.call("ivr_preprocess", h, q, 1, 2, 2, 0, mean, mean, 2, 2, D, s)
    assert stub.calls[-1][1][6] is mean
    _ffi.call("ivr_tower_set_weight", h, b"w", 0x10, 4)
    assert stub.calls[-1][1][1] == b"w"


@pytest.mark.parametrize("args, text", [
    ((C.c_void_p(1), "rows", 2, False), "ivr_index_add: argument 1"),          # a str is no address
    ((C.c_void_p(1), None, 2.0, False), "ivr_index_add: argument 2"),          # a float in an integer slot
    ((C.c_void_p(1), None, np.float32(2), False), "ivr_index_add: argument 2"),
])
def test_call_rejects_a_wrong_argument_type(stub, args, text):
    with pytest.raises(TypeError, match=re.escape(text)):
        _ffi.call("ivr_index_add", *args)
    assert not stub.calls


def test_call_rejects_an_int_in_a_float_slot(stub):
    q = torch.zeros((1, 4))
    with pytest.raises(TypeError, match="ivr_index_range_search: argument 3"):
        _ffi.call("ivr_index_range_search", C.c_void_p(1), q, 1, 1, False, 0, q, q, q, 0)
    assert not stub.calls


@pytest.mark.parametrize("name, n", [("ivr_index_add", 1), ("ivr_index_add", 6), ("ivr_index_reset", 0), ("ivr_index_reset", 2),
                                     ("ivr_api_version", 1)])
def test_call_rejects_a_wrong_argument_count(stub, name, n):
    with pytest.raises(TypeError, match=name):
        _ffi.call(name, *([None] * n))
    assert not stub.calls


@pytest.mark.parametrize("rc, exc", [(-1, ValueError), (-3, MemoryError), (-2, _ffi.IvrError), (-4, _ffi.IvrError), (5, _ffi.IvrError)])
def test_call_maps_a_status_to_the_exception(stub, rc, exc):
    stub.rc = rc
    with pytest.raises(exc) as e:
        _ffi.call("ivr_index_reset", C.c_void_p(1))
    assert type(e.value) is exc and str(e.value) == "ivr_index_reset: boom"
    with pytest.raises(exc) as e:
        _ffi.call("ivr_tower_finalize", C.c_void_p(1), 8, what="ivr_tower_finalize(x)")
    assert str(e.value) == "ivr_tower_finalize(x): boom"


def test_call_returns_the_value_of_a_value_export(stub):
    stub.rc = 42
    for name in ("ivr_index_ntotal", "ivr_index_dim", "ivr_index_has_ids", "ivr_bin_index_ntotal", "ivr_graph_ntotal",
                 "ivr_tower_workspace_bytes"):
        assert _ffi.call(name, C.c_void_p(1)) == 42
    for name in ("ivr_api_version", "ivr_graph_max_ef", "ivr_graph_max_cand", "ivr_bin_index_block_rows"):
        assert _ffi.call(name) == 42
    assert _ffi.call("ivr_preprocess_scratch_bytes", 1, 2, 3, 0, 4) == 42
    assert _ffi.call("ivr_frame_quality_scratch_bytes", 1, 2, 3) == 42
    stub.rc = -1                                      # a negative value is a value, not a status
    assert _ffi.call("ivr_index_ntotal", None) == -1


def test_call_fills_the_stream_only_when_it_is_left_out(stub):
    h, own = C.c_void_p(1), C.c_void_p(0x77)
    _ffi.call("ivr_index_add", h, None, 0, False)
    assert stub.calls[-1][1][4].value == 0x5EED
    _ffi.call("ivr_index_add", h, None, 0, False, own)
    assert stub.calls[-1][1][4] is own
    _ffi.call("ivr_index_add", h, None, 0, False, None)            # NULL = the null stream: given, so kept
    assert stub.calls[-1][1][4] is None and len(stub.calls[-1][1]) == 5
    assert stub.devices == []                                       # no device asked for, none entered
    with pytest.raises(TypeError, match="ivr_index_reset"):         # no stream slot to fill
        _ffi.call("ivr_index_reset")


def test_call_runs_under_the_device_and_resolves_the_context(stub):
    dev = torch.device("cuda", 3)
    x = torch.zeros((2, 4))
    _ffi.call("ivr_l2_normalize", _ffi.CTX, x, 2, 4, None, device=dev)
    a = stub.calls[-1][1]
    assert stub.devices == [dev] and a[0].value == 0xC003 and a[5].value == 0x5EED
    _ffi.call("ivr_l2_normalize", _ffi.CTX, x, 2, 4, None, device=1)
    assert stub.devices == [dev, 1] and stub.calls[-1][1][0].value == 0xC001
    with pytest.raises(TypeError, match="ivr_l2_normalize: argument 0"):      # CTX needs a device to name
        _ffi.call("ivr_l2_normalize", _ffi.CTX, x, 2, 4, None)


def _declarations():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return {m.group(2): (m.group(1).strip(), m.group(3))
            for m in re.finditer(r"^((?:const\s+)?[a-z0-9_]+\s*\*?)\s*(ivr_[a-z0-9_]+)\s*\(([^;{]*)\)\s*;", src, flags=re.M)}


def test_every_export_is_classified():
    decl = _declarations()
    assert set(decl) == set(_ffi._SIGS)
    assert _ffi._VALUE <= set(_ffi._SIGS) and set(_ffi._STREAM) <= set(_ffi._SIGS)
    for name, (res, args) in _ffi._SIGS.items():
        ret, params = decl[name]
        # a status is exactly an `int` whose header comment does not promise a value: every other return type is a value
        assert (name in _ffi._VALUE) or res is C.c_int, name
        if ret != "int":
            assert name in _ffi._VALUE, name
        # the stream slot is where the header has its ivr_stream parameter
        slots = [i for i, p in enumerate(params.split(",")) if re.search(r"\bivr_stream\b", p)]
        assert slots == ([_ffi._STREAM[name]] if name in _ffi._STREAM else []), name
        if name in _ffi._STREAM:
            assert args[_ffi._STREAM[name]] is C.c_void_p
    for name in ("ivr_index_ntotal", "ivr_bin_index_ntotal", "ivr_graph_ntotal", "ivr_index_dim", "ivr_index_has_ids", "ivr_api_version",
                 "ivr_graph_max_ef", "ivr_graph_max_cand", "ivr_bin_index_block_rows", "ivr_preprocess_scratch_bytes",
                 "ivr_frame_quality_scratch_bytes", "ivr_tower_workspace_bytes"):
        assert name in _ffi._VALUE, name
    for name in ("ivr_index_search", "ivr_index_reset", "ivr_index_destroy", "ivr_init", "ivr_gemm", "ivr_tower_finalize"):
        assert name not in _ffi._VALUE, name


def test_handle_supplies_handle_device_and_stream(stub):
    class Thing(_ffi.Handle):
        _DESTROY = "ivr_index_destroy"

    t = Thing()
    assert t._h is None
    t.close()                                                        # nothing opened: nothing destroyed
    t._open("ivr_index_create", 2, 24, 0)
    name, a = stub.calls[-1]
    assert name == "ivr_index_create" and a[0].value == 0xC002 and a[1:3] == (24, 0) and _byref_of(a[3], t._h)
    assert t.device == torch.device("cuda", 2) and t._lib is stub and stub.devices == [t.device]
    t._h.value = 0x1234
    x = torch.zeros((2, 24))
    t._call("ivr_index_add", x, 2, False)
    name, a = stub.calls[-1]
    assert name == "ivr_index_add" and a[0] is t._h and a[1] == x.data_ptr() and a[4].value == 0x5EED
    assert stub.devices == [t.device, t.device]
    h = t._h
    t.close()
    assert stub.calls[-1] == ("ivr_index_destroy", (h,)) and t._h is None
    n = len(stub.calls)
    t.close()
    t.__del__()
    assert len(stub.calls) == n


# -- staging ---------------------------------------------------------------------------------------------------------------------
def test_staging_reports_what_is_a_copy():
    a = np.arange(12, dtype=np.float32).reshape(3, 4)
    own = torch.from_numpy(a.copy())
    for x in (a, a.astype(np.float64), own.t().contiguous().t(), own[:, ::2], own.to(torch.float64)):
        t, staged = _staging.queries_f32(x, x.shape[1], CPU)
        assert staged and t.dtype == torch.float32 and t.is_contiguous() and t.device == CPU
        assert np.array_equal(t.numpy(), np.asarray(x, dtype=np.float32))
        assert _staging.is_staged(_staging.dev_f32(x, CPU), x)
    t, staged = _staging.queries_f32(own, 4, CPU)
    assert not staged and t.data_ptr() == own.data_ptr() and not _staging.is_staged(_staging.dev_f32(own, CPU), own)
    with pytest.raises(ValueError, match=r"^expected a numpy array or a torch tensor$"):
        _staging.dev_f32([[1.0, 2.0]], CPU)


def test_staging_makes_one_query_a_row():
    v = np.arange(4, dtype=np.float32)
    for x in (v, torch.from_numpy(v), v.tolist()):
        q = _staging.as_rows(x)
        assert tuple(q.shape) == (1, 4)
        t, _ = _staging.queries_f32(q, 4, CPU)
        assert tuple(t.shape) == (1, 4)
    assert tuple(_staging.as_rows(v, tensors_too=False).shape) == (1, 4)
    assert tuple(_staging.as_rows(v.tolist(), tensors_too=False).shape) == (1, 4)
    assert tuple(_staging.as_rows(torch.from_numpy(v), tensors_too=False).shape) == (4,)       # FlatIPIndex.search leaves a tensor alone
    m = v.reshape(2, 2)
    assert _staging.as_rows(m) is m
    one = torch.from_numpy(v)
    t, staged = _staging.queries_f32(_staging.as_rows(one), 4, CPU)
    assert not staged and t.data_ptr() == one.data_ptr()             # the reshaped view is the caller's own storage


def test_staging_uint8_codes():
    c = np.arange(16, dtype=np.uint8).reshape(2, 8)
    own = torch.from_numpy(c.copy())
    t = _staging.dev_u8(c, 8, CPU, "search")
    assert _staging.is_staged(t, c) and t.dtype == torch.uint8 and np.array_equal(t.numpy(), c)
    assert not _staging.is_staged(_staging.dev_u8(own, 8, CPU, "search"), own)
    wide = torch.from_numpy(np.arange(32, dtype=np.uint8).reshape(2, 16))[:, ::2]
    assert _staging.is_staged(_staging.dev_u8(wide, 8, CPU, "search"), wide)
    assert tuple(_staging.dev_u8(c[0], 8, CPU, "search").shape) == (1, 8)
    assert not _staging.is_staged(_staging.dev_u8(own[0], 8, CPU, "search"), own[0])
    with pytest.raises(ValueError, match=r"^add: codes must be uint8, got int32$"):
        _staging.dev_u8(c.astype(np.int32), 8, CPU, "add")
    with pytest.raises(ValueError, match=r"^add: codes must be a uint8 numpy array or torch tensor$"):
        _staging.dev_u8(own.to(torch.int32), 8, CPU, "add")
    with pytest.raises(ValueError, match=r"^search expects uint8 \[n,8\], got \(2, 4\)$"):
        _staging.dev_u8(c[:, :4], 8, CPU, "search")
    with pytest.raises(ValueError, match=r"^search expects uint8 \[n,8\], got \(4,\)$"):
        _staging.dev_u8(c[0, :4], 8, CPU, "search")


def test_sync_if_staged_waits_only_for_a_copy(monkeypatch):
    waits = []

    class Stream:
        def synchronize(self):
            waits.append(1)
    monkeypatch.setattr(torch.cuda, "current_stream", lambda device=None: waits.append(device) or Stream())
    _staging.sync_if_staged(False, "dev")
    assert waits == []
    _staging.sync_if_staged(True, "dev")
    assert waits == ["dev", 1]


# -- the shared checks: the texts the index classes raise ---------------------------------------------------------------------------
def _raises(text):
    return pytest.raises(ValueError, match="^" + re.escape(text) + "$")


def test_shared_checks_raise_the_index_texts():
    assert _ffi.IVR_MAX_K == 2048 and _ffi.IVR_GRAPH_MAX_EF == 256
    assert _staging.check_k(5.0, 2048) == 5 and _staging.check_k(2048, 2048) == 2048 and _staging.check_k(1, 256) == 1
    with _raises("k=0 outside [1,2048]"):
        _staging.check_k(0, _ffi.IVR_MAX_K)
    with _raises("k=2049 outside [1,2048]"):
        _staging.check_k(2049, _ffi.IVR_MAX_K)
    with _raises("k=257 outside [1,256]"):
        _staging.check_k(257, _ffi.IVR_GRAPH_MAX_EF)
    with _raises("Query dimension ((3, 5)) != index dimension (4)"):
        _staging.queries_f32(np.zeros((3, 5), np.float32), 4, CPU)
    with _raises("Query dimension ((4,)) != index dimension (4)"):
        _staging.queries_f32(torch.zeros(4), 4, CPU)
    for what in ("add", "add_with_ids", "update_vectors", "train", "sa_encode"):
        with _raises(f"{what} expects [n,24], got (3, 5)"):
            _staging.check_rows(np.zeros((3, 5), np.float32), 24, what)
    with _raises("add expects [n,24], got (24,)"):
        _staging.check_rows(torch.zeros(24), 24, "add")
    with _raises("add expects [n,24], got ()"):
        _staging.check_rows([[0.0] * 24], 24, "add")
    _staging.check_rows(np.zeros((0, 24), np.float32), 24, "add")
    with _raises("search: no queries"):
        _staging.check_nq(0)
    with _raises("range_search: no queries"):
        _staging.check_nq(0, "range_search")
    _staging.check_nq(1)
    D, I = _staging.alloc_DI(3, 5, CPU)
    assert (D.dtype, I.dtype, tuple(D.shape), tuple(I.shape)) == (torch.float32, torch.int64, (3, 5), (3, 5))
    assert _staging.alloc_DI(3, 5, CPU, torch.int32)[0].dtype == torch.int32


def test_typed_params_and_metric_constants():
    from ivr_amd import ivf
    from ivr_amd.graph import SearchParametersHNSW
    from ivr_amd.index import IDSelectorRange, SearchParameters
    assert (_faiss.METRIC_INNER_PRODUCT, _faiss.METRIC_L2) == (0, 1)
    assert ivf.METRIC_INNER_PRODUCT is _faiss.METRIC_INNER_PRODUCT and ivf.METRIC_L2 is _faiss.METRIC_L2
    import ivr_amd
    assert (ivr_amd.METRIC_INNER_PRODUCT, ivr_amd.METRIC_L2) == (0, 1)
    assert _faiss.typed_params(None, ivf.SearchParametersIVF, "IVFFlatIndex") is None
    p = ivf.SearchParametersIVF(nprobe=3)
    assert _faiss.typed_params(p, ivf.SearchParametersIVF, "IVFFlatIndex") is p
    with _raises("params must be a SearchParametersIVF, got SearchParameters"):
        _faiss.typed_params(SearchParameters(), ivf.SearchParametersIVF, "IVFFlatIndex")
    with _raises("params must be a SearchParametersHNSW, got dict"):
        _faiss.typed_params({}, SearchParametersHNSW, "GraphFlatIndex")
    with _raises("search: ID selectors are not supported on IVFFlatIndex"):
        _faiss.typed_params(ivf.SearchParametersIVF(sel=IDSelectorRange(0, 1)), ivf.SearchParametersIVF, "IVFFlatIndex")
    with _raises("search: ID selectors are not supported on GraphFlatIndex"):
        _faiss.typed_params(SearchParametersHNSW(sel=IDSelectorRange(0, 1)), SearchParametersHNSW, "GraphFlatIndex")


def test_integer_table_checks_raise_the_index_texts():
    good = np.array([[0, 3], [-1, 2]], np.int32)
    for a in (good, torch.from_numpy(good), good.astype(np.uint8), torch.from_numpy(good).to(torch.int64)):
        t = _staging.int_tensor(a, "search_preassigned: assign")
        assert isinstance(t, torch.Tensor) and not t.dtype.is_floating_point and tuple(t.shape) == (2, 2)
    # IVFFlatIndex.search_preassigned
    with _raises("search_preassigned: assign must be integers, got float32"):
        _staging.int_tensor(good.astype(np.float32), "search_preassigned: assign")
    for bad in (torch.zeros((2, 2)), torch.zeros((2, 2), dtype=torch.bool), [[0, 1]], None):
        with _raises("search_preassigned: assign must be an integer numpy array or torch tensor"):
            _staging.int_tensor(bad, "search_preassigned: assign")
    with _raises("search_preassigned: assign entries must lie in [-1, 4)"):
        _staging.check_entries(torch.tensor([[0, 4]]), 4, "search_preassigned: assign entries")
    with _raises("search_preassigned: assign entries must lie in [-1, 4)"):
        _staging.check_entries(torch.tensor([[-2, 1]]), 4, "search_preassigned: assign entries")
    _staging.check_entries(torch.tensor([[-1, 3]]), 4, "search_preassigned: assign entries")
    # GraphFlatIndex.set_graph / add(graph=...)
    for who in ("set_graph", "add"):
        with _raises(f"{who}: the graph must hold integers, got float64"):
            _staging.int_tensor(good.astype(np.float64), f"{who}: the graph", "hold")
        for bad in (torch.zeros((2, 2)), torch.zeros((2, 2), dtype=torch.complex64), torch.zeros((2, 2), dtype=torch.bool), "graph"):
            with _raises(f"{who}: the graph must be an integer numpy array or torch tensor"):
                _staging.int_tensor(bad, f"{who}: the graph", "hold")
        with _raises(f"{who}: entries must lie in [-1, 200)"):
            _staging.check_entries(torch.tensor([[200, 0]], dtype=torch.int32), 200, f"{who}: entries")
    # GraphFlatIndex.search_from
    e = _staging.entry_table([[0, 5], [-7, 2**40]], 2, 64, "search_from")
    assert e.dtype == np.int32 and e.flags.c_contiguous and e.tolist() == [[0, 5], [-1, 2**31 - 1]]
    for bad in (np.zeros((2, 1), np.float32), np.zeros(2, np.int64), np.zeros((3, 1), np.int64), np.zeros((2, 0), np.int64),
                np.zeros((2, 65), np.int64)):
        with _raises("search_from: entries must be integers [2,1..64]"):
            _staging.entry_table(bad, 2, 64, "search_from")
    assert _ffi.IVR_GRAPH_MAX_DEGREE == 64
