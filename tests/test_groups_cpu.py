"""CPU suite of the grouped search (ivr_amd/grouping.py, csrc/search_groups.hip): the numpy definitions group_search_ref /
best_per_segment_ref against a brute force that sorts in Python, seg_off_from_labels, the ABI of the three new entry points and the
argument checks that need no device.  No compute call reaches a device."""
import ctypes
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
from group_cases import FLT_MAX, brute_best, brute_groups, small_scores
from ivr_amd import _ffi, grouping
from ivr_amd.index import FlatIPIndex

NEW = ("ivr_group_piece_rows", "ivr_index_search_groups", "ivr_index_best_per_segment")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(got, want):
    return all(a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(got, want))


# -- the definition against the brute force ------------------------------------------------------------------------------------------
def test_definitions_are_the_brute_force_on_small_cases_with_ties():
    tied_inside = tied_across = short = unused = 0
    for S, seg in small_scores():
        N = S.shape[1]
        ids = np.arange(N, dtype=np.int64)[::-1] * 3 + 100
        for G, g in [(1, 1), (3, 2), (5, 64), (40, 1), (2048, 1)]:
            for labels in (None, ids):
                got = grouping.group_search_ref(S, G, g, seg, labels)
                want = brute_groups(S, G, g, seg, labels)
                assert same(got, want), f"N={N} G={G} g={g} seg={seg}"
            Gseg, D, I = got
            unused += int((Gseg == -1).sum())
            short += int(((I == -1) & (Gseg[:, :, None] >= 0)).sum())
            if g > 1:
                tied_inside += int(((bits(D[:, :, :-1]) == bits(D[:, :, 1:])) & (I[:, :, 1:] >= 0)).sum())
            if G > 1:
                tied_across += int(((bits(D[:, :-1, 0]) == bits(D[:, 1:, 0])) & (Gseg[:, 1:] >= 0)).sum())
        for labels in (None, ids):
            assert same(grouping.best_per_segment_ref(S, seg, labels), brute_best(S, seg, labels))
    assert tied_inside > 0 and tied_across > 0 and short > 0 and unused > 0       # the cases do hold what they are there for


def test_hand_made_case():
    #             row 0    1    2    3     4    5    6    7
    S = np.array([[0.5, 0.9, 0.9, 0.1, -0.0, 0.9, 0.3, 2.0]], np.float32)
    seg = np.array([1, 3, 3, 4, 7], np.int64)               # [1,3) [3,3) empty [3,4) [4,7); rows 0 and 7 belong to no group
    Gseg, D, I = grouping.group_search_ref(S, 4, 2, seg)
    assert Gseg.tolist() == [[0, 3, 2, -1]]                 # 0.9 twice: the lower best row = the lower segment first; then 0.1; one unused
    assert I.tolist() == [[[1, 2], [5, 6], [3, -1], [-1, -1]]]
    want = np.array([[[0.9, 0.9], [0.9, 0.3], [0.1, -FLT_MAX], [-FLT_MAX, -FLT_MAX]]], np.float32)
    assert np.array_equal(bits(D), bits(want))
    D, I = grouping.best_per_segment_ref(S, seg)
    assert I.tolist() == [[1, -1, 3, 5]] and np.array_equal(bits(D), bits(np.array([[0.9, -FLT_MAX, 0.1, 0.9]], np.float32)))
    # -0.0 ranks as +0.0 (the lower row wins the tie) and is reported as +0.0
    Gseg, D, I = grouping.group_search_ref(np.array([[-0.0, 0.0, -1.0]], np.float32), 1, 3)
    assert I.tolist() == [[[0, 1, 2]]] and bits(D)[0, 0].tolist() == [0, 0, 0xBF800000]
    # without seg_off the whole index is one segment, and so it is with one segment over everything; offsets past N are clipped
    a = grouping.group_search_ref(S, 2, 3)
    assert a[0].tolist() == [[0, -1]] and a[2][0, 0].tolist() == [7, 1, 2]
    assert same(a, grouping.group_search_ref(S, 2, 3, [0, 8])) and same(a, grouping.group_search_ref(S, 2, 3, [-4, 99]))
    assert grouping.best_per_segment_ref(S)[1].tolist() == [[7]]
    # labels of an id-mapped index; Gseg stays segment numbers
    ids = np.arange(8, dtype=np.int64) + 50
    Gseg, D, I = grouping.group_search_ref(S, 2, 1, seg, ids)
    assert Gseg.tolist() == [[0, 3]] and I.tolist() == [[[51], [55]]]
    # no stored rows: unused slots only
    Gseg, D, I = grouping.group_search_ref(np.zeros((2, 0), np.float32), 3, 2, [0, 4])
    assert (Gseg == -1).all() and (I == -1).all() and (D == -FLT_MAX).all() and D.shape == (2, 3, 2)


def test_seg_off_from_labels():
    assert grouping.seg_off_from_labels(["a", "a", "b", "c", "c", "c"]).tolist() == [0, 2, 3, 6]
    assert grouping.seg_off_from_labels(np.array([7, 7, 7])).tolist() == [0, 3]
    assert grouping.seg_off_from_labels(["x"]).tolist() == [0, 1]
    assert grouping.seg_off_from_labels([]).tolist() == [0, 0]
    off = grouping.seg_off_from_labels(f"L{i // 5:02d}" for i in range(23))
    assert off.dtype == np.int64 and off.tolist() == [0, 5, 10, 15, 20, 23]
    with pytest.raises(ValueError, match=r"label 'a' are not contiguous \(row 3"):
        grouping.seg_off_from_labels(["a", "a", "b", "a"])


# -- ABI and surfaces ------------------------------------------------------------------------------------------------------------------
def _header():
    return re.sub(r"/\*.*?\*/", "", open(f"{ROOT}/include/ivr_api.h").read(), flags=re.S)


def _ctype_of(decl):
    decl = decl.strip()
    if "*" in decl or decl.startswith("ivr_stream"):
        return ctypes.c_void_p
    return {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "float": ctypes.c_float}[decl.split()[0]]


@pytest.mark.parametrize("name,names", [
    (NEW[0], []),
    (NEW[1], ["idx", "q", "nq", "seg_off", "nseg", "G", "g", "normalize_q", "Gseg", "D", "I", "stream"]),
    (NEW[2], ["idx", "q", "nq", "seg_off", "nseg", "normalize_q", "D", "I", "stream"])])
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


def test_limits_of_the_library():
    assert re.search(r"#define\s+IVR_GROUP_MAX_ROWS\s+64\b", _header())
    assert grouping.GROUP_MAX_ROWS == _ffi.IVR_GROUP_MAX_ROWS == 64
    rows = grouping.group_piece_rows()
    assert rows >= 64 and rows % 16 == 0


def test_library_rejects_bad_arguments_before_any_device_call():
    lib = _ffi.load()
    assert lib.ivr_index_search_groups(None, None, 1, None, 0, 1, 1, 0, None, None, None, None) == -1
    assert b"NULL" in lib.ivr_last_error(None)
    assert lib.ivr_index_best_per_segment(None, None, 1, None, 0, 0, None, None, None) == -1
    assert b"NULL" in lib.ivr_last_error(None)
    fake = ctypes.create_string_buffer(64)                 # stands for the handle and the buffers: a rejected call reads none of them
    p = ctypes.cast(fake, ctypes.c_void_p)

    def groups(nq=1, seg=None, nseg=0, G=1, g=1):
        rc = lib.ivr_index_search_groups(p, p, nq, seg, nseg, G, g, 0, p, p, p, None)
        return rc, lib.ivr_last_error(None)

    for bad, text in [(dict(G=0), b"G=0 < 1"), (dict(G=-2), b"G=-2 < 1"), (dict(g=0), b"g=0 outside [1,64]"), (dict(g=65), b"g=65 outside [1,64]"),
                      (dict(G=33, g=64), b"G * g = 2112 > 2048"), (dict(G=2049), b"G * g = 2049 > 2048"), (dict(nq=0), b"nq=0 < 1"),
                      (dict(seg=p, nseg=0), b"nseg=0 with seg_off")]:
        rc, err = groups(**bad)
        assert rc == -1 and text in err, (bad, err)
    assert lib.ivr_index_best_per_segment(p, p, 0, None, 0, 0, p, p, None) == -1 and b"nq=0 < 1" in lib.ivr_last_error(None)
    assert lib.ivr_index_best_per_segment(p, p, 1, p, 0, 0, p, p, None) == -1 and b"nseg=0 with seg_off" in lib.ivr_last_error(None)
    assert lib.ivr_index_best_per_segment(p, p, 1 << 16, p, 1 << 15, 0, p, p, None) == -1 and b">= 2^31" in lib.ivr_last_error(None)


def test_lazy_package_exports_resolve():
    import ivr_amd
    for name in ("group_search", "group_search_device", "best_per_segment", "best_per_segment_device", "group_search_ref",
                 "best_per_segment_ref", "seg_off_from_labels"):
        assert name in ivr_amd.__all__
        assert getattr(ivr_amd, name) is getattr(grouping, name)


def test_argument_checks_name_the_offending_values():
    index = FlatIPIndex.__new__(FlatIPIndex)             # no handle: every check below fails before the library is called
    index.d, index.device = 8, torch.device("cpu")
    x = np.zeros((2, 8), np.float32)
    with pytest.raises(ValueError, match="FlatIPIndex"):
        grouping.group_search_device(object(), x, 3)
    with pytest.raises(ValueError, match="n_groups=0 < 1"):
        grouping.group_search_device(index, x, 0)
    with pytest.raises(ValueError, match=r"group_size=65 outside \[1,64\]"):
        grouping.group_search_device(index, x, 3, 65)
    with pytest.raises(ValueError, match=r"group_size=0 outside \[1,64\]"):
        grouping.group_search_device(index, x, 3, 0)
    with pytest.raises(ValueError, match=r"n_groups \* group_size = 2112 > 2048"):
        grouping.group_search_device(index, x, 33, 64)
    with pytest.raises(ValueError, match="n_groups must be an integer, got float"):
        grouping.group_search_device(index, x, 3.0)
    with pytest.raises(ValueError, match=r"seg_off\[1\]=5 > seg_off\[2\]=3"):
        grouping.group_search_device(index, x, 3, seg_off=np.array([0, 5, 3]))
    with pytest.raises(ValueError, match=r"\[nseg\+1\]"):
        grouping.best_per_segment_device(index, x, np.array([0]))
    with pytest.raises(ValueError, match="Query dimension"):
        grouping.best_per_segment_device(index, np.zeros((2, 9), np.float32), np.array([0, 4]))
    with pytest.raises(ValueError, match="group_size=65"):
        grouping.group_search_ref(np.zeros((1, 4), np.float32), 1, 65)
    with pytest.raises(ValueError, match="ascending"):
        grouping.group_search_ref(np.zeros((1, 4), np.float32), 1, 1, [0, 3, 2])
