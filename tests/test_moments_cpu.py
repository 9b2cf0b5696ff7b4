"""CPU suite of the moment search (ivr_amd/moments.py, csrc/search_moments.hip): the numpy definitions moments_ref /
moment_search_ref / moment_range_search_ref against a brute force that walks the rows in Python, the hand-made case of the design,
the ABI of the three new entry points and the argument checks that need no device.  No compute call reaches a device."""
import ctypes
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
from moment_cases import FLT_MAX, brute_moments, brute_range, brute_topk, ordered, small_cases
from ivr_amd import _ffi, moments
from ivr_amd.index import FlatIPIndex

NEW = ("ivr_moment_block_rows", "ivr_index_search_moments", "ivr_index_range_search_moments")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(got, want):
    return len(got) == len(want) and all(a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))
                                         for a, b in zip(got, want))


# -- the definition against the brute force ------------------------------------------------------------------------------------------
def test_definitions_are_the_brute_force_on_small_cases():
    bridged = split = tied = unused = dropped = 0
    for S, thr, gap, seg in small_cases():
        N = S.shape[1]
        ids = np.arange(N, dtype=np.int64)[::-1] * 3 + 100
        per = moments.moments_ref(S, thr, gap, seg)
        for q in range(S.shape[0]):
            want = brute_moments(S[q], thr, gap, seg)
            assert per[q].dtype == np.int64 and per[q].tolist() == [list(m) for m in want], f"N={N} thr={thr} gap={gap} seg={seg}"
            bridged += sum(hi - lo + 1 > cnt for lo, hi, cnt, _ in want)
            split += sum(b[0] - a[1] - 1 <= gap for a, b in zip(want, want[1:]))          # only a segment boundary keeps these apart
            tied += sum(sum(ordered(S[q, r]) == ordered(S[q, peak]) and S[q, r] >= np.float32(thr) for r in range(lo, hi + 1)) > 1
                        for lo, hi, _, peak in want)
        for labels in (None, ids):
            assert same(moments.moment_range_search_ref(S, thr, gap, seg, labels), brute_range(S, thr, gap, seg, labels))
            for k, min_count, rank in [(1, 1, "peak"), (3, 1, "count"), (4, 2, "peak"), (2048, 1, "count"), (5, 3, "count")]:
                got = moments.moment_search_ref(S, k, thr, gap, min_count, rank, seg, labels)
                assert same(got, brute_topk(S, k, thr, gap, min_count, rank, seg, labels)), f"N={N} k={k} min_count={min_count} rank={rank}"
                if labels is None:
                    unused += int((got[1] == -1).sum())
                    dropped += sum(sum(m[2] < min_count for m in brute_moments(S[q], thr, gap, seg)) for q in range(S.shape[0]))
    assert bridged > 0 and split > 0 and tied > 0 and unused > 0 and dropped > 0      # the cases do hold what they are there for


def test_hand_made_case():
    S = np.array([[0.9, 0.2, 0.8, 0.1, 0.1, 0.7, 0.95, 0.3]], np.float32)
    thr = 0.7                                                # equals a score: row 5 being hot pins the >=
    assert [tuple(m) for m in moments.moments_ref(S, thr, 1)[0]] == [(0, 2, 2, 0), (5, 6, 2, 6)]
    assert [tuple(m) for m in moments.moments_ref(S, thr, 0)[0]] == [(0, 0, 1, 0), (2, 2, 1, 2), (5, 6, 2, 6)]
    assert [tuple(m) for m in moments.moments_ref(S, thr, 1, [0, 6, 8])[0]] == [(0, 2, 2, 0), (5, 5, 1, 5), (6, 6, 1, 6)]
    D, I, Lo, Hi, Cnt = moments.moment_search_ref(S, 3, thr, max_gap=1, rank="peak")
    assert I.tolist() == [[6, 0, -1]] and np.array_equal(bits(D), bits(np.array([[0.95, 0.9, -FLT_MAX]], np.float32)))
    assert Lo.tolist() == [[5, 0, -1]] and Hi.tolist() == [[6, 2, -1]] and Cnt.tolist() == [[2, 2, 0]]
    # by count the lower lo wins the tie; min_count drops the single rows of max_gap 0
    assert moments.moment_search_ref(S, 3, thr, max_gap=1, rank="count")[2].tolist() == [[0, 5, -1]]
    assert moments.moment_search_ref(S, 3, thr, max_gap=0, min_count=2)[1].tolist() == [[6, -1, -1]]
    lims, D, I, Lo, Hi, Cnt = moments.moment_range_search_ref(S, thr, 1, [0, 6, 8], ids=np.arange(8) + 50)
    assert lims.tolist() == [0, 3] and I.tolist() == [50, 55, 56] and Lo.tolist() == [0, 5, 6] and Hi.tolist() == [2, 5, 6]
    assert Cnt.tolist() == [2, 1, 1] and np.array_equal(bits(D), bits(np.array([0.9, 0.7, 0.95], np.float32)))
    # a NaN score is never hot, -0.0 ranks as +0.0 (the lower row wins) and is reported as +0.0; rows outside the offsets belong to nothing
    Z = np.array([[0.0, -0.0, np.nan, -0.0, 5.0]], np.float32)
    assert [tuple(m) for m in moments.moments_ref(Z, -1.0, 0)[0]] == [(0, 1, 2, 0), (3, 4, 2, 4)]
    assert [tuple(m) for m in moments.moments_ref(Z, -1.0, 1, [1, 4])[0]] == [(1, 3, 2, 1)]
    assert bits(moments.moment_search_ref(Z, 1, -1.0, 1, seg_off=[1, 4])[0]).tolist() == [[0]]
    # no stored rows, and a threshold above every score: unused slots and lims of zeros
    out = moments.moment_search_ref(np.zeros((2, 0), np.float32), 3, 0.0)
    assert (out[0] == -FLT_MAX).all() and all((o == -1).all() for o in out[1:4]) and (out[4] == 0).all() and out[0].shape == (2, 3)
    out = moments.moment_range_search_ref(S, 2.0)
    assert out[0].tolist() == [0, 0] and all(len(o) == 0 for o in out[1:]) and out[1].dtype == np.float32


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
    (NEW[1], ["idx", "q", "nq", "seg_off", "nseg", "threshold", "max_gap", "min_count", "rank", "k", "normalize_q", "D", "I", "Lo", "Hi", "Cnt",
              "stream"]),
    (NEW[2], ["idx", "q", "nq", "seg_off", "nseg", "threshold", "max_gap", "normalize_q", "lims", "D", "I", "Lo", "Hi", "Cnt", "cap", "stream"])])
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


def test_constants_of_the_library():
    assert re.search(r"#define\s+IVR_MOMENT_RANK_PEAK\s+0\b", _header()) and re.search(r"#define\s+IVR_MOMENT_RANK_COUNT\s+1\b", _header())
    assert _ffi.IVR_MOMENT_RANK == {"peak": 0, "count": 1}
    rows = moments.moment_block_rows()
    assert rows >= 64 and rows % 16 == 0


def test_library_rejects_bad_arguments_before_any_device_call():
    lib = _ffi.load()
    assert lib.ivr_index_search_moments(None, None, 1, None, 0, 0.0, 0, 1, 0, 1, 0, None, None, None, None, None, None) == -1
    assert b"NULL" in lib.ivr_last_error(None)
    assert lib.ivr_index_range_search_moments(None, None, 1, None, 0, 0.0, 0, 0, None, None, None, None, None, None, 0, None) == -1
    assert b"NULL" in lib.ivr_last_error(None)
    fake = ctypes.create_string_buffer(64)                 # stands for the handle and the buffers: a rejected call reads none of them
    p = ctypes.cast(fake, ctypes.c_void_p)

    def topk(nq=1, seg=None, nseg=0, thr=0.5, gap=0, min_count=1, rank=0, k=1, q=p, D=p, I=p, Lo=p, Hi=p, Cnt=p):
        rc = lib.ivr_index_search_moments(p, q, nq, seg, nseg, thr, gap, min_count, rank, k, 0, D, I, Lo, Hi, Cnt, None)
        return rc, lib.ivr_last_error(None)

    def rng(nq=1, seg=None, nseg=0, thr=0.5, gap=0, lims=p, D=p, I=p, Lo=p, Hi=p, Cnt=p, cap=4):
        rc = lib.ivr_index_range_search_moments(p, p, nq, seg, nseg, thr, gap, 0, lims, D, I, Lo, Hi, Cnt, cap, None)
        return rc, lib.ivr_last_error(None)

    shared = [(dict(nq=0), b"nq=0 < 1"), (dict(seg=p, nseg=0), b"nseg=0 with seg_off"), (dict(thr=float("nan")), b"threshold is NaN"),
              (dict(gap=-1), b"max_gap=-1 outside"), (dict(gap=2**31 - 1), b"max_gap=2147483647 outside"), (dict(D=None), b"NULL"),
              (dict(I=None), b"NULL"), (dict(Lo=None), b"NULL"), (dict(Hi=None), b"NULL"), (dict(Cnt=None), b"NULL")]
    for bad, text in shared + [(dict(q=None), b"NULL"), (dict(min_count=0), b"min_count=0 < 1"), (dict(rank=2), b"rank=2"),
                               (dict(rank=-1), b"rank=-1"), (dict(k=0), b"k=0 outside [1,2048]"), (dict(k=2049), b"k=2049 outside [1,2048]")]:
        rc, err = topk(**bad)
        assert rc == -1 and text in err, (bad, err)
    for bad, text in shared + [(dict(lims=None), b"NULL"), (dict(cap=-1), b"cap=-1 < 0")]:
        rc, err = rng(**bad)
        assert rc == -1 and text in err, (bad, err)


def test_lazy_package_exports_resolve():
    import ivr_amd
    for name in ("moment_search", "moment_search_device", "moment_range_search", "moment_range_search_device", "moments_ref",
                 "moment_search_ref", "moment_range_search_ref", "moment_block_rows"):
        assert name in ivr_amd.__all__
        assert getattr(ivr_amd, name) is getattr(moments, name)


def test_argument_checks_name_the_offending_values():
    index = FlatIPIndex.__new__(FlatIPIndex)             # no handle: every check below fails before the library is called
    index.d, index.device = 8, torch.device("cpu")
    x = np.zeros((2, 8), np.float32)
    with pytest.raises(ValueError, match="FlatIPIndex"):
        moments.moment_search_device(object(), x, 3, 0.5)
    with pytest.raises(ValueError, match=r"k=0 outside \[1,2048\]"):
        moments.moment_search_device(index, x, 0, 0.5)
    with pytest.raises(ValueError, match=r"k=2049 outside \[1,2048\]"):
        moments.moment_search_device(index, x, 2049, 0.5)
    with pytest.raises(ValueError, match="k must be an integer, got float"):
        moments.moment_search_device(index, x, 3.0, 0.5)
    with pytest.raises(ValueError, match="min_count=0 < 1"):
        moments.moment_search_device(index, x, 3, 0.5, min_count=0)
    with pytest.raises(ValueError, match="rank='mean' is neither"):
        moments.moment_search_device(index, x, 3, 0.5, rank="mean")
    with pytest.raises(ValueError, match="threshold=nan is NaN"):
        moments.moment_search_device(index, x, 3, float("nan"))
    with pytest.raises(ValueError, match="threshold must be a number, got str"):
        moments.moment_range_search_device(index, x, "0.5")
    with pytest.raises(ValueError, match=r"max_gap=-1 outside \[0,2\^31-2\]"):
        moments.moment_range_search_device(index, x, 0.5, max_gap=-1)
    with pytest.raises(ValueError, match=r"max_gap=2147483647 outside"):
        moments.moment_search_device(index, x, 3, 0.5, max_gap=2**31 - 1)
    with pytest.raises(ValueError, match="max_gap must be an integer, got float"):
        moments.moment_search_device(index, x, 3, 0.5, max_gap=1.0)
    with pytest.raises(ValueError, match="cap=-1 < 0"):
        moments.moment_range_search_device(index, x, 0.5, cap=-1)
    with pytest.raises(ValueError, match=r"seg_off\[1\]=5 > seg_off\[2\]=3"):
        moments.moment_search_device(index, x, 3, 0.5, seg_off=np.array([0, 5, 3]))
    with pytest.raises(ValueError, match="Query dimension"):
        moments.moment_range_search_device(index, np.zeros((2, 9), np.float32), 0.5)
    with pytest.raises(ValueError, match="ascending"):
        moments.moments_ref(np.zeros((1, 4), np.float32), 0.5, 0, [0, 3, 2])
    with pytest.raises(ValueError, match="min_count=0"):
        moments.moment_search_ref(np.zeros((1, 4), np.float32), 1, 0.5, min_count=0)
