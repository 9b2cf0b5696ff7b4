"""CPU suite of the video search (ivr_amd/videos.py, csrc/search_videos.hip): the numpy definitions video_scores_ref /
video_search_ref against an enumeration in Python with float64 / int arithmetic, the fixed point on ties at half, the ABI of the two
new entry points and the argument checks that need no device.  No compute call reaches a device."""
import ctypes
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
from ivr_amd import _ffi, videos
from ivr_amd.index import FlatIPIndex
from video_cases import FLT_MAX, MODES, brute_search, brute_videos, row_counts, small_scores

NEW = ("ivr_index_video_scores", "ivr_index_video_search")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# -- the definition against the enumeration ----------------------------------------------------------------------------------------
def test_definitions_are_the_enumeration_on_small_cases_with_ties():
    empty = tied = unused = left_out = 0
    for S, seg, sets in small_scores():
        want = brute_videos(S, seg, sets)
        nrows = row_counts(S.shape[1], seg)
        sums = videos.video_sums_ref(S, seg, sets)
        assert sums[3].tolist() == nrows
        nsets = len(sums[2])
        for mode in MODES:
            V = videos.video_scores_ref(S, seg, sets, mode)
            assert V.dtype == np.float32 and np.array_equal(bits(V), bits(want[mode])), f"{mode} N={S.shape[1]} seg={seg} sets={sets}"
            assert np.array_equal(bits(V), bits(videos.video_scores_ref(S, seg, sets, mode, sums)))
            empty += int((V == -FLT_MAX).sum())
            for k in (1, 3, 40):
                for exclude in (None, np.arange(nsets) % len(nrows), np.full(nsets, -1), np.full(nsets, len(nrows))):
                    Vseg, D = videos.video_search_ref(S, k, seg, sets, mode, exclude)
                    Vw, Dw = brute_search(want[mode], k, nrows, exclude)
                    assert np.array_equal(Vseg, Vw) and np.array_equal(bits(D), bits(Dw)), f"{mode} k={k} exclude={exclude}"
                    unused += int((Vseg == -1).sum())
                    if exclude is not None:
                        left_out += int(sum(0 <= e < len(nrows) and nrows[e] > 0 for e in exclude))
                        assert not (Vseg == np.asarray(exclude)[:, None]).any() or (np.asarray(exclude) == -1).all()
                    tied += int(((bits(D[:, :-1]) == bits(D[:, 1:])) & (Vseg[:, 1:] >= 0)).sum())
    assert empty > 0 and tied > 0 and unused > 0 and left_out > 0                 # the cases do hold what they are there for


def test_fix_rounds_ties_at_half_to_even_and_folds_the_zeros():
    h = 2.0 ** -25
    t = np.array([h, 3 * h, 5 * h, -h, -3 * h, 0.75 * 2.0 ** -24, 1.0, -256.0, 256.0, -0.0], np.float32)
    assert videos.fix(t).tolist() == [0, 2, 2, 0, -2, 1, 1 << 24, -(1 << 32), 1 << 32, 0]
    assert videos.fix(t).dtype == np.int64
    # a score whose fixed point is a tie at half enters both sums rounded to even
    S = np.array([[h, 3 * h], [5 * h, -3 * h]], np.float32)
    Fsum, Bsum, m, n = videos.video_sums_ref(S)
    assert Fsum.tolist() == [[2 + 2]] and Bsum.tolist() == [[2 + 2]] and m.tolist() == [2] and n.tolist() == [2]
    # -0.0 counts as +0.0: the maximum of (-0.0, -1) is reported through +0.0
    V = videos.video_scores_ref(np.array([[-0.0, -1.0]], np.float32), mode="forward")
    assert bits(V).tolist() == [[0]]


def test_hand_made_case():
    #              row 0    1     2    3    4    5
    S = np.array([[0.5, 0.25, -1.0, 0.0, 2.0, 0.5],
                  [1.0, 0.75, 0.5, -0.5, 1.0, 3.0]], np.float32)
    seg = np.array([1, 3, 3, 4, 9], np.int64)               # [1,3) [3,3) empty [3,4) [4,6) clipped; row 0 belongs to no video
    V = {mode: videos.video_scores_ref(S, seg, None, mode) for mode in MODES}
    assert V["forward"].tolist() == [[(0.25 + 0.75) / 2, -FLT_MAX, (0.0 - 0.5) / 2, (2.0 + 3.0) / 2]]
    assert V["backward"].tolist() == [[(0.75 + 0.5) / 2, -FLT_MAX, 0.0, (2.0 + 3.0) / 2]]
    assert V["symmetric"].tolist() == [[0.5625, -FLT_MAX, -0.125, 2.5]]
    Vseg, D = videos.video_search_ref(S, 4, seg)
    assert Vseg.tolist() == [[3, 0, 2, -1]] and D.tolist() == [[2.5, 0.5625, -0.125, -FLT_MAX]]
    Vseg, D = videos.video_search_ref(S, 2, seg, exclude=[3])
    assert Vseg.tolist() == [[0, 2]]
    # two sets of one member each: forward is the best frame of the video
    Vf = videos.video_scores_ref(S, seg, [0, 1, 2], "forward")
    assert Vf.tolist() == [[0.25, -FLT_MAX, 0.0, 2.0], [0.75, -FLT_MAX, -0.5, 3.0]]
    # equal scores: the lower video first
    Vseg, D = videos.video_search_ref(np.array([[1.0, 0.5, 1.0, 1.0]], np.float32), 3, np.arange(5))
    assert Vseg.tolist() == [[0, 2, 3]]
    # without seg_off the index is one video; offsets past N are clipped
    assert videos.video_scores_ref(S).shape == (1, 1)
    assert np.array_equal(videos.video_scores_ref(S), videos.video_scores_ref(S, [-4, 99]))
    # no stored rows: every video is empty
    V0 = videos.video_scores_ref(np.zeros((2, 0), np.float32), [0, 4, 9])
    assert V0.shape == (1, 2) and (V0 == -FLT_MAX).all()
    Vseg, D = videos.video_search_ref(np.zeros((2, 0), np.float32), 3, [0, 4, 9])
    assert (Vseg == -1).all() and (D == -FLT_MAX).all()


def test_symmetric_mode_is_symmetric_on_a_symmetric_score_matrix():
    rng = np.random.default_rng(3)
    n = 23
    A = rng.standard_normal((n, n)).astype(np.float32)
    S = np.maximum(A, A.T)                                  # S[i, r] == S[r, i]: the rows are their own queries
    off = np.array([0, 4, 5, 5, 12, 20, 23], np.int64)
    V = videos.video_scores_ref(S, off, off[[0, 1, 2, 4, 5, 6]], "symmetric")     # the sets are the non-empty videos
    full = [0, 1, 3, 4, 5]
    W = V[:, full]
    assert np.array_equal(bits(W), bits(W.T))
    F = videos.video_scores_ref(S, off, off[[0, 1, 2, 4, 5, 6]], "forward")[:, full]
    B = videos.video_scores_ref(S, off, off[[0, 1, 2, 4, 5, 6]], "backward")[:, full]
    assert np.array_equal(bits(F), bits(B.T)) and not np.array_equal(bits(F), bits(F.T))


# -- ABI and surfaces ------------------------------------------------------------------------------------------------------------------
def _header():
    return re.sub(r"/\*.*?\*/", "", open(f"{ROOT}/include/ivr_api.h").read(), flags=re.S)


def _ctype_of(decl):
    decl = decl.strip()
    if "*" in decl or decl.startswith("ivr_stream"):
        return ctypes.c_void_p
    return {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "float": ctypes.c_float}[decl.split()[0]]


@pytest.mark.parametrize("name,names", [
    (NEW[0], ["idx", "q", "nq", "set_off", "nsets", "seg_off", "nseg", "mode", "normalize_q", "V", "stream"]),
    (NEW[1], ["idx", "q", "nq", "set_off", "nsets", "seg_off", "nseg", "mode", "normalize_q", "k", "exclude", "Vseg", "D", "stream"])])
def test_header_binding_and_library_agree(name, names):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", _header())
    assert m, f"{name} not declared in ivr_api.h"
    params = [p.strip() for p in m.group(1).split(",")]
    assert [re.sub(r"[\s*]+", " ", p).split()[-1] for p in params] == names
    res, args = _ffi._SIGS[name]
    assert res is ctypes.c_int and args == [_ctype_of(p) for p in params]
    assert _ffi._STREAM[name] == len(params) - 1 and name not in _ffi._VALUE and name in _ffi.EXPORTS
    assert hasattr(ctypes.CDLL(_ffi.LIB_PATH), name)


def test_limits_and_modes_of_the_library():
    assert re.search(r"#define\s+IVR_VIDEO_MAX_MEMBERS\s+4096\b", _header())
    assert videos.VIDEO_MAX_MEMBERS == _ffi.IVR_VIDEO_MAX_MEMBERS == 4096
    for name, number in (("FORWARD", 0), ("BACKWARD", 1), ("SYMMETRIC", 2)):
        assert re.search(rf"#define\s+IVR_VIDEO_{name}\s+{number}\b", _header())
        assert _ffi.IVR_VIDEO_MODE[name.lower()] == number
    from ivr_amd import tagging
    assert tagging.MASS_ONE == 1 << 24


def test_library_rejects_bad_arguments_before_any_device_call():
    lib = _ffi.load()
    assert lib.ivr_index_video_scores(None, None, 1, None, 0, None, 0, 2, 0, None, None) == -1
    assert b"NULL" in lib.ivr_last_error(None)
    assert lib.ivr_index_video_search(None, None, 1, None, 0, None, 0, 2, 0, 1, None, None, None, None) == -1
    assert b"NULL" in lib.ivr_last_error(None)
    fake = ctypes.create_string_buffer(64)                 # stands for the handle and the buffers: a rejected call reads none of them
    p = ctypes.cast(fake, ctypes.c_void_p)

    def search(nq=1, sets=None, nsets=0, seg=None, nseg=0, mode=2, k=1, Vseg=p, D=p):
        rc = lib.ivr_index_video_search(p, p, nq, sets, nsets, seg, nseg, mode, 0, k, None, Vseg, D, None)
        return rc, lib.ivr_last_error(None)

    for bad, text in [(dict(nq=0), b"nq=0 < 1"), (dict(sets=p, nsets=0), b"nsets=0 with set_off"), (dict(seg=p, nseg=0), b"nseg=0 with seg_off"),
                      (dict(mode=3), b"mode=3 is none of"), (dict(mode=-1), b"mode=-1 is none of"), (dict(k=0), b"k=0 outside [1,2048]"),
                      (dict(k=2049), b"k=2049 outside [1,2048]"), (dict(nq=4097), b"one set of 4097 members > 4096"), (dict(Vseg=None), b"NULL"),
                      (dict(D=None), b"NULL")]:
        rc, err = search(**bad)
        assert rc == -1 and text in err, (bad, err)
    assert lib.ivr_index_video_scores(p, p, 1, None, 0, None, 0, 7, 0, p, None) == -1 and b"mode=7" in lib.ivr_last_error(None)
    assert lib.ivr_index_video_scores(p, p, 1, None, 0, None, 0, 0, 0, None, None) == -1 and b"NULL" in lib.ivr_last_error(None)


def test_lazy_package_exports_resolve():
    import ivr_amd
    for name in ("video_scores", "video_scores_device", "video_search", "video_search_device", "related_videos", "video_scores_ref",
                 "video_search_ref", "video_sums_ref"):
        assert name in ivr_amd.__all__
        assert getattr(ivr_amd, name) is getattr(videos, name)


def test_argument_checks_name_the_offending_values():
    index = FlatIPIndex.__new__(FlatIPIndex)             # no handle: every check below fails before the library is called
    index.d, index.device = 8, torch.device("cpu")
    x = np.zeros((6, 8), np.float32)
    for call in (lambda *a, **kw: videos.video_scores_device(*a, **kw), lambda i, x, **kw: videos.video_search_device(i, x, 3, **kw)):
        with pytest.raises(ValueError, match="FlatIPIndex"):
            call(object(), x)
        with pytest.raises(ValueError, match="set 1 is empty"):
            call(index, x, set_off=np.array([0, 2, 2, 6]))
        with pytest.raises(ValueError, match=r"set_off\[1\]=5 > set_off\[2\]=3"):
            call(index, x, set_off=np.array([0, 5, 3, 6]))
        with pytest.raises(ValueError, match=r"set_off \[0,7\] outside the 6 members"):
            call(index, x, set_off=np.array([0, 7]))
        with pytest.raises(ValueError, match=r"set_off must be integers \[nsets\+1\]"):
            call(index, x, set_off=np.array([0.0, 6.0]))
        with pytest.raises(ValueError, match="set 0 has 4097 members > 4096"):
            call(index, np.zeros((4097, 8), np.float32))
        with pytest.raises(ValueError, match="set 1 has 4097 members > 4096"):
            call(index, np.zeros((4100, 8), np.float32), set_off=np.array([0, 3, 4100]))
        with pytest.raises(ValueError, match="mode must be 'forward', 'backward' or 'symmetric', got 'chamfer'"):
            call(index, x, mode="chamfer")
        with pytest.raises(ValueError, match=r"seg_off\[1\]=5 > seg_off\[2\]=3"):
            call(index, x, seg_off=np.array([0, 5, 3]))
        with pytest.raises(ValueError, match="Query dimension"):
            call(index, np.zeros((2, 9), np.float32))
    with pytest.raises(ValueError, match=r"k=0 outside \[1,2048\]"):
        videos.video_search_device(index, x, 0)
    with pytest.raises(ValueError, match=r"exclude must be \[2\]"):
        videos.video_search_device(index, x, 3, set_off=np.array([0, 2, 6]), exclude=np.array([1]))
    with pytest.raises(ValueError, match="FlatIPIndex"):
        videos.related_videos(object(), np.array([0, 4]), 3)
    with pytest.raises(ValueError, match="mode must be"):
        videos.related_videos(index, np.array([0, 4]), 3, mode="max")
    with pytest.raises(ValueError, match="set 0 is empty"):
        videos.video_scores_ref(np.zeros((3, 4), np.float32), set_off=[0, 0, 3])
    with pytest.raises(ValueError, match="ascending"):
        videos.video_scores_ref(np.zeros((3, 4), np.float32), seg_off=[0, 3, 2])
    with pytest.raises(ValueError, match="mode must be"):
        videos.video_scores_ref(np.zeros((3, 4), np.float32), mode="both")
