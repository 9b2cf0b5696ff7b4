"""CPU suite of the clip search (ivr_amd/temporal.py, csrc/search_seq.hip): the numpy definitions (sequence_*_ref) against a literal
float64 restatement of the reference's TemporalAnalyzer loops around sklearn's cosine_similarity (core.py:3584-3702, 3812-3828), the
host bookkeeping of the class, the ABI of the two new entry points and the argument checks that need no device.  No compute call
reaches a device."""
import ctypes
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
from ivr_amd import _ffi, temporal
from ivr_amd.index import FlatIPIndex
from temporal_cases import (D_FEAT, MARGIN, as_result_list, clip_case, reference_find, reference_scene_boundaries,
                            reference_sequence_similarity, reference_transition_frames)

THRESHOLD = 0.5
NEW = ("ivr_index_search_sequences", "ivr_index_range_search_sequences")


def frame_scores(target, database):
    """What the index computes, in numpy float32: both sides L2-normalised (zero rows stay zero), then inner products."""
    def unit(x):
        n = np.sqrt((x * x).sum(1, dtype=np.float32)).astype(np.float32)
        n[n == 0] = 1
        return (x / n[:, None]).astype(np.float32)
    return (unit(target) @ unit(database).T).astype(np.float32)


# -- refs against the reference --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [1, 2, 5])
@pytest.mark.parametrize("nkind", ["L-1", "L", "40"])
@pytest.mark.parametrize("tkind", ["L", "L+1", "12"])
def test_refs_match_the_reference_loops(L, nkind, tkind):
    T = {"L": L, "L+1": L + 1, "12": 12}[tkind]
    N = {"L-1": L - 1, "L": L, "40": 40}[nkind]
    target, database = clip_case(T, N, L)
    means = []
    want = reference_find(target.astype(np.float64), database.astype(np.float64), L, THRESHOLD, means)
    # the precondition of an identical list: no float64 mean so close to the threshold that float32 may fall on the other side, and
    # no two kept means so close that float32 may order them differently
    assert all(abs(v - THRESHOLD) > MARGIN for v in means), "seed puts a window mean within 1e-4 of the threshold"
    kept = sorted(v for _, v in want)
    assert all(b - a > 1e-5 for a, b in zip(kept, kept[1:])), "seed puts two kept window means within 1e-5 of each other"
    if N == 40:
        assert 0 < len(want) < len(means), "the case must keep some windows and drop some"
    S = frame_scores(target, database)
    lims, D, I = temporal.sequence_range_ref(S, L, THRESHOLD)
    got = as_result_list(lims, D, I)
    assert [s for s, _ in got] == [s for s, _ in want]
    tol = (D_FEAT + L + 8) * 2.0 ** -24            # a length-d float32 dot product of unit rows, L additions and a division
    assert all(abs(a - b) <= tol for (_, a), (_, b) in zip(got, want))
    assert lims.dtype == np.int64 and len(lims) == T - L + 2 and lims[0] == 0 and lims[-1] == len(want)
    # the top-k ref ranks the same windows: its k best per target window are the best of that window's kept list
    k = 3
    Dk, Ik = temporal.sequence_search_ref(S, L, k)
    assert Dk.shape == (T - L + 1, k) and Ik.dtype == np.int64
    W, ok = temporal.sequence_scores_ref(S, L)
    for t in range(T - L + 1):
        order = sorted(range(W.shape[1]), key=lambda s: (-float(W[t, s]), s))[:k]
        assert Ik[t, :len(order)].tolist() == order and (Ik[t, len(order):] == -1).all()
        assert Dk[t, :len(order)].tolist() == [float(W[t, s]) for s in order]
        assert (Dk[t, len(order):] == np.float32(-np.finfo(np.float32).max)).all()


def test_window_score_rounds_every_addition_on_its_own():
    # 1 + 2^-24 + 2^-24: float32 drops each half-ulp in turn (ties to even), a wider accumulator would keep their sum
    S = np.zeros((3, 3), np.float32)
    S[0, 0], S[1, 1], S[2, 2] = 1.0, 2.0 ** -24, 2.0 ** -24
    W, ok = temporal.sequence_scores_ref(S, 3)
    assert W.shape == (1, 1) and ok.tolist() == [True]
    assert W[0, 0] == np.float32(1.0) / np.float32(3.0)
    assert np.float32((1.0 + 2.0 ** -23) / 3.0) != W[0, 0]


def test_segments_ties_and_padding_of_the_refs():
    S = np.ones((3, 12), np.float32)                  # every window scores 1: ties rank by start row
    seg = np.array([1, 4, 4, 6, 11], np.int64)        # [1,4) [4,4) empty, [4,6) shorter than L = 3, [6,11); rows 0 and 11 outside
    W, ok = temporal.sequence_scores_ref(S, 3, seg)
    assert np.flatnonzero(ok).tolist() == [1, 6, 7, 8]
    D, I = temporal.sequence_search_ref(S, 3, 6, seg)
    assert I.tolist() == [[1, 6, 7, 8, -1, -1]]
    assert D[0, :4].tolist() == [1.0] * 4 and (D[0, 4:] == np.float32(-np.finfo(np.float32).max)).all()
    ids = np.arange(100, 112)[::-1].copy()
    assert temporal.sequence_search_ref(S, 3, 2, seg, ids=ids)[1].tolist() == [[110, 105]]
    lims, Dr, Ir = temporal.sequence_range_ref(S, 3, 1.0, seg)             # >= keeps a score equal to the threshold
    assert lims.tolist() == [0, 4] and Ir.tolist() == [1, 6, 7, 8]
    assert temporal.sequence_range_ref(S, 3, np.nextafter(np.float32(1), np.float32(2)), seg)[0].tolist() == [0, 0]
    S[0, 1] = np.nan                                                       # a NaN score matches nothing
    assert temporal.sequence_range_ref(S, 3, -np.inf, seg)[2].tolist() == [6, 7, 8]
    S = -np.zeros((1, 2), np.float32)                                      # -0.0 is reported as +0.0
    assert not np.signbit(temporal.sequence_search_ref(S, 1, 1)[0]).any()
    assert not np.signbit(temporal.sequence_range_ref(S, 1, 0.0)[1]).any()
    with pytest.raises(ValueError):
        temporal.sequence_range_ref(S, 1, float("nan"))
    with pytest.raises(ValueError):
        temporal.sequence_scores_ref(np.zeros((2, 5), np.float32), 3)


# -- bookkeeping of the class ----------------------------------------------------------------------------------------------------------
@pytest.fixture
def host_cosine(monkeypatch):
    """rowwise_cosine without a device: the same values in float64, as a CPU tensor."""
    from ivr_amd import filters

    def cos(a, b):
        a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
        na, nb = np.linalg.norm(a, axis=1), np.linalg.norm(b, axis=1)
        return torch.from_numpy((a * b).sum(1) / (np.where(na == 0, 1, na) * np.where(nb == 0, 1, nb)))
    monkeypatch.setattr(filters, "rowwise_cosine", cos)


@pytest.mark.parametrize("n,threshold,min_len", [(40, 0.3, 5), (40, 0.6, 3), (12, 0.3, 5), (9, 0.3, 5), (40, 0.95, 1), (40, -1.0, 5)])
def test_detect_scene_boundaries_keeps_the_reference_bookkeeping(host_cosine, n, threshold, min_len):
    rng = np.random.default_rng(n * 7 + min_len)
    scenes = rng.standard_normal((8, D_FEAT))
    cuts = np.sort(rng.choice(np.arange(1, n), 7, replace=False))
    which = np.searchsorted(cuts, np.arange(n), side="right")                 # short and long scenes, some below min_len
    features = (scenes[which] + 0.15 * rng.standard_normal((n, D_FEAT))).astype(np.float32)
    ta = temporal.TemporalAnalyzer()
    got = ta.detect_scene_boundaries(features, threshold, min_len)
    want = reference_scene_boundaries(features.astype(np.float64), threshold, min_len)
    assert got == want
    assert ta.get_transition_frames(features, got) == reference_transition_frames(features, want)


def test_class_checks_and_host_helpers():
    ta = temporal.TemporalAnalyzer()
    with pytest.raises(ValueError):
        ta.detect_scene_boundaries([[1.0, 2.0]])
    with pytest.raises(ValueError):
        ta.detect_scene_boundaries(np.zeros(4, np.float32))
    with pytest.raises(ValueError):
        ta.find_similar_sequences([[1.0]], np.zeros((4, 1), np.float32))
    with pytest.raises(ValueError):
        ta.find_similar_sequences(np.zeros(4, np.float32), np.zeros((4, 1), np.float32))
    with pytest.raises(ValueError):
        ta.get_transition_frames(np.zeros((4, 2), np.float32), ((0, 1), (2, 3)))
    # fewer frames than the window on either side: the reference's empty list, before any device is touched
    assert ta.find_similar_sequences(np.zeros((4, 3), np.float32), np.zeros((9, 3), np.float32), 5) == []
    assert ta.find_similar_sequences(np.zeros((9, 3), np.float32), np.zeros((4, 3), np.float32), 5) == []
    rng = np.random.default_rng(3)
    a, b = rng.standard_normal((5, 8)), rng.standard_normal((5, 8))
    assert abs(ta._compute_sequence_similarity(a, b) - reference_sequence_similarity(a, b)) < 1e-12
    assert ta._compute_sequence_similarity(a, b[:4]) == 0.0
    assert not hasattr(ta, "analyze_temporal_patterns")


# -- ABI and surfaces ------------------------------------------------------------------------------------------------------------------
def _header():
    return re.sub(r"/\*.*?\*/", "", open(f"{ROOT}/include/ivr_api.h").read(), flags=re.S)


def _ctype_of(decl):
    decl = decl.strip()
    if "*" in decl or decl.startswith("ivr_stream"):
        return ctypes.c_void_p
    return {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "float": ctypes.c_float}[decl.split()[0]]


@pytest.mark.parametrize("name,names", [
    (NEW[0], ["idx", "q", "T", "L", "seg_off", "nseg", "k", "normalize_q", "D", "I", "stream"]),
    (NEW[1], ["idx", "q", "T", "L", "seg_off", "nseg", "threshold", "normalize_q", "lims", "D", "I", "cap", "stream"])])
def test_header_binding_and_library_agree(name, names):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", _header())
    assert m, f"{name} not declared in ivr_api.h"
    params = [p.strip() for p in m.group(1).split(",")]
    assert [re.sub(r"[\s*]+", " ", p).split()[-1] for p in params] == names
    res, args = _ffi._SIGS[name]
    assert res is ctypes.c_int and args == [_ctype_of(p) for p in params]
    assert _ffi._STREAM[name] == len(params) - 1
    assert name in _ffi.EXPORTS and name not in _ffi._VALUE
    assert hasattr(ctypes.CDLL(_ffi.LIB_PATH), name)


def test_api_version_is_still_11_and_no_class_grew_a_method():
    assert _ffi.API_VERSION == 11 and _ffi.load().ivr_api_version() == 11
    assert re.search(r"#define\s+IVR_API_VERSION\s+11\b", _header())
    assert re.search(r"#define\s+IVR_SEQ_MAX_LEN\s+64\b", _header()) and _ffi.IVR_SEQ_MAX_LEN == 64 == temporal.SEQ_MAX_LEN
    assert not [n for n in dir(FlatIPIndex) if "sequence" in n]


def test_library_rejects_bad_arguments_before_any_device_call():
    lib = _ffi.load()
    assert lib.ivr_index_search_sequences(None, None, 5, 5, None, 0, 1, 0, None, None, None) == -1
    assert b"NULL" in lib.ivr_last_error(None)
    assert lib.ivr_index_range_search_sequences(None, None, 5, 5, None, 0, 0.5, 0, None, None, None, 0, None) == -1
    assert b"NULL" in lib.ivr_last_error(None)


def test_lazy_package_exports_resolve():
    import ivr_amd
    for name in ("TemporalAnalyzer", "sequence_search", "sequence_search_device", "sequence_range_search", "sequence_range_search_device",
                 "sequence_scores_ref", "sequence_search_ref", "sequence_range_ref"):
        assert name in ivr_amd.__all__
        assert getattr(ivr_amd, name) is getattr(temporal, name)


def test_argument_checks_name_the_offending_values():
    index = FlatIPIndex.__new__(FlatIPIndex)             # no handle: every check below fails before the library is called
    index.d, index.device = 8, torch.device("cpu")
    x = np.zeros((6, 8), np.float32)
    with pytest.raises(ValueError, match="FlatIPIndex"):
        temporal.sequence_search_device(object(), x, 2, 1)
    with pytest.raises(ValueError, match=r"\(6, 7\)"):
        temporal.sequence_search_device(index, x[:, :7], 2, 1)
    with pytest.raises(ValueError, match=r"L=0 outside \[1,64\]"):
        temporal.sequence_search_device(index, x, 0, 1)
    with pytest.raises(ValueError, match=r"L=65 outside \[1,64\]"):
        temporal.sequence_range_search_device(index, np.zeros((70, 8), np.float32), 65, 0.5)
    with pytest.raises(ValueError, match="T=6 frames < L=7"):
        temporal.sequence_search_device(index, x, 7, 1)
    with pytest.raises(ValueError, match="integer"):
        temporal.sequence_search_device(index, x, 2.5, 1)
    with pytest.raises(ValueError, match=r"k=0 outside \[1,2048\]"):
        temporal.sequence_search_device(index, x, 2, 0)
    with pytest.raises(ValueError, match="k=2049"):
        temporal.sequence_search_device(index, x, 2, 2049)
    with pytest.raises(ValueError, match="NaN"):
        temporal.sequence_range_search_device(index, x, 2, float("nan"))
    with pytest.raises(ValueError, match="cap=-1"):
        temporal.sequence_range_search_device(index, x, 2, 0.5, cap=-1)
    with pytest.raises(ValueError, match=r"seg_off\[1\]=5 > seg_off\[2\]=3"):
        temporal.sequence_search_device(index, x, 2, 1, seg_off=np.array([0, 5, 3]))
    with pytest.raises(ValueError, match="integers"):
        temporal.sequence_search_device(index, x, 2, 1, seg_off=np.array([0.0, 5.0]))
    with pytest.raises(ValueError, match=r"\[nseg\+1\]"):
        temporal.sequence_search_device(index, x, 2, 1, seg_off=np.array([0]))
