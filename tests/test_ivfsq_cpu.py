"""CPU suite of the inverted-file index over scalar-quantiser codes (ivr_amd/ivfsq.py, csrc/search_ivfsq.hip): the binding, the
argument checks that run before any HIP call, the constructor's refusals and the numpy definitions the GPU suite compares the kernels
with (the packed layout and the scan)."""
import ctypes
import os
import re

import numpy as np
import pytest

import ivr_amd
from conftest import ROOT
from ivr_amd import _ffi, _ivf
from ivr_amd.ivfpq import IVFPQIndex, ivfpq_positions_ref
from ivr_amd.ivfsq import (IndexIVFScalarQuantizer, IVFSQIndex, ivfsq_pack_ref, ivfsq_scan_ref, ivfsq_score_bound,
                           ivfsq_unpack_ref)
from ivr_amd.sq import ScalarQuantizer, sq_scan_ref, sq_score_bound

FLT_MAX = np.finfo(np.float32).max
NEW_EXPORTS = ("ivr_ivfsq_create", "ivr_ivfsq_destroy", "ivr_ivfsq_reset", "ivr_ivfsq_ntotal", "ivr_ivfsq_set_lists", "ivr_ivfsq_get_codes",
               "ivr_ivfsq_search")
WITH_STREAM = ("ivr_ivfsq_set_lists", "ivr_ivfsq_get_codes", "ivr_ivfsq_search")
SIZES = [0, 1, 63, 64, 65, 130]


def test_names_are_declared_exported_bound_and_listed():
    header = open(os.path.join(ROOT, "include", "ivr_api.h")).read()
    assert re.search(r"#define\s+IVR_SQ_MAX_D\s+1024\b", header) and _ffi.IVR_SQ_MAX_D == 1024
    for name in ("IVFSQIndex", "IndexIVFScalarQuantizer", "ivfsq_scan_ref", "ivfsq_pack_ref", "ivfsq_unpack_ref", "ivfsq_score_bound"):
        assert name in ivr_amd.__all__
        assert getattr(ivr_amd, name) is getattr(ivr_amd.ivfsq, name)
    lib = ctypes.CDLL(_ffi.LIB_PATH)
    for name in NEW_EXPORTS:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in _ffi.EXPORTS and hasattr(lib, name)
        assert (name in _ffi._STREAM) == (name in WITH_STREAM)
    # entry for entry the list store of ivr_ivfpq, but for the search's query form
    for name in NEW_EXPORTS[:-1]:
        assert _ffi._SIGS[name] == _ffi._SIGS[name.replace("ivfsq", "ivfpq")]


@pytest.mark.parametrize("name", ["ivr_ivfsq_create", "ivr_ivfsq_reset", "ivr_ivfsq_set_lists", "ivr_ivfsq_get_codes", "ivr_ivfsq_search"])
def test_null_arguments_are_refused_before_any_hip_call(name):
    lib = _ffi.load()
    assert lib.ivr_index_reset(None) == -1                          # leaves another message in the slot
    args = [0 if t in (_ffi._i, _ffi._i64) else None for t in _ffi._SIGS[name][1]]
    assert getattr(lib, name)(*args) == -1
    msg = lib.ivr_last_error(None)
    assert name.encode() in msg and b"NULL" in msg


def test_both_coded_list_indexes_stand_on_one_layer():
    assert issubclass(IVFSQIndex, _ivf.CodedInvertedFileIndex) and issubclass(IVFPQIndex, _ivf.CodedInvertedFileIndex)
    assert not issubclass(IVFSQIndex, IVFPQIndex) and not issubclass(IVFPQIndex, IVFSQIndex)
    shared = ("add_with_ids", "search_device", "search_preassigned_device", "reconstruct_batch", "list_codes", "reset", "by_residual")
    for name in shared:                                            # stated once, in the layer
        assert name not in vars(IVFSQIndex) and name not in vars(IVFPQIndex) and name in vars(_ivf.CodedInvertedFileIndex)
    public = [n for n in sorted(dir(IVFSQIndex)) if not n.startswith("_")]
    assert public == ["add", "add_with_ids", "assign", "by_residual", "centroids", "close", "compute_query_codes_device", "is_trained",
                      "list_codes", "list_ids", "list_sizes", "nprobe", "ntotal", "reconstruct", "reconstruct_batch", "reset", "search",
                      "search_codes_preassigned_device", "search_device", "search_preassigned", "search_preassigned_device", "train"]


class _NeverTouched:
    """In the quantizer's place where the constructor must refuse before it looks at the quantizer."""

    def __getattr__(self, name):
        raise AssertionError(f"the quantizer was touched ({name}) before the arguments were checked")


@pytest.mark.parametrize("args, text", [
    ((32, 4, ScalarQuantizer.QT_4bit), "QT_8bit"),
    ((32, 4, ScalarQuantizer.QT_fp16), "QT_8bit"),
    ((32, 4, ScalarQuantizer.QT_8bit, ivr_amd.METRIC_L2), "METRIC_L2"),
    ((32, 4, ScalarQuantizer.QT_8bit, 7), "METRIC_INNER_PRODUCT"),
    ((0, 4), "d=0"),
    ((1025, 4), "d=1025"),
    ((32, 0), "nlist=0"),
])
def test_constructor_refusals_without_a_gpu(args, text):
    with pytest.raises(ValueError, match=text):
        IndexIVFScalarQuantizer(_NeverTouched(), *args)


def test_constructor_refuses_a_quantizer_of_another_type():
    with pytest.raises(ValueError, match="must be a FlatIPIndex"):
        IndexIVFScalarQuantizer(object(), 32, 4)


def lists_of(sizes, d, seed=0):
    rng = np.random.default_rng(seed)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    return rng.integers(0, 256, (int(off[-1]), d), dtype=np.uint8), off


@pytest.mark.parametrize("d", [16, 100, 1024])
def test_pack_unpack_round_trip_and_zero_pads(d):
    codes, off = lists_of(SIZES, d, seed=d)
    codes[codes == 128] = 129                   # every stored byte nonzero: whatever is zero in the layout is a pad
    packed = ivfsq_pack_ref(codes, off)
    ks = (d + 63) // 64
    groups = sum((s + 63) // 64 for s in SIZES)
    assert packed.dtype == np.int8 and packed.shape == (4 * groups, ks, 64, 16)
    assert np.array_equal(ivfsq_unpack_ref(packed, off, d), codes)
    assert np.count_nonzero(packed) == codes.size                    # pad bytes and pad rows are zero
    # a bijection on the stored bytes: packing what was unpacked gives the same bytes
    assert np.array_equal(ivfsq_pack_ref(ivfsq_unpack_ref(packed, off, d), off), packed)
    # where a row lives: the positions are ivfpq_positions_ref's; position P is row P % 16 of tile P // 16, and byte b of the row is
    # byte b % 16 of lane P % 16 + 16 ((b % 64) // 16) of piece b // 64, stored as code - 128
    pos, goff = ivfpq_positions_ref(off)
    assert goff.tolist() == [0, 0, 1, 2, 3, 5, 8]
    r = int(off[5]) + 70                          # row 70 of the list of 130
    P = int(pos[r])
    assert P == 64 * 5 + 70
    for b in (0, 15, d // 2 + 1, d - 1):
        assert packed[P // 16, b // 64, P % 16 + 16 * ((b % 64) // 16), b % 16] == int(codes[r, b]) - 128
    with pytest.raises(ValueError):
        ivfsq_unpack_ref(packed[:-4], off, d)                        # fewer groups than the lists need
    with pytest.raises(ValueError):
        ivfsq_pack_ref(codes, off[:-1])                              # offsets that do not end at n
    with pytest.raises(ValueError):
        ivfsq_pack_ref(codes.astype(np.int8), off)


def plain_scan(t, scale, bias, coarse, assign, off, codes, ids, k):
    """ivfsq_scan_ref as a double loop over queries and probed rows, with Python integers and one float32 operation at a time."""
    out_D, out_I = [], []
    for i in range(len(t)):
        first = {}
        for j in sorted(range(assign.shape[1]), key=lambda j: (assign[i, j], j)):      # ascending, stable
            if assign[i, j] >= 0:
                first.setdefault(int(assign[i, j]), j)
        found = []
        for l, j in first.items():
            for r in range(int(off[l]), int(off[l + 1])):
                acc = sum(int(a) * (int(c) - 128) for a, c in zip(t[i], codes[r]))
                D = np.float32(acc) * np.float32(scale[i])
                D = np.float32(D) + np.float32(bias[i])
                D = np.float32(D) + (np.float32(0.0) if coarse is None else np.float32(coarse[i, j]))
                D = np.float32(D) + np.float32(0.0)                  # -0.0 counts and is reported as +0.0
                found.append((-float(D), r))
        found.sort()                                                 # D descending, then the lower row: the lower list, the earlier row
        found = found[:k]
        out_D.append([np.float32(-s) for s, _ in found] + [np.float32(-FLT_MAX)] * (k - len(found)))
        out_I.append([int(ids[r]) for _, r in found] + [-1] * (k - len(found)))
    return np.array(out_D, np.float32), np.array(out_I, np.int64)


def test_scan_against_a_plain_double_loop():
    """Tiny inputs with skipped entries, a list named twice with two coarse scores, equal rows in two lists and k beyond the probed
    rows."""
    rng = np.random.default_rng(5)
    d, sizes = 5, [3, 0, 2, 4]
    codes, off = lists_of(sizes, d, seed=6)
    codes[4] = codes[0]                                              # list 2 holds a row of list 0
    codes[6] = codes[1]                                              # and list 3 one
    ids = rng.permutation(len(codes)).astype(np.int64) + 100
    t = rng.integers(-16256, 16257, (4, d)).astype(np.int16)
    scale = rng.uniform(1e-4, 1e-3, 4).astype(np.float32)
    bias = rng.uniform(0.5, 1.5, 4).astype(np.float32)
    assign = np.array([[0, 2, 3, 1], [3, -1, 3, 0], [-1, -1, 1, -1], [2, 0, 2, 2]], np.int64)
    coarse = rng.uniform(0.0, 1.0, assign.shape).astype(np.float32)
    coarse[0] = 0.25                                                 # equal coarse scores: the equal rows tie across lists
    for c in (coarse, None):
        for k in (1, 4, 12):
            D, I = ivfsq_scan_ref(t, scale, bias, c, assign, off, codes, ids, k)
            Dp, Ip = plain_scan(t, scale, bias, c, assign, off, codes, ids, k)
            assert np.array_equal(I, Ip) and D.tobytes() == Dp.tobytes()
    D, I = ivfsq_scan_ref(t, scale, bias, coarse, assign, off, codes, ids, 12)
    assert (I[2] == -1).all() and (D[2] == -FLT_MAX).all()           # only an empty list and -1 entries
    assert (I[0, 9:] == -1).all() and (I[0, :9] >= 100).all()        # 9 rows probed, k = 12
    # query 0: the tied rows come out adjacent, the one in the lower list first
    where = {int(v): n for n, v in enumerate(I[0])}
    assert where[int(ids[4])] == where[int(ids[0])] + 1 and where[int(ids[6])] == where[int(ids[1])] + 1
    # query 1 names list 3 twice: after the stable ascending sort [-1, 0, 3, 3] the first mention is entry 0, not entry 2
    one = ivfsq_scan_ref(t[1:2], scale[1:2], bias[1:2], coarse[1:2, [3, 0]], np.array([[0, 3]]), off, codes, ids, 12)
    assert one[0].tobytes() == D[1:2].tobytes() and np.array_equal(one[1], I[1:2])
    for bad in ([[4]], [[-2]]):
        with pytest.raises(ValueError):
            ivfsq_scan_ref(t[:1], scale[:1], bias[:1], None, np.array(bad), off, codes, ids, 1)
    with pytest.raises(ValueError):
        ivfsq_scan_ref(t[:1].astype(np.int32), scale[:1], bias[:1], None, assign[:1], off, codes, ids, 1)


def test_one_list_without_coarse_gives_the_scores_of_the_sq_scan():
    rng = np.random.default_rng(9)
    codes, off = lists_of([200], 24, seed=10)
    t = rng.integers(-16256, 16257, (3, 24)).astype(np.int16)
    scale, bias = rng.uniform(1e-4, 1e-3, 3).astype(np.float32), rng.uniform(0.5, 1.5, 3).astype(np.float32)
    for k in (1, 10, 200, 260):
        D, I = ivfsq_scan_ref(t, scale, bias, None, np.zeros((3, 1), np.int64), off, codes, np.arange(200), k)
        Ds, _ = sq_scan_ref(t, scale, bias, codes, k)
        assert D.tobytes() == (Ds + np.float32(0.0)).astype(np.float32).tobytes()
        assert sorted(I[0][I[0] >= 0].tolist()) == sorted(set(I[0][I[0] >= 0].tolist()))


def test_score_bound_is_the_sq_bound_plus_the_coarse_and_last_rounding_terms():
    rng = np.random.default_rng(11)
    d, n, nq = 12, 7, 3
    q = rng.standard_normal((nq, d)).astype(np.float32)
    codes = rng.integers(0, 256, (n, d), dtype=np.uint8)
    trained = np.concatenate([-np.ones(d), 2 * np.ones(d)]).astype(np.float32)
    scale = rng.uniform(1e-4, 1e-3, nq).astype(np.float32)
    cent = rng.standard_normal((n, d)).astype(np.float32)
    D = rng.standard_normal((nq, n)).astype(np.float32)
    b = ivfsq_score_bound(q, codes, trained, scale, cent, D)
    extra = (d + 2) * 2.0 ** -24 * (np.abs(q.astype(np.float64)) @ np.abs(cent.astype(np.float64)).T) + 2.0 ** -23 * np.abs(D.astype(np.float64))
    assert b.shape == (nq, n) and b.dtype == np.float64
    assert np.allclose(b, sq_score_bound(q, codes, trained, scale) + extra, rtol=1e-12, atol=0)
