"""CPU suite of the inverted-file index over product-quantised codes (ivr_amd/ivfpq.py, csrc/search_ivfpq.hip): the binding, the
argument checks that run before any HIP call, the constructor's refusals and the numpy definitions the GPU suite compares the
kernels with (the packed layout and the scan)."""
import ctypes
import os
import re

import numpy as np
import pytest

import ivr_amd
from conftest import ROOT
from ivr_amd import _ffi
from ivr_amd.ivfpq import IndexIVFPQ, ivfpq_pack_ref, ivfpq_positions_ref, ivfpq_scan_ref, ivfpq_unpack_ref
from ivr_amd.pq import pq_scan_ref

FLT_MAX = np.finfo(np.float32).max
NEW_EXPORTS = ("ivr_ivfpq_create", "ivr_ivfpq_destroy", "ivr_ivfpq_reset", "ivr_ivfpq_ntotal", "ivr_ivfpq_probe_queries",
               "ivr_ivfpq_set_lists", "ivr_ivfpq_get_codes", "ivr_ivfpq_search")
WITH_STREAM = ("ivr_ivfpq_set_lists", "ivr_ivfpq_get_codes", "ivr_ivfpq_search")
SIZES = [0, 1, 63, 64, 65, 130]


def test_api_version_and_names():
    header = open(os.path.join(ROOT, "include", "ivr_api.h")).read()
    assert re.search(r"#define\s+IVR_API_VERSION\s+11\b", header)
    assert _ffi.API_VERSION == 11 and _ffi.load().ivr_api_version() == 11
    for name in ("IVFPQIndex", "IndexIVFPQ", "ivfpq_scan_ref", "ivfpq_pack_ref", "ivfpq_unpack_ref"):
        assert name in ivr_amd.__all__
        assert getattr(ivr_amd, name) is getattr(ivr_amd.ivfpq, name)
    lib = ctypes.CDLL(_ffi.LIB_PATH)
    for name in NEW_EXPORTS:
        assert name in _ffi.EXPORTS and hasattr(lib, name)
        assert (name in _ffi._STREAM) == (name in WITH_STREAM)
    assert _ffi.load().ivr_ivfpq_probe_queries() >= 1


@pytest.mark.parametrize("name", ["ivr_ivfpq_create", "ivr_ivfpq_reset", "ivr_ivfpq_set_lists", "ivr_ivfpq_get_codes", "ivr_ivfpq_search"])
def test_null_arguments_are_refused_before_any_hip_call(name):
    lib = _ffi.load()
    assert lib.ivr_index_reset(None) == -1                          # leaves another message in the slot
    args = [0 if t in (_ffi._i, _ffi._i64) else None for t in _ffi._SIGS[name][1]]
    assert getattr(lib, name)(*args) == -1
    msg = lib.ivr_last_error(None)
    assert name.encode() in msg and b"NULL" in msg


class _NeverTouched:
    """In the quantizer's place where the constructor must refuse before it looks at the quantizer."""

    def __getattr__(self, name):
        raise AssertionError(f"the quantizer was touched ({name}) before the arguments were checked")


@pytest.mark.parametrize("args, text", [
    ((32, 4, 4, 4), "nbits"),
    ((32, 4, 4, 8, ivr_amd.METRIC_L2), "METRIC_L2"),
    ((32, 4, 4, 8, 7), "METRIC_INNER_PRODUCT"),
    ((30, 4, 4), "multiple of M"),
    ((1024, 4, 256), "M=256"),
    ((32, 4, 0), "M=0"),
    ((32, 0, 4), "nlist=0"),
])
def test_constructor_refusals_without_a_gpu(args, text):
    with pytest.raises(ValueError, match=text):
        IndexIVFPQ(_NeverTouched(), *args)


def test_constructor_refuses_a_quantizer_of_another_type():
    with pytest.raises(ValueError, match="must be a FlatIPIndex"):
        IndexIVFPQ(object(), 32, 4, 4)


def lists_of(sizes, M, seed=0):
    rng = np.random.default_rng(seed)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    return rng.integers(0, 256, (int(off[-1]), M), dtype=np.uint8), off


@pytest.mark.parametrize("M", [2, 16, 24, 64, 128])
def test_pack_unpack_round_trip_and_zero_pads(M):
    codes, off = lists_of(SIZES, M, seed=M)
    codes[codes == 0] = 1                       # every stored byte nonzero: whatever is zero in the layout is a pad
    packed = ivfpq_pack_ref(codes, off)
    W = {2: 1, 16: 1, 24: 2, 64: 4, 128: 8}[M]
    groups = sum((s + 63) // 64 for s in SIZES)
    assert packed.dtype == np.uint8 and packed.shape == (groups, W, 64, 16)
    assert np.array_equal(ivfpq_unpack_ref(packed, off, M), codes)
    assert np.count_nonzero(packed) == codes.size                    # pad bytes and pad rows are zero
    # where a row lives: list l starts at a whole group, row i of it is lane i % 64 of group goff[l] + i // 64, byte b is byte b % 16 of word b // 16
    pos, goff = ivfpq_positions_ref(off)
    assert goff.tolist() == [0, 0, 1, 2, 3, 5, 8]
    r = int(off[5]) + 70                          # row 70 of the list of 130
    assert pos[r] == 64 * 5 + 70
    assert packed[6, (M - 1) // 16, 6, (M - 1) % 16] == codes[r, M - 1]
    with pytest.raises(ValueError):
        ivfpq_unpack_ref(packed[:-1], off, M)                        # fewer groups than the lists need
    with pytest.raises(ValueError):
        ivfpq_pack_ref(codes, off[:-1])                              # offsets that do not end at n


def random_tables(rng, nq, M, values=None):
    if values is None:
        return rng.standard_normal((nq, M, 256)).astype(np.float32)
    return rng.choice(np.asarray(values, np.float32), (nq, M, 256))


def test_one_list_without_coarse_is_the_pq_scan_to_the_bit():
    rng = np.random.default_rng(1)
    codes, off = lists_of([200], 8, seed=2)
    T = random_tables(rng, 3, 8)
    zero, a = np.zeros((3, 1), np.float32), np.zeros((3, 1), np.int64)
    for k in (1, 10, 200, 260):
        D, I = ivfpq_scan_ref(T, zero, a, off, codes, np.arange(200), k)
        Dp, Ip = pq_scan_ref(T, codes, k)
        assert D.tobytes() == Dp.tobytes() and np.array_equal(I, Ip)


def test_several_lists_without_coarse_keep_the_pq_scores():
    rng = np.random.default_rng(3)
    codes, off = lists_of(SIZES, 6, seed=4)
    T = random_tables(rng, 4, 6)
    nlist = len(SIZES)
    a = np.tile(rng.permutation(nlist), (4, 1))                      # every list, in some order
    D, I = ivfpq_scan_ref(T, np.zeros((4, nlist), np.float32), a, off, codes, np.arange(len(codes)) + 1000, 50)
    Dp, Ip = pq_scan_ref(T, codes, 50)
    assert D.tobytes() == Dp.tobytes()
    assert np.array_equal(I, Ip + 1000)                              # list order is row order here, so the tie rules coincide


def test_hand_case_ties_duplicates_skips_and_padding():
    # three lists of 2, 1 and 2 rows; M = 1; the table maps code c to c / 4
    off = np.array([0, 2, 3, 5], np.int64)
    codes = np.array([[4], [8], [8], [4], [8]], np.uint8)            # scores without coarse: 1, 2 | 2 | 1, 2
    ids = np.array([50, 40, 30, 20, 10], np.int64)
    T = (np.arange(256, dtype=np.float32) / 4).reshape(1, 1, 256)
    zero = np.zeros((1, 3), np.float32)
    # ties: the lower list first, inside a list the earlier row; whatever order the lists are named in
    for a in ([0, 1, 2], [2, 0, 1], [1, 2, 0]):
        D, I = ivfpq_scan_ref(T, zero, np.array([a]), off, codes, ids, 6)
        assert I.tolist() == [[40, 30, 10, 50, 20, -1]] and D.tolist() == [[2, 2, 2, 1, 1, -FLT_MAX]]
    # -1 is skipped; a list named twice counts once, with the coarse score of its first mention after the stable sort: assign
    # [2, -1, 2, 0] sorts to [-1, 0, 2, 2] with coarse [9, 0.5, 3, 7], so list 2 gets 3 and not 7
    D, I = ivfpq_scan_ref(T, np.array([[3, 9, 7, 0.5]], np.float32), np.array([[2, -1, 2, 0]]), off, codes, ids, 5)
    assert I.tolist() == [[10, 20, 40, 50, -1]]
    assert D.tolist() == [[5.0, 4.0, 2.5, 1.5, -FLT_MAX]]
    # a nonzero coarse score changes the order between lists
    D, I = ivfpq_scan_ref(T, np.array([[0, 1.5, 0]], np.float32), np.array([[0, 1, 2]]), off, codes, ids, 2)
    assert I.tolist() == [[30, 40]] and D.tolist() == [[3.5, 2.0]]
    # nothing probed: padding only
    D, I = ivfpq_scan_ref(T, zero[:, :1], np.array([[-1]]), off, codes, ids, 2)
    assert (I == -1).all() and (D == -FLT_MAX).all()
    # coarse goes first: (1e8 + -1e8) + 1 is 1 in float32, (-1e8 + 1) + 1e8 with the coarse score last would be 0
    T2 = np.zeros((1, 2, 256), np.float32)
    T2[0, 0, 1], T2[0, 1, 1] = -1e8, 1.0
    D, _ = ivfpq_scan_ref(T2, np.array([[1e8]], np.float32), np.array([[0]]), np.array([0, 1]), np.array([[1, 1]], np.uint8), [0], 1)
    assert D[0, 0] == np.float32(1.0)
    assert (np.float32(-1e8) + np.float32(1.0)) + np.float32(1e8) == np.float32(0.0)
    # -0.0 counts and is reported as +0.0
    T3 = np.zeros((1, 1, 256), np.float32)
    T3[0, 0, 0] = -0.0
    D, I = ivfpq_scan_ref(T3, np.array([[-0.0]], np.float32), np.array([[0]]), np.array([0, 2]), np.array([[0], [1]], np.uint8), [7, 8], 2)
    assert I.tolist() == [[7, 8]] and not np.signbit(D).any()
    for bad in ([[3]], [[-2]]):
        with pytest.raises(ValueError):
            ivfpq_scan_ref(T, zero[:, :1], np.array(bad), off, codes, ids, 1)
