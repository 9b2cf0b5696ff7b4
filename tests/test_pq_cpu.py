"""CPU suite of the product-quantisation index (ivr_amd/pq.py, csrc/search_pq.hip): the binding, the argument checks that run before
any HIP call, the constructor's refusals and the numpy definitions the GPU suite compares the kernels with."""
import numpy as np
import pytest

import ivr_amd
from ivr_amd import _ffi
from ivr_amd.pq import IndexPQ, PQIndex, pq_encode_ref, pq_scan_ref, pq_tables_ref

FLT_MAX = np.finfo(np.float32).max
NEW_EXPORTS = ("ivr_pq_encode", "ivr_pq_tables", "ivr_bin_index_search_pq")


def test_api_version_and_names():
    assert _ffi.API_VERSION == 11 and _ffi.load().ivr_api_version() == 11
    for name in ("PQIndex", "IndexPQ", "pq_encode_ref", "pq_tables_ref", "pq_scan_ref"):
        assert name in ivr_amd.__all__
        assert getattr(ivr_amd, name) is getattr(ivr_amd.pq, name)
    for name in NEW_EXPORTS:
        assert name in _ffi.EXPORTS and name in _ffi._STREAM


@pytest.mark.parametrize("name", NEW_EXPORTS)
def test_null_arguments_are_refused_before_any_hip_call(name):
    lib = _ffi.load()
    assert lib.ivr_index_reset(None) == -1                          # leaves another message in the slot
    args = [0 if t in (_ffi._i, _ffi._i64) else None for t in _ffi._SIGS[name][1]]
    assert getattr(lib, name)(*args) == -1
    msg = lib.ivr_last_error(None)
    assert name.encode() in msg and b"NULL" in msg


def tables(M, rows):
    """T [1,M,256] whose entry (m, j) is rows[m][j] for the j given, 0 elsewhere."""
    T = np.zeros((1, M, 256), np.float32)
    for m, r in enumerate(rows):
        for j, v in r.items():
            T[0, m, j] = v
    return T


def test_scan_ref_adds_in_ascending_m_in_float32():
    T = tables(3, [{1: 1e8}, {1: -1e8}, {1: 1.0}])
    codes = np.array([[1, 1, 1]], np.uint8)
    D, I = pq_scan_ref(T, codes, 1)
    assert D[0, 0] == np.float32(1.0) and I[0, 0] == 0                     # (1e8 + -1e8) + 1
    a, b, c = np.float32(1e8), np.float32(-1e8), np.float32(1.0)
    assert (c + b) + a == np.float32(0.0)                                  # descending m gives other bits
    assert np.float32(np.float64(a) + np.float64(c)) + b == np.float32(0.0)   # and so does (T0 + T2) + T1


def test_scan_ref_ties_zero_sign_and_padding():
    T = tables(2, [{0: 0.5, 1: 0.25, 2: -0.0}, {0: 0.5, 1: 0.75, 2: -0.0}])
    codes = np.array([[1, 1], [0, 0], [2, 2], [0, 0], [1, 1]], np.uint8)   # scores 1, 1, -0, 1, 1
    D, I = pq_scan_ref(T, codes, 7)
    assert I.tolist() == [[0, 1, 3, 4, 2, -1, -1]]                         # equal scores: the lower row first; k > n: padding
    assert D[0, :4].tolist() == [1.0] * 4
    assert D[0, 4] == 0.0 and not np.signbit(D[0, 4])                      # -0.0 is reported as +0.0
    assert (D[0, 5:] == -FLT_MAX).all()
    # -0.0 counts as +0.0 when ranking: a row scoring +0.0 behind one scoring -0.0 keeps its place
    T = tables(1, [{0: -0.0, 1: 0.0}])
    D, I = pq_scan_ref(T, np.array([[0], [1], [0]], np.uint8), 3)
    assert I.tolist() == [[0, 1, 2]] and not np.signbit(D).any()
    D, I = pq_scan_ref(T, np.zeros((0, 1), np.uint8), 2)
    assert (I == -1).all() and (D == -FLT_MAX).all()
    with pytest.raises(ValueError):
        pq_scan_ref(T, np.zeros((3, 2), np.uint8), 1)                      # codes of another M


def test_encode_ref_picks_the_lower_of_identical_centroids():
    rng = np.random.default_rng(3)
    C = rng.standard_normal((2, 256, 4)).astype(np.float32)
    C[0, 200] = C[0, 7]
    C[1, 9] = C[1, 255]
    x = np.concatenate([C[0, 200], C[1, 255]])[None]
    codes, dist = pq_encode_ref(x, C)
    assert codes.dtype == np.uint8 and codes.tolist() == [[7, 9]]
    assert dist.shape == (1, 2, 256) and dist[0, 0, 7] == dist[0, 0, 200] == 0.0


def test_tables_ref_is_the_float64_inner_product():
    rng = np.random.default_rng(4)
    C = rng.standard_normal((3, 256, 2)).astype(np.float32)
    q = rng.standard_normal((5, 6)).astype(np.float32)
    T = pq_tables_ref(q, C)
    assert T.dtype == np.float64 and T.shape == (5, 3, 256)
    assert T[4, 2, 17] == float(q[4, 4]) * float(C[2, 17, 0]) + float(q[4, 5]) * float(C[2, 17, 1])


@pytest.mark.parametrize("args, text", [
    ((30, 4), "multiple of M"),
    ((32, 4, 4), "nbits"),
    ((32, 4, 8, ivr_amd.METRIC_L2), "METRIC_L2"),
    ((32, 4, 8, 7), "METRIC_INNER_PRODUCT"),
    ((1024, 256), "M=256"),
    ((32, 0), "M=0"),
])
def test_constructor_refusals(args, text):
    for make in (IndexPQ, PQIndex):
        with pytest.raises(ValueError, match=text):
            make(*args)
