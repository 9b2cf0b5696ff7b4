"""CPU suite of the 4-bit product-quantisation index (ivr_amd/pqfs.py, csrc/search_pqfs.hip): the binding, the argument checks that
run before any HIP call, the constructor's refusals, and the numpy definitions the GPU suite compares the kernels with."""
import numpy as np
import pytest

import ivr_amd
from ivr_amd import _ffi
from ivr_amd.pq import IndexPQ
from ivr_amd.pqfs import (IndexPQFastScan, PQFastScanIndex, pqfs_encode_ref, pqfs_pack_ref, pqfs_quantize_ref, pqfs_scan_ref,
                          pqfs_score_bound, pqfs_tables_ref, pqfs_unpack_ref)

FLT_MAX = np.finfo(np.float32).max
F = np.float32
MS = (2, 6, 16, 30, 64, 128, 256)
NEW_EXPORTS = ("ivr_pqfs_pass_queries", "ivr_pqfs_encode", "ivr_pqfs_tables", "ivr_pqfs_quantize", "ivr_pqfs_index_create",
               "ivr_pqfs_index_destroy", "ivr_pqfs_index_reset", "ivr_pqfs_index_ntotal", "ivr_pqfs_index_add", "ivr_pqfs_index_get_codes",
               "ivr_pqfs_index_search")
WITH_STREAM = ("ivr_pqfs_encode", "ivr_pqfs_tables", "ivr_pqfs_quantize", "ivr_pqfs_index_add", "ivr_pqfs_index_get_codes",
               "ivr_pqfs_index_search")
NAMES = ("PQFastScanIndex", "IndexPQFastScan", "pqfs_pack_ref", "pqfs_unpack_ref", "pqfs_encode_ref", "pqfs_tables_ref",
         "pqfs_quantize_ref", "pqfs_scan_ref", "pqfs_score_bound")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# -- binding -------------------------------------------------------------------------------------------------------------------
def test_names_and_exports():
    assert _ffi.load().ivr_api_version() == _ffi.API_VERSION
    for name in NAMES:
        assert name in ivr_amd.__all__
        assert getattr(ivr_amd, name) is getattr(ivr_amd.pqfs, name)
    lib = _ffi.load()
    for name in NEW_EXPORTS:
        assert name in _ffi.EXPORTS and hasattr(lib, name)
        assert (name in _ffi._STREAM) == (name in WITH_STREAM)
    assert _ffi.IVR_PQFS_MAX_M == 256
    P = lib.ivr_pqfs_pass_queries()
    assert 1 <= P <= 64


@pytest.mark.parametrize("name", [n for n in NEW_EXPORTS if n != "ivr_pqfs_pass_queries"])
def test_null_arguments_are_refused_before_any_hip_call(name):
    lib = _ffi.load()
    assert lib.ivr_index_reset(None) == -1                          # leaves another message in the slot
    args = [0 if t in (_ffi._i, _ffi._i64) else None for t in _ffi._SIGS[name][1]]
    assert getattr(lib, name)(*args) == -1
    msg = lib.ivr_last_error(None)
    assert name.encode() in msg and b"NULL" in msg


# -- constructor ---------------------------------------------------------------------------------------------------------------
def test_attributes_and_refusals():
    idx = IndexPQFastScan(96, 12)
    assert isinstance(idx, PQFastScanIndex)
    assert (idx.d, idx.M, idx.dsub, idx.nbits, idx.ksub, idx.code_size) == (96, 12, 8, 4, 16, 6)
    assert idx.ntotal == 0 and idx.is_trained is False and idx.metric_type == ivr_amd.METRIC_INNER_PRODUCT
    assert idx.centroids.shape == (12, 16, 8) and idx.centroids.dtype == np.float32
    with pytest.raises(ValueError, match="only nbits=4 is supported, got 8"):
        IndexPQFastScan(96, 12, 8)
    with pytest.raises(ValueError, match="METRIC_L2 is not supported"):
        IndexPQFastScan(96, 12, 4, ivr_amd.METRIC_L2)
    for M in (0, 1, 7, 258, 512):
        with pytest.raises(ValueError, match=f"M={M} odd or outside"):
            IndexPQFastScan(M * 2 if M else 8, M)
    with pytest.raises(ValueError, match="not a multiple of M=12"):
        IndexPQFastScan(100, 12)
    x = np.zeros((20, 96), F)
    with pytest.raises(RuntimeError, match="add: the index is not trained"):
        idx.add(x)
    with pytest.raises(RuntimeError, match="search: the index is not trained"):
        idx.search(x[:1], 3)
    with pytest.raises(RuntimeError, match="sa_encode: the index is not trained"):
        idx.sa_encode(x)
    with pytest.raises(ValueError, match=r"centroids expects \[12,16,8\]"):
        idx.centroids = np.zeros((12, 256, 8), F)
    with pytest.raises(ValueError, match="15 training rows for 16 centroids"):
        idx.train(x[:15])
    idx.centroids = np.ones((12, 16, 8), F)
    assert idx.is_trained


def test_pqindex_keeps_refusing_4_bits():
    with pytest.raises(ValueError, match="only nbits=8"):
        IndexPQ(64, 8, 4)


# -- the numpy definitions -----------------------------------------------------------------------------------------------------
def test_pack_round_trip_and_nibble_order():
    rng = np.random.default_rng(0)
    c = rng.integers(0, 16, (37, 10)).astype(np.uint8)
    p = pqfs_pack_ref(c)
    assert p.dtype == np.uint8 and p.shape == (37, 5)
    assert np.array_equal(pqfs_unpack_ref(p), c)
    assert np.array_equal(pqfs_pack_ref(np.array([[1, 2, 15, 0]])), np.array([[0x21, 0x0f]], np.uint8))       # faiss: low nibble first
    allb = np.arange(256, dtype=np.uint8).reshape(-1, 1)
    assert np.array_equal(pqfs_pack_ref(pqfs_unpack_ref(allb)), allb)
    for bad in (np.zeros((2, 3)), np.full((2, 2), 16)):
        with pytest.raises(ValueError):
            pqfs_pack_ref(bad)


def test_encode_ref_prefers_the_lower_centroid():
    rng = np.random.default_rng(1)
    cent = rng.standard_normal((4, 16, 3)).astype(F)
    cent[1, 9] = cent[1, 2]                                          # identical centroids
    x = rng.standard_normal((50, 12)).astype(F)
    x[:10, 3:6] = cent[1, 9]
    codes, dist = pqfs_encode_ref(x, cent)
    assert codes.shape == (50, 4) and dist.shape == (50, 4, 16) and codes.max() < 16
    assert (codes[:10, 1] == 2).all() and (codes[:, 1] != 9).all()
    assert np.array_equal(codes, dist.argmin(-1))
    T = pqfs_tables_ref(x, cent)
    assert T.shape == (50, 4, 16) and np.allclose(T[7, 3, 5], x[7, 9:12].astype(np.float64) @ cent[3, 5])


def test_scan_ref_orders_by_integer_then_row():
    # M = 2: table 0 scores its code, table 1 is flat.  Rows: codes (3,0) (5,1) (5,9) (3,0) (0,0)
    U = np.zeros((1, 2, 16), np.uint8)
    U[0, 0] = np.arange(16) * 10
    U[0, 1] = 7
    codes = pqfs_pack_ref(np.array([[3, 0], [5, 1], [5, 9], [3, 0], [0, 0]]))
    D, I = pqfs_scan_ref(U, [F(0.5)], [F(-1)], codes, 7)
    assert I.tolist() == [[1, 2, 0, 3, 4, -1, -1]]
    assert D[0, :5].tolist() == [27.5, 27.5, 17.5, 17.5, 2.5] and (D[0, 5:] == -FLT_MAX).all()
    # two acc that round to one D keep the integer order: a bias of 2^24 absorbs a step of 1
    U2 = np.zeros((1, 2, 16), np.uint8)
    U2[0, 0, :3] = (0, 1, 1)
    D2, I2 = pqfs_scan_ref(U2, [F(1)], [F(2.0 ** 24)], pqfs_pack_ref(np.array([[0, 0], [1, 0], [2, 0]])), 3)
    assert I2.tolist() == [[1, 2, 0]] and (_bits(D2) == _bits(F(2.0 ** 24))).all()
    D0, I0 = pqfs_scan_ref(U, [F(1)], [F(0)], np.zeros((0, 1), np.uint8), 2)
    assert (I0 == -1).all() and (D0 == -FLT_MAX).all()
    with pytest.raises(ValueError):
        pqfs_scan_ref(U, [F(1)], [F(0)], np.zeros((3, 2), np.uint8), 2)          # M / 2 bytes per row


@pytest.mark.parametrize("M", MS)
def test_quantize_ref_invariants_and_bound(M):
    rng = np.random.default_rng(100 + M)
    nq, n = 6, 3000
    T = (rng.standard_normal((nq, M, 16)) * rng.choice([0.01, 1.0, 30.0], (nq, M, 1)) + rng.standard_normal((nq, M, 1))).astype(F)
    U, scale, bias = pqfs_quantize_ref(T)
    assert U.dtype == np.uint8 and scale.dtype == F and bias.dtype == F
    lo = T.min(axis=2)
    span = (T.max(axis=2) - lo).max(axis=1)
    # without the clamp: the same integers
    raw = np.rint(((T - lo[:, :, None]).astype(F) * (F(255) / span)[:, None, None]).astype(F))
    assert raw.min() >= 0 and raw.max() <= 255 and np.array_equal(raw.astype(np.uint8), U)
    assert (U.min(axis=2) == 0).all() and (U.max() == 255)          # every slice touches 0, the widest one 255
    codes = rng.integers(0, 16, (n, M)).astype(np.uint8)
    acc = np.zeros((nq, n), np.int64)
    exact = np.zeros((nq, n))
    for m in range(M):
        acc += U[:, m, codes[:, m]]
        exact += T[:, m, codes[:, m]].astype(np.float64)
    assert acc.max() <= 255 * M
    D, I = pqfs_scan_ref(U, scale, bias, pqfs_pack_ref(codes), n)
    assert (np.diff(np.take_along_axis(acc, I, axis=1), axis=1) <= 0).all()
    err = np.abs(D.astype(np.float64) - np.take_along_axis(exact, I, axis=1))
    bound = pqfs_score_bound(T)
    assert (err <= bound[:, None]).all()
    assert (bound <= (M * span / 510.0) * 1.001 + 1e-4 * np.abs(lo).sum(axis=1)).all()     # the quantisation step dominates it


def test_quantize_ref_degenerate_spans():
    M = 6
    T = np.zeros((4, M, 16), F)
    T[0] = np.arange(M, dtype=F)[:, None] - 2                       # span == 0: every slice constant
    T[1, 3, 5] = F(1e-39)                                            # a subnormal span: 255 / span overflows
    T[2] = T[0]
    T[2, 4, 7] += F(3)                                               # one slice alone varies
    T[3, :, :] = F(-7)
    T[3, 0, 0] = np.nextafter(F(-7), F(0))                           # the smallest span at that magnitude
    U, scale, bias = pqfs_quantize_ref(T)
    assert not U[0].any() and scale[0] == 0 and bias[0] == F(sum(range(M)) - 2 * M)
    assert not U[1].any() and scale[1] == 0 and bias[1] == 0
    assert U[2].sum() == 255 and U[2, 4, 7] == 255 and scale[2] == F(3) / F(255)
    assert U[3].sum() == 255 and U[3, 0, 0] == 255
    codes = pqfs_pack_ref(np.array([[0] * M, [0, 0, 0, 0, 7, 0]]))
    D, I = pqfs_scan_ref(U, scale, bias, codes, 2)
    assert I[0].tolist() == [0, 1] and (D[0] == bias[0]).all()      # D = bias where the tables are flat
    assert I[2].tolist() == [1, 0] and D[2, 0] == F(255) * scale[2] + bias[2]
    bound = pqfs_score_bound(T)
    assert bound[0] < 1e-5 and bound[1] >= M * 1e-39 and bound[1] < 1e-30
