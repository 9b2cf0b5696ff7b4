"""CPU suite of the scalar-quantiser index (ivr_amd/sq.py, csrc/search_sq.hip): the binding, the argument checks that run before any
HIP call, the constructor's refusals, the numpy definitions the GPU suite compares the kernels with, and the recall of the integer
ranking against faiss's float decode."""
import numpy as np
import pytest

import ivr_amd
from ivr_amd import _ffi
from ivr_amd.sq import (IndexScalarQuantizer, ScalarQuantizer, SQIndex, sq_decode_ref, sq_encode_ref, sq_query_ref, sq_scan_ref,
                        sq_score_bound, sq_split_ref, sq_train_ref)

FLT_MAX = np.finfo(np.float32).max
F = np.float32
NEW_EXPORTS = ("ivr_sq_encode", "ivr_sq_query", "ivr_sq_index_create", "ivr_sq_index_destroy", "ivr_sq_index_reset",
               "ivr_sq_index_ntotal", "ivr_sq_index_add", "ivr_sq_index_get_codes", "ivr_sq_index_search")
WITH_STREAM = ("ivr_sq_encode", "ivr_sq_query", "ivr_sq_index_add", "ivr_sq_index_get_codes", "ivr_sq_index_search")


def test_api_version_and_names():
    assert _ffi.API_VERSION == 11 and _ffi.load().ivr_api_version() == 11
    for name in ("SQIndex", "IndexScalarQuantizer", "ScalarQuantizer", "sq_encode_ref", "sq_decode_ref", "sq_query_ref", "sq_scan_ref"):
        assert name in ivr_amd.__all__
        assert getattr(ivr_amd, name) is getattr(ivr_amd.sq, name)
    for name in NEW_EXPORTS:
        assert name in _ffi.EXPORTS
        assert (name in _ffi._STREAM) == (name in WITH_STREAM)
    assert (ScalarQuantizer.QT_8bit, ScalarQuantizer.QT_4bit, ScalarQuantizer.QT_fp16, ScalarQuantizer.QT_6bit) == (0, 1, 4, 6)


@pytest.mark.parametrize("name", NEW_EXPORTS)
def test_null_arguments_are_refused_before_any_hip_call(name):
    lib = _ffi.load()
    assert lib.ivr_index_reset(None) == -1                          # leaves another message in the slot
    args = [0 if t in (_ffi._i, _ffi._i64) else None for t in _ffi._SIGS[name][1]]
    assert getattr(lib, name)(*args) == -1
    msg = lib.ivr_last_error(None)
    assert name.encode() in msg and b"NULL" in msg


@pytest.mark.parametrize("args, text", [
    ((0,), "d=0"),
    ((1025,), "d=1025"),
    ((64, ScalarQuantizer.QT_4bit), "QT_8bit"),
    ((64, ScalarQuantizer.QT_fp16), "QT_8bit"),
    ((64, ScalarQuantizer.QT_8bit, ivr_amd.METRIC_L2), "METRIC_L2"),
])
def test_constructor_refusals(args, text):
    for make in (IndexScalarQuantizer, SQIndex):
        with pytest.raises(ValueError, match=text):
            make(*args)


def test_untrained_index_refuses_add_and_search():
    x = IndexScalarQuantizer(8)
    assert not x.is_trained and x.ntotal == 0 and x.code_size == 8
    rows = np.zeros((3, 8), F)
    for call in (lambda: x.add(rows), lambda: x.search(rows, 1), lambda: x.sa_encode(rows), lambda: x.compute_query_codes(rows),
                 lambda: x.search_codes(np.zeros((1, 8), np.int16), np.ones(1, F), np.zeros(1, F), 1)):
        with pytest.raises(RuntimeError, match="not trained"):
            call()
    with pytest.raises(ValueError):
        x.trained = np.zeros(15, F)
    with pytest.raises(ValueError, match="finite"):
        x.trained = np.full(16, np.nan, F)
    with pytest.raises(ValueError):
        x.train(np.zeros((0, 8), F))
    with pytest.raises(ValueError, match="finite"):
        x.train(np.full((2, 8), np.inf, F))
    x.trained = np.arange(16, dtype=np.float64)                      # assignable while empty: trained from then on
    assert x.is_trained and x.trained.dtype == np.float32


# -- encoder ---------------------------------------------------------------------------------------------------------------------
def test_train_ref_is_min_and_range():
    x = np.array([[1.0, -2.0, 5.0], [3.0, -7.0, 5.0], [2.0, 0.5, 5.0]], F)
    assert sq_train_ref(x).tolist() == [1.0, -7.0, 5.0, 2.0, 7.5, 0.0]


def test_encode_ref_on_hand_made_values():
    tr = np.array([-1.0, 0.0, 3.0, 0.0, 2.0, 1.0, 0.0, 1.0], F)      # vmin | vdiff; column 2 has no range
    vmin, vmax = tr[:4], tr[:4] + tr[4:]
    assert sq_encode_ref(vmin[None], tr).tolist() == [[0, 0, 0, 0]]
    assert sq_encode_ref(vmax[None], tr).tolist() == [[255, 255, 0, 255]]
    assert sq_encode_ref(np.array([[-5.0, -0.1, -9.0, -1e30], [9.0, 1.5, 9.0, 1e30]], F), tr).tolist() == [[0, 0, 0, 0], [255, 255, 0, 255]]
    # truncation, not rounding: 255 * xi = 127.9 is bucket 127
    assert sq_encode_ref(np.array([[0.0, 0.0, 0.0, F(127.9) / F(255)]], F), tr)[0, 3] == 127
    # the largest float whose float32 product 255f * xi stays below the edge 128 truncates down; the next one is bucket 128
    x = F(128) / F(255)
    while F(255) * x >= F(128):
        x = np.nextafter(x, F(0))
    up = np.nextafter(x, F(1))
    assert F(255) * up >= F(128)
    assert sq_encode_ref(np.array([[0, 0, 0, x], [0, 0, 0, up]], F), tr)[:, 3].tolist() == [127, 128]


def test_decode_ref_is_the_bucket_centre_in_float32():
    tr = np.array([-1.0, 0.25, 2.0, 0.0], F)
    got = sq_decode_ref(np.array([[0, 7], [255, 200]], np.uint8), tr)
    assert got.dtype == np.float32
    assert got[0, 0] == F(-1.0) + F(2.0) * ((F(0) + F(0.5)) / F(255))
    assert got[1, 0] == F(-1.0) + F(2.0) * ((F(255) + F(0.5)) / F(255))
    assert got[:, 1].tolist() == [0.25, 0.25]


# -- query preparation -----------------------------------------------------------------------------------------------------------
def test_query_ref_zero_extremes_and_half_to_even():
    tr = np.concatenate([np.zeros(3, F), np.full(3, 255, F)])        # gain = 1, offset = 128.5
    t, s, b = sq_query_ref(np.zeros((1, 3), F), tr)
    assert t.dtype == np.int16 and t.tolist() == [[0, 0, 0]] and s.tolist() == [1.0] and b.tolist() == [0.0]
    t, s, b = sq_query_ref(np.array([[1.0, -1.0, 0.5]], F), tr)
    assert t.tolist() == [[16256, -16256, 8128]] and s[0] == F(1) / F(16256) and s.dtype == np.float32
    assert b[0] == 0.5 * 128.5
    # scale = 2^-14 exactly, so w / scale = 2.5 and 3.5 are exact halves: they round to the even neighbour
    t, s, b = sq_query_ref(np.array([[16256 / 16384, 2.5 / 16384, -3.5 / 16384]], F), tr)
    assert s[0] == F(2.0 ** -14) and t.tolist() == [[16256, 2, -4]]


def test_split_ref_halves():
    t = np.array([16256, -16256, 0, 63, 64, -64, -65, 127 * 128 - 64], np.int16)
    h, l = sq_split_ref(t)
    assert h.dtype == np.int8 and l.dtype == np.int8
    assert (128 * h.astype(np.int32) + l == t).all()
    assert h.tolist() == [127, -127, 0, 0, 1, 0, -1, 127] and l.tolist() == [0, 0, 0, 63, -64, -64, 63, -64]


# -- scan ------------------------------------------------------------------------------------------------------------------------
def _codes(cp):
    return (np.asarray(cp, np.int64) + 128).astype(np.uint8)


def test_scan_ref_ties_padding_and_empty():
    t = np.array([[2, -1]], np.int16)
    codes = _codes([[1, 0], [3, 4], [1, 0], [0, -2], [-5, 0]])       # acc 2, 2, 2, 2, -10
    one, zero = np.ones(1, F), np.zeros(1, F)
    D, I = sq_scan_ref(t, one, zero, codes, 7)
    assert I.tolist() == [[0, 1, 2, 3, 4, -1, -1]]                   # equal acc: the lower row first; k > n: padding
    assert D[0, :5].tolist() == [2.0, 2.0, 2.0, 2.0, -10.0] and (D[0, 5:] == -FLT_MAX).all()
    D, I = sq_scan_ref(t, np.array([0.5], F), np.array([1.0], F), codes, 2)
    assert D.dtype == np.float32 and I.dtype == np.int64 and D.tolist() == [[2.0, 2.0]] and I.tolist() == [[0, 1]]
    D, I = sq_scan_ref(t, one, zero, np.zeros((0, 2), np.uint8), 2)
    assert (I == -1).all() and (D == -FLT_MAX).all()
    with pytest.raises(ValueError):
        sq_scan_ref(t, one, zero, np.zeros((3, 3), np.uint8), 1)      # codes of another d
    with pytest.raises(ValueError):
        sq_scan_ref(np.array([[16257, 0]], np.int16), one, zero, codes, 1)


def test_scan_ref_holds_the_extreme_accumulator_without_wrapping():
    codes = np.zeros((2, 1024), np.uint8)                            # c' = -128 everywhere
    codes[1] = 255                                                   # c' = 127
    t = np.stack([np.full(1024, 16256, np.int16), np.full(1024, -16256, np.int16)])
    D, I = sq_scan_ref(t, np.ones(2, F), np.zeros(2, F), codes, 2)
    assert I.tolist() == [[1, 0], [0, 1]]
    assert D.astype(np.float64).tolist() == [[16256.0 * 127 * 1024, -2130706432.0], [2130706432.0, -16256.0 * 127 * 1024]]


def test_scan_ref_rounds_every_step_in_float32():
    # acc = 2^24 + 1: float32(acc) = 2^24 (half to even), + 1 = 2^24 + 1 -> 2^24 again; in float64 the sum is 2^24 + 2, a float32
    t = np.array([[16256] * 9 + [1025]], np.int16)
    codes = _codes([[127] * 8 + [16, 1]])
    acc = int(t[0].astype(np.int64) @ (codes[0].astype(np.int64) - 128))
    assert acc == 2 ** 24 + 1
    D, _ = sq_scan_ref(t, np.ones(1, F), np.ones(1, F), codes, 1)
    assert D[0, 0] == F(2 ** 24)
    assert F(np.float64(acc) * 1.0 + 1.0) == F(2 ** 24 + 2)


# -- recall of the definition ----------------------------------------------------------------------------------------------------
def _unit(rng, n, d):
    x = rng.standard_normal((n, d)).astype(np.float32)
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def clustered(n, d, ncent, nq, seed=1234):
    """Unit rows around ncent random unit centres, row = normalize(centre[j] + g / sqrt(d)), and nq queries of the same kind."""
    rng = np.random.default_rng(seed)
    c = _unit(rng, ncent, d)

    def draw(m):
        x = c[rng.integers(0, ncent, m)] + rng.standard_normal((m, d)).astype(np.float32) / np.float32(d ** 0.5)
        return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)
    return draw(n), draw(nq)


def _recall(I, truth):
    return float(np.mean([len(set(a) & set(b)) / len(b) for a, b in zip(I.tolist(), truth.tolist())]))


def test_integer_ranking_recalls_what_the_float_decode_recalls():
    """Measured: recall@10 of the float64 decode ranking 0.9905, of the integer ranking 0.9905 (5,003 x 64 rows, 200 queries)."""
    X, Q = clustered(5003, 64, 64, 200)
    tr = sq_train_ref(X)
    codes = sq_encode_ref(X, tr)
    exact = np.argsort(-(Q.astype(np.float64) @ X.astype(np.float64).T), axis=1, kind="stable")[:, :10]
    vmin, vdiff = tr[:64].astype(np.float64), tr[64:].astype(np.float64)
    dec = vmin + vdiff * (codes.astype(np.float64) + 0.5) / 255.0
    S = Q.astype(np.float64) @ dec.T
    r_float = _recall(np.argsort(-S, axis=1, kind="stable")[:, :10], exact)
    t, s, b = sq_query_ref(Q, tr)
    D, I = sq_scan_ref(t, s, b.astype(np.float32), codes, 10)
    r_int = _recall(I, exact)
    print(f"recall@10 against the exact top-10: float64 decode {r_float:.4f}, integer ranking {r_int:.4f}")
    assert r_int >= r_float - 0.01
    # and every reported score lies within the stated bound of faiss's score
    bound = np.take_along_axis(sq_score_bound(Q, codes, tr, s), I, axis=1)
    err = np.abs(D.astype(np.float64) - np.take_along_axis(S, I, axis=1))
    print(f"largest |D - <q, decode>| / bound = {(err / bound).max():.3f}")
    assert (err <= bound).all()
