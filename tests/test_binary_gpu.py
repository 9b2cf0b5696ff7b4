"""GPU suite of the binary flat index (ivr_amd/binary.py BinaryFlatIndex, csrc/search_binary.hip).

Everything here is integer and exact.  The oracle is numpy: dist = unpackbits(a ^ b).sum(), order = lexsort((row, dist)); D and I
must be equal element for element, pad slots (k > ntotal) are INT32_MAX and -1.  Sizes are taken from ivr_bin_index_block_rows() so
that they sit on both sides of a workgroup block and of a 64-row wave group; ties, which the counting selection has to break by row,
are forced by short codes, few distinct codes and hand-built distance profiles."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

INT32_MAX = np.iinfo(np.int32).max
_POP = np.unpackbits(np.arange(256, dtype=np.uint8)[:, None], axis=1).sum(1).astype(np.int64)


def _block():
    from ivr_amd import _ffi
    return _ffi.load().ivr_bin_index_block_rows()


def oracle(X, Q, k):
    """X uint8 [n,c], Q uint8 [nq,c] -> (D int32 [nq,k], I int64 [nq,k]) by full sort, ties to the lower row."""
    nq, n = len(Q), len(X)
    D = np.full((nq, k), INT32_MAX, np.int32)
    I = np.full((nq, k), -1, np.int64)
    if n:
        dist = _POP[Q[:, None, :] ^ X[None, :, :]].sum(2)
        rows = np.arange(n)
        for q in range(nq):
            order = np.lexsort((rows, dist[q]))[:k]
            D[q, :len(order)] = dist[q, order]
            I[q, :len(order)] = order
    return D, I


def check(index, X, Q, k):
    D, I = index.search(Q, k)
    assert D.dtype == np.int32 and I.dtype == np.int64 and D.shape == I.shape == (len(Q), k)
    Dr, Ir = oracle(X, Q, k)
    assert np.array_equal(D, Dr)
    assert np.array_equal(I, Ir)


def make(X):
    from ivr_amd.binary import BinaryFlatIndex
    idx = BinaryFlatIndex(8 * X.shape[1])
    idx.add(X)
    assert idx.ntotal == len(X)
    return idx


def with_distance(rng, dist, d_bits=64):
    """One code at Hamming distance `dist` from the all-zero code: `dist` random bit positions set."""
    bits = np.zeros(d_bits, np.uint8)
    bits[rng.choice(d_bits, dist, replace=False)] = 1
    return np.packbits(bits, bitorder="little")


SIZES = ["1", "63", "64", "65", "B-1", "B", "B+1", "2*B+5"]


def _size(s):
    return int(eval(s, {"B": _block()}))


# 8 .. 320: the sizes named by the contract (1 to 3 words of 16 bytes); 512, 1000, 2048: the 4-, 8- and 16-word kernels
@pytest.mark.parametrize("d_bits", [8, 64, 128, 256, 320, 512, 1000, 2048])
@pytest.mark.parametrize("size", SIZES)
def test_sizes(size, d_bits):
    n = _size(size)
    rng = np.random.default_rng(1000 * d_bits + n)
    X = rng.integers(0, 256, (n, d_bits // 8), dtype=np.uint8)
    Q = rng.integers(0, 256, (17, d_bits // 8), dtype=np.uint8)
    Q[:3] = X[rng.integers(0, n, 3)]                  # stored rows as queries: distance 0
    Q[3] = X[n - 1] ^ np.uint8(1)                     # one bit away from the last row
    idx = make(X)
    try:
        for k in (1, 10):                             # k = 10 > n = 1: pad slots
            check(idx, X, Q, k)
    finally:
        idx.close()


@pytest.mark.parametrize("nq", [1, 17, 70])
@pytest.mark.parametrize("k", [1, 10, 2048])
def test_short_codes_many_ties(k, nq):
    """d_bits = 8, 1,000 rows: at most 9 distinct distances, so every result is decided by the row order inside a tie bin; k = 2048
    exceeds the 1,000 rows (pad slots), nq = 70 crosses the query chunk of 64."""
    rng = np.random.default_rng(11)
    X = rng.integers(0, 256, (1000, 1), dtype=np.uint8)
    Q = rng.integers(0, 256, (nq, 1), dtype=np.uint8)
    idx = make(X)
    try:
        check(idx, X, Q, k)
    finally:
        idx.close()


@pytest.mark.parametrize("k", [1, 10, 2048])
def test_three_distinct_codes(k):
    B = _block()
    rng = np.random.default_rng(12)
    values = rng.integers(0, 256, (3, 16), dtype=np.uint8)
    X = values[rng.integers(0, 3, 9 * B + 5)]
    Q = np.concatenate([values, rng.integers(0, 256, (14, 16), dtype=np.uint8)])
    idx = make(X)
    try:
        check(idx, X, Q, k)
    finally:
        idx.close()


@pytest.mark.parametrize("k", [1, 10, 2048])
def test_all_rows_identical(k):
    B = _block()
    rng = np.random.default_rng(13)
    code = rng.integers(0, 256, (1, 32), dtype=np.uint8)
    X = np.repeat(code, 12 * B + 7, axis=0)
    Q = np.concatenate([code, rng.integers(0, 256, (2, 32), dtype=np.uint8)])
    idx = make(X)
    try:
        D, I = idx.search(Q, k)
        assert np.array_equal(I, np.tile(np.arange(k), (3, 1)))        # rows 0 .. k-1, whatever the distance
        assert (D[0] == 0).all()
        check(idx, X, Q, k)
    finally:
        idx.close()


@pytest.mark.parametrize("inside", [8, 10, 11, 15])
def test_tie_bin_straddles_a_block_boundary(inside):
    """3 rows nearer than the tie bin; the tie bin (distance 2) is rows B-10 .. B+10, across the boundary of blocks 0 and 1; k = 3 +
    inside ends in front of, at, just behind and well behind the boundary."""
    B = _block()
    rng = np.random.default_rng(14)
    n = 2 * B + 5
    X = np.stack([with_distance(rng, 5) for _ in range(n)])
    for r in range(B - 10, B + 11):
        X[r] = with_distance(rng, 2)
    for r, dist in ((7, 0), (B + 40, 1), (2 * B + 1, 1)):
        X[r] = with_distance(rng, dist)
    Q = np.zeros((1, 8), np.uint8)
    idx = make(X)
    try:
        k = 3 + inside
        D, I = idx.search(Q, k)
        assert I[0].tolist() == [7, B + 40, 2 * B + 1] + list(range(B - 10, B - 10 + inside))
        assert D[0].tolist() == [0, 1, 1] + [2] * inside
        check(idx, X, Q, k)
    finally:
        idx.close()


def test_tie_bin_in_the_last_block_only():
    """The rows below the threshold sit in blocks 0 and 1, every row of the tie bin in the (partly filled) last block."""
    B = _block()
    rng = np.random.default_rng(15)
    n = 2 * B + 5
    X = np.stack([with_distance(rng, 9) for _ in range(n)])
    for r in (0, 70, B - 1, B + 3):
        X[r] = with_distance(rng, 1)
    for r in range(2 * B, n):
        X[r] = with_distance(rng, 3)
    Q = np.zeros((1, 8), np.uint8)
    idx = make(X)
    try:
        for k in (5, 6, 9, 10):
            D, I = idx.search(Q, k)
            tie = min(k - 4, 5)
            assert I[0, :4 + tie].tolist() == [0, 70, B - 1, B + 3] + list(range(2 * B, 2 * B + tie))
            check(idx, X, Q, k)
    finally:
        idx.close()


def test_empty_index_and_k_beyond_ntotal():
    from ivr_amd.binary import IndexBinaryFlat
    rng = np.random.default_rng(16)
    idx = IndexBinaryFlat(64)
    try:
        Q = rng.integers(0, 256, (3, 8), dtype=np.uint8)
        for k in (1, 10, 2048):
            D, I = idx.search(Q, k)
            assert (D == INT32_MAX).all() and (I == -1).all() and D.dtype == np.int32 and I.dtype == np.int64
        X = rng.integers(0, 256, (5, 8), dtype=np.uint8)
        idx.add(X)
        D, I = idx.search(Q, 10)
        assert (D[:, 5:] == INT32_MAX).all() and (I[:, 5:] == -1).all()
        check(idx, X, Q, 10)
        check(idx, X, Q, 2048)
    finally:
        idx.close()


def test_growth_two_adds_reconstruct_and_reset():
    from ivr_amd.binary import BinaryFlatIndex
    B = _block()
    rng = np.random.default_rng(17)
    X = rng.integers(0, 4, (5 * B + 9, 5), dtype=np.uint8)          # few distinct bytes: ties
    Q = rng.integers(0, 4, (17, 5), dtype=np.uint8)
    one, two = BinaryFlatIndex(40), BinaryFlatIndex(40)
    try:
        one.add(X)
        split = B // 2 + 3                                          # inside the first block and not on a 64-row boundary
        two.add(X[:split])
        check(two, X[:split], Q, 10)
        two.add(torch.from_numpy(X[split:]).cuda())                 # grows the capacity; a CUDA tensor this time
        assert one.ntotal == two.ntotal == len(X)
        for idx in (one, two):
            assert np.array_equal(idx.reconstruct_n(), X)
            assert np.array_equal(idx.reconstruct_n(B - 3, 70), X[B - 3:B + 67])
            check(idx, X, Q, 10)
        D1, I1 = one.search(Q, 100)
        D2, I2 = two.search(Q, 100)
        assert np.array_equal(D1, D2) and np.array_equal(I1, I2)
        two.reset()
        assert two.ntotal == 0 and (two.search(Q, 3)[1] == -1).all()
        Y = rng.integers(0, 256, (70, 5), dtype=np.uint8)
        two.add(Y)
        assert np.array_equal(two.reconstruct_n(), Y)
        check(two, Y, Q, 10)
    finally:
        one.close()
        two.close()


def test_search_twice_is_identical_and_device_form():
    rng = np.random.default_rng(18)
    X = rng.integers(0, 256, (3000, 2), dtype=np.uint8)
    Q = rng.integers(0, 256, (70, 2), dtype=np.uint8)
    idx = make(X)
    try:
        D1, I1 = idx.search(Q, 100)
        D2, I2 = idx.search(Q, 100)
        assert np.array_equal(I1, I2) and np.array_equal(D1, D2)
        Dd, Id = idx.search_device(torch.from_numpy(Q).cuda(), 100)
        assert Dd.is_cuda and Dd.dtype == torch.int32 and Id.dtype == torch.int64
        assert np.array_equal(Id.cpu().numpy(), I1) and np.array_equal(Dd.cpu().numpy(), D1)
        check(idx, X, Q, 100)
    finally:
        idx.close()


def test_pad_bits_are_ignored():
    """nbits = 13 through the C ABI: the 3 pad bits of the second byte carry garbage in the stored codes and in the queries."""
    from ivr_amd import _ffi
    lib = _ffi.load()
    rng = np.random.default_rng(19)
    X = rng.integers(0, 256, (300, 2), dtype=np.uint8)
    Q = rng.integers(0, 256, (5, 2), dtype=np.uint8)
    mask = np.array([0xff, 0x1f], np.uint8)
    h = C.c_void_p()
    _ffi.check(lib.ivr_bin_index_create(_ffi.context(torch.cuda.current_device()), 13, 0, C.byref(h)))
    try:
        x, q = torch.from_numpy(X).cuda(), torch.from_numpy(Q).cuda()
        D = torch.empty((5, 20), dtype=torch.int32, device="cuda")
        I = torch.empty((5, 20), dtype=torch.int64, device="cuda")
        out = torch.empty((300, 2), dtype=torch.uint8, device="cuda")
        s = _ffi.stream_ptr()
        _ffi.check(lib.ivr_bin_index_add(h, C.c_void_p(x.data_ptr()), 300, s))
        _ffi.check(lib.ivr_bin_index_search(h, C.c_void_p(q.data_ptr()), 5, 20, C.c_void_p(D.data_ptr()), C.c_void_p(I.data_ptr()), s))
        _ffi.check(lib.ivr_bin_index_get_codes(h, 0, 300, C.c_void_p(out.data_ptr()), s))
        torch.cuda.synchronize()
        Dr, Ir = oracle(X & mask, Q & mask, 20)
        assert np.array_equal(D.cpu().numpy(), Dr) and np.array_equal(I.cpu().numpy(), Ir)
        assert np.array_equal(out.cpu().numpy(), X & mask)
    finally:
        lib.ivr_bin_index_destroy(h)


def test_errors():
    from ivr_amd import _ffi
    from ivr_amd.binary import BinaryFlatIndex, IndexBinaryFlat
    for d in (0, 12, 63):
        with pytest.raises(ValueError):
            IndexBinaryFlat(d)
    idx = BinaryFlatIndex(64)
    try:
        X = np.zeros((4, 8), np.uint8)
        idx.add(X)
        with pytest.raises(ValueError):
            idx.add(np.zeros((4, 7), np.uint8))                 # wrong code width
        with pytest.raises(ValueError):
            idx.add(np.zeros((4, 8), np.float32))
        with pytest.raises(ValueError):
            idx.search(np.zeros((1, 9), np.uint8), 1)
        with pytest.raises(ValueError):
            idx.search(X, 0)
        with pytest.raises(ValueError):
            idx.search(X, _ffi.IVR_MAX_K + 1)
        # the library itself refuses the same k
        D = torch.empty((4, 1), dtype=torch.int32, device="cuda")
        I = torch.empty((4, 1), dtype=torch.int64, device="cuda")
        q = torch.from_numpy(X).cuda()
        lib = _ffi.load()
        for k in (0, _ffi.IVR_MAX_K + 1):
            assert lib.ivr_bin_index_search(idx._h, C.c_void_p(q.data_ptr()), 4, k, C.c_void_p(D.data_ptr()), C.c_void_p(I.data_ptr()),
                                            _ffi.stream_ptr()) == -1
        assert idx.ntotal == 4
    finally:
        idx.close()


@pytest.mark.parametrize("k", [10, 2048])
def test_more_rows_than_one_step_of_the_prefix_pass(k):
    """The prefix over the 64-row groups of a query advances 8192 groups (524,288 rows) per step and carries the running total into
    the next: 2 * 8192 * 64 + 77 rows make two full steps and a partial third.  8-bit codes keep every distance bin crowded, so the
    rank of a tie row is a sum over all three steps."""
    rng = np.random.default_rng(20)
    n = 2 * 8192 * 64 + 77
    X = rng.integers(0, 256, (n, 1), dtype=np.uint8)
    X[: n - 300] |= 0x0f                                  # the rows nearest to query 0 (distance <= 3) all sit in the last step ...
    X[5] = 0x01                                           # ... except one in the first
    Q = np.array([[0x00], [0xff], [0x5a]], np.uint8)
    idx = make(X)
    try:
        check(idx, X, Q, k)
    finally:
        idx.close()
