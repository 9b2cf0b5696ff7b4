"""GPU suite of IndexLSH (ivr_amd/binary.py) and its encoder ivr_sign_encode (csrc/search_binary.hip).

 - packing: the codes are, bit for bit, packbits(proj - thr >= 0, bitorder="little") of the float32 projections the SAME launch
   wrote, pad bits zero;
 - arithmetic: with small integer inputs every partial sum is exact in float32 in any order, so proj must equal the int64 product and
   an exactly zero projection must set its bit;
 - against float64: a bit may differ from x64 @ rrot64.T >= 0 only where |proj64| <= 2 d 2^-24 sum|x_i||r_ji| (twice the float32
   dot-product rounding bound); that at most 1 % of all bits lie inside the margin is a condition on the inputs, checked first;
 - search is BinaryFlatIndex.search on sa_encode of the same data; threshold training follows faiss's median rule."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(64, 256), (100, 100), (512, 256), (768, 320)]
N = 300


def unit_rows(seed, n, d):
    x = np.random.default_rng(seed).standard_normal((n, d))
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


def pack(bits):
    return np.packbits(bits.astype(np.uint8), axis=1, bitorder="little")


def encode_with_proj(lsh, x):
    codes, proj = lsh.sa_encode_device(x, want_proj=True)
    return codes.cpu().numpy(), proj.cpu().numpy()


@pytest.mark.parametrize("d,nbits", SHAPES)
@pytest.mark.parametrize("trained", [False, True])
def test_packing_is_exact(d, nbits, trained):
    from ivr_amd.binary import IndexLSH
    x = unit_rows(100 + d, N, d)
    lsh = IndexLSH(d, nbits, train_thresholds=trained)
    try:
        if trained:
            lsh.train(unit_rows(200 + d, 501, d))
            assert lsh.is_trained and lsh.thresholds.shape == (nbits,) and lsh.thresholds.dtype == np.float32
            assert np.abs(lsh.thresholds).max() > 0
        thr = lsh.thresholds if trained else np.zeros(nbits, np.float32)
        codes, proj = encode_with_proj(lsh, x)
        assert codes.dtype == np.uint8 and codes.shape == (N, (nbits + 7) // 8) and proj.dtype == np.float32
        want = pack(proj - thr[None, :] >= np.float32(0))
        assert np.array_equal(codes, want)
        if nbits % 8:                                                        # pad bits of the last byte are zero
            assert (codes[:, -1] >> (nbits % 8) == 0).all()
        assert np.array_equal(lsh.sa_encode(x), codes)                       # without proj: the same bits
        assert np.array_equal(lsh.sa_encode(torch.from_numpy(x).cuda()), codes)
    finally:
        lsh.close()


@pytest.mark.parametrize("d,nbits", SHAPES + [(37, 70)])
def test_integer_inputs_are_exact(d, nbits):
    """x in [-3, 3], rrot in [-2, 2] with all-zero rows: |partial sums| <= 6 d < 2^24, exact in float32 in any order."""
    from ivr_amd.binary import IndexLSH
    rng = np.random.default_rng(300 + d)
    x = rng.integers(-3, 4, (N, d)).astype(np.float32)
    rot = rng.integers(-2, 3, (nbits, d)).astype(np.float32)
    zero_rows = [0, 5, 17, nbits // 2, nbits - 1]
    rot[zero_rows] = 0
    x[3] = 0                                                                 # a whole row of exactly zero projections
    lsh = IndexLSH(d, nbits)
    try:
        lsh.rrot = rot
        codes, proj = encode_with_proj(lsh, x)
        exact = x.astype(np.int64) @ rot.astype(np.int64).T
        assert np.array_equal(proj.astype(np.int64), exact) and np.array_equal(proj, exact.astype(np.float32))
        assert (exact == 0).sum() >= len(zero_rows) * N
        bits = np.unpackbits(codes, axis=1, bitorder="little")[:, :nbits]
        assert np.array_equal(bits, (exact >= 0).astype(np.uint8))
        assert (bits[:, zero_rows] == 1).all() and (bits[3] == 1).all()      # an exactly zero projection sets its bit
    finally:
        lsh.close()


@pytest.mark.parametrize("d,nbits", [(64, 40), (100, 100), (512, 256), (77, 13)])
def test_without_rotation_takes_the_first_coordinates(d, nbits):
    from ivr_amd.binary import IndexLSH
    rng = np.random.default_rng(400 + d)
    x = rng.integers(-3, 4, (N, d)).astype(np.float32)
    lsh = IndexLSH(d, nbits, rotate_data=False)
    try:
        codes, proj = encode_with_proj(lsh, x)
        assert np.array_equal(proj, x[:, :nbits])
        assert np.array_equal(codes, pack(x[:, :nbits] >= 0))
    finally:
        lsh.close()
    with pytest.raises(ValueError):
        IndexLSH(64, 65, rotate_data=False)


@pytest.mark.parametrize("d,nbits", SHAPES)
def test_bits_against_float64(d, nbits):
    from ivr_amd.binary import IndexLSH
    x = unit_rows(500 + d, 1000, d)
    lsh = IndexLSH(d, nbits)
    try:
        r64, x64 = lsh.rrot.astype(np.float64), x.astype(np.float64)
        p64 = x64 @ r64.T
        margin = 2.0 * d * 2.0 ** -24 * (np.abs(x64) @ np.abs(r64).T)
        near = np.abs(p64) <= margin
        assert near.mean() <= 0.01, f"{near.mean():.4%} of the bits inside the rounding margin: the inputs do not test anything"
        bits = np.unpackbits(lsh.sa_encode(x), axis=1, bitorder="little")[:, :nbits]
        wrong = bits != (p64 >= 0)
        print(f"d={d} nbits={nbits}: {near.mean():.4%} of the bits inside the margin, {wrong.sum()} differ, {(wrong & ~near).sum()} outside it")
        assert not (wrong & ~near).any()
    finally:
        lsh.close()


@pytest.mark.parametrize("d,nbits", SHAPES)
def test_search_is_the_binary_search_of_the_codes(d, nbits):
    from ivr_amd.binary import BinaryFlatIndex, IndexLSH
    x = unit_rows(600 + d, 700, d)
    q = np.concatenate([x[[5, 333, 699]], unit_rows(601 + d, 14, d)])
    lsh = IndexLSH(d, nbits)
    flat = BinaryFlatIndex(8 * lsh.code_size)
    try:
        assert (lsh.d, lsh.nbits, lsh.code_size, lsh.rotate_data, lsh.train_thresholds) == (d, nbits, (nbits + 7) // 8, True, False)
        assert lsh.is_trained and lsh.ntotal == 0 and lsh.metric_type == 1
        lsh.add(x[:300])
        lsh.add(torch.from_numpy(x[300:]).cuda())
        assert lsh.ntotal == 700
        codes = lsh.sa_encode(x)
        assert np.array_equal(lsh.codes, codes)
        flat.add(codes)
        for k in (1, 10, 800):
            D, I = lsh.search(q, k)
            Db, Ib = flat.search(lsh.sa_encode(q), k)
            assert D.dtype == np.float32 and I.dtype == np.int64
            assert np.array_equal(I, Ib) and np.array_equal(D, Db.astype(np.float32))
        D, I = lsh.search(q, 800)
        assert (D[:, 700:] == np.float32(2147483648.0)).all() and (I[:, 700:] == -1).all()
        assert (np.diff(D, axis=1) >= 0).all()
        # a stored row finds itself at distance 0 (and is the lowest row at that distance unless a twin precedes it)
        D, I = lsh.search(x[[5, 333, 699]], 1)
        assert (D[:, 0] == 0).all()
        assert all((codes[i] == codes[r]).all() and i <= r for i, r in zip(I[:, 0], (5, 333, 699)))
        Dd, Id = lsh.search_device(torch.from_numpy(q).cuda(), 10)
        assert Dd.is_cuda and Dd.dtype == torch.float32 and np.array_equal(Id.cpu().numpy(), lsh.search(q, 10)[1])
        lsh.reset()
        assert lsh.ntotal == 0 and (lsh.search(q, 2)[1] == -1).all()
    finally:
        lsh.close()
        flat.close()


@pytest.mark.parametrize("d,nbits", [(64, 256), (100, 100)])
def test_trained_thresholds_split_every_bit_in_half(d, nbits):
    from ivr_amd.binary import IndexLSH
    n = 501
    x = unit_rows(700 + d, n, d)
    lsh = IndexLSH(d, nbits, train_thresholds=True)
    try:
        assert not lsh.is_trained
        with pytest.raises(RuntimeError):
            lsh.add(x)
        lsh.train(x)
        assert lsh.is_trained
        _, proj = encode_with_proj(lsh, x)
        assert np.array_equal(lsh.thresholds, np.sort(proj, axis=0)[n // 2])           # faiss's median rule, on the kernel's own proj
        ones = np.unpackbits(lsh.sa_encode(x), axis=1, bitorder="little")[:, :nbits].sum(0)
        assert (ones == (n + 1) // 2).all()
        lsh.add(x)
        assert lsh.ntotal == n
    finally:
        lsh.close()


def test_state_errors():
    from ivr_amd.binary import IndexLSH
    lsh = IndexLSH(64, 32)
    try:
        x = unit_rows(800, 10, 64)
        rot = lsh.rrot.copy()
        with pytest.raises(ValueError):
            lsh.rrot = rot[:, :10]
        lsh.rrot = rot[::-1]                                # allowed while empty
        assert np.array_equal(lsh.rrot, rot[::-1])
        lsh.add(x)
        with pytest.raises(RuntimeError):
            lsh.rrot = rot
        with pytest.raises(ValueError):
            lsh.add(np.zeros((3, 65), np.float32))
        with pytest.raises(ValueError):
            lsh.search(x, 0)
        with pytest.raises(ValueError):
            lsh.search(np.zeros((1, 63), np.float32), 1)
        lsh.reset()
        lsh.rrot = rot                                      # and again after reset
    finally:
        lsh.close()
    with pytest.raises(ValueError):
        IndexLSH(64, 0)
    with pytest.raises(ValueError):
        IndexLSH(64, 2049)


def test_own_cluster_is_nearer_in_hamming_distance():
    """Sanity, not a gate on quality: clustered unit vectors (a dominant axis plus noise, the construction of the inverted-file
    suite); the mean Hamming distance to rows of the query's own cluster is below the mean distance to rows of other clusters."""
    from ivr_amd.binary import IndexLSH
    d, nbits, nclu, n = 512, 256, 13, 1300
    rng = np.random.default_rng(900)
    clu = rng.integers(0, nclu, n)
    x = np.eye(nclu, d)[clu] + 0.3 * rng.standard_normal((n, d)) / np.sqrt(d)
    x = (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)
    lsh = IndexLSH(d, nbits)
    try:
        lsh.add(x)
        D, I = lsh.search(x[:50], n)
        own = clu[I] == clu[:50, None]
        assert D[own].mean() < D[~own].mean()
    finally:
        lsh.close()


@pytest.mark.parametrize("n", [4096, 4097])
def test_row_counts_on_both_sides_of_the_encoder_switch(n):
    """ivr_sign_encode runs up to 4096 rows through the instantiation that keeps four chunks of loads in flight and more rows through
    the one-chunk instantiation; the summation order is the same, so the bits of a row must not depend on how many rows travel with
    it.  Exact integers pin proj itself, real-valued rows the equality of the two paths."""
    from ivr_amd.binary import IndexLSH
    d, nbits = 100, 70
    rng = np.random.default_rng(1000 + n)
    lsh = IndexLSH(d, nbits)
    try:
        x = unit_rows(1100 + n, n, d)
        codes, proj = encode_with_proj(lsh, x)
        few_codes, few_proj = encode_with_proj(lsh, x[-300:])              # 300 rows: always the small-batch instantiation
        assert np.array_equal(codes[-300:], few_codes) and np.array_equal(proj[-300:], few_proj)
        assert np.array_equal(codes, pack(proj >= np.float32(0)))
        xi = rng.integers(-3, 4, (n, d)).astype(np.float32)
        rot = rng.integers(-2, 3, (nbits, d)).astype(np.float32)
        lsh.rrot = rot
        codes, proj = encode_with_proj(lsh, xi)
        exact = xi.astype(np.int64) @ rot.astype(np.int64).T
        assert np.array_equal(proj, exact.astype(np.float32))
        assert np.array_equal(codes, pack(exact >= 0))
    finally:
        lsh.close()
