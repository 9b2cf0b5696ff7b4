"""CPU suite: the IndexIDMap2 container of ivr_amd.faiss_io (round trip only: the layout is unpinned, see the module docstring)."""
import numpy as np
import pytest

from ivr_amd import faiss_io


def _sample(n=37, d=12):
    rng = np.random.default_rng(5)
    ids = rng.permutation(10 * n)[:n].astype(np.int64)
    ids[::5] += 3 * 10**12                          # above 2^32
    return rng.standard_normal((n, d)).astype(np.float32), ids


@pytest.mark.parametrize("metric", ["ip", "l2"])
def test_round_trip(tmp_path, metric):
    X, ids = _sample()
    path = str(tmp_path / "index.faiss")
    faiss_io.write_idmap_index(path, X, ids, metric=metric)
    V, I, m = faiss_io.read_idmap_index(path)
    assert m == metric and V.dtype == np.float32 and I.dtype == np.int64
    assert np.array_equal(V.view(np.uint32), X.view(np.uint32)) and np.array_equal(I, ids)
    assert I.max() > 2**32
    raw = open(path, "rb").read()
    assert raw[:4] == b"IxM2" and len(raw) == 37 + 45 + X.nbytes + 8 + ids.nbytes
    # the nested index is the flat container byte for byte
    flat = str(tmp_path / "flat.faiss")
    faiss_io.write_flat_index(flat, X, metric=metric)
    assert raw[37:37 + 45 + X.nbytes] == open(flat, "rb").read()


def test_reads_the_plain_idmap_fourcc_and_an_empty_index(tmp_path):
    X, ids = _sample()
    path = str(tmp_path / "index.faiss")
    faiss_io.write_idmap_index(path, X, ids)
    raw = bytearray(open(path, "rb").read())
    raw[:4] = b"IxMp"
    open(path, "wb").write(bytes(raw))
    V, I, m = faiss_io.read_idmap_index(path)
    assert np.array_equal(V, X) and np.array_equal(I, ids)
    faiss_io.write_idmap_index(path, np.zeros((0, 8), np.float32), np.zeros(0, np.int64))
    V, I, m = faiss_io.read_idmap_index(path)
    assert V.shape == (0, 8) and I.shape == (0,)


def test_flat_reader_refuses_and_names_the_other_reader(tmp_path):
    X, ids = _sample()
    path = str(tmp_path / "index.faiss")
    faiss_io.write_idmap_index(path, X, ids)
    with pytest.raises(ValueError, match="read_idmap_index"):
        faiss_io.read_flat_index(path)
    faiss_io.write_flat_index(path, X)
    with pytest.raises(ValueError, match="not an IndexIDMap"):
        faiss_io.read_idmap_index(path)


def test_truncated_files(tmp_path):
    X, ids = _sample()
    path = str(tmp_path / "index.faiss")
    faiss_io.write_idmap_index(path, X, ids)
    raw = open(path, "rb").read()
    for cut in (len(raw) - 1, len(raw) - 8 * 5, len(raw) - ids.nbytes, len(raw) - ids.nbytes - 3, 37 + 45 + 100, 20):
        open(path, "wb").write(raw[:cut])
        with pytest.raises(ValueError, match="truncated"):
            faiss_io.read_idmap_index(path)


def test_writer_checks_its_arguments(tmp_path):
    X, ids = _sample()
    path = str(tmp_path / "index.faiss")
    with pytest.raises(ValueError):
        faiss_io.write_idmap_index(path, X, ids[:-1])
    with pytest.raises(ValueError):
        faiss_io.write_idmap_index(path, X, ids.astype(np.float64))
