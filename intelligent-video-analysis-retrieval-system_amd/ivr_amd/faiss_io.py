"""Legacy `index.faiss` files: read/write of the flat-index container that
`faiss.write_index` / `faiss.read_index` produce at `core.py:987` / `core.py:1057`, so an index saved by the
reference loads into the HBM-resident index and vice versa.

`faiss` is an un-vendored, un-pinned dependency that is absent from this image; the layout below restates its
published serialisation of `IndexFlat` (impl/index_write.cpp) from the format's documentation and is therefore
UNPINNED here (only the round trip through this module is tested):

    uint32  fourcc            "IxFI" (inner product) or "IxF2" (L2), little endian
    int32   d
    int64   ntotal
    int64   dummy, dummy      (1 << 20 each)
    uint8   is_trained
    int32   metric_type       0 = METRIC_INNER_PRODUCT, 1 = METRIC_L2
    uint64  count             number of float32 values = ntotal * d
    float32 xb[count]         rows, row-major

`write_idmap_index` / `read_idmap_index` do the same for the `IndexIDMap2` container that wraps a flat index with
caller-chosen ids (what `FlatIPIndex.add_with_ids` holds).  It too restates impl/index_write.cpp and is UNPINNED (round
trip only):

    uint32  fourcc            "IxM2" (IndexIDMap2; "IxMp" = IndexIDMap is read as well)
    int32   d
    int64   ntotal
    int64   dummy, dummy
    uint8   is_trained
    int32   metric_type
    ...                       the nested flat index, exactly as above (its own fourcc and header included)
    uint64  count             number of ids = ntotal
    int64   id_map[count]
"""
import struct

import numpy as np

FOURCC_IP = struct.unpack("<I", b"IxFI")[0]
FOURCC_L2 = struct.unpack("<I", b"IxF2")[0]
_HEADER = struct.Struct("<IiqqqBiQ")      # packed, no padding: 4+4+8+8+8+1+4+8 = 45 bytes
FOURCC_IDMAP2 = struct.unpack("<I", b"IxM2")[0]
FOURCC_IDMAP = struct.unpack("<I", b"IxMp")[0]
_INDEX_HEADER = struct.Struct("<IiqqqBi")  # the index header alone (no vector count behind it): 37 bytes


def write_flat_index(path, vectors, metric="ip"):
    v = np.ascontiguousarray(vectors, dtype=np.float32)
    if v.ndim != 2:
        raise ValueError("vectors must be [n,d]")
    with open(path, "wb") as f:
        _write_flat(f, v, metric)


def _write_flat(f, v, metric):
    n, d = v.shape
    f.write(_HEADER.pack(FOURCC_IP if metric == "ip" else FOURCC_L2, d, n, 1 << 20, 1 << 20, 1, 0 if metric == "ip" else 1, n * d))
    f.write(v.tobytes())


def read_flat_index(path):
    """-> (vectors float32 [n,d], metric "ip" | "l2").  Raises ValueError for anything but a flat index."""
    return _read_flat_at(path, 0)


def _read_flat_at(path, offset):
    """The flat index that starts `offset` bytes into the file."""
    with open(path, "rb") as f:
        f.seek(offset)
        head = f.read(_HEADER.size)
        if len(head) < _HEADER.size:
            raise ValueError(f"{path}: truncated header")
        fourcc, d, n, _, _, trained, metric, count = _HEADER.unpack(head)
        if fourcc not in (FOURCC_IP, FOURCC_L2):
            if fourcc in (FOURCC_IDMAP2, FOURCC_IDMAP):
                raise ValueError(f"{path}: an IndexIDMap file (fourcc {fourcc:#x}), not a flat index: read it with read_idmap_index")
            raise ValueError(f"{path}: not a flat FAISS index (fourcc {fourcc:#x}); only IndexFlatIP / IndexFlatL2 files "
                             "are supported (the reference coerces every configured type to IndexFlatIP, core.py:1205-1219)")
        if d <= 0 or n < 0 or count != n * d:
            raise ValueError(f"{path}: inconsistent header d={d} ntotal={n} count={count}")
        data = np.fromfile(f, dtype=np.float32, count=count)
        if data.size != count:
            raise ValueError(f"{path}: truncated payload ({data.size} of {count} floats)")
    return data.reshape(n, d), ("ip" if metric == 0 else "l2")


def write_idmap_index(path, vectors, ids, metric="ip"):
    """An IndexIDMap2 file around the flat index of `vectors` [n,d], with `ids` int64 [n] as its id_map."""
    v = np.ascontiguousarray(vectors, dtype=np.float32)
    if v.ndim != 2:
        raise ValueError("vectors must be [n,d]")
    i = np.asarray(ids)
    if not np.issubdtype(i.dtype, np.integer) or i.reshape(-1).shape[0] != v.shape[0]:
        raise ValueError(f"ids must be {v.shape[0]} integers")
    i = np.ascontiguousarray(i.reshape(-1), dtype=np.int64)
    n, d = v.shape
    with open(path, "wb") as f:
        f.write(_INDEX_HEADER.pack(FOURCC_IDMAP2, d, n, 1 << 20, 1 << 20, 1, 0 if metric == "ip" else 1))
        _write_flat(f, v, metric)
        f.write(struct.pack("<Q", n))
        f.write(i.tobytes())


def read_idmap_index(path):
    """-> (vectors float32 [n,d], ids int64 [n], metric "ip" | "l2") of an IndexIDMap2 / IndexIDMap file around a flat index.
    Raises ValueError for anything else and for a truncated file."""
    with open(path, "rb") as f:
        head = f.read(_INDEX_HEADER.size)
        if len(head) < _INDEX_HEADER.size:
            raise ValueError(f"{path}: truncated header")
        fourcc, d, n, _, _, _, _ = _INDEX_HEADER.unpack(head)
        if fourcc not in (FOURCC_IDMAP2, FOURCC_IDMAP):
            raise ValueError(f"{path}: not an IndexIDMap file (fourcc {fourcc:#x})")
        offset = f.tell()
    # the nested flat index through its own reader, which checks it; it stops behind the vectors
    vectors, metric = _read_flat_at(path, offset)
    if vectors.shape != (n, d):
        raise ValueError(f"{path}: the nested index is {vectors.shape}, the id map's header says [{n},{d}]")
    with open(path, "rb") as f:
        f.seek(offset + _HEADER.size + vectors.size * 4)
        raw = f.read(8)
        if len(raw) < 8:
            raise ValueError(f"{path}: truncated id vector (no count)")
        count = struct.unpack("<Q", raw)[0]
        if count != n:
            raise ValueError(f"{path}: {count} ids for {n} rows")
        ids = np.fromfile(f, dtype=np.int64, count=count)
        if ids.size != count:
            raise ValueError(f"{path}: truncated id vector ({ids.size} of {count} ids)")
    return vectors, ids, metric
