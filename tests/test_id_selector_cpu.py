"""CPU suite: the faiss ID selectors reduce to the filter fields of the C ABI (ivr_id_filter), and their bitmap bytes are faiss
IDSelectorBitmap order (numpy.packbits(mask, bitorder="little")).  No GPU: the device upload is not exercised here."""
import numpy as np
import pytest
import torch

from ivr_amd.index import IDSelectorBatch, IDSelectorBitmap, IDSelectorRange, SearchParameters, _selector


def _members(sel, n):
    return np.array([sel.is_member(i) for i in range(n)], bool)


def test_range_fields():
    s = IDSelectorRange(12345, 67891)
    assert (s.lo, s.hi, s._bits) == (12345, 67891, None)
    assert s.is_member(12345) and s.is_member(67890) and not s.is_member(67891) and not s.is_member(12344)
    e = IDSelectorRange(10, 5)
    assert not _members(e, 20).any()


@pytest.mark.parametrize("n", [1, 7, 8, 9, 1000, 4099])
def test_bitmap_bytes_match_packbits(n):
    rng = np.random.default_rng(n)
    mask = rng.random(n) < 0.4
    packed = np.packbits(mask, bitorder="little")
    for src in (packed, torch.from_numpy(packed.copy())):
        s = IDSelectorBitmap(src)
        assert np.array_equal(s._bits, packed)
        assert (s.lo, s.hi, s.nbits, s._byte0) == (0, 8 * len(packed), 8 * len(packed), 0)
        assert np.array_equal(_members(s, n), mask)
    assert not s.is_member(8 * len(packed)) and not s.is_member(-1)
    s2 = IDSelectorBitmap(len(packed) - 1 if len(packed) > 1 else 0, packed)
    assert s2.nbits == 8 * max(len(packed) - 1, 0)


def test_batch_is_a_bitmap_over_its_range():
    ids = np.array([1000, 1003, 1003, 1017, 1064, -4], np.int64)
    s = IDSelectorBatch(ids)
    assert (s.lo, s.hi, s.nbits) == (1000, 1065, 1065)
    assert s._byte0 == 1000 >> 3
    mask = np.zeros(1065, bool)
    mask[[1000, 1003, 1017, 1064]] = True
    full = np.packbits(mask, bitorder="little")
    # the stored bytes are the faiss bitmap's from byte min(ids) >> 3 on
    assert np.array_equal(s._bits, full[s._byte0:])
    assert np.array_equal(_members(s, 1100), np.pad(mask, (0, 35)))
    empty = IDSelectorBatch([])
    assert empty.lo >= empty.hi


def test_bad_arguments_raise_value_error():
    with pytest.raises(ValueError):
        IDSelectorBitmap(np.zeros(4, np.int64))
    with pytest.raises(ValueError):
        IDSelectorBitmap(torch.zeros(4, dtype=torch.int32))
    with pytest.raises(ValueError):
        IDSelectorBitmap(9, np.zeros(4, np.uint8))
    with pytest.raises(ValueError):
        IDSelectorBatch(np.array([0.5]))
    with pytest.raises(ValueError):
        SearchParameters(sel=[1, 2])
    with pytest.raises(ValueError):
        _selector(params={"sel": None})
    with pytest.raises(ValueError):
        _selector(params=SearchParameters(), sel=IDSelectorRange(0, 1))
    assert _selector(params=SearchParameters()) is None
    r = IDSelectorRange(0, 1)
    assert _selector(params=SearchParameters(sel=r)) is r


def test_bitmap_intersected_with_a_range():
    mask = np.zeros(100, bool)
    mask[[3, 10, 50, 90]] = True
    s = IDSelectorBitmap(np.packbits(mask, bitorder="little"), lo=5, hi=60)
    assert (s.lo, s.hi, s.nbits) == (5, 60, 104)
    assert np.flatnonzero(_members(s, 104)).tolist() == [10, 50]
    clipped = IDSelectorBitmap(np.packbits(mask, bitorder="little"), lo=-7, hi=10 ** 6)
    assert (clipped.lo, clipped.hi) == (0, 104)
