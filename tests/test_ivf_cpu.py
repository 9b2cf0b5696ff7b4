"""CPU suite of the inverted-file index: the two new entry points of the C ABI (ivr_index_search_lists, ivr_segment_mean) exist at
API version 11 and reject NULL arguments with IVR_ERR_INVALID before any HIP call (the pattern of
test_abi.py::test_error_slot_without_gpu), and the pure-numpy helpers of ivr_amd/ivf.py do what their docstrings define: list
offsets, the sample permutation of the k-means, the repair of empty clusters."""
import ctypes

import numpy as np
import pytest

from ivr_amd import _ffi

IVR_ERR_INVALID = -1
NEW = ("ivr_index_search_lists", "ivr_segment_mean")


def test_entry_points_are_bound_and_exported():
    lib = ctypes.CDLL(_ffi.LIB_PATH)
    for name in NEW:
        assert name in _ffi.EXPORTS, name
        assert hasattr(lib, name), name


def test_api_version_is_still_11():
    assert _ffi.API_VERSION == 11
    assert _ffi.load().ivr_api_version() == 11


def test_entry_points_reject_null_arguments():
    lib = _ffi.load()
    for name, args in (("ivr_index_search_lists", (None, None, 4, None, 1, None, 1, 0, 1, 0, None, None, None)),
                       ("ivr_segment_mean", (None, None, 0, None, 1, 4, 0, None, None))):
        assert getattr(lib, name)(*args) == IVR_ERR_INVALID, name
        assert b"NULL" in lib.ivr_last_error(None), name
        assert name.encode() in lib.ivr_last_error(None), name


def test_package_exports_the_class():
    import ivr_amd
    from ivr_amd import ivf
    assert ivr_amd.IVFFlatIndex is ivf.IVFFlatIndex
    assert ivr_amd.IndexIVFFlat is ivf.IndexIVFFlat
    assert ivr_amd.SearchParametersIVF is ivf.SearchParametersIVF
    assert ivr_amd.METRIC_INNER_PRODUCT == 0


def test_list_offsets():
    from ivr_amd.ivf import list_offsets
    off = list_offsets(np.array([2, 0, 2, 2, 5, 0]), 7)
    assert off.dtype == np.int64
    assert off.tolist() == [0, 2, 2, 5, 5, 5, 6, 6]
    assert list_offsets(np.zeros(0, np.int64), 3).tolist() == [0, 0, 0, 0]
    for bad in ([3], [-1]):
        with pytest.raises(ValueError):
            list_offsets(np.array(bad), 3)


def test_kmeans_sample_is_the_seeded_permutation():
    from ivr_amd.ivf import kmeans_sample
    perm = np.random.RandomState(1234).permutation(1000)
    s = kmeans_sample(1000, 4, max_points_per_centroid=50, seed=1234)
    assert s.dtype == np.int64 and len(s) == 200
    assert np.array_equal(s, perm[:200])
    # fewer rows than the cap: all of them, still permuted (the first nlist are the initial centroids)
    assert np.array_equal(kmeans_sample(1000, 4, 256, 1234), perm)
    assert np.array_equal(kmeans_sample(1000, 4, 50, 1234), kmeans_sample(1000, 4, 50, 1234))
    assert not np.array_equal(kmeans_sample(1000, 4, 50, 1234), kmeans_sample(1000, 4, 50, 99))


def test_split_empty_clusters_hand_case():
    from ivr_amd.ivf import split_empty_clusters
    e = np.float32(1.0 / 1024.0)
    c = np.array([[1, 2, 3, 4], [9, 9, 9, 9], [10, 20, 30, 40], [7, 7, 7, 7], [5, 6, 7, 8]], np.float32)
    counts = np.array([4, 0, 9, 0, 5], np.int64)
    touched = split_empty_clusters(c, counts)
    # cluster 1 splits cluster 2 (9 rows -> 5 + 4); then the largest are clusters 2 and 4 with 5 rows each: the lower one, 2, splits again
    assert touched == [1, 2, 3]
    assert counts.tolist() == [4, 4, 3, 2, 5]
    base = np.array([10, 20, 30, 40], np.float32)
    plus, minus = np.array([1 + e, 1 - e, 1 + e, 1 - e], np.float32), np.array([1 - e, 1 + e, 1 - e, 1 + e], np.float32)
    assert np.array_equal(c[1], base * plus)
    mid = base * minus                      # cluster 2 after the first split
    assert np.array_equal(c[3], mid * plus)
    assert np.array_equal(c[2], mid * minus)
    assert np.array_equal(c[0], np.array([1, 2, 3, 4], np.float32)) and np.array_equal(c[4], np.array([5, 6, 7, 8], np.float32))
    assert counts.sum() == 18
    # nothing empty: nothing changes
    c2, n2 = c.copy(), counts.copy()
    assert split_empty_clusters(c2, n2) == [] and np.array_equal(c2, c) and np.array_equal(n2, counts)
