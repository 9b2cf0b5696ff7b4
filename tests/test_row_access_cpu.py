"""CPU suite: the row-access entry points of the C ABI (ivr_index_gather, ivr_index_scatter, ivr_index_search_reconstruct) exist at
API version 11 and reject a NULL handle with IVR_ERR_INVALID before any HIP call, as test_abi.py::test_error_slot_without_gpu checks
for ivr_index_reset."""
from ivr_amd import _ffi

IVR_ERR_INVALID = -1


def test_api_version_is_11():
    assert _ffi.API_VERSION == 11
    assert _ffi.load().ivr_api_version() == 11


def test_row_access_entry_points_reject_null_handles():
    lib = _ffi.load()
    for name, args in (("ivr_index_gather", (None, None, 4, None, None)),
                       ("ivr_index_scatter", (None, None, None, 4, 0, None)),
                       ("ivr_index_search_reconstruct", (None, None, 1, 1, 0, 0, None, None, None, None, None))):
        assert getattr(lib, name)(*args) == IVR_ERR_INVALID, name
        assert b"NULL" in lib.ivr_last_error(None), name
        assert name.encode() in lib.ivr_last_error(None), name
