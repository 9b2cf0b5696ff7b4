"""CPU suite of the binary / LSH indexes (ivr_amd/binary.py, csrc/search_binary.hip): the ABI of the new entry points and the
numpy definition of the default rotation.  No compute call reaches a device."""
import ctypes
import re

import numpy as np
import pytest

from conftest import ROOT
from ivr_amd import _ffi

NEW = ["ivr_bin_index_create", "ivr_bin_index_destroy", "ivr_bin_index_reset", "ivr_bin_index_ntotal", "ivr_bin_index_block_rows",
       "ivr_bin_index_add", "ivr_bin_index_get_codes", "ivr_bin_index_search", "ivr_sign_encode"]


def _header():
    src = open(f"{ROOT}/include/ivr_api.h").read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def test_header_binding_and_library_agree_on_the_new_symbols():
    declared = set(re.findall(r"\b(ivr_[a-z0-9_]+)\s*\(", _header()))
    lib = ctypes.CDLL(_ffi.LIB_PATH)
    for name in NEW:
        assert name in declared, f"{name} not declared in ivr_api.h"
        assert name in _ffi.EXPORTS, f"{name} not bound in _ffi"
        assert hasattr(lib, name), f"{name} not exported by the library"
    assert re.search(r"#define\s+IVR_BIN_MAX_BITS\s+2048\b", _header())


def test_api_version_is_still_11():
    assert _ffi.API_VERSION == 11
    assert _ffi.load().ivr_api_version() == 11
    assert re.search(r"#define\s+IVR_API_VERSION\s+11\b", _header())


def test_null_handles_are_rejected():
    lib = _ffi.load()
    out = ctypes.c_void_p()
    assert lib.ivr_bin_index_create(None, 256, 0, ctypes.byref(out)) == -1
    assert b"NULL" in lib.ivr_last_error(None)
    assert lib.ivr_bin_index_reset(None) == -1
    assert b"NULL" in lib.ivr_last_error(None)
    assert lib.ivr_bin_index_add(None, None, 1, None) == -1
    assert lib.ivr_bin_index_get_codes(None, 0, 1, None, None) == -1
    assert lib.ivr_bin_index_search(None, None, 1, 1, None, None, None) == -1
    assert lib.ivr_sign_encode(None, None, 1, 64, None, None, 64, None, None, None) == -1
    assert lib.ivr_bin_index_ntotal(None) == 0
    assert lib.ivr_bin_index_destroy(None) == 0


def test_block_rows_is_a_positive_multiple_of_64():
    b = _ffi.load().ivr_bin_index_block_rows()
    assert b > 0 and b % 64 == 0


@pytest.mark.parametrize("d,nbits", [(100, 100), (512, 256), (64, 256)])
def test_lsh_rotation(d, nbits):
    from ivr_amd import lsh_rotation
    r = lsh_rotation(d, nbits)
    assert r.shape == (nbits, d) and r.dtype == np.float32 and r.flags["C_CONTIGUOUS"]
    assert np.array_equal(r, lsh_rotation(d, nbits, seed=5))            # two calls, and seed 5 is the default
    assert not np.array_equal(r, lsh_rotation(d, nbits, seed=6))
    r64 = r.astype(np.float64)
    if nbits <= d:
        assert np.abs(r64 @ r64.T - np.eye(nbits)).max() < 1e-5         # orthonormal rows
    else:
        assert np.abs(r64.T @ r64 - np.eye(d)).max() < 1e-5             # orthonormal columns


def test_lsh_rotation_is_the_written_definition():
    from ivr_amd.binary import lsh_rotation
    d, nbits = 24, 40
    a = np.random.RandomState(5).standard_normal((40, 40))
    q, r = np.linalg.qr(a)
    q = q * np.sign(np.diag(r))
    assert np.array_equal(lsh_rotation(d, nbits), q[:nbits, :d].astype(np.float32))
