"""The layer IndexLSH, PQIndex, SQIndex and PQFastScanIndex share (ivr_amd/_coded.py, and _pqbase.py for the two product quantisers):
folding the classes onto it gave none of them a public name and took none away, and the staging chunk has one definition."""
import os
import re

import pytest

from ivr_amd import _coded
from ivr_amd.binary import IndexLSH
from ivr_amd.pq import PQIndex
from ivr_amd.pqfs import PQFastScanIndex
from ivr_amd.sq import SQIndex

# recorded from the classes as they were before the fold
SURFACE = {
    IndexLSH: ["add", "close", "codes", "ntotal", "reset", "rrot", "sa_encode", "sa_encode_device", "search", "search_device",
               "thresholds", "train"],
    PQIndex: ["add", "centroids", "close", "codes", "compute_tables", "compute_tables_device", "ntotal", "reconstruct", "reconstruct_n",
              "reset", "sa_decode", "sa_decode_device", "sa_encode", "sa_encode_device", "search", "search_device", "search_tables",
              "search_tables_device", "train"],
    SQIndex: ["add", "add_codes", "close", "codes", "compute_query_codes", "compute_query_codes_device", "ntotal", "reconstruct",
              "reconstruct_n", "reset", "sa_decode", "sa_decode_device", "sa_encode", "sa_encode_device", "search", "search_codes",
              "search_codes_device", "search_device", "train", "trained"],
    PQFastScanIndex: ["add", "add_codes", "centroids", "close", "codes", "compute_tables", "compute_tables_device", "ntotal",
                      "quantize_tables_device", "reconstruct", "reconstruct_n", "reset", "sa_decode", "sa_decode_device", "sa_encode",
                      "sa_encode_device", "search", "search_device", "search_tables", "search_tables_device", "train"],
}


@pytest.mark.parametrize("cls", list(SURFACE), ids=lambda c: c.__name__)
def test_public_surface_is_unchanged(cls):
    assert [n for n in sorted(dir(cls)) if not n.startswith("_")] == SURFACE[cls]
    assert issubclass(cls, _coded.CodedIndex)
    assert issubclass(cls, _coded.DecodableIndex) == (cls is not IndexLSH)       # IndexLSH's codes decode to nothing


def test_encode_chunk_has_one_definition():
    assert _coded.ENCODE_CHUNK == 1 << 18
    pkg = os.path.dirname(_coded.__file__)
    for name in ("binary.py", "pq.py", "pqfs.py", "sq.py", "_pqbase.py"):
        with open(os.path.join(pkg, name)) as f:
            text = f.read()
        assert not re.search(r"1\s*<<\s*18|ENCODE_CHUNK\s*=|262144", text), name
