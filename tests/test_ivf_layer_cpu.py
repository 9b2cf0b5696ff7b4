"""The layer IVFFlatIndex and IVFPQIndex share (ivr_amd/_ivf.py) and the k-means under it (ivr_amd/_kmeans.py): folding the two classes
onto the layer gave neither a public name and took none away, ivr_amd.ivf still exports what it always did, and the k-means has one
home that pq.py reaches without going through a sibling index module."""
import os
import re

import pytest

from ivr_amd import _ivf, _kmeans, ivf
from ivr_amd.ivf import IVFFlatIndex
from ivr_amd.ivfpq import IVFPQIndex

# recorded from the classes as they were before the fold
SURFACE = {
    IVFFlatIndex: ["add", "add_with_ids", "assign", "centroids", "close", "list_ids", "list_sizes", "nprobe", "ntotal", "reconstruct",
                   "reconstruct_batch", "remove_ids", "reset", "search", "search_device", "search_preassigned",
                   "search_preassigned_device", "train"],
    IVFPQIndex: ["add", "add_with_ids", "assign", "by_residual", "centroids", "close", "compute_tables_device", "is_trained",
                 "list_codes", "list_ids", "list_sizes", "nprobe", "ntotal", "reconstruct", "reconstruct_batch", "reset", "search",
                 "search_device", "search_preassigned", "search_preassigned_device", "search_tables_preassigned_device", "train"],
}
IVF_EXPORTS = ["list_offsets", "kmeans_sample", "split_empty_clusters", "SearchParametersIVF", "check_quantizer", "METRIC_INNER_PRODUCT",
               "METRIC_L2", "IndexIVFFlat", "IVFFlatIndex"]


@pytest.mark.parametrize("cls", list(SURFACE), ids=lambda c: c.__name__)
def test_public_surface_is_unchanged(cls):
    assert [n for n in sorted(dir(cls)) if not n.startswith("_")] == SURFACE[cls]
    assert issubclass(cls, _ivf.InvertedFileIndex)


def test_neither_index_is_built_on_the_other():
    assert not issubclass(IVFPQIndex, IVFFlatIndex) and not issubclass(IVFFlatIndex, IVFPQIndex)


def test_ivf_module_still_exports_the_shared_names():
    for name in IVF_EXPORTS:
        assert hasattr(ivf, name), name
    assert ivf.kmeans_sample is _kmeans.kmeans_sample and ivf.split_empty_clusters is _kmeans.split_empty_clusters
    assert ivf.SearchParametersIVF is _ivf.SearchParametersIVF and ivf.check_quantizer is _ivf.check_quantizer


def test_pq_does_not_import_from_the_ivf_module():
    for name in ("pq.py", "_pqbase.py"):                             # PQIndex.train and its k-means step are in _pqbase.py
        with open(os.path.join(os.path.dirname(_ivf.__file__), name)) as f:
            text = f.read()
        assert not re.search(r"^\s*(from\s+(\.|ivr_amd\.)ivf\s+import|import\s+ivr_amd\.ivf\b|from\s+\.\s+import\s+.*\bivf\b)", text, re.M)
    assert re.search(r"^from \. import .*\b_kmeans\b", text, re.M)
