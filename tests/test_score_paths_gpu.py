"""Every exact float32 score path of the flat index against one baseline, to the bit: the streamed-tile loop (search, clip search,
inverted lists, DBSCAN, neighbour graph) and the pair-score loop (re-score, range search) share one accumulation order
(csrc/search_internal.h), so each must report the scores S that FlatIPIndex.rescore_device reports for the stored rows as queries.
d = 112, 128, 144 are 7, 8 and 9 chunks of 16 floats: the tail alone, one full trip of eight, a trip and a tail.  N = 40 and 65 are
query blocks of 3 tiles, and of 4 + 1."""
import functools

import numpy as np
import pytest
import torch

from cluster_cases import EPS, SEGMENTS, drifting_chains
from ivr_amd import cluster, neighbors, temporal
from ivr_amd.index import FlatIPIndex
from ivr_amd.ivf import IVFFlatIndex
from test_knn_graph_gpu import self_scores

pytestmark = pytest.mark.gpu

shapes = pytest.mark.parametrize("N", (40, 65))
dims = pytest.mark.parametrize("d", (112, 128, 144))


@functools.lru_cache(maxsize=None)
def case(N, d):
    """(index, rows on the device, S, every row of S sorted descending): built and scored once, shared by the tests below and left
    unchanged.  A reported score of -0.0 is +0.0, so the sorted rows have 0.0 added."""
    X = drifting_chains(N, d)
    index = FlatIPIndex(d)
    index.add(X)
    S = self_scores(index)
    return index, torch.from_numpy(X).to(index.device), S, -np.sort(-(S + np.float32(0)), axis=1)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def ranked(D, I, S, ranks, what):
    """D [N,N] is every row of S in descending order, and I names the row behind each score."""
    D, I = D.cpu().numpy(), I.cpu().numpy()
    assert np.array_equal(bits(D), bits(ranks)), f"{what}: scores differ in rows {np.unique(np.nonzero(bits(D) != bits(ranks))[0])[:10]}"
    assert np.array_equal(np.sort(I, axis=1), np.tile(np.arange(len(S)), (len(S), 1))), f"{what}: labels are no permutation"
    assert np.array_equal(bits(np.take_along_axis(S, I, 1) + np.float32(0)), bits(D)), f"{what}: a label names another row's score"


@dims
@shapes
def test_flat_search(N, d):
    index, rows, S, ranks = case(N, d)
    ranked(*index.search_device(rows, N), S, ranks, "search")


@dims
@shapes
def test_range_search(N, d):
    index, rows, S, _ = case(N, d)
    radius = float(np.nextafter(S.min(), np.float32(-np.inf)))
    lims, D, I, total = index.range_search_device(rows, radius)
    assert int(total.item()) == N * N and np.array_equal(lims.cpu().numpy(), np.arange(N + 1) * N)
    assert np.array_equal(I.cpu().numpy().reshape(N, N), np.tile(np.arange(N), (N, 1)))
    assert np.array_equal(bits(D.cpu().numpy().reshape(N, N)), bits(S))


@dims
@shapes
def test_clip_search_of_one_frame(N, d):
    index, rows, S, ranks = case(N, d)
    ranked(*temporal.sequence_search_device(index, rows, 1, N), S, ranks, "sequence_search")


@dims
@shapes
def test_inverted_lists_all_probed(N, d):
    index, rows, S, ranks = case(N, d)
    ivf = IVFFlatIndex(d, 4)
    ivf.train(rows.cpu().numpy())
    ivf.add(rows.cpu().numpy())
    ivf.nprobe = 4
    ranked(*ivf.search_device(rows, N), S, ranks, "IVFFlatIndex.search")


@dims
@shapes
def test_neighbour_graph(N, d):
    index, rows, S, _ = case(N, d)
    got, want = neighbors.knn_graph(index, N - 1), neighbors.knn_graph_ref(S, N - 1)
    assert np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])


@pytest.mark.parametrize("segments", (False, True))
@dims
@shapes
def test_dbscan(N, d, segments):
    index, rows, S, _ = case(N, d)
    seg = np.minimum(SEGMENTS, N) if segments else None
    for g, w in zip(cluster.dbscan(index, EPS, 2, seg), cluster.dbscan_ref(S, EPS, 2, seg)):
        assert g.dtype == w.dtype and np.array_equal(g, w)
