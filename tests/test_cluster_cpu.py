"""CPU suite of the frame clustering (ivr_amd/cluster.py, csrc/cluster.hip): the numpy definition dbscan_ref against sklearn's DBSCAN on
the float64 1 - cosine matrix the reference hands it (filter_research_update.py:113-134), the list plumbing and the numpy restatement
of the representative step on hand cases, the ABI of the two new entry points and the argument checks that need no device.  No
compute call reaches a device."""
import ctypes
import re

import numpy as np
import pytest
import torch

from cluster_cases import (DS, MIN_SAMPLES, NS, border_and_noise, clear_winner, contested_border, distances64, drifting_chains,
                           reference_representative, sklearn_dbscan, snapped_eps)
from conftest import ROOT
from ivr_amd import _ffi, cluster
from ivr_amd.index import FlatIPIndex
from oracle.reduce_ref import flat_score_bound

NEW = ("ivr_index_dbscan", "ivr_segment_best_cosine")


def scores32(X):
    """What the index computes for unit rows, in numpy float32."""
    return (X @ X.T).astype(np.float32)


# -- the definition against sklearn ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("d", DS)
def test_dbscan_ref_is_sklearn_dbscan(d, N):
    """labels_ and core_sample_indices_ of sklearn on the float64 distances, for eps snapped into the widest gap of the pair distances
    within +-20 % of 0.05 and of 0.02.  The precondition of an identical result: no float64 distance so close to eps that a float32
    score may fall on the other side (half the gap exceeds flat_score_bound)."""
    X = drifting_chains(N, d)
    D, S = distances64(X), scores32(X)
    border = noise = 0
    for nominal in (0.05, 0.02):
        eps, margin = snapped_eps(D, nominal, d)
        assert margin > flat_score_bound(d, 1.0), f"seed leaves no gap around eps={nominal}: {margin:.2e}"
        assert np.abs((1.0 - S.astype(np.float64)) - D).max() < margin
        for min_samples in MIN_SAMPLES:
            got = cluster.dbscan_ref(S, eps, min_samples)
            want = sklearn_dbscan(D, eps, min_samples)
            for g, w, what in zip(got, want, ("labels", "core", "nclusters")):
                assert g.dtype == w.dtype and np.array_equal(g, w), f"{what} differ (eps={eps}, min_samples={min_samples})"
            b, n = border_and_noise(got[0], got[1])
            border, noise = border + b, noise + n
    assert noise > 0 and (border > 0 or N < 3)           # a border row needs a core row with two neighbours


def test_contested_border_row_takes_the_lower_root_under_every_order():
    X = contested_border()
    rng = np.random.default_rng(5)
    seen = set()
    for p in [np.arange(9), np.arange(9)[::-1]] + [rng.permutation(9) for _ in range(40)]:
        Xp = X[p]
        got = cluster.dbscan_ref(scores32(Xp), 0.05, 4)
        want = sklearn_dbscan(distances64(Xp), 0.05, 4)
        assert all(np.array_equal(g, w) for g, w in zip(got, want))
        mid = int(np.flatnonzero(p == 4)[0])
        assert got[1][mid] == 0 and got[1].sum() == 8 and got[2][0] == 2
        first = int(np.flatnonzero(got[1])[0])           # the lowest core row is the root of cluster 0
        assert got[0][mid] == got[0][first] == 0
        seen.add(bool(p[first] < 4))
    assert seen == {True, False}                           # both clumps won somewhere


def test_segments_of_the_definition():
    S = np.ones((12, 12), np.float32)                      # every pair is an edge: a segment is one cluster when it has min_samples rows
    seg = np.array([1, 4, 4, 6, 11], np.int64)             # [1,4) [4,4) empty [4,6) [6,11); rows 0 and 11 outside
    labels, core, ncl = cluster.dbscan_ref(S, 0.0, 3, seg)
    assert labels.tolist() == [-1, 0, 0, 0, -1, -1, 0, 0, 0, 0, 0, -1]
    assert core.tolist() == [0, 1, 1, 1, 0, 0, 1, 1, 1, 1, 1, 0] and ncl.tolist() == [1, 0, 0, 1]
    labels, core, ncl = cluster.dbscan_ref(S, 0.0, 1, seg)                 # a row counts itself; outside a segment it is still no core
    assert labels.tolist() == [-1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, -1] and core[0] == core[11] == 0 and ncl.tolist() == [1, 0, 1, 1]
    S = np.eye(4, dtype=np.float32)                        # no edge at all: min_samples = 1 makes every row its own cluster, numbered per segment
    labels, core, ncl = cluster.dbscan_ref(S, 0.5, 1, [0, 2, 4])
    assert labels.tolist() == [0, 1, 0, 1] and ncl.tolist() == [2, 2]
    # <= keeps a distance equal to eps; only S[j, i] with j > i is read
    S = np.zeros((2, 2), np.float32)
    S[1, 0], S[0, 1] = 0.75, -5.0
    assert cluster.dbscan_ref(S, 0.25, 2)[0].tolist() == [0, 0]
    assert cluster.dbscan_ref(S, np.nextafter(np.float32(0.25), np.float32(0)), 2)[0].tolist() == [-1, -1]
    S[1, 0] = np.nan                                       # a NaN score is no edge
    assert cluster.dbscan_ref(S, np.inf, 2)[0].tolist() == [-1, -1]
    with pytest.raises(ValueError):
        cluster.dbscan_ref(np.zeros((2, 3), np.float32), 0.1, 2)


# -- lists and representatives ---------------------------------------------------------------------------------------------------------
def test_cluster_members_orders_by_segment_cluster_row():
    labels = np.array([-1, 1, 0, 1, -1, 0, 0, -1, 0, 1, 0], np.int32)
    off, members = cluster.cluster_members(labels, np.array([2], np.int32))
    assert off.tolist() == [0, 5, 8] and members.tolist() == [2, 5, 6, 8, 10, 1, 3, 9]
    assert off.dtype == torch.int64 and members.dtype == torch.int64
    seg = np.array([1, 4, 4, 9, 11], np.int64)             # [1,4): rows 1..3, [4,4) empty, [4,9): rows 4..8, [9,11): rows 9, 10
    off, members = cluster.cluster_members(labels, np.array([2, 0, 1, 2], np.int32), seg)
    assert members.tolist() == [2, 1, 3, 5, 6, 8, 10, 9]
    assert off.tolist() == [0, 1, 3, 6, 7, 8]
    off, members = cluster.cluster_members(np.full(5, -1, np.int32), np.array([0], np.int32))
    assert off.tolist() == [0] and members.tolist() == []
    off, members = cluster.cluster_members(torch.tensor([0, -1, 0]), torch.tensor([1]))
    assert off.tolist() == [0, 2] and members.tolist() == [0, 2]


def test_representatives_ref_on_hand_cases():
    e = np.eye(4, dtype=np.float32)
    X = np.stack([e[0], e[1], (e[0] + e[1]) / np.float32(2), e[2], e[2], np.zeros(4, np.float32)])
    # cluster 0: the row along the mean wins; cluster 1: two equal rows, the earlier member; cluster 2 is empty; cluster 3: a zero
    # row has cosine 0 and loses to anything positive
    reps = cluster.representatives_ref(X, [0, 3, 5, 5, 7], [0, 1, 2, 4, 3, 5, 0])
    assert reps.dtype == np.int64 and reps.tolist() == [2, 4, -1, 0]
    assert cluster.representatives_ref(X, [0, 2], [1, 0]).tolist() == [1]              # a tie of two goes to the earlier member
    assert cluster.representatives_ref(X, [0], []).tolist() == []


def test_representatives_ref_follows_the_reference_where_the_winner_is_clear():
    """Over the clusters of the 700-row cases with min_samples = 3 (every cluster has three rows at least; a cluster of two ties by
    symmetry): where the best two float64 cosines differ by more than flat_score_bound the float32 restatement names the
    reference's frame, and at least 90 % of the clusters are that clear."""
    for d in DS:
        X = drifting_chains(700, d)
        labels, core, ncl = cluster.dbscan_ref(scores32(X), 0.05, 3)
        off, members = (t.numpy() for t in cluster.cluster_members(labels, ncl))
        reps = cluster.representatives_ref(X, off, members)
        clear = 0
        for c in range(len(off) - 1):
            m, gaps = members[off[c]:off[c + 1]].tolist(), []
            want = reference_representative(m, X, gaps)
            assert len(m) >= 3
            if clear_winner(gaps[0], d):
                clear += 1
                assert reps[c] == want
        assert len(off) - 1 >= 30 and clear >= 0.9 * (len(off) - 1), f"d={d}: {clear} of {len(off) - 1} clusters have a clear winner"


def test_fma_emulation_rounds_once():
    x, y = np.float32(1 + 2.0 ** -12), np.float32(1 + 2.0 ** -12)           # x y = 1 + 2^-11 + 2^-24: the tail decides a tie
    acc = np.float32(2.0 ** -24)
    got = cluster._fma32(np.array([x]), np.array([y]), np.array([acc]))[0]
    assert got == np.float32(1 + 2.0 ** -11 + 2.0 ** -23)                      # 1 + 2^-11 + 2^-23 exactly: no rounding at all
    # x y = 2^-24 + 2^-60, so 1 + x y lies just above the float32 tie 1 + 2^-24: float64 rounds the sum onto the tie, and rounding
    # that to float32 (ties to even) would give 1
    x, y = np.float32((2 ** 12 + 1) * 2.0 ** -30), np.float32((2 ** 24 - 2 ** 12 + 1) * 2.0 ** -30)
    assert float(x) * float(y) == 2.0 ** -24 + 2.0 ** -60 and 1.0 + float(x) * float(y) == 1.0 + 2.0 ** -24
    got = cluster._fma32(np.array([x]), np.array([y]), np.array([np.float32(1)]))[0]
    assert got == np.float32(1 + 2.0 ** -23)


# -- ABI and surfaces ------------------------------------------------------------------------------------------------------------------
def _header():
    return re.sub(r"/\*.*?\*/", "", open(f"{ROOT}/include/ivr_api.h").read(), flags=re.S)


def _ctype_of(decl):
    decl = decl.strip()
    if "*" in decl or decl.startswith("ivr_stream"):
        return ctypes.c_void_p
    return {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "float": ctypes.c_float}[decl.split()[0]]


@pytest.mark.parametrize("name,names", [
    (NEW[0], ["idx", "eps", "min_samples", "seg_off", "nseg", "labels", "core", "nclusters", "stream"]),
    (NEW[1], ["ctx", "rows", "n", "seg_off", "nseg", "d", "centers", "best", "score", "stream"])])
def test_header_binding_and_library_agree(name, names):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", _header())
    assert m, f"{name} not declared in ivr_api.h"
    params = [p.strip() for p in m.group(1).split(",")]
    assert [re.sub(r"[\s*]+", " ", p).split()[-1] for p in params] == names
    res, args = _ffi._SIGS[name]
    assert res is ctypes.c_int and args == [_ctype_of(p) for p in params]
    assert _ffi._STREAM[name] == len(params) - 1
    assert name in _ffi.EXPORTS and name not in _ffi._VALUE
    assert hasattr(ctypes.CDLL(_ffi.LIB_PATH), name)


def test_api_version_is_still_11_and_no_class_grew_a_method():
    assert _ffi.API_VERSION == 11 and _ffi.load().ivr_api_version() == 11
    assert re.search(r"#define\s+IVR_API_VERSION\s+11\b", _header())
    assert not [n for n in dir(FlatIPIndex) if "dbscan" in n.lower() or "cluster" in n.lower()]


def test_library_rejects_bad_arguments_before_any_device_call():
    lib = _ffi.load()
    assert lib.ivr_index_dbscan(None, 0.05, 2, None, 0, None, None, None, None) == -1
    assert b"NULL" in lib.ivr_last_error(None)
    assert lib.ivr_segment_best_cosine(None, None, 0, None, 1, 4, None, None, None, None) == -1
    assert b"NULL" in lib.ivr_last_error(None)


def test_lazy_package_exports_resolve():
    import ivr_amd
    for name in ("dbscan", "dbscan_device", "dbscan_ref", "cluster_members", "select_representatives", "representatives_ref",
                 "cluster_similar_frames", "select_representative_frame"):
        assert name in ivr_amd.__all__
        assert getattr(ivr_amd, name) is getattr(cluster, name)
    assert cluster.CLUSTER_EPS == 0.05 and cluster.MIN_CLUSTER_SIZE == 2


def test_argument_checks_name_the_offending_values():
    index = FlatIPIndex.__new__(FlatIPIndex)             # no handle: every check below fails before the library is called
    index.d, index.device = 8, torch.device("cpu")
    with pytest.raises(ValueError, match="FlatIPIndex"):
        cluster.dbscan_device(object(), 0.05)
    with pytest.raises(ValueError, match=r"eps=-0\.5 is negative or NaN"):
        cluster.dbscan_device(index, -0.5)
    with pytest.raises(ValueError, match=r"eps=nan is negative or NaN"):
        cluster.dbscan_device(index, float("nan"))
    with pytest.raises(ValueError, match="eps must be a number, got str"):
        cluster.dbscan_device(index, "0.05")
    with pytest.raises(ValueError, match=r"min_samples=0 outside \[1,2\^31\)"):
        cluster.dbscan_device(index, 0.05, 0)
    with pytest.raises(ValueError, match="min_samples must be an integer, got float"):
        cluster.dbscan_device(index, 0.05, 2.5)
    with pytest.raises(ValueError, match=r"seg_off\[1\]=5 > seg_off\[2\]=3"):
        cluster.dbscan_device(index, 0.05, 2, seg_off=np.array([0, 5, 3]))
    with pytest.raises(ValueError, match="integers"):
        cluster.dbscan_device(index, 0.05, 2, seg_off=np.array([0.0, 5.0]))
    with pytest.raises(ValueError, match=r"\[nseg\+1\]"):
        cluster.dbscan_device(index, 0.05, 2, seg_off=np.array([0]))
    with pytest.raises(ValueError, match="FlatIPIndex"):
        cluster.select_representatives(object(), torch.zeros(2, dtype=torch.int64), torch.zeros(1, dtype=torch.int64))
    with pytest.raises(ValueError, match="members must be a contiguous int64 tensor"):
        cluster.select_representatives(index, torch.zeros(2, dtype=torch.int64), torch.zeros(1, dtype=torch.int32))
    # the reference's early returns need no device either
    assert cluster.cluster_similar_frames([]) == [] and cluster.cluster_similar_frames([np.ones(4)]) == [[0]]
    assert cluster.select_representative_frame([7], None) == 7
