"""GPU suite: the error bounds of the bf16 candidate scan at their edge.  The rows of tests/bound_cases.py put a true neighbour's
approximate score 0.95 .. 1.0 of the analytic bound below its exact one and outside the re-scored groups, so the search returns it only
if the device check (select_topk_kernel), the pruned re-score (rescore_groups_kernel), the range candidates (range_candidates_kernel)
and every kernel that maintains maxnorm / maxdelta use a bound that is large enough; the `safe` rows fail if it is a quarter too
large.  tests/test_scan_bound_cpu.py proves on the numpy model that the cases do what they claim, including that the expected ids
below are the float64 top-k by a margin float32 scoring cannot cross.  Everything here is compared for equality.

Redone counts (scan_stats()[1], the last chunk: every batch here is one chunk).  A hidden row lies outside the re-scored groups, so a
correct result for an adversarial query is only possible through the exact pass: all of them must be counted (small batches hold
nothing else; large ones add Gaussian fillers, which may or may not fire).  `safe` and `prune` batches hold no fillers and no query
may be redone."""
import os

import numpy as np
import pytest
import torch

import bound_cases as B

pytestmark = pytest.mark.gpu

_CACHE = {}


def _index_with(env, d, X=None, capacity=0):
    from ivr_amd.index import FlatIPIndex
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        idx = FlatIPIndex(d, capacity=len(X) if X is not None else capacity)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v
    if X is not None:
        idx.add(X, normalize=False)
    return idx


def _indexes(name, d):
    """(candidate-scan index, IVR_SCAN_BF16=0 index) over the case's rows, built once per module"""
    if (name, d) not in _CACHE:
        X = B.make(name, d)["X"]
        _CACHE[(name, d)] = (_index_with({}, d, X), _index_with({"IVR_SCAN_BF16": "0"}, d, X))
    return _CACHE[(name, d)]


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else t.dtype)


def _search_checked(idx, exact, case, nq, fillers=True):
    """One batch: the candidate scan ran, D and I carry the bits of the exact float32 scan, the adversarial queries return the float64
    top-k.  Returns (redone, number of adversarial queries)."""
    Q, adv = B.queries(case, nq, fillers=fillers)
    k = case["k"]
    D, I = idx.search_device(Q, k, normalize=False)
    has16, redone = idx.scan_stats()
    assert has16, nq
    De, Ie = exact.search_device(Q, k, normalize=False)
    assert not exact.scan_stats()[0]
    assert torch.equal(I, Ie), (nq, (I != Ie).nonzero()[:5].tolist())
    assert torch.equal(_bits(D), _bits(De)), nq
    if len(case["winners"]):
        got = I.cpu().numpy()[adv]
        assert np.array_equal(got, np.broadcast_to(case["winners"], got.shape)), (nq, got[:3].tolist(), case["winners"].tolist())
    return redone, int(adv.sum())


def _nqs(case):
    return tuple(B.SMALL_NQ if "small" in case["paths"] or case["kind"] == "qrem" else ()) + tuple(B.BIG_NQ)


@pytest.mark.parametrize("d", B.DIMS)
@pytest.mark.parametrize("name", ["sharp_k1", "sharp_k10", "tied_k1", "qrem"])
def test_hidden_neighbours_are_found_through_the_exact_pass(name, d):
    """qrem with at most 64 queries: q_hi + q_lo keeps the query's remainder, W's group is re-scored and W is returned either way; the
    check still cannot pass there (the first excluded group holds a decoy within E_small of W), so those queries are redone too."""
    case = B.make(name, d)
    idx, exact = _indexes(name, d)
    for nq in _nqs(case):
        redone, nadv = _search_checked(idx, exact, case, nq)
        print(f"{name} d={d} nq={nq}: {redone} redone, {nadv} adversarial")
        assert redone == nq if nq <= 64 else nadv <= redone <= nq, (nq, redone, nadv)


@pytest.mark.parametrize("d", B.DIMS)
@pytest.mark.parametrize("name", ["safe_k1", "safe_k10"])
def test_safe_rows_pass_the_check_without_a_fallback(name, d):
    case = B.make(name, d)
    idx, exact = _indexes(name, d)
    for nq in _nqs(case):
        redone, nadv = _search_checked(idx, exact, case, nq, fillers=False)
        assert nadv == nq and redone == 0, (nq, redone)


@pytest.mark.parametrize("d", B.DIMS)
def test_pruned_rescore_keeps_the_tile_inside_twice_the_bound(d):
    case = B.make("prune", d)
    idx, exact = _indexes("prune", d)
    full = _index_with({"IVR_SCAN_PRUNE": "0"}, d, case["X"])
    for nq in B.BIG_NQ:
        for fillers in (True, False):
            redone, nadv = _search_checked(idx, exact, case, nq, fillers=fillers)
            assert fillers or redone == 0, (nq, redone)        # the verification passes: the re-score alone decides
            Q, _ = B.queries(case, nq, fillers=fillers)
            D, I = idx.search_device(Q, 1, normalize=False)
            Df, If = full.search_device(Q, 1, normalize=False)
            assert torch.equal(I, If) and torch.equal(_bits(D), _bits(Df)), nq


def _store(path, d, case):
    """An index that held the filler rows alone (small maxnorm / maxdelta) and got the special rows through `path`."""
    X, F, N = case["X"], case["F"], case["N"]
    special = np.sort(np.concatenate([case["hidden"], case["top"], case["low"]]))
    r0, r1 = int(special[0]), int(special[-1]) + 1
    if r0 % 16 == 0:
        r0 -= 3                                              # an unaligned start for the appends and the overwrite
    assert r0 > 0 and r0 % 16 != 0
    dev = torch.device("cuda")
    if path == "add":
        idx = _index_with({}, d, F[:r0])
        idx.add(X[r0:])
    elif path == "add_with_ids":
        idx = _index_with({}, d, capacity=r0)
        idx.add_with_ids(F[:r0], np.arange(r0))
        idx.add_with_ids(X[r0:], np.arange(r0, N))
    elif path == "write":
        idx = _index_with({}, d, F)
        idx.write(r0, X[r0:r1])
    elif path == "write_ring":
        idx = _index_with({}, d, F)
        n = 1300                                             # divides N = 6500; every batch after the first starts unaligned
        assert N % n == 0 and n % 16 != 0
        cursor = torch.zeros(1, dtype=torch.int64, device=dev)
        for i in range(0, N, n):
            idx.write_ring(torch.tensor(X[i:i + n], device=dev), cursor)
        assert int(cursor.item()) == 0
    elif path == "scatter_device":
        idx = _index_with({}, d, F)
        idx.scatter_device(torch.tensor(special, device=dev), torch.tensor(X[special], device=dev))
        torch.cuda.synchronize()
    elif path == "reset_add":
        idx = _index_with({}, d, F)
        idx.search_device(B.queries(case, 10)[0], 1)
        idx.reset()
        idx.add(X)
    else:
        raise ValueError(path)
    return idx


@pytest.mark.parametrize("d", B.DIMS)
@pytest.mark.parametrize("path", ["add", "add_with_ids", "write", "write_ring", "scatter_device", "reset_add"])
def test_every_row_writing_path_keeps_the_bounds_inputs_valid(path, d):
    """A path that leaves maxnorm or maxdelta at the fillers' values makes e five to ten times too small: the check passes and a decoy
    is returned for H."""
    case = B.make("sharp_k1", d)
    _, exact = _indexes("sharp_k1", d)
    idx = _store(path, d, case)
    assert idx.ntotal == case["N"]
    assert np.array_equal(idx.reconstruct_n(0, case["N"]).view(np.uint32), case["X"].view(np.uint32))
    for nq in (10, 65):
        redone, nadv = _search_checked(idx, exact, case, nq)
        print(f"{path} d={d} nq={nq}: {redone} redone, {nadv} adversarial")
        assert redone == nq if nq <= 64 else nadv <= redone <= nq, (nq, redone, nadv)


@pytest.mark.parametrize("d", B.DIMS)
def test_range_search_keeps_groups_within_the_bound_of_the_radius(d):
    case = B.make("sharp_k1", d)
    idx, exact = _indexes("sharp_k1", d)
    for nq in (1, 10):
        Q = np.random.default_rng(d + nq).standard_normal((nq, d)).astype(np.float32)
        Q[0] = case["q"]
        Q[nq // 2] = case["q"]
        for radius, ids in B.range_radii(case):
            lims, D, I = idx.range_search(Q, radius)
            le, De, Ie = exact.range_search(Q, radius)
            assert np.array_equal(lims, le) and np.array_equal(I, Ie) and np.array_equal(D.view(np.uint32), De.view(np.uint32)), (nq, radius)
            for qi in {0, nq // 2}:
                assert np.array_equal(I[lims[qi]:lims[qi + 1]], ids), (nq, radius, qi)


@pytest.mark.parametrize("d", B.DIMS)
def test_nonfinite_scan_copy_sends_every_query_through_the_exact_pass(d):
    case = B.make("nonfinite", d)
    idx, exact = _indexes("nonfinite", d)
    for nq in (10, 64, 65, 300):
        redone, _ = _search_checked(idx, exact, case, nq)
        assert redone == nq, (nq, redone)
