"""GPU: the key sources of select_topk_kernel that only a search reaches (SrcGroupMax, SrcTilesOf, SrcKeys; outputs OUT_GROUPS,
OUT_DI, OUT_DI_IDS and the *_POS variants) under BULK TIES, which leave the selector's survivor path for its fallbacks.

Rows are base * {1, 0.5, 0.25, 0, -1} by a seeded assignment: every score is an exact power-of-two multiple of <q, base>, so a fifth
of the index ties bit for bit at every level, the levels lie far apart, and the expected result is unambiguous - within a level the
lowest rows first.  N = 70_000 / 300_000 / 1_048_641 gives 1094 / 4688 / 16385 group keys: the selector's 256-thread, 1024-thread
cached and uncached layouts.  65 queries take the large-batch scan (for k <= 128), 3 the chunked one."""
import functools
import os

import numpy as np
import pytest
import torch

from oracle import search_ref as S

pytestmark = pytest.mark.gpu

D_ = 16
PALETTE = np.array([1.0, 0.5, 0.25, 0.0, -1.0], dtype=np.float32)
K_MAX, NQ_MAX = 300, 65


def _exact_index(d, capacity):
    """A FlatIPIndex without the bf16 candidate scan (the switch is read when the index is created)."""
    from ivr_amd.index import FlatIPIndex
    old = os.environ.get("IVR_SCAN_BF16")
    os.environ["IVR_SCAN_BF16"] = "0"
    try:
        return FlatIPIndex(d, capacity=capacity)
    finally:
        if old is None:
            del os.environ["IVR_SCAN_BF16"]
        else:
            os.environ["IVR_SCAN_BF16"] = old


@functools.lru_cache(maxsize=None)
def _setup(N):
    """Rows, queries, the float64 brute force for the largest k and query count (smaller ones are its prefixes), and the two
    indexes (with and without the bf16 candidate scan) on the same rows - all made once per N and never modified."""
    from ivr_amd.index import FlatIPIndex
    rng = np.random.default_rng(N)
    base = rng.standard_normal(D_).astype(np.float32)
    X = PALETTE[rng.integers(0, len(PALETTE), N)][:, None] * base[None, :]          # exact: the factors are powers of two (or 0)
    assert X.dtype == np.float32
    along = rng.uniform(0.5, 2.0, NQ_MAX) * rng.choice([-1.0, 1.0], NQ_MAX)         # both signs: the -1 level wins for some queries
    Q = (along[:, None] * base[None, :] + 0.3 * rng.standard_normal((NQ_MAX, D_))).astype(np.float32)
    t = Q.astype(np.float64) @ base.astype(np.float64)
    assert np.abs(t).min() > 0.1 * float(base.astype(np.float64) @ base)           # <q, base> well away from 0
    Dr, Ir = S.flat_ip_search(X, Q, K_MAX, dtype=np.float64)
    assert all(len(np.unique(Dr[q])) <= len(PALETTE) for q in range(NQ_MAX))        # the oracle's ties are bit-exact too
    idx = FlatIPIndex(D_, capacity=N)
    idx.add(X)
    exact = _exact_index(D_, N)
    exact.add(X)
    for a in (X, Q, Dr, Ir):
        a.setflags(write=False)
    return X, Q, Dr, Ir, idx, exact


CASES = [(N, nq, k) for N in (70_000, 300_000) for nq in (3, NQ_MAX) for k in (1, 10, 65, 300)] + \
        [(1_048_641, nq, k) for nq in (3, NQ_MAX) for k in (10, 300)]


@pytest.mark.parametrize("N,nq,k", CASES)
def test_tied_rows_search_equals_float64_oracle_and_exact_scan(N, nq, k):
    X, Q, Dr, Ir, idx, exact = _setup(N)
    Dt, It = idx.search_device(Q[:nq], k)
    De, Ie = exact.search_device(Q[:nq], k)
    print(f"N={N} nq={nq} k={k}: scan_stats = {idx.scan_stats()} (bf16 copy, queries of the last chunk redone exactly)")
    D, I = Dt.cpu().numpy(), It.cpu().numpy()
    bad = np.argwhere(I != Ir[:nq, :k])
    assert bad.size == 0, (bad[:5], I[tuple(bad[0])], Ir[tuple(bad[0])])
    assert np.abs(D - Dr[:nq, :k]).max() < 1e-5 * np.abs(Dr[:nq, :k]).max()
    assert not exact.scan_stats()[0]
    assert torch.equal(It, Ie) and torch.equal(Dt, De)


@pytest.mark.parametrize("nq", [3, NQ_MAX])
def test_tied_rows_on_an_id_mapped_index_and_with_reconstruct(nq):
    """N = 70_000, k = 10 on the other outputs of the final selection: labels from the id table (OUT_DI_IDS), and the positions
    behind search_and_reconstruct, plain (OUT_DI_POS) and id-mapped (OUT_DI_IDS_POS)."""
    from ivr_amd.index import FlatIPIndex
    N, k = 70_000, 10
    X, Q, Dr, Ir, idx, exact = _setup(N)
    Ir, Dr = Ir[:nq, :k], Dr[:nq, :k]
    ids = (np.random.default_rng(11).permutation(N) + (1 << 32) + 5).astype(np.int64)
    mapped = FlatIPIndex(D_, capacity=N)
    mapped.add_with_ids(X, ids)
    D0, I0 = idx.search(Q[:nq], k)
    Dm, Im = mapped.search(Q[:nq], k)
    print(f"id-mapped nq={nq}: scan_stats = {mapped.scan_stats()}")
    assert np.array_equal(Im, ids[Ir]) and np.array_equal(I0, Ir)
    assert np.array_equal(Dm.view(np.uint32), D0.view(np.uint32))
    D1, I1, R1 = idx.search_and_reconstruct(Q[:nq], k)
    D2, I2, R2 = mapped.search_and_reconstruct(Q[:nq], k)
    assert np.array_equal(I1, Ir) and np.array_equal(R1, X[Ir])
    assert np.array_equal(I2, ids[Ir]) and np.array_equal(R2, X[Ir])
    assert np.array_equal(D1.view(np.uint32), D0.view(np.uint32)) and np.array_equal(D2.view(np.uint32), D0.view(np.uint32))
