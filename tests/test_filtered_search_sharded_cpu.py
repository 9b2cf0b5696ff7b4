"""CPU suite: ShardedIndex.search / range_search with a global ID selector, world_size 2 over gloo.  Each rank's shard is a numpy
double with the search_device / range_search_device(sel=) surface of FlatIPIndex; the merged result must equal float64 over all rows
restricted to the allowed ids, including a selector that allows no row of one rank."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import PKG, ROOT

NEG_FLT_MAX = np.float32(-np.finfo(np.float32).max)


def _allowed(sel, ids):
    return np.array([sel is None or sel.is_member(i) for i in ids], bool)


def topk_ref(X, Q, k, sel=None, id_base=0):
    """float64 top k among the allowed ids (id_base + row), ties to the lower id; (-FLT_MAX, -1) padded."""
    S = Q.astype(np.float64) @ X.astype(np.float64).T
    ids = id_base + np.arange(len(X))
    ok = _allowed(sel, ids)
    D = np.full((len(Q), k), NEG_FLT_MAX, np.float32)
    I = np.full((len(Q), k), -1, np.int64)
    for q, s in enumerate(S):
        cand = np.nonzero(ok)[0]
        o = cand[np.lexsort((cand, -s[cand]))][:k]
        D[q, :len(o)] = s[o]
        I[q, :len(o)] = ids[o]
    return D, I


def range_ref(X, Q, radius, sel=None, id_base=0):
    S = Q.astype(np.float64) @ X.astype(np.float64).T
    ok = _allowed(sel, id_base + np.arange(len(X)))
    lims, D, I = [0], [], []
    for s in S:
        r = np.nonzero((s > radius) & ok)[0]
        D.append(s[r])
        I.append(r + id_base)
        lims.append(lims[-1] + len(r))
    return np.array(lims, np.int64), np.concatenate(D), np.concatenate(I).astype(np.int64)


class FilterShard:
    """Test double with the FlatIPIndex surface the sharded filtered search needs."""

    def __init__(self, d):
        self.d = d
        self.rows = np.zeros((0, d), np.float32)

    @property
    def ntotal(self):
        return len(self.rows)

    def add(self, x):
        self.rows = np.concatenate([self.rows, np.asarray(x, np.float32)])

    def search_device(self, q, k, normalize=False, id_base=0, sel=None):
        D, I = topk_ref(self.rows, np.asarray(q), k, sel, id_base)
        return torch.from_numpy(D), torch.from_numpy(I)

    def range_search_device(self, q, radius, normalize=False, id_base=0, cap=None, sel=None):
        lims, D, I = range_ref(self.rows, np.asarray(q), radius, sel, id_base)
        lims = torch.from_numpy(lims)
        return lims, torch.from_numpy(D.astype(np.float32)), torch.from_numpy(I), lims[-1:]


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _selectors(n):
    from ivr_amd.index import IDSelectorBatch, IDSelectorBitmap, IDSelectorRange
    rng = np.random.default_rng(5)
    mask = rng.random(n) < 0.3
    return [IDSelectorBatch([3, 7, 7, 11, n + 40]),                 # every allowed id on rank 0; rank 1 has none
            IDSelectorRange(n // 2 - 3, n - 1),                       # straddles the shard boundary
            IDSelectorBitmap(np.packbits(mask, bitorder="little")),
            IDSelectorBatch([])]


def _worker(rank, world, port, n, ret):
    for p in (ROOT, PKG, os.path.join(ROOT, "tests")):
        sys.path.insert(0, p)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from ivr_amd.index import SearchParameters
    from ivr_amd.sharded import ShardedIndex, shard_bounds
    rng = np.random.default_rng(77)
    d = 16
    X = rng.standard_normal((n, d)).astype(np.float32)
    Q = rng.standard_normal((4, d)).astype(np.float32)
    lo, hi = shard_bounds(n, world)[rank]
    sh = ShardedIndex(FilterShard(d), d, merge="host")
    sh.add_local(X[lo:hi])
    ok = True
    for sel in _selectors(n):
        p = SearchParameters(sel=sel)
        D, I = sh.search(Q, 8, params=p)
        Dr, Ir = topk_ref(X, Q, 8, sel)
        ok = ok and np.array_equal(I.numpy(), Ir) and np.allclose(D.numpy(), Dr, rtol=1e-6, atol=1e-5)
        lims, Dg, Ig = sh.range_search(Q, 0.5, params=p)
        lr, _, Irr = range_ref(X, Q, 0.5, sel)
        ok = ok and np.array_equal(lims.numpy(), lr) and np.array_equal(Ig.numpy(), Irr)
    ret[rank] = bool(ok)
    dist.barrier()
    dist.destroy_process_group()


def test_two_rank_filtered_search_over_gloo():
    world, n = 2, 200
    ctx = mp.get_context("spawn")
    ret = ctx.Manager().dict()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, n, ret)) for r in range(world)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(120)
        assert p.exitcode == 0
    assert all(ret.get(r) for r in range(world)), dict(ret)


def test_world_one_passes_the_selector():
    from ivr_amd.index import IDSelectorRange, SearchParameters
    from ivr_amd.sharded import ShardedIndex
    rng = np.random.default_rng(3)
    X = rng.standard_normal((50, 8)).astype(np.float32)
    Q = rng.standard_normal((3, 8)).astype(np.float32)
    sh = ShardedIndex(FilterShard(8), 8)
    sh.local.add(X)
    sel = IDSelectorRange(10, 20)
    D, I = sh.search(Q, 4, params=SearchParameters(sel=sel))
    assert np.array_equal(I.numpy(), topk_ref(X, Q, 4, sel)[1])
    # without params the local call gets no sel keyword (shards without filtering keep working)
    D, I = sh.search(Q, 4)
    assert np.array_equal(I.numpy(), topk_ref(X, Q, 4)[1])
    with pytest.raises(ValueError):
        sh.search(Q, 4, params="all")
