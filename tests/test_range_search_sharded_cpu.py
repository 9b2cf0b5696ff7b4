"""CPU suite: ShardedIndex.range_search with world_size 2 over gloo.  Each rank's shard is a numpy double with the
range_search_device surface of FlatIPIndex; the merged result must equal a float64 brute force over all rows, including a
query for which one rank has no hits at all."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import PKG, ROOT


def range_ref(X, Q, radius, id_base=0):
    """float64 range search: (lims, D, I), ids ascending within a query."""
    S = Q.astype(np.float64) @ X.astype(np.float64).T
    lims, D, I = [0], [], []
    for s in S:
        ids = np.nonzero(s > radius)[0]
        D.append(s[ids])
        I.append(ids + id_base)
        lims.append(lims[-1] + len(ids))
    return np.array(lims, np.int64), np.concatenate(D) if D else np.zeros(0), np.concatenate(I).astype(np.int64)


class RangeShard:
    """Test double with the FlatIPIndex surface the sharded range search needs."""

    def __init__(self, d):
        self.d = d
        self.rows = np.zeros((0, d), np.float32)

    @property
    def ntotal(self):
        return len(self.rows)

    def add(self, x):
        self.rows = np.concatenate([self.rows, np.asarray(x, np.float32)])

    def range_search_device(self, q, radius, normalize=False, id_base=0, cap=None):
        q = np.asarray(q, np.float64)
        if normalize:
            q = q / np.maximum(np.linalg.norm(q, axis=1, keepdims=True), 1e-30)
        lims, D, I = range_ref(self.rows, q, radius, id_base)
        lims = torch.from_numpy(lims)
        return lims, torch.from_numpy(D.astype(np.float32)), torch.from_numpy(I), lims[-1:]


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, n, ret):
    for p in (ROOT, PKG, os.path.join(ROOT, "tests")):
        sys.path.insert(0, p)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from ivr_amd.sharded import ShardedIndex, shard_bounds
    rng = np.random.default_rng(77)
    d = 32
    X = rng.standard_normal((n, d)).astype(np.float32)
    Q = rng.standard_normal((5, d)).astype(np.float32)
    lo, hi = shard_bounds(n, world)[rank]
    # query 4 is row 0 scaled by 10: its score with row 0 (about 320) is far above every other score, so at radius 200 rank 0
    # returns one row and rank 1 none
    Q[4] = X[0] * 10.0
    ok = True
    sh = ShardedIndex(RangeShard(d), d)
    sh.add_local(X[lo:hi])
    assert sh.ntotal == n and sh.id_base == lo
    for rad in (200.0, 2.0, float("inf"), float("-inf")):
        lims, D, I = sh.range_search(Q, rad)
        lr, Dr, Ir = range_ref(X, Q, rad)
        ok = ok and np.array_equal(lims.numpy(), lr) and np.array_equal(I.numpy(), Ir)
        if rad == 200.0:
            ok = ok and lims.numpy().tolist() == [0, 0, 0, 0, 0, 1] and I.numpy().tolist() == [0]
        ok = ok and np.allclose(D.numpy(), Dr, rtol=1e-6, atol=1e-5)
        gathered = [None] * world
        dist.all_gather_object(gathered, (lims.numpy().tolist(), I.numpy().tolist()))
        ok = ok and all(g == gathered[0] for g in gathered)
    ret[rank] = bool(ok)
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("n", [400, 3])
def test_two_rank_sharded_range_search_over_gloo(n):
    world = 2
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


def test_world_one_returns_the_local_result():
    from ivr_amd.sharded import ShardedIndex
    rng = np.random.default_rng(3)
    X = rng.standard_normal((50, 8)).astype(np.float32)
    Q = rng.standard_normal((3, 8)).astype(np.float32)
    sh = ShardedIndex(RangeShard(8), 8)
    sh.local.add(X)
    lims, D, I = sh.range_search(Q, 0.5)
    lr, _, Ir = range_ref(X, Q, 0.5)
    assert np.array_equal(lims.numpy(), lr) and np.array_equal(I.numpy(), Ir)
