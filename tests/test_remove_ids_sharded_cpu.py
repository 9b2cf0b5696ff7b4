"""CPU suite: ShardedIndex.remove_ids with global ids, world_size 2 over gloo.  Each rank's shard is a numpy double with the add /
ntotal / search_device / remove_ids surface of FlatIPIndex; after every removal all ranks must report the same global count and
ntotal, and search must equal a single numpy shard over the surviving rows."""
import os
import socket
import sys

import numpy as np
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import PKG, ROOT

NEG_FLT_MAX = np.float32(-np.finfo(np.float32).max)


class NumpyShard:
    """Test double with the FlatIPIndex surface the sharded removal needs."""

    def __init__(self, d):
        self.d = d
        self.rows = np.zeros((0, d), np.float32)

    @property
    def ntotal(self):
        return len(self.rows)

    def add(self, x):
        self.rows = np.concatenate([self.rows, np.asarray(x, np.float32)])

    def search_device(self, q, k, normalize=False, id_base=0):
        S = np.asarray(q).astype(np.float64) @ self.rows.astype(np.float64).T
        D = np.full((len(S), k), NEG_FLT_MAX, np.float32)
        I = np.full((len(S), k), -1, np.int64)
        for i, s in enumerate(S):
            o = np.lexsort((np.arange(len(s)), -s))[:k]
            D[i, :len(o)] = s[o]
            I[i, :len(o)] = id_base + o
        return torch.from_numpy(D), torch.from_numpy(I)

    def remove_ids(self, sel, id_base=0):
        gone = np.array([sel.is_member(id_base + r) for r in range(len(self.rows))], bool)
        self.rows = self.rows[~gone]
        return int(gone.sum())


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
    from ivr_amd.index import IDSelectorBatch, IDSelectorRange
    from ivr_amd.sharded import ShardedIndex, shard_bounds
    rng = np.random.default_rng(77)
    d = 16
    X = rng.standard_normal((n, d)).astype(np.float32)
    Q = rng.standard_normal((4, d)).astype(np.float32)
    lo, hi = shard_bounds(n, world)[rank]
    sh = ShardedIndex(NumpyShard(d), d, merge="host")
    sh.add_local(X[lo:hi])
    alive = np.ones(n, bool)                               # over the ORIGINAL rows; global ids are positions among the alive ones
    out = []
    # a range across the shard boundary (rows n/2-7 .. n/2+12), then - in the ids of what is left - a batch on rank 1 only
    for sel in (IDSelectorRange(n // 2 - 7, n // 2 + 13), IDSelectorBatch([n - 40, n - 41, n - 41, n - 25, 10 * n])):
        ids = np.flatnonzero(alive)
        gone = np.array([sel.is_member(i) for i in range(len(ids))], bool)
        alive[ids[gone]] = False
        count = sh.remove_ids(sel)
        ref = NumpyShard(d)
        ref.add(X[alive])
        D, I = sh.search(Q, 8)
        Dr, Ir = ref.search_device(Q, 8)
        ok = count == int(gone.sum()) and sh.ntotal == int(alive.sum()) and sh.local.ntotal == int(alive[lo:hi].sum())
        ok = ok and sh.id_base == int(alive[:lo].sum())
        ok = ok and np.array_equal(I.numpy(), Ir.numpy()) and np.allclose(D.numpy(), Dr.numpy(), rtol=1e-6, atol=1e-5)
        out.append((bool(ok), int(count), int(sh.ntotal)))
    ret[rank] = out
    dist.barrier()
    dist.destroy_process_group()


def test_two_rank_remove_ids_over_gloo():
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
    assert ret[0] == ret[1], dict(ret)                     # the same global count and ntotal on every rank
    assert [r[0] for r in ret[0]] == [True, True], dict(ret)
    assert [r[1:] for r in ret[0]] == [(20, 180), (3, 177)]


def test_world_one_remove_ids():
    from ivr_amd.index import IDSelectorRange
    from ivr_amd.sharded import ShardedIndex
    rng = np.random.default_rng(3)
    X = rng.standard_normal((50, 8)).astype(np.float32)
    sh = ShardedIndex(NumpyShard(8), 8)
    sh.add_local(X)
    assert sh.remove_ids(IDSelectorRange(10, 20)) == 10
    assert sh.ntotal == 40 and sh.id_base == 0
    assert np.array_equal(sh.local.rows, np.delete(X, np.arange(10, 20), axis=0))
