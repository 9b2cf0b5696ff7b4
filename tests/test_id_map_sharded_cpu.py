"""CPU suite: ShardedIndex over id-mapped shards (add_local_with_ids), world_size 2 over gloo.  Each rank's shard is a numpy double
with the add_with_ids / ntotal / search_device / range_search_device / remove_ids surface of an id-mapped FlatIPIndex: labels are
the stored ids, selectors name stored ids, id_base is taken and ignored.  After every call both ranks must agree with each other and
with a single numpy shard over all rows, and a removal on rank 0 must leave the labels of rank 1's rows as they were."""
import os
import socket
import sys

import numpy as np
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import PKG, ROOT

NEG_FLT_MAX = np.float32(-np.finfo(np.float32).max)


class NumpyIdShard:
    """Test double of an id-mapped FlatIPIndex: rows in storage order, ids[r] the label of row r."""

    def __init__(self, d):
        self.d = d
        self.rows = np.zeros((0, d), np.float32)
        self.ids = np.zeros(0, np.int64)

    @property
    def ntotal(self):
        return len(self.rows)

    def add_with_ids(self, x, ids):
        self.rows = np.concatenate([self.rows, np.asarray(x, np.float32)])
        self.ids = np.concatenate([self.ids, np.asarray(ids, np.int64)])

    def _scores(self, q, sel):
        S = np.asarray(q).astype(np.float64) @ self.rows.astype(np.float64).T
        ok = np.ones(len(self.rows), bool) if sel is None else np.array([sel.is_member(int(i)) for i in self.ids], bool)
        return S, ok

    def search_device(self, q, k, normalize=False, id_base=0, sel=None):
        S, ok = self._scores(q, sel)
        D = np.full((len(S), k), NEG_FLT_MAX, np.float32)
        I = np.full((len(S), k), -1, np.int64)
        rows = np.flatnonzero(ok)
        for i, s in enumerate(S):
            o = rows[np.lexsort((rows, -s[rows]))[:k]]       # ties: the lower ROW first, whatever its label
            D[i, :len(o)] = s[o]
            I[i, :len(o)] = self.ids[o]
        return torch.from_numpy(D), torch.from_numpy(I)

    def range_search_device(self, q, radius, normalize=False, id_base=0, sel=None):
        S, ok = self._scores(q, sel)
        lims, D, I = [0], [], []
        for s in S:
            hit = np.flatnonzero(ok & (s > radius))          # ascending row order
            lims.append(lims[-1] + len(hit))
            D.append(s[hit].astype(np.float32))
            I.append(self.ids[hit])
        lims = torch.tensor(lims, dtype=torch.int64)
        return lims, torch.from_numpy(np.concatenate(D)), torch.from_numpy(np.concatenate(I)), lims[-1:]

    def remove_ids(self, sel, id_base=0):
        if isinstance(sel, np.ndarray):                      # an integer array, wrapped as FlatIPIndex.remove_ids does
            from ivr_amd.index import IDSelectorBatch
            sel = IDSelectorBatch(sel)
        gone = np.array([sel.is_member(int(i)) for i in self.ids], bool)
        self.rows, self.ids = self.rows[~gone], self.ids[~gone]
        return int(gone.sum())


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _same(a, b):
    return all(np.array_equal(np.asarray(x), np.asarray(y)) for x, y in zip(a, b))


def _worker(rank, world, port, n, ret):
    for p in (ROOT, PKG, os.path.join(ROOT, "tests")):
        sys.path.insert(0, p)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from ivr_amd.index import IDSelectorBatch, IDSelectorRange, SearchParameters
    from ivr_amd.sharded import ShardedIndex, shard_bounds
    rng = np.random.default_rng(77)
    d = 16
    X = rng.standard_normal((n, d)).astype(np.float32)
    Q = rng.standard_normal((4, d)).astype(np.float32)
    ids = (3 * 10**12 + rng.permutation(10 * n)[:n]).astype(np.int64)      # a permutation spread over both ranks
    lo, hi = shard_bounds(n, world)[rank]
    sh = ShardedIndex(NumpyIdShard(d), d, merge="host")
    sh.add_local_with_ids(X[lo:hi], ids[lo:hi])
    ref = NumpyIdShard(d)
    ref.add_with_ids(X, ids)
    out = []

    def check(tag, sel=None):
        params = None if sel is None else SearchParameters(sel=sel)
        D, I = sh.search(Q, 8, params=params)
        Dr, Ir = ref.search_device(Q, 8, sel=sel)
        ok = np.array_equal(I.numpy(), Ir.numpy()) and np.array_equal(D.numpy(), Dr.numpy())
        got = sh.range_search(Q, 1.5, params=params)
        want = ref.range_search_device(Q, 1.5, sel=sel)[:3]
        ok = ok and _same([t.numpy() for t in got], [t.numpy() for t in want])
        out.append((tag, bool(ok), int(sh.ntotal), I.numpy().tolist(), got[0].numpy().tolist()))

    check("plain")
    some = IDSelectorBatch(np.concatenate([ids[::3], [int(ids.max()) + 5, -7]]))              # rows of both ranks, and ids nobody stores
    check("batch", some)
    check("range", IDSelectorRange(int(ids.min()) + 2 * n, int(ids.min()) + 7 * n))
    # remove rows of rank 0 only: the labels of rank 1's rows must not change
    I_before = sh.local.search_device(Q, 8)[1].numpy().copy()
    victims = ids[5:40:2]
    count = sh.remove_ids(victims)
    ref.remove_ids(IDSelectorBatch(victims))
    I_after = sh.local.search_device(Q, 8)[1].numpy()
    stable = rank == 0 or np.array_equal(I_before, I_after)
    out.append(("removed", bool(stable), int(count), int(sh.local.ntotal), int(sh.id_base)))
    check("after_remove")
    check("after_remove_batch", some)
    # a removal across both ranks by a selector
    sel = IDSelectorRange(int(ids.min()) + 4 * n, int(ids.min()) + 6 * n)
    count = sh.remove_ids(sel)
    out.append(("removed2", count == ref.remove_ids(sel), int(count), int(sh.ntotal)))
    check("after_remove2")
    ret[rank] = out
    dist.barrier()
    dist.destroy_process_group()


def test_two_rank_id_mapped_shards_over_gloo():
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
    r0, r1 = ret[0], ret[1]
    assert [e[0] for e in r0] == [e[0] for e in r1]
    for a, b in zip(r0, r1):
        assert a[1] is True and b[1] is True, (a[0], a[:3], b[:3])
        if not a[0].startswith("removed"):
            assert a == b, a[0]                              # identical results on every rank
    removed = dict((e[0], e) for e in r0)["removed"], dict((e[0], e) for e in r1)["removed"]
    assert removed[0][2] == removed[1][2] == 18              # the global count on both ranks
    assert removed[0][3] == 100 - 18 and removed[1][3] == 100 and removed[1][4] == 100 - 18


def test_world_one_id_mapped_shard():
    from ivr_amd.index import IDSelectorBatch
    from ivr_amd.sharded import ShardedIndex
    rng = np.random.default_rng(3)
    X = rng.standard_normal((50, 8)).astype(np.float32)
    ids = rng.permutation(500)[:50].astype(np.int64)
    sh = ShardedIndex(NumpyIdShard(8), 8)
    sh.add_local_with_ids(X, ids)
    assert sh.ntotal == 50
    assert sh.remove_ids(IDSelectorBatch(ids[10:20])) == 10
    assert sh.ntotal == 40 and np.array_equal(sh.local.ids, np.delete(ids, np.arange(10, 20)))
    D, I = sh.search(X[30:31], 1)
    assert I[0, 0] == ids[30]
