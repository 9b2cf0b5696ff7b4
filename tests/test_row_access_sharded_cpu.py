"""CPU suite: ShardedIndex.reconstruct_batch, world_size 2 over gloo.  Each rank's shard is a numpy double with the surface the call
needs of a FlatIPIndex (add / add_with_ids / ntotal / has_ids / reconstruct_batch_device).  Both ranks must return the same rows as a
single numpy shard over all rows: plain shards resolve a global row through the synced shard bounds, id-mapped shards resolve a label to
the lowest rank that stores it (the lowest global storage position), and an id nobody stores raises on both ranks after the
collectives, so that neither rank is left waiting for the other."""
import os
import socket
import sys

import numpy as np
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import PKG, ROOT


class NumpyRowShard:
    """Test double of a FlatIPIndex shard, plain (add) or id-mapped (add_with_ids): rows in storage order."""

    def __init__(self, d):
        self.d = d
        self.rows = np.zeros((0, d), np.float32)
        self.ids = None

    @property
    def ntotal(self):
        return len(self.rows)

    @property
    def has_ids(self):
        return self.ids is not None

    def add(self, x):
        self.rows = np.concatenate([self.rows, np.asarray(x, np.float32)])

    def add_with_ids(self, x, ids):
        self.ids = np.concatenate([self.ids if self.has_ids else np.zeros(0, np.int64), np.asarray(ids, np.int64)])
        self.add(x)

    def reconstruct_batch_device(self, keys):
        keys = np.asarray(keys, np.int64).reshape(-1)
        if self.has_ids:
            low = {}
            for r, i in enumerate(self.ids.tolist()):
                low.setdefault(i, r)
            rows = np.asarray([low.get(int(k), -1) for k in keys], np.int64)
        else:
            rows = np.where((keys >= 0) & (keys < self.ntotal), keys, -1)
        R = np.full((len(keys), self.d), np.nan, np.float32)
        R[rows >= 0] = self.rows[rows[rows >= 0]]
        return torch.from_numpy(rows), torch.from_numpy(R)


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
    rng = np.random.default_rng(91)
    d = 12
    X = rng.standard_normal((n, d)).astype(np.float32)
    lo, hi = shard_bounds(n, world)[rank]
    out = []

    def run(tag, sh, keys, want):
        try:
            got = sh.reconstruct_batch(keys)
            out.append((tag, want is not None and got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32)),
                        got.view(np.uint32).tolist()))
        except RuntimeError as e:
            out.append((tag, want is None, str(e)))

    # plain shards: ids are global rows
    plain = ShardedIndex(NumpyRowShard(d), d, merge="host")
    plain.add_local(X[lo:hi])
    keys = np.concatenate([rng.integers(0, n, 40), [0, n - 1, n // 2 - 1, n // 2]]).astype(np.int64)     # both shards, both edges, repeats
    run("plain", plain, keys, X[keys])
    run("plain_missing_high", plain, np.asarray([3, n, 5]), None)
    run("plain_missing_negative", plain, np.asarray([-1]), None)
    run("plain_empty", plain, np.zeros(0, np.int64), X[:0])
    run("plain_again", plain, keys[:7], X[keys[:7]])                         # the ranks are still in step after the errors
    # id-mapped shards: labels spread over both ranks, one of them stored on both and twice on rank 1
    ids = (3 * 10**12 + rng.permutation(10 * n)[:n]).astype(np.int64)
    a, b, c = 7, n // 2 + 11, n // 2 + 30                                     # row a on rank 0, rows b < c on rank 1
    ids[b] = ids[c] = ids[a]
    ids[n // 2 + 50] = ids[n // 2 + 5]                                         # and one stored twice on rank 1 only: its lower row
    mapped = ShardedIndex(NumpyRowShard(d), d, merge="host")
    mapped.add_local_with_ids(X[lo:hi], ids[lo:hi])
    one = NumpyRowShard(d)
    one.add_with_ids(X, ids)                                                  # a single shard over all rows: the lowest storage position
    pick = rng.permutation(n)[:40]
    keys = np.concatenate([ids[pick], [ids[a], ids[n // 2 + 50], ids[0], ids[n - 1]]])
    want = one.reconstruct_batch_device(keys)[1].numpy()
    out.append(("mapped_ref", bool(np.array_equal(want[40].view(np.uint32), X[a].view(np.uint32))
                                   and np.array_equal(want[41].view(np.uint32), X[n // 2 + 5].view(np.uint32))), None))
    run("mapped", mapped, keys, want)
    run("mapped_missing", mapped, np.asarray([ids[3], ids.max() + 1, -4]), None)
    run("mapped_again", mapped, keys[38:], want[38:])
    ret[rank] = out
    dist.barrier()
    dist.destroy_process_group()


def test_two_rank_reconstruct_batch_over_gloo():
    world, n = 2, 200
    ctx = mp.get_context("spawn")
    ret = ctx.Manager().dict()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, n, ret)) for r in range(world)]
    for p in procs:
        p.start()
    try:
        for p in procs:
            p.join(120)                                                       # a rank left waiting in a collective fails here
            assert p.exitcode == 0
    finally:
        for p in procs:
            if p.is_alive():
                p.kill()
    r0, r1 = ret[0], ret[1]
    assert [e[0] for e in r0] == [e[0] for e in r1] and len(r0) == 9
    for a, b in zip(r0, r1):
        assert a[1] is True and b[1] is True, (a[0], a[2] if isinstance(a[2], str) else None)
        assert a == b, a[0]                                                   # identical rows, and identical errors, on every rank
    errors = [e for e in r0 if "missing" in e[0]]
    assert len(errors) == 3 and all("not in the index" in e[2] for e in errors)


def test_world_one_reconstruct_batch():
    from ivr_amd.sharded import ShardedIndex
    rng = np.random.default_rng(4)
    X = rng.standard_normal((30, 8)).astype(np.float32)
    sh = ShardedIndex(NumpyRowShard(8), 8)
    sh.add_local(X)
    assert np.array_equal(sh.reconstruct_batch([4, 29, 4]), X[[4, 29, 4]])
    try:
        sh.reconstruct_batch([30])
    except RuntimeError:
        pass
    else:
        raise AssertionError("a missing id must raise")
