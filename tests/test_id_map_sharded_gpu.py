"""GPU: id-mapped shards (FlatIPIndex.add_with_ids) behind the sharded path: two real HIP shards on one GPU with the emulated merge of
test_sharded_gpu.py, and ShardedIndex at world_size 1.  The yardstick is a single id-mapped index over all rows: merged results equal
its results bit for bit, and a removal on shard 0 leaves the labels of shard 1's rows as they were."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N, D_, K = 3001, 512, 10


def _setup():
    from ivr_amd.index import FlatIPIndex
    from ivr_amd.sharded import shard_bounds
    rng = np.random.default_rng(91)
    X = rng.standard_normal((N, D_)).astype(np.float32)
    X /= np.linalg.norm(X, axis=1, keepdims=True)
    X[2000] = X[10]                                          # a tie across the shards: shard 0's row ranks first
    ids = (3 * 10**12 + rng.permutation(10 * N)[:N]).astype(np.int64)
    Q = np.concatenate([X[10:11], rng.standard_normal((11, D_)).astype(np.float32)])
    bounds = shard_bounds(N, 2)
    shards = []
    for lo, hi in bounds:
        s = FlatIPIndex(D_)
        s.add_with_ids(X[lo:hi], ids[lo:hi])
        shards.append(s)
    whole = FlatIPIndex(D_)
    whole.add_with_ids(X, ids)
    return X, ids, Q, bounds, shards, whole


def _merged_search(shards, bounds, Q, sel=None):
    from ivr_amd.index import topk_merge
    parts = [s.search_device(Q, K, id_base=lo, sel=sel) for s, (lo, _) in zip(shards, bounds)]     # id_base is carried, and ignored
    return topk_merge(torch.stack([p[0] for p in parts]), torch.stack([p[1] for p in parts]))


def _merged_range(shards, bounds, Q, radius, sel=None):
    from ivr_amd.sharded import merge_range, pack_range
    res = [s.range_search_device(Q, radius, id_base=lo, sel=sel) for s, (lo, _) in zip(shards, bounds)]
    counts = torch.stack([r[0][1:] - r[0][:-1] for r in res])
    width = int(counts.sum(1).max().item())
    packed = torch.stack([pack_range(r[1], r[2], int(r[3].item()), width) for r in res])
    return merge_range(counts, packed)


def _agree(shards, bounds, whole, Q, sel=None):
    from ivr_amd.index import SearchParameters
    Dm, Im = _merged_search(shards, bounds, Q, sel)
    Dw, Iw = whole.search_device(Q, K, sel=sel)
    assert torch.equal(Dm.view(torch.int32), Dw.view(torch.int32)) and torch.equal(Im, Iw)
    lm, Dr, Ir = _merged_range(shards, bounds, Q, 0.12, sel)
    lw, Dwr, Iwr = whole.range_search(Q, 0.12, params=None if sel is None else SearchParameters(sel=sel))
    assert lw[-1] > 0
    assert np.array_equal(lm.cpu().numpy(), lw) and np.array_equal(Ir.cpu().numpy(), Iwr)
    assert np.array_equal(Dr.cpu().numpy().view(np.uint32), Dwr.view(np.uint32))
    return Im.cpu().numpy()


def test_two_id_mapped_shards_agree_with_one_index():
    from ivr_amd.index import IDSelectorBatch, IDSelectorRange
    X, ids, Q, bounds, shards, whole = _setup()
    I = _agree(shards, bounds, whole, Q)
    assert list(I[0, :2]) == [ids[10], ids[2000]]
    batch = IDSelectorBatch(np.concatenate([ids[::3], [int(ids.max()) + 9]]))
    _agree(shards, bounds, whole, Q, batch)
    _agree(shards, bounds, whole, Q, IDSelectorRange(int(ids.min()) + 2 * N, int(ids.min()) + 7 * N))
    # a removal that touches shard 0 only: shard 1 answers with the same labels as before
    before = shards[1].search_device(Q, K)[1].clone()
    victims = ids[5:900:2]
    assert shards[0].remove_ids(victims) == len(victims) and shards[1].remove_ids(victims) == 0
    assert whole.remove_ids(victims) == len(victims)
    assert torch.equal(shards[1].search_device(Q, K)[1], before)
    assert np.array_equal(shards[1].id_map, ids[bounds[1][0]:])
    I = _agree(shards, bounds, whole, Q)
    assert not np.isin(I, victims).any()
    _agree(shards, bounds, whole, Q, batch)
    # and one across both shards, by a selector over stored ids
    sel = IDSelectorRange(int(ids.min()) + 4 * N, int(ids.min()) + 6 * N)
    assert shards[0].remove_ids(sel) + shards[1].remove_ids(sel) == whole.remove_ids(sel) > 0
    _agree(shards, bounds, whole, Q)


def test_world_one_sharded_index_with_ids():
    from ivr_amd.index import FlatIPIndex, IDSelectorBatch, SearchParameters
    from ivr_amd.sharded import ShardedIndex
    X, ids, Q, bounds, shards, whole = _setup()
    one = ShardedIndex(FlatIPIndex(D_), D_)
    one.add_local_with_ids(X, ids)
    assert one.ntotal == N and one.local.has_ids
    Dw, Iw = whole.search_device(Q, K)
    D1, I1 = one.search(Q, K)
    assert torch.equal(I1, Iw) and torch.equal(D1, Dw)
    assert one.remove_ids(ids[100:200]) == 100 and one.ntotal == N - 100
    sel = IDSelectorBatch(ids[::5])
    whole.remove_ids(ids[100:200])
    D1, I1 = one.search(Q, K, params=SearchParameters(sel=sel))
    Dw, Iw = whole.search_device(Q, K, sel=sel)
    assert torch.equal(I1, Iw) and torch.equal(D1, Dw)
