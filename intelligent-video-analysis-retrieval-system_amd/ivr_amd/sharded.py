"""Row-sharded exact search across the GPUs of one node (one process per GPU).

MI355X-native replacement of the reference's only distributed pattern - scatter the
query vector to peers over HTTP, gather their top-k lists, concatenate and sort
(`system.py:1715-1757`, `api.py:877-925`): here every rank owns a contiguous row
range of the index in its own HBM, the (small) query batch is replicated, each rank
scans its shard, and ONE all-gather of the per-shard (score, global id) candidates
over RCCL/xGMI (`torch.distributed`, backend "nccl") is followed by a k-way merge.
The message is nq*k*12 bytes per rank (1000x10 -> 120 KB): latency-bound, so a single
collective is the right shape; no other exchange exists on this path.

The class is agnostic of how a shard is searched: `local` only needs
`search_device(q, k, normalize=, id_base=) -> (D, I)` tensors, `add`, `ntotal` (and
`range_search_device(q, radius, normalize=, id_base=) -> (lims, D, I, total)` for range_search; both with `sel=` for a filtered
search; `remove_ids(sel, id_base=) -> int` for remove_ids; `reconstruct_batch_device(keys) -> (rows, R)` and `has_ids` for
reconstruct_batch).  On GPUs that
is `ivr_amd.index.FlatIPIndex`; the world_size-2 gloo tests on CPU plug the oracle in.
"""
import numpy as np
import torch
import torch.distributed as dist

NEG_FLT_MAX = -3.4028234663852886e38


def shard_bounds(n_rows, world_size):
    """Contiguous row ranges [lo, hi) per rank; the first n_rows % world_size ranks take one extra row."""
    base, extra = divmod(int(n_rows), int(world_size))
    out, lo = [], 0
    for r in range(world_size):
        hi = lo + base + (1 if r < extra else 0)
        out.append((lo, hi))
        lo = hi
    return out


def merge_host(D_parts, I_parts, k):
    """Host-side final merge (north_star): D_parts/I_parts [G,nq,k] with global ids, shards in ascending id
    order.  Sort by score descending, ties to the lower id; unused slots are (-FLT_MAX, -1)."""
    D_parts = D_parts.detach().cpu()
    I_parts = I_parts.detach().cpu()
    G, nq, kk = D_parts.shape
    d = D_parts.permute(1, 0, 2).reshape(nq, G * kk)
    i = I_parts.permute(1, 0, 2).reshape(nq, G * kk)
    d = torch.where(i >= 0, d, torch.full_like(d, float("-inf")))
    # stable sort on the score keeps candidate order among ties = ascending (shard, rank) = ascending id
    order = torch.sort(d, dim=1, descending=True, stable=True).indices
    # a candidate whose score IS -inf ties with the unused slots: a second stable pass puts every candidate before every unused slot
    valid_first = torch.sort((torch.gather(i, 1, order) < 0).to(torch.int8), dim=1, stable=True).indices
    order = torch.gather(order, 1, valid_first)[:, :k]
    D = torch.gather(d, 1, order)
    I = torch.gather(i, 1, order)
    D = torch.where(I >= 0, D, torch.full_like(D, NEG_FLT_MAX))
    if D.shape[1] < k:
        pad = k - D.shape[1]
        D = torch.cat([D, torch.full((nq, pad), NEG_FLT_MAX)], 1)
        I = torch.cat([I, torch.full((nq, pad), -1, dtype=torch.int64)], 1)
    return D, I


def pack_range(D, I, n, width):
    """The first n range-search results of one shard -> int32 [width, 3] (score bits, id lo, id hi), zero padded: the wire format
    of the range search's all-gather."""
    cand = torch.zeros((width, 3), dtype=torch.int32, device=D.device)
    if n:
        cand[:n, 0] = D[:n].contiguous().view(torch.int32)
        cand[:n, 1] = (I[:n] & 0xFFFFFFFF).to(torch.int32)      # low word, wrapped into int32
        cand[:n, 2] = (I[:n] >> 32).to(torch.int32)
    return cand


def merge_range(counts, packed):
    """Merge per-shard range-search results: counts int64 [parts, nq] (results per query of each shard), packed int32
    [parts, width, 3] (pack_range of each shard), parts in ascending id order -> (lims [nq+1], D, I).  Query i's results are the
    shards' parts for query i in shard order, so ids stay ascending; only index arithmetic, no sort."""
    parts, nq = counts.shape
    dev = packed.device
    lims = torch.zeros(nq + 1, dtype=torch.int64, device=dev)
    lims[1:] = torch.cumsum(counts.sum(0), 0)
    totals = counts.sum(1)
    # entry e of shard r that belongs to query i goes to lims[i] + (results of lower shards for query i) + (e - shard r's start of i)
    before = torch.cumsum(counts, 0) - counts
    starts = torch.cumsum(counts, 1) - counts
    shift = (lims[:-1].unsqueeze(0) + before - starts).reshape(-1)
    qid = torch.arange(parts * nq, device=dev).repeat_interleave(counts.reshape(-1))      # (shard, query) of each entry
    local_e = torch.arange(qid.numel(), device=dev) - (torch.cumsum(totals, 0) - totals).repeat_interleave(totals)
    flat = packed[qid // nq, local_e]
    total = qid.numel()
    D = torch.empty(total, dtype=torch.float32, device=dev)
    I = torch.empty(total, dtype=torch.int64, device=dev)
    dest = shift[qid] + local_e
    D[dest] = flat[:, 0].contiguous().view(torch.float32)
    I[dest] = (flat[:, 1].to(torch.int64) & 0xFFFFFFFF) | (flat[:, 2].to(torch.int64) << 32)
    return lims, D, I


class ShardedIndex:
    """Shards built with add_local label their rows id_base + row, and id_base follows the counts of the lower ranks.  Shards built
    with add_local_with_ids (id-mapped, FlatIPIndex.add_with_ids) carry the global ids themselves: id_base is still kept up to date
    and passed down but unused, the ids a search returns and the ids a selector or remove_ids names are the stored ones on every
    rank, and a removal on one rank changes no id on another.  Candidates still merge in rank order, so equal scores rank the
    lower rank's row first."""

    def __init__(self, local, d, group=None, merge="device"):
        self.local = local
        self.d = int(d)
        self.group = group
        self.merge = merge
        self.rank = dist.get_rank(group) if dist.is_initialized() else 0
        self.world = dist.get_world_size(group) if dist.is_initialized() else 1
        self.id_base = 0
        self._counts = [0] * self.world

    # -- build -------------------------------------------------------------------------------
    def add_local(self, rows, normalize=False):
        """Append this rank's rows, then agree on every shard's global id offset (one tiny all-gather of counts;
        build-time only, never on the search path)."""
        self.local.add(rows, normalize=normalize) if normalize else self.local.add(rows)
        self.sync_counts()

    def add_local_with_ids(self, rows, ids, normalize=False):
        """Append this rank's rows under global ids of the caller's choosing (local.add_with_ids), then agree on the counts."""
        self.local.add_with_ids(rows, ids, normalize=normalize) if normalize else self.local.add_with_ids(rows, ids)
        self.sync_counts()

    def sync_counts(self):
        n = int(self.local.ntotal)
        if self.world > 1:
            counts = [None] * self.world
            dist.all_gather_object(counts, n, group=self.group)
        else:
            counts = [n]
        self._counts = [int(c) for c in counts]
        self.id_base = int(sum(self._counts[:self.rank]))

    @property
    def ntotal(self):
        return int(sum(self._counts))

    def remove_ids(self, sel):
        """faiss remove_ids(sel) over all shards: sel names GLOBAL ids (a selector, or an integer array as FlatIPIndex.remove_ids takes
        it).  Every rank removes its own rows, then the counts are agreed on again (sync_counts: the one collective, as after
        add_local), so each shard's id_base follows the rows that left the shards below it.  Returns the global number of removed
        rows, identical on every rank: the difference of the summed counts.  Shards are not re-balanced.  On id-mapped shards sel names
        stored ids and the ids of the surviving rows stay as they are on every rank."""
        before = self.ntotal
        self.local.remove_ids(sel, id_base=self.id_base)
        self.sync_counts()
        return before - self.ntotal

    def reconstruct_batch(self, ids):
        """faiss reconstruct_batch over all shards: ids [n] GLOBAL ids, replicated on every rank -> numpy float32 [n,d], identical on
        every rank.  Plain shards: an id is a global row and belongs to the shard whose synced bounds hold it.  Id-mapped shards: the
        lowest rank that stores the id answers, with its lowest row under it: the lowest global storage position.  Two collectives:
        an all-gather of the found flags (n int64 per rank), then ONE all-gather of every rank's rows, n * d * world floats in all:
        meant for result-list sizes, not for bulk export.  RuntimeError on every rank, after both collectives (no rank is left
        waiting), when an id names no row."""
        keys = torch.from_numpy(np.ascontiguousarray(np.asarray(ids).reshape(-1).astype(np.int64)))
        # plain shards: global row -> this shard's row; the rows of other shards fall outside [0, ntotal) and come back as -1
        local_keys = keys if getattr(self.local, "has_ids", False) else keys - self.id_base
        rows, R = self.local.reconstruct_batch_device(local_keys)
        n = keys.numel()
        found = (rows >= 0).to(torch.int64).contiguous()
        R = R.contiguous()
        if self.world > 1:
            found_all = torch.empty(self.world * n, dtype=torch.int64, device=found.device)
            dist.all_gather_into_tensor(found_all, found, group=self.group)
            R_all = torch.empty((self.world * n, self.d), dtype=torch.float32, device=R.device)
            dist.all_gather_into_tensor(R_all, R, group=self.group)
            found_all, R_all = found_all.view(self.world, n), R_all.view(self.world, n, self.d)
        else:
            found_all, R_all = found.view(1, n), R.view(1, n, self.d)
        ranks = torch.arange(self.world, device=found_all.device).unsqueeze(1)
        owner = torch.where(found_all > 0, ranks, torch.full_like(ranks, self.world)).min(0).values      # the lowest rank that holds the id
        missing = torch.nonzero(owner == self.world).reshape(-1).cpu()
        if missing.numel():
            raise RuntimeError(f"reconstruct_batch: id {int(keys[missing[0]])} is not in the index ({missing.numel()} of {n} missing)")
        return R_all[owner, torch.arange(n, device=owner.device)].cpu().numpy()

    # -- search ------------------------------------------------------------------------------
    @staticmethod
    def _sel_kw(params):
        """params (SearchParameters or None) -> the sel= keyword of the local call.  The selector names GLOBAL ids; each rank's id_base
        carries its shard offset, so the same selector is valid on every rank and no extra exchange is needed."""
        if params is None:
            return {}
        from .index import _selector
        sel = _selector(params)
        return {} if sel is None else {"sel": sel}

    def search(self, q, k, normalize=False, params=None):
        """q [nq,d] replicated on every rank -> (D [nq,k], I [nq,k] global ids), identical on every rank.  params =
        SearchParameters(sel=...) over global ids: the top k among the allowed ids of all shards."""
        D, I = self.local.search_device(q, k, normalize=normalize, id_base=self.id_base, **self._sel_kw(params))
        return self.exchange(D, I)

    def range_search(self, q, radius, normalize=False, params=None):
        """Exact range search over all shards: q [nq,d] replicated on every rank -> (lims [nq+1], D, I global ids), identical on
        every rank and laid out like FlatIPIndex.range_search (ids ascending within a query).  Two collectives: an all-gather of the
        per-query counts, then ONE all-gather of the packed (score, id) results padded to the largest rank's total.  Shards are
        contiguous and ascending, so concatenating each query's parts in rank order keeps its ids ascending: no sort."""
        lims, D, I, _ = self.local.range_search_device(q, radius, normalize=normalize, id_base=self.id_base, **self._sel_kw(params))
        if self.world == 1:
            return lims, D, I
        nq = lims.numel() - 1
        dev = lims.device
        counts = (lims[1:] - lims[:-1]).contiguous()
        counts_all = torch.empty(self.world * nq, dtype=torch.int64, device=dev)
        dist.all_gather_into_tensor(counts_all, counts, group=self.group)
        counts_all = counts_all.view(self.world, nq)
        totals = counts_all.sum(1)
        width = int(totals.max().item())
        if width == 0:
            return merge_range(counts_all, torch.empty((self.world, 0, 3), dtype=torch.int32, device=dev))
        gathered = torch.empty((self.world * width, 3), dtype=torch.int32, device=dev)
        dist.all_gather_into_tensor(gathered, pack_range(D, I, int(totals[self.rank].item()), width), group=self.group)
        return merge_range(counts_all, gathered.view(self.world, width, 3))

    def exchange(self, D, I):
        """The single exchange step of the path: this rank's candidates (D [nq,k] scores, I [nq,k] GLOBAL ids, unused slots -1)
        -> the merged top-k over all shards, identical on every rank.  ONE all-gather of nq*k*12 bytes per rank - (score f32,
        id i64) packed as three int32 words per candidate - then the k-way merge.  Enqueued on the current stream (RCCL work is
        stream-ordered), so it can follow a replayed HIP graph that produced D and I (streaming.StreamingSession)."""
        if self.world == 1:
            return D, I
        nq, k = D.shape
        if self.merge == "device" and D.is_cuda:
            # pack (one launch) -> the all-gather -> merge straight from the gathered buffer (one launch)
            from .index import topk_merge_packed, topk_pack
            cand = topk_pack(D, I)
            gathered = torch.empty((self.world * nq, k, 3), dtype=torch.int32, device=D.device)     # concatenated along dim 0
            dist.all_gather_into_tensor(gathered, cand, group=self.group)
            return topk_merge_packed(gathered.view(self.world, nq, k, 3))
        cand = torch.empty((nq, k, 3), dtype=torch.int32, device=D.device)
        cand[..., 0] = D.contiguous().view(torch.int32)
        cand[..., 1:] = I.contiguous().view(torch.int32).view(nq, k, 2)
        gathered = torch.empty((self.world * nq, k, 3), dtype=torch.int32, device=D.device)
        dist.all_gather_into_tensor(gathered, cand, group=self.group)
        gathered = gathered.view(self.world, nq, k, 3)
        Dg = gathered[..., 0].contiguous().view(torch.float32)
        Ig = gathered[..., 1:].contiguous().view(torch.int64).view(self.world, nq, k)
        return merge_host(Dg, Ig, k)


def stride_frames(n_frames, rank, world):
    """Frame i is embedded on GPU i mod G: indices owned by `rank`."""
    return np.arange(rank, n_frames, world)
