"""Graph index in the place of faiss.IndexHNSWFlat, built and searched in MI355X HBM.

Stands in for the `faiss.IndexHNSWFlat(dimension, 32)` the reference accepts as "IndexHNSW" in `_create_index` (`core.py:1213-1214`).
It is NOT a port of faiss's HNSW and it is parity-unpinned against faiss: faiss inserts one row at a time at random levels, which
can neither be reproduced nor suits this chip.  What is built here is ONE layer of fixed out-degree R = 2 M (HNSW's level-0 width):

  build    exact kNN lists (the storage's own float32 top-k), HNSW's neighbour-selection heuristic over them (ivr_graph_prune),
           then reverse edges (graph_link_ref; integer plumbing in torch)
  entry    a small exactly-searched sample of the rows stands in for HNSW's upper layers: the best n_entry of it start the walk
  search   a best-first walk with a candidate list of ef = max(efSearch, k) rows (ivr_graph_search)

Scores are inner products only, and each carries the bits FlatIPIndex.search gives the same (query, row).  All orders are
(score descending, row ascending), the tie rule of the flat index.  The contract is the four numpy functions below
(graph_prune_ref, graph_link_ref, graph_build_ref, graph_search_ref): the GPU code equals them element for element.

faiss's own default metric for IndexHNSWFlat is L2; on the unit-norm rows the reference stores the ranking is the same and D is the
inner product.
"""
import time

import numpy as np
import torch

from . import _ffi, _staging
from ._faiss import FLT_MAX, METRIC_INNER_PRODUCT, search_numpy, to_numpy, typed_params
from .index import FlatIPIndex, normalize_L2

_KNN_BLOCK = 1 << 16          # rows per kNN search of the build: bounds the query workspace of the storage


# -- the definitions: pure numpy, no GPU ---------------------------------------------------------------------------------------
def _ip(a, b):
    """float32 inner products a @ b.T (accumulated in float64, -0.0 folded onto +0.0 as the index's score keys do)."""
    s = (np.asarray(a, np.float64) @ np.asarray(b, np.float64).T).astype(np.float32)
    return s + np.float32(0)


def _key_order(scores, rows):
    """Positions that put (scores, rows) into (score descending, row ascending) order."""
    return np.lexsort((rows, -scores.astype(np.float64)))


def graph_prune_ref(x, cand, M):
    """HNSW's neighbour-selection heuristic (faiss shrink_neighbor_list with distance -ip, no fill-up with pruned candidates).
    x float32 [n,d]; cand int [n,C]: the candidate rows of every base row r in (score descending, row ascending) order, -1 padded,
    never r itself.  Walk cand[r] in order and keep c iff s(c, g) <= s(r, c) for every g kept so far; stop at M kept.
    Returns (nbr int32 [n,M], nbr_score float32 [n,M]); unused slots are -1 with score 0."""
    x = np.asarray(x, np.float32)
    cand = np.asarray(cand).reshape(len(x), -1)
    n, M = len(x), int(M)
    nbr = np.full((n, M), -1, np.int32)
    sc = np.zeros((n, M), np.float32)
    for r in range(n):
        c = cand[r][(cand[r] >= 0) & (cand[r] < n)]
        if not len(c):
            continue
        xc = x[c]
        g = _ip(xc, xc)
        sb = _ip(x[r:r + 1], xc)[0]
        kept = []
        for i in range(len(c)):
            if not kept or (g[i, kept] <= sb[i]).all():
                kept.append(i)
                if len(kept) == M:
                    break
        nbr[r, :len(kept)] = c[kept]
        sc[r, :len(kept)] = sb[kept]
    return nbr, sc


def graph_link_ref(nbr, nbr_score, R):
    """Reverse edges.  Row c of the graph starts with its forward neighbours nbr[c] in their order; every forward edge r -> c then
    offers r to row c, the offers of one c taken in (score descending, r ascending) order, an r already present skipped, until the
    row holds R entries.  Returns int32 [n,R], -1 padded."""
    nbr = np.asarray(nbr)
    n, R = len(nbr), int(R)
    rows = [[int(v) for v in nbr[c] if v >= 0][:R] for c in range(n)]
    offers = [[] for _ in range(n)]
    for r in range(n):
        for j, c in enumerate(nbr[r]):
            if c >= 0:
                offers[int(c)].append((-float(nbr_score[r][j]), r))
    graph = np.full((n, R), -1, np.int32)
    for c in range(n):
        row = rows[c]
        for _, r in sorted(offers[c]):
            if len(row) >= R:
                break
            if r not in row:
                row.append(r)
        graph[c, :len(row)] = row
    return graph


def graph_knn_ref(x, C):
    """cand int32 [n,C]: the C best rows for query x[r] in (score descending, row ascending) order with row r itself left out (by row
    number, so duplicates of x[r] stay candidates)."""
    x = np.asarray(x, np.float32)
    n = len(x)
    s = _ip(x, x)
    order = np.argsort(-s.astype(np.float64), axis=1, kind="stable")         # ties: the lower row first
    order = order[order != np.arange(n)[:, None]].reshape(n, n - 1)
    return order[:, :C].astype(np.int32)


def graph_build_ref(x, M, efConstruction):
    """The graph GraphFlatIndex.add builds over x: C = min(efConstruction, n - 1) candidates per row (graph_knn_ref), pruned to M
    (graph_prune_ref), linked with R = 2 M (graph_link_ref).  int32 [n, 2 M]; n = 1 gives one row of -1."""
    x = np.asarray(x, np.float32)
    n, M = len(x), int(M)
    C = min(int(efConstruction), n - 1)
    if C < 1:
        return np.full((n, 2 * M), -1, np.int32)
    nbr, sc = graph_prune_ref(x, graph_knn_ref(x, C), M)
    return graph_link_ref(nbr, sc, 2 * M)


def graph_search_ref(x, graph, q, k, ef, entries, max_expansions):
    """Best-first walk.  x float32 [n,d], graph int [n,R], q float32 [nq,d], entries int [nq,ne]; ef >= k.  Per query:
        L := the distinct valid rows of entries (-1 and repeats skipped) with their scores, in key order, cut to ef
        repeat at most max_expansions times:
            cur := the first entry of L not yet expanded; none -> stop
            new := the distinct neighbours of cur (-1 skipped, first occurrence kept) that are not in L now, scored
            L := the first ef of sort(L + new) in key order
    Returns (D float32 [nq,k], I int64 [nq,k], n_expanded int32 [nq]); unused slots are (-FLT_MAX, -1) as FlatIPIndex.search pads.
    There is deliberately no visited set: a row that was rejected or pushed out of a full L has a key below L's worst, and L's
    worst only improves, so offering it again changes nothing."""
    x = np.asarray(x, np.float32)
    q = np.asarray(q, np.float32).reshape(-1, x.shape[1])
    graph, entries = np.asarray(graph), np.asarray(entries).reshape(len(q), -1)
    n, k, ef = len(x), int(k), int(ef)
    D = np.full((len(q), k), -FLT_MAX, np.float32)
    I = np.full((len(q), k), -1, np.int64)
    nexp = np.zeros(len(q), np.int32)

    def distinct(rows, skip):
        out = []
        for r in rows:
            r = int(r)
            if 0 <= r < n and r not in skip and r not in out:
                out.append(r)
        return np.asarray(out, np.int64)

    for i in range(len(q)):
        rows = distinct(entries[i], ())
        sc = _ip(q[i:i + 1], x[rows])[0] if len(rows) else np.zeros(0, np.float32)
        o = _key_order(sc, rows)[:ef]
        rows, sc, done = rows[o], sc[o], np.zeros(len(o), bool)
        for _ in range(int(max_expansions)):
            todo = np.flatnonzero(~done)
            if not len(todo):
                break
            cur = todo[0]
            done[cur] = True
            nexp[i] += 1
            new = distinct(graph[rows[cur]], set(rows.tolist()))
            if not len(new):
                continue
            rows = np.concatenate([rows, new])
            sc = np.concatenate([sc, _ip(q[i:i + 1], x[new])[0]])
            done = np.concatenate([done, np.zeros(len(new), bool)])
            o = _key_order(sc, rows)[:ef]
            rows, sc, done = rows[o], sc[o], done[o]
        m = min(k, len(rows))
        D[i, :m], I[i, :m] = sc[:m], rows[:m]
    return D, I, nexp


def entry_sample(ntotal, entry_sample=4096, seed=1234):
    """The rows of the entry index: sort(RandomState(seed).permutation(ntotal)[:min(ntotal, entry_sample)]), int64."""
    return np.sort(np.random.RandomState(seed).permutation(int(ntotal))[:min(int(ntotal), int(entry_sample))]).astype(np.int64)


# -- the link step on the device -------------------------------------------------------------------------------------------------
def link_device(nbr, nbr_score, R):
    """graph_link_ref on CUDA tensors (nbr int32 [n,M] with the kept neighbours in front and distinct, nbr_score float32 [n,M]) ->
    int32 [n,R], M <= R.  Integer plumbing: an offer whose src is already a forward neighbour of dst is taken out, the edge list (src
    ascending as it is made) is put into (dst, score descending, src) order by two stable sorts, and an offer's slot is the forward
    count of dst plus its rank in the run."""
    n, M = nbr.shape
    R = int(R)
    if M > R:
        raise ValueError(f"link_device: M={M} > R={R}")
    dev = nbr.device
    graph = torch.full((n, R), -1, dtype=torch.int32, device=dev)
    graph[:, :M] = nbr
    valid = nbr >= 0
    src = torch.arange(n, dtype=torch.int64, device=dev).unsqueeze(1).expand(n, M)[valid]        # ascending
    dst = nbr[valid].to(torch.int64)
    sc = nbr_score[valid]
    present = torch.isin(dst * n + src, src * n + dst)       # dst -> src is a forward edge: src already sits in row dst
    src, dst, sc = src[~present], dst[~present], sc[~present]
    o = torch.sort(sc, descending=True, stable=True).indices                                    # src stays ascending within a score
    src, dst = src[o], dst[o]
    o = torch.sort(dst, stable=True).indices
    src, dst = src[o], dst[o]
    first = torch.cumsum(torch.bincount(dst, minlength=n), 0) - torch.bincount(dst, minlength=n)
    slot = valid.sum(1)[dst] + torch.arange(len(dst), dtype=torch.int64, device=dev) - first[dst]
    ok = slot < R
    graph[dst[ok], slot[ok]] = src[ok].to(torch.int32)
    return graph


class _HNSWKnobs:
    """faiss's index.hnsw: efConstruction, efSearch, plus the knobs of this implementation."""

    def __init__(self):
        self._efc = 40
        self.efSearch = 16
        self.max_expansions = 0       # 0: 8 * ef
        self.n_entry = 8
        self.entry_sample = 4096

    @property
    def efConstruction(self):
        return self._efc

    @efConstruction.setter
    def efConstruction(self, v):
        if not 1 <= int(v) <= _ffi.IVR_GRAPH_MAX_CAND:
            raise ValueError(f"efConstruction={v} outside [1,{_ffi.IVR_GRAPH_MAX_CAND}]")
        self._efc = int(v)


class SearchParametersHNSW:
    """faiss.SearchParametersHNSW(efSearch=..., sel=...): efSearch overrides the index attribute for one call.  Selectors are not
    supported on GraphFlatIndex: search raises ValueError when sel is set."""

    def __init__(self, efSearch=None, sel=None):
        if efSearch is not None and int(efSearch) < 1:
            raise ValueError(f"SearchParametersHNSW: efSearch={efSearch} < 1")
        self.efSearch = None if efSearch is None else int(efSearch)
        self.sel = sel


class GraphFlatIndex(_ffi.Handle):
    """Single-layer graph index with exact float32 inner-product scores on one GPU, in the place of faiss IndexHNSWFlat (see the
    module docstring: not a port, parity-unpinned against faiss; the contract is graph_build_ref / graph_search_ref).

    search(x, k) returns (D, I) under the contract of FlatIPIndex.search: float32 descending, int64 row numbers, -1 padding.  Rows
    are labelled by position.  Every add() call rebuilds the graph over ALL stored rows (kNN lists, prune, link): add in large
    batches."""
    _DESTROY = "ivr_graph_destroy"

    def __init__(self, d, M=32, device=None):
        self.d, self.M = int(d), int(M)
        if self.d < 1 or not 1 <= 2 * self.M <= _ffi.IVR_GRAPH_MAX_DEGREE:
            raise ValueError(f"GraphFlatIndex: d={d} M={M} (2 M at most {_ffi.IVR_GRAPH_MAX_DEGREE})")
        self._storage = FlatIPIndex(self.d, device=device)
        self._entry = FlatIPIndex(self.d, device=self._storage.device.index)
        self.metric_type = METRIC_INNER_PRODUCT
        self.is_trained = True
        self.hnsw = _HNSWKnobs()
        self.build_times = {}         # seconds of the last add(): knn / prune / link
        self._open("ivr_graph_create", self._storage.device.index, self.d, 2 * self.M)
        self._graph = torch.zeros((0, 2 * self.M), dtype=torch.int32, device=self.device)

    @property
    def ntotal(self):
        return self._storage.ntotal

    # -- build -----------------------------------------------------------------------------------
    def add(self, x, normalize=False, graph=None):
        """Append rows labelled ntotal, ntotal + 1, ... and rebuild the graph over all stored rows.  graph: the neighbour table an
        earlier build made over the same rows (graph(), e.g. saved with numpy.save); it is installed through set_graph, with its
        checks, in place of the kNN / prune / link steps."""
        _staging.check_rows(x, self.d, "add")
        if len(x) == 0:
            return
        if graph is not None:
            graph = self._checked_graph(graph, self.ntotal + len(x), "add")      # refused before any row is stored
        self._storage.add(x, normalize=normalize)
        self._build(graph)

    def _timed(self, name, t0):
        torch.cuda.current_stream().synchronize()
        now = time.perf_counter()
        self.build_times[name] = self.build_times.get(name, 0.0) + now - t0
        return now

    def _build(self, graph=None):
        """Rows, neighbour table and entry sample over all stored rows.  graph: a checked table (_checked_graph) that is installed in
        place of the kNN / prune / link steps."""
        n, M, st = self.ntotal, self.M, self._storage
        Cn = min(self.hnsw.efConstruction, n - 1)
        self.build_times = {}
        with torch.cuda.device(self.device):
            allrows = torch.arange(n, dtype=torch.int64, device=self.device)
            torch.cuda.current_stream().synchronize()
            t0 = time.perf_counter()
            # the graph's own row-major copy; the gathered rows are dropped again before the kNN lists are made
            rows = torch.cat([st.gather_device(allrows[i:i + _KNN_BLOCK]) for i in range(0, n, _KNN_BLOCK)]) if n > _KNN_BLOCK \
                else st.gather_device(allrows)
            self._call("ivr_graph_set_rows", rows, n)
            del rows                                     # same stream: the block is not reused before the copy has run
            if graph is not None:
                self._install(graph)
            elif Cn < 1:
                self._install(torch.full((n, 2 * M), -1, dtype=torch.int32, device=self.device))
            else:
                cand = torch.empty((n, Cn), dtype=torch.int32, device=self.device)
                for i in range(0, n, _KNN_BLOCK):
                    blk = allrows[i:i + _KNN_BLOCK]
                    I = st.search_device(st.gather_device(blk), Cn + 1)[1]
                    own = I == blk.unsqueeze(1)
                    own[~own.any(1), -1] = True          # the own row is absent among duplicates: the last entry goes
                    cand[i:i + _KNN_BLOCK] = I[~own].view(-1, Cn).to(torch.int32)
                t0 = self._timed("knn", t0)
                nbr = torch.empty((n, M), dtype=torch.int32, device=self.device)
                nsc = torch.empty((n, M), dtype=torch.float32, device=self.device)
                self._call("ivr_graph_prune", cand, Cn, M, nbr, nsc)
                t0 = self._timed("prune", t0)
                self._install(link_device(nbr, nsc, 2 * M))
                self._timed("link", t0)
            # the entry index: an exactly-searched sample that returns row numbers
            er = entry_sample(n, self.hnsw.entry_sample)
            self._entry.reset()
            ert = torch.from_numpy(er).to(self.device)
            self._entry._add_device(st.gather_device(ert), False, er)

    def _install(self, graph):
        graph = graph.contiguous()
        self._call("ivr_graph_set_neighbors", graph, len(graph))
        self._graph = graph

    def graph(self):
        """The neighbour table, numpy int32 [ntotal, 2 M], -1 padded."""
        return self._graph.cpu().numpy()

    def set_graph(self, graph):
        """Install a caller-made neighbour table: integers [ntotal, 2 M] (numpy or torch).  ValueError for a wrong shape, a non-integer
        dtype or an entry >= ntotal or < -1, checked on the tensor before anything is launched."""
        self._install(self._checked_graph(graph, self.ntotal, "set_graph"))

    def _checked_graph(self, graph, n, who):
        """graph as an int32 tensor [n, 2 M] on the device, or ValueError."""
        graph = _staging.int_tensor(graph, f"{who}: the graph", "hold")
        if tuple(graph.shape) != (n, 2 * self.M):
            raise ValueError(f"{who}: expected [{n},{2 * self.M}], got {tuple(graph.shape)}")
        with torch.cuda.device(self.device):
            graph = graph.to(self.device)
            if graph.numel():
                _staging.check_entries(graph, n, f"{who}: entries")
            return graph.to(torch.int32)

    # -- search ----------------------------------------------------------------------------------
    def _queries(self, x, k):
        t, staged = _staging.queries_f32(_staging.as_rows(x), self.d, self.device)
        k = _staging.check_k(k, _ffi.IVR_GRAPH_MAX_EF)
        _staging.check_nq(t.shape[0])
        return t, k, staged

    def search(self, x, k, params=None):
        """(D, I) numpy arrays under the contract of FlatIPIndex.search.  params = SearchParametersHNSW(efSearch=...) overrides
        efSearch for this call; a selector raises ValueError."""
        params = typed_params(params, SearchParametersHNSW, "GraphFlatIndex")
        return search_numpy(self, x, k, efSearch=None if params is None else params.efSearch)

    def search_device(self, x, k, normalize=False, efSearch=None):
        """Device-resident search: CUDA tensors.  The entries are the best n_entry rows of the entry sample for each query.
        normalize: a copy of the queries is L2-normalised once (normalize_L2) and serves the entry search and the walk."""
        t, k, staged = self._queries(x, k)
        with torch.cuda.device(self.device):
            if self.ntotal == 0:
                return (torch.full((t.shape[0], k), -FLT_MAX, dtype=torch.float32, device=self.device),
                        torch.full((t.shape[0], k), -1, dtype=torch.int64, device=self.device))
            if normalize:
                t = t.clone()
                normalize_L2(t)
            ne = max(1, min(int(self.hnsw.n_entry), self._entry.ntotal, _ffi.IVR_GRAPH_MAX_DEGREE))
            entries = self._entry.search_device(t, ne)[1].to(torch.int32)
            D, I, _ = self._walk(t, k, entries, efSearch, None)
            _staging.sync_if_staged(staged)
        return D, I

    def search_from(self, x, k, entries, efSearch=None, max_expansions=None, return_stats=False, normalize=False):
        """The walk from caller-chosen entries: integers [nq, ne] (ne <= 64; -1 and repeats are skipped, as are rows outside the
        index).  normalize: ivr_graph_search L2-normalises the queries itself (normalize_q).  Returns numpy (D, I), and with
        return_stats also n_expanded int32 [nq]."""
        t, k, _ = self._queries(x, k)
        e = _staging.entry_table(entries, t.shape[0], _ffi.IVR_GRAPH_MAX_DEGREE, "search_from")
        with torch.cuda.device(self.device):
            D, I, nexp = self._walk(t, k, torch.from_numpy(e).to(self.device), efSearch, max_expansions, normalize)
            return to_numpy((D, I, nexp) if return_stats else (D, I))

    def _walk(self, t, k, entries, efSearch, max_expansions, normalize=False):
        ef = max(int(self.hnsw.efSearch if efSearch is None else efSearch), k)
        if ef < 1 or ef > _ffi.IVR_GRAPH_MAX_EF:
            raise ValueError(f"efSearch={ef} outside [1,{_ffi.IVR_GRAPH_MAX_EF}]")
        mx = int(self.hnsw.max_expansions if max_expansions is None else max_expansions)
        if mx <= 0:
            mx = 8 * ef
        nq = t.shape[0]
        entries = entries.contiguous()
        D, I = _staging.alloc_DI(nq, k, self.device)
        nexp = torch.empty(nq, dtype=torch.int32, device=self.device)
        self._call("ivr_graph_search", t, nq, k, ef, entries, entries.shape[1], min(mx, 2**31 - 1), bool(normalize), D, I, nexp)
        return D, I, nexp

    # -- maintenance -----------------------------------------------------------------------------
    def reconstruct(self, i):
        return self._storage.reconstruct(i)

    def reconstruct_n(self, start=0, n=None):
        return self._storage.reconstruct_n(start, n)

    def reset(self):
        """Drop the rows, the graph and the entry sample."""
        self._storage.reset()
        self._entry.reset()
        self._call("ivr_graph_reset")
        self._graph = torch.zeros((0, 2 * self.M), dtype=torch.int32, device=self.device)

    def close(self):
        """Release the index (storage, entry sample and graph)."""
        for x in (getattr(self, "_storage", None), getattr(self, "_entry", None)):
            if x is not None:
                x.close()
        super().close()


def IndexHNSWFlat(d, M=32, metric=METRIC_INNER_PRODUCT):
    """faiss.IndexHNSWFlat(d, M, faiss.METRIC_INNER_PRODUCT) in name and knobs (see GraphFlatIndex for what it is instead).  ValueError
    for a metric other than inner product: faiss's own default for this class is METRIC_L2, which on unit-norm rows ranks the same."""
    if metric != METRIC_INNER_PRODUCT:
        raise ValueError(f"IndexHNSWFlat: only METRIC_INNER_PRODUCT ({METRIC_INNER_PRODUCT}) is supported, got {metric}")
    return GraphFlatIndex(d, M)
