#!/usr/bin/env python3
"""GraphFlatIndex (IndexHNSWFlat's place) against FlatIPIndex on the same rows: wall time of add split into kNN / prune / link, and
per (nq, efSearch) the time of a search, the mean expansions per query and recall@10 against the flat search.

    python tools/bench_graph.py [--rows 1000000] [--M 32] [--timeout-build S] [--timeout-measure S] [--workdir DIR]

Rows: `--rows` x 512 unit-norm float32 around 1000 random unit centres, row = normalize(centre[j] + g / sqrt(d)) with j uniform and g
standard normal, drawn on the device by torch.Generator(device="cuda").manual_seed(1234) in blocks of 250,000 rows: centres first,
then per block j and g (the rows of tools/bench_ivf.py and tools/bench_lsh.py).  Queries: 1000 more rows of the same distribution
from manual_seed(4321), the first nq of them.  The kNN lists of the build are an exact top-(efConstruction + 1) search of every row
against every row: rows^2 pairs, so the build time grows with the square of --rows.  The time limit of the build step is sized to
that: three times rows^2 / KNN_PAIRS_PER_S (the rate the build of 1M rows reached in profiles/r16a_bench_graph.log), at least 300 s.

The run is a chain of steps, each a child process of its own under `timeout`; a step that fails ends the chain.  The graph is built
once: the build step leaves the neighbour table in --workdir (a temporary directory by default, removed at the end) and the measure
step installs it over the same rows instead of building again.
    build          generate, one add() of all rows: wall seconds of kNN / prune / link (GraphFlatIndex.build_times), out-degree
    measure        generate, store the rows in both indexes, install the table, and per nq in (1, 10, 1000) and efSearch in (16, 64,
                   256), k = 10: 3 warm-up calls, then the median over repeated calls (queries resident on the device) of the time
                   between two device events around GraphFlatIndex.search_device (entry search included) and around
                   FlatIPIndex.search_device; the mean expansions per query (search_from with the same entries) and recall@10 =
                   |graph top-10 & flat top-10| / 10 over the nq queries"""
import argparse
import os
import shutil
import subprocess
import sys
import tempfile

KNN_PAIRS_PER_S = 715e9       # measured: the top-41 lists of 1M x 512 rows took 1.40 s (profiles/r16a_bench_graph.log)

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=1_000_000)
ap.add_argument("--M", type=int, default=32)
ap.add_argument("--timeout-build", type=int, default=None, help="seconds for the build step (default: sized to --rows)")
ap.add_argument("--timeout-measure", type=int, default=600, help="seconds for the measure step")
ap.add_argument("--workdir", default=None, help="where the build step leaves the neighbour table for the measure step")
ap.add_argument("--step", default=None, help="internal: build | measure")
args = ap.parse_args()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D, NCENT, NQS, EFS, K = 512, 1000, (1, 10, 1000), (16, 64, 256), 10

if args.step is None:
    t_build = args.timeout_build or max(300, int(3 * args.rows * args.rows / KNN_PAIRS_PER_S))
    work = args.workdir or tempfile.mkdtemp(prefix="bench_graph_")
    rc = 0
    try:
        for step, limit in (("build", t_build), ("measure", args.timeout_measure)):
            rc = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--rows", str(args.rows),
                                 "--M", str(args.M), "--workdir", work, "--step", step]).returncode
            if rc != 0:
                print(f"step {step} (limit {limit} s) ended with status {rc}: stopping", flush=True)
                break
    finally:
        if args.workdir is None:
            shutil.rmtree(work, ignore_errors=True)
    sys.exit(rc)

sys.path.insert(0, os.path.join(ROOT, "intelligent-video-analysis-retrieval-system_amd"))
import time  # noqa: E402

import numpy as np  # noqa: E402
import torch  # noqa: E402

from ivr_amd.graph import GraphFlatIndex  # noqa: E402
from ivr_amd.index import FlatIPIndex  # noqa: E402

assert torch.cuda.is_available(), "bench_graph.py needs a GPU"
N = args.rows


def draw(g, centres, n):
    j = torch.randint(0, len(centres), (n,), generator=g, device="cuda")
    x = centres[j] + torch.randn((n, D), generator=g, device="cuda") / D ** 0.5
    return x / x.norm(dim=1, keepdim=True)


def rows():
    g = torch.Generator(device="cuda").manual_seed(1234)
    c = torch.randn((NCENT, D), generator=g, device="cuda")
    c = c / c.norm(dim=1, keepdim=True)
    return c, torch.cat([draw(g, c, min(250_000, N - i)) for i in range(0, N, 250_000)])


def event_ms(fn, budget_s=1.0):
    """median ms between two device events around fn(), after 3 warm-up calls; enough repeats to fill budget_s, 5 to 100"""
    for _ in range(3):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ts = []
    reps = 5
    while len(ts) < reps:
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
        if len(ts) == 1:
            reps = int(min(100, max(5, budget_s * 1e3 / max(ts[0], 1e-3))))
    ts.sort()
    return ts[len(ts) // 2], len(ts)


centres, X = rows()
idx = GraphFlatIndex(D, M=args.M)
TABLE = os.path.join(args.workdir, f"graph_{N}_{args.M}.npy")
if args.step == "build":
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    idx.add(X)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    bt = idx.build_times
    np.save(TABLE, idx.graph())
    deg = (idx._graph >= 0).sum(1).float()
    print(f"# bench_graph: {N} x {D} rows around {NCENT} centres, M = {args.M} (degree {2 * args.M}), efConstruction = {idx.hnsw.efConstruction}",
          flush=True)
    print(f"add ({N} rows, one call): {wall:.2f} s wall; kNN {bt.get('knn', 0):.2f} s ({N * N / max(bt.get('knn', 0), 1e-9) / 1e9:.0f} G pairs/s), "
          f"prune {bt.get('prune', 0):.3f} s, link {bt.get('link', 0):.3f} s; out-degree mean {deg.mean().item():.2f}, "
          f"max {int(deg.max().item())}, rows at full degree {(deg == 2 * args.M).float().mean().item():.4f}", flush=True)
    sys.exit(0)

idx.add(X, graph=np.load(TABLE))  # the rows without a build of their own: the table of the build step goes in
flat = FlatIPIndex(D, capacity=N)
flat.add(X)
del X
Qall = draw(torch.Generator(device="cuda").manual_seed(4321), centres, 1000)
print(" nq |  ef | graph search ms (reps) | per query | expansions | recall@10 | flat search ms (reps) | graph / flat", flush=True)
for nq in NQS:
    Q = Qall[:nq].contiguous()
    t_flat, reps_f = event_ms(lambda: flat.search_device(Q, K))
    If = flat.search_device(Q, K)[1].cpu().numpy()
    entries = idx._entry.search_device(Q, idx.hnsw.n_entry)[1].cpu().numpy()
    for ef in EFS:
        t_g, reps = event_ms(lambda: idx.search_device(Q, K, efSearch=ef))
        Ig = idx.search_device(Q, K, efSearch=ef)[1].cpu().numpy()
        nexp = idx.search_from(Q, K, entries, efSearch=ef, return_stats=True)[2]
        recall = float(np.mean([len(set(If[i]) & set(Ig[i])) / K for i in range(nq)]))
        print(f"{nq:4d} | {ef:3d} | {t_g:15.4f} ({reps:3d}) | {t_g / nq:9.5f} | {nexp.mean():10.1f} | {recall:9.4f} | {t_flat:14.4f} ({reps_f:3d}) | "
              f"{t_g / t_flat:8.3f}", flush=True)
