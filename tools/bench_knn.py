#!/usr/bin/env python3
"""The neighbour graph (ivr_amd/neighbors.py) against the two routes to the same lists that exist without it.

    python tools/bench_knn.py [--sizes 20000:1,20000:100,100000:1,100000:200,1000000:2000] [--timeout 600] [--no-graph] [--only-knn]

A size is rows:segments; the rows are cut into that many equal folders.  Rows: 512-d unit-norm float32, drawn on the device by
torch.Generator(device="cuda").manual_seed(1234): every 20 consecutive rows are one static shot, row = normalize(centre + 0.2 g /
sqrt(d)) around a random unit centre of their own (cosine about 0.96 inside a shot, about 0 between shots), so a threshold of 0.7 keeps
the 19 other rows of the shot.  k = 10, threshold 0.7 and none.

Every size is measured by one child process under `timeout`, one after the other; the first one that fails ends the run.  It reports
    knn_graph  knn_graph_device(index, 10, seg_off, threshold): median time between two device events over at least 5 calls after 2
               warm-up calls, offsets resident on the device; then the kernels of one profiled call (event pairs around the score
               kernel lengthen the call: read them as shares)
    (a)        filters.similarity_graph folder by folder on the host copy of the rows: one temporary index per folder, every row a
               query, the result copied back, the dict built on the host; host wall clock of one pass (best of 2 up to 100,000 rows)
    (b)        one segment only: search_device(gather_device(block), k + 1) over the whole index in blocks of 65,536 rows, as
               GraphFlatIndex's build does; device events as above.  Also GraphFlatIndex(512).add(rows).build_times["knn"] (its own k
               + 1 = efConstruction + 1; --no-graph leaves it out), and whether the lists of (b) without the own row equal knn_graph's.
--only-knn measures knn_graph alone: with IVR_LIB naming a library built with other constants it gives the variant table of DESIGN.md."""
import argparse
import os
import subprocess
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--sizes", default="20000:1,20000:100,100000:1,100000:200,1000000:2000")
ap.add_argument("--timeout", type=int, default=600, help="seconds for each measuring process")
ap.add_argument("--no-graph", action="store_true")
ap.add_argument("--only-knn", action="store_true", help="knn_graph alone, without the routes (a) and (b)")
ap.add_argument("--step", default=None, help="internal: rows:segments of the measuring process")
args = ap.parse_args()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D, SHOT, K, THRESHOLD, BLOCK = 512, 20, 10, 0.7, 1 << 16

if args.step is None:
    for size in args.sizes.split(","):
        cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--step", size]
        rc = subprocess.run(cmd + (["--no-graph"] if args.no_graph else []) + (["--only-knn"] if args.only_knn else [])).returncode
        if rc != 0:
            print(f"the measuring process of {size} ended with status {rc}: nothing more is started", flush=True)
            sys.exit(rc)
    sys.exit(0)

sys.path.insert(0, os.path.join(ROOT, "intelligent-video-analysis-retrieval-system_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from ivr_amd import _ffi, filters  # noqa: E402
from ivr_amd.index import FlatIPIndex  # noqa: E402
from ivr_amd.neighbors import knn_graph_device  # noqa: E402

assert torch.cuda.is_available(), "bench_knn.py needs a GPU"
N, NSEG = (int(v) for v in args.step.split(":"))


def event_ms(fn, budget_s=1.0):
    """median ms between two device events around fn(), after 2 warm-up calls; enough repeats to fill budget_s, 5 to 50"""
    for _ in range(2):
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
            reps = int(min(50, max(5, budget_s * 1e3 / max(ts[0], 1e-3))))
    ts.sort()
    return ts[len(ts) // 2], len(ts)


def profiled(fn):
    torch.cuda.synchronize()
    _ffi.profile_enable(2)
    _ffi.profile_reset()
    fn()
    torch.cuda.synchronize()
    prof = _ffi.profile_read()
    _ffi.profile_enable(False)
    return " ".join(f"{name} {v['ms']:.4f} ms x{v['launches']}" for name, v in sorted(prof.items()))


g = torch.Generator(device="cuda").manual_seed(1234)
centres = torch.randn((-(-N // SHOT), D), generator=g, device="cuda")
centres = centres / centres.norm(dim=1, keepdim=True)
X = centres.repeat_interleave(SHOT, 0)[:N] + 0.2 * torch.randn((N, D), generator=g, device="cuda") / D ** 0.5
del centres
X = (X / X.norm(dim=1, keepdim=True)).contiguous()
index = FlatIPIndex(D, capacity=N)
index.add(X)
seg = np.linspace(0, N, NSEG + 1).astype(np.int64)
seg_dev = None if NSEG == 1 else torch.from_numpy(seg).cuda()
pairs = float((np.diff(seg).astype(np.float64) ** 2).sum())
name = f"{N} rows, {NSEG} segment{'s' if NSEG > 1 else ''}"
print(f"# bench_knn: {name} of {N // NSEG} x {D} ({N * D * 4 / 1e6:.1f} MB float32), k = {K}; {pairs:.3g} ordered pairs", flush=True)

for thr in (THRESHOLD, None):
    ms, reps = event_ms(lambda: knn_graph_device(index, K, seg_dev, thr))
    print(f"{name}: knn_graph_device threshold {thr}: {ms:.3f} ms (device events, median of {reps}), {pairs / ms / 1e6:.1f} G pairs/s",
          flush=True)
print(f"{name}: kernels of one profiled call: " + profiled(lambda: knn_graph_device(index, K, seg_dev, THRESHOLD)), flush=True)
if args.only_knn:
    sys.exit(0)
I_own = knn_graph_device(index, K, seg_dev, None)[1]

Xh = X.cpu().numpy()
keys = list(range(N))


def route_a():
    out = {}
    for lo, hi in zip(seg[:-1].tolist(), seg[1:].tolist()):
        out.update(filters.similarity_graph(Xh[lo:hi], keys[lo:hi], K, THRESHOLD))
    return out


best = None
for _ in range(2 if N <= 100_000 else 1):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    got = route_a()
    torch.cuda.synchronize()
    t = (time.perf_counter() - t0) * 1e3
    best = t if best is None else min(best, t)
cnt = knn_graph_device(index, K, seg_dev, THRESHOLD)[2].cpu().numpy()
print(f"{name}: (a) filters.similarity_graph folder by folder: {best:.1f} ms wall; lists of the same length as knn_graph's: "
      f"{sum(len(got[r]) == cnt[r] for r in range(N))} of {N}", flush=True)
del Xh, got

if NSEG == 1:
    allrows = torch.arange(N, dtype=torch.int64, device="cuda")

    def route_b():
        return [index.search_device(index.gather_device(allrows[i:i + BLOCK]), K + 1)[1] for i in range(0, N, BLOCK)]

    ms, reps = event_ms(route_b)
    I = torch.cat(route_b())
    own = I == allrows.unsqueeze(1)
    own[~own.any(1), -1] = True
    same = int((I[~own].view(N, K) == I_own).all(1).sum())
    print(f"{name}: (b) search_device(gather_device(block), k + 1) in blocks of {BLOCK}: {ms:.3f} ms (device events, median of {reps}), "
          f"{pairs / ms / 1e6:.1f} G pairs/s; rows with knn_graph's list: {same} of {N}", flush=True)
    if not args.no_graph:
        from ivr_amd.graph import GraphFlatIndex
        gi = GraphFlatIndex(D)
        gi.add(X)
        print(f"{name}: GraphFlatIndex.add build_times (s), efConstruction = {gi.hnsw.efConstruction}: "
              + " ".join(f"{k} {v:.3f}" for k, v in gi.build_times.items()), flush=True)
