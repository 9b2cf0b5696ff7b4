#!/usr/bin/env python3
"""IndexPQ (M bytes per row) alone and as the base of IndexRefineFlat, against FlatIPIndex and IndexLSH + re-ranking on the same rows:
what training, adding and searching cost and what recall the codes keep.

    python tools/bench_pq.py [--rows 1000000] [--timeout 900]

Rows and queries are those of tools/bench_lsh.py and tools/bench_refine.py: `--rows` x 512 unit-norm float32 around 1000 random unit
centres, row = normalize(centre[j] + g / sqrt(d)), drawn on the device by torch.Generator(device="cuda").manual_seed(1234) in blocks
of 250,000 rows; queries: 1000 more rows of the same distribution from manual_seed(4321), the first nq of them.  k = 10.

The run is a chain of steps, one per M in (32, 64), each a child process of its own under `timeout`; a step that fails ends the chain.
A step generates the rows, trains IndexPQ(512, M) on the first block (train draws its 65,536-row sample from it; wall clock around a
device synchronisation), adds every block to IndexRefineFlat(IndexPQ) (its refine_index is the FlatIPIndex the comparison uses: one
copy of the rows; add time = the PQ encoder and code append alone, summed over the blocks) and to an IndexLSH(512, 256), and then
reports, per nq in (1, 1000):
    pq        IndexPQ.search_device(Q, 10), with its tables, scan, key and selection kernels from one profiled call (event pairs
              around every kernel lengthen the call: compare them with each other, not with the medians)
    refine    IndexRefineFlat.search_device(Q, 10, k_factor) at k_factor 1, 4 and 16
    flat      FlatIPIndex.search_device(Q, 10)
    lsh       IndexLSH.search_device(Q, 10 * 50) + FlatIPIndex.rescore_device: the LSH + re-ranking of tools/bench_refine.py at
              k_factor 50, and at 200
each as the median time between two device events after 3 warm-up calls (queries resident on the device), with recall@10 =
|top-10 & flat top-10| / 10 averaged over the queries."""
import argparse
import os
import subprocess
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=1_000_000)
ap.add_argument("--timeout", type=int, default=900, help="seconds per step")
ap.add_argument("--step", default=None, help="internal: measure")
ap.add_argument("--M", type=int, default=64)
args = ap.parse_args()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D, NCENT, NQS, K, KFS, MS, LSH_KFS = 512, 1000, (1, 1000), 10, (1, 4, 16), (32, 64), (50, 200)

if args.step is None:
    base = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--rows", str(args.rows)]
    for step in [["--step", "measure", "--M", str(m)] for m in MS]:
        rc = subprocess.run(base + step).returncode
        if rc != 0:
            print(f"step {' '.join(step)} ended with status {rc}: stopping", flush=True)
            sys.exit(rc)
    sys.exit(0)

sys.path.insert(0, os.path.join(ROOT, "intelligent-video-analysis-retrieval-system_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from ivr_amd import _ffi  # noqa: E402
from ivr_amd.binary import IndexLSH  # noqa: E402
from ivr_amd.pq import IndexPQ  # noqa: E402
from ivr_amd.refine import IndexRefineFlat  # noqa: E402

assert torch.cuda.is_available(), "bench_pq.py needs a GPU"
N, M = args.rows, args.M


def draw(g, centres, n):
    j = torch.randint(0, len(centres), (n,), generator=g, device="cuda")
    x = centres[j] + torch.randn((n, D), generator=g, device="cuda") / D ** 0.5
    return x / x.norm(dim=1, keepdim=True)


def event_ms(fn, budget_s=0.5):
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
    return ts[len(ts) // 2]


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def recall(I, If):
    return float(np.mean([len(set(If[i]) & set(I[i])) / K for i in range(len(If))]))


g = torch.Generator(device="cuda").manual_seed(1234)
centres = torch.randn((NCENT, D), generator=g, device="cuda")
centres = centres / centres.norm(dim=1, keepdim=True)
pq = IndexPQ(D, M)
index = IndexRefineFlat(pq)
lsh = IndexLSH(D, 256)
flat = index.refine_index
t_train = t_add = 0.0
for i in range(0, N, 250_000):
    x = draw(g, centres, min(250_000, N - i))
    if i == 0:
        t_train = wall_ms(lambda: pq.train(x))
    t_add += wall_ms(lambda: pq.add(x))
    flat.add(x)
    lsh.add(x)
    del x
Qall = draw(torch.Generator(device="cuda").manual_seed(4321), centres, 1000)
print(f"# bench_pq: {N} x {D} rows around {NCENT} centres, M = {M} (dsub = {D // M}), k = {K}; codes {N * M / 1e6:.1f} MB, LSH codes "
      f"{N * lsh.code_size / 1e6:.1f} MB, float32 rows {N * D * 4 / 1e6:.1f} MB; train (25 iterations, 65,536 sampled rows) {t_train:.1f} ms, "
      f"add {t_add:.1f} ms = {t_add / N * 1e3:.3f} us per row", flush=True)
for nq in NQS:
    Q = Qall[:nq].contiguous()
    t_flat = event_ms(lambda: flat.search_device(Q, K))
    If = flat.search_device(Q, K)[1].cpu().numpy()
    t_pq = event_ms(lambda: pq.search_device(Q, K))
    r_pq = recall(pq.search_device(Q, K)[1].cpu().numpy(), If)
    torch.cuda.synchronize()
    _ffi.profile_enable(2)
    _ffi.profile_reset()
    pq.search_device(Q, K)
    torch.cuda.synchronize()
    prof = _ffi.profile_read()
    _ffi.profile_enable(False)
    kern = ", ".join(f"{n} {prof[n]['ms']:.4f}" for n in ("pq_tables", "pq_scan", "pq_select_groups", "pq_keys", "pq_select_rows") if n in prof)
    print(f"## M = {M}, nq = {nq}: flat {t_flat:.4f} ms; pq alone {t_pq:.4f} ms = {t_pq / t_flat:.2f} x flat, recall@{K} {r_pq:.4f}; "
          f"kernels of one profiled call (ms): {kern}", flush=True)
    print("base | k_factor |   kc | whole ms | whole / flat | recall@10", flush=True)
    for kf in KFS:
        t = event_ms(lambda: index.search_device(Q, K, k_factor=kf))
        r = recall(index.search_device(Q, K, k_factor=kf)[1].cpu().numpy(), If)
        print(f"pq{M:<2d} | {kf:8d} | {K * kf:4d} | {t:8.4f} | {t / t_flat:12.3f} | {r:9.4f}", flush=True)
    for kf in LSH_KFS:
        def lsh_refine():
            return flat.rescore_device(Q, lsh.search_device(Q, K * kf)[1].contiguous(), K)
        t = event_ms(lsh_refine)
        r = recall(lsh_refine()[1].cpu().numpy(), If)
        print(f"lsh  | {kf:8d} | {K * kf:4d} | {t:8.4f} | {t / t_flat:12.3f} | {r:9.4f}", flush=True)
