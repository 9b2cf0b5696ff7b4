#!/usr/bin/env python3
"""IndexScalarQuantizer (QT_8bit, d bytes per row) alone and as the base of IndexRefineFlat, against FlatIPIndex, IndexLSH + re-ranking
and IndexPQ (M = 64) on the same rows: what training, adding and searching cost and what recall the codes keep.

    python tools/bench_sq.py [--rows 1000000] [--timeout 600]

Rows and queries are those of tools/bench_lsh.py, tools/bench_refine.py and tools/bench_pq.py: `--rows` x 512 unit-norm float32 around
1000 random unit centres, row = normalize(centre[j] + g / sqrt(d)), drawn on the device by torch.Generator(device="cuda")
.manual_seed(1234) in blocks of 250,000 rows; queries: 1000 more rows of the same distribution from manual_seed(4321), the first nq of
them.  k = 10.

The run is a chain of steps, one per nq in (1, 10, 64, 1000), each a child process of its own under `timeout`; a step that fails ends
the chain.  A step generates the rows, trains IndexScalarQuantizer(512) on the first block (minimum and range of every coordinate; wall
clock around a device synchronisation), adds every block to IndexRefineFlat(IndexScalarQuantizer) (its refine_index is the FlatIPIndex
the comparison uses: one copy of the rows; add time = the encoder and the code append alone, summed over the blocks), to an
IndexLSH(512, 256) and to an IndexPQ(512, 64) trained on the first block, and then reports:
    sq        SQIndex.search_device(Q, 10), with its query, stage, scan, key, selection and finish kernels from one profiled call (event
              pairs around every kernel lengthen the call: compare them with each other, not with the medians) and the scan's bytes
              per second (the stored codes once per pass of 32 queries)
    refine    IndexRefineFlat.search_device(Q, 10, k_factor) at k_factor 1, 2 and 4
    flat      FlatIPIndex.search_device(Q, 10)
    lsh       IndexLSH.search_device(Q, 10 * 50) + FlatIPIndex.rescore_device: the LSH + re-ranking of tools/bench_refine.py at
              k_factor 50, and at 200
    pq        IndexPQ(512, 64).search_device(Q, 10)
each as the median time between two device events after 3 warm-up calls (queries resident on the device), with recall@10 =
|top-10 & flat top-10| / 10 averaged over the queries."""
import argparse
import os
import subprocess
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=1_000_000)
ap.add_argument("--timeout", type=int, default=600, help="seconds per step")
ap.add_argument("--step", default=None, help="internal: measure")
ap.add_argument("--nq", type=int, default=1)
args = ap.parse_args()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D, NCENT, NQS, K, KFS, PQ_M, LSH_KFS = 512, 1000, (1, 10, 64, 1000), 10, (1, 2, 4), 64, (50, 200)

if args.step is None:
    base = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--rows", str(args.rows)]
    for step in [["--step", "measure", "--nq", str(nq)] for nq in NQS]:
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
from ivr_amd.sq import IndexScalarQuantizer  # noqa: E402

assert torch.cuda.is_available(), "bench_sq.py needs a GPU"
N, nq = args.rows, args.nq


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
sq = IndexScalarQuantizer(D)
index = IndexRefineFlat(sq)
lsh = IndexLSH(D, 256)
pq = IndexPQ(D, PQ_M)
flat = index.refine_index
t_train = t_add = 0.0
for i in range(0, N, 250_000):
    x = draw(g, centres, min(250_000, N - i))
    if i == 0:
        t_train = wall_ms(lambda: sq.train(x))
        pq.train(x)
    t_add += wall_ms(lambda: sq.add(x))
    flat.add(x)
    lsh.add(x)
    pq.add(x)
    del x
Q = draw(torch.Generator(device="cuda").manual_seed(4321), centres, 1000)[:nq].contiguous()
print(f"# bench_sq: {N} x {D} rows around {NCENT} centres, k = {K}, nq = {nq}; codes {N * D / 1e6:.1f} MB, LSH codes "
      f"{N * lsh.code_size / 1e6:.1f} MB, PQ codes {N * PQ_M / 1e6:.1f} MB, float32 rows {N * D * 4 / 1e6:.1f} MB; train (first block) "
      f"{t_train:.1f} ms, add {t_add:.1f} ms = {t_add / N * 1e3:.3f} us per row", flush=True)
t_flat = event_ms(lambda: flat.search_device(Q, K))
If = flat.search_device(Q, K)[1].cpu().numpy()
t_sq = event_ms(lambda: sq.search_device(Q, K))
r_sq = recall(sq.search_device(Q, K)[1].cpu().numpy(), If)
torch.cuda.synchronize()
_ffi.profile_enable(2)
_ffi.profile_reset()
sq.search_device(Q, K)
torch.cuda.synchronize()
prof = _ffi.profile_read()
_ffi.profile_enable(False)
names = ("sq_query", "sq_stage", "sq_scan", "sq_select_groups", "sq_keys", "sq_select_rows", "sq_finish")
kern = ", ".join(f"{n} {prof[n]['ms']:.4f}" for n in names if n in prof)
scan = prof.get("sq_scan")
rate = f"{scan['work'] / scan['ms'] / 1e9:.3f} TB/s over {scan['work'] / 1e6:.0f} MB" if scan and scan["ms"] > 0 else "n/a"
print(f"## nq = {nq}: flat {t_flat:.4f} ms; sq alone {t_sq:.4f} ms = {t_sq / t_flat:.2f} x flat, recall@{K} {r_sq:.4f}; kernels of one "
      f"profiled call (ms): {kern}; scan {rate}", flush=True)
print("base | k_factor |   kc | whole ms | whole / flat | recall@10", flush=True)
for kf in KFS:
    t = event_ms(lambda: index.search_device(Q, K, k_factor=kf))
    r = recall(index.search_device(Q, K, k_factor=kf)[1].cpu().numpy(), If)
    print(f"sq   | {kf:8d} | {K * kf:4d} | {t:8.4f} | {t / t_flat:12.3f} | {r:9.4f}", flush=True)
for kf in LSH_KFS:
    def lsh_refine():
        return flat.rescore_device(Q, lsh.search_device(Q, K * kf)[1].contiguous(), K)
    t = event_ms(lsh_refine)
    r = recall(lsh_refine()[1].cpu().numpy(), If)
    print(f"lsh  | {kf:8d} | {K * kf:4d} | {t:8.4f} | {t / t_flat:12.3f} | {r:9.4f}", flush=True)
t = event_ms(lambda: pq.search_device(Q, K))
r = recall(pq.search_device(Q, K)[1].cpu().numpy(), If)
print(f"pq{PQ_M} | {'-':>8s} | {K:4d} | {t:8.4f} | {t / t_flat:12.3f} | {r:9.4f}", flush=True)
