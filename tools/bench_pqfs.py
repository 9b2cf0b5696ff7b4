#!/usr/bin/env python3
"""IndexPQFastScan (M / 2 bytes per row, 4-bit codes) alone and as the base of IndexRefineFlat, beside IndexPQ at the same bytes per
row, IndexScalarQuantizer and FlatIPIndex on the same rows in the same process: what a search costs and what recall the codes keep.

    python tools/bench_pqfs.py [--rows 1000000] [--timeout 900]

Rows and queries are those of tools/bench_pq.py: `--rows` x 512 unit-norm float32 around 1000 random unit centres, row =
normalize(centre[j] + g / sqrt(d)), drawn on the device by torch.Generator(device="cuda").manual_seed(1234) in blocks of 250,000 rows;
queries: 1000 more rows of the same distribution from manual_seed(4321), the first nq of them.  k = 10.

The run is a chain of steps, one per M in (128, 64), each a child process of its own under `timeout`; a step that fails ends the
chain.  A step generates the rows, trains IndexPQFastScan(512, M), IndexPQ(512, M / 2) (the same bytes per row) and
IndexScalarQuantizer(512) on the first block (wall clock around a device synchronisation), adds every block to
IndexRefineFlat(IndexPQFastScan) (its refine_index is the FlatIPIndex the comparison uses) and to the other two, notes the device's
clocks, and then reports, per nq in (1, 10, 64, 1000):
    pqfs      IndexPQFastScan.search_device(Q, 10), with its kernels from one profiled call (event pairs around every kernel
              lengthen the call: compare them with each other, not with the medians) and the bytes per second the scan asks for
              (code bytes of the index times the passes over it, over the scan kernel's time)
    pq, sq    IndexPQ.search_device and IndexScalarQuantizer.search_device
    flat      FlatIPIndex.search_device(Q, 10)
    refine    IndexRefineFlat.search_device(Q, 10, k_factor) at k_factor 1, 4 and 16
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
ap.add_argument("--M", type=int, default=128)
args = ap.parse_args()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D, NCENT, NQS, K, KFS, MS = 512, 1000, (1, 10, 64, 1000), 10, (1, 4, 16), (128, 64)

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
from ivr_amd.pq import IndexPQ  # noqa: E402
from ivr_amd.pqfs import IndexPQFastScan  # noqa: E402
from ivr_amd.refine import IndexRefineFlat  # noqa: E402
from ivr_amd.sq import IndexScalarQuantizer  # noqa: E402

assert torch.cuda.is_available(), "bench_pqfs.py needs a GPU"
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


def clocks():
    """the device's current shader and memory clocks as rocm-smi shows them (read only), or why they could not be read"""
    try:
        out = subprocess.run(["rocm-smi", "-d", "0", "--showclocks"], capture_output=True, text=True, timeout=30).stdout
        return "; ".join(" ".join(ln.split()) for ln in out.splitlines() if "sclk" in ln or "mclk" in ln) or "not shown"
    except Exception as e:  # noqa: BLE001
        return f"not read ({type(e).__name__})"


g = torch.Generator(device="cuda").manual_seed(1234)
centres = torch.randn((NCENT, D), generator=g, device="cuda")
centres = centres / centres.norm(dim=1, keepdim=True)
fs, pq, sq = IndexPQFastScan(D, M), IndexPQ(D, M // 2), IndexScalarQuantizer(D)
index = IndexRefineFlat(fs)
flat = index.refine_index
t_train = t_train_pq = t_add = 0.0
for i in range(0, N, 250_000):
    x = draw(g, centres, min(250_000, N - i))
    if i == 0:
        t_train = wall_ms(lambda: fs.train(x))
        t_train_pq = wall_ms(lambda: pq.train(x))
        sq.train(x)
    t_add += wall_ms(lambda: fs.add(x))
    flat.add(x)
    pq.add(x)
    sq.add(x)
    del x
Qall = draw(torch.Generator(device="cuda").manual_seed(4321), centres, 1000)
P = _ffi.load().ivr_pqfs_pass_queries()
code_bytes = -(-N // 256) * -(-M // 8) * 1024
print(f"# bench_pqfs: {N} x {D} rows around {NCENT} centres, M = {M} x 4 bits (dsub = {D // M}), k = {K}; codes {N * M / 2e6:.1f} MB "
      f"({code_bytes / 1e6:.1f} MB stored), IndexPQ M = {M // 2}: {N * M / 2e6:.1f} MB, SQ codes {N * D / 1e6:.1f} MB, float32 rows "
      f"{N * D * 4 / 1e6:.1f} MB; train (25 iterations, 4,096 sampled rows) {t_train:.1f} ms (IndexPQ: {t_train_pq:.1f} ms), add {t_add:.1f} "
      f"ms = {t_add / N * 1e3:.3f} us per row; {P} queries per pass; clocks: {clocks()}", flush=True)
for nq in NQS:
    Q = Qall[:nq].contiguous()
    t_flat = event_ms(lambda: flat.search_device(Q, K))
    If = flat.search_device(Q, K)[1].cpu().numpy()
    t_fs = event_ms(lambda: fs.search_device(Q, K))
    t_pq = event_ms(lambda: pq.search_device(Q, K))
    t_sq = event_ms(lambda: sq.search_device(Q, K))
    r_fs = recall(fs.search_device(Q, K)[1].cpu().numpy(), If)
    r_pq = recall(pq.search_device(Q, K)[1].cpu().numpy(), If)
    r_sq = recall(sq.search_device(Q, K)[1].cpu().numpy(), If)
    torch.cuda.synchronize()
    _ffi.profile_enable(2)
    _ffi.profile_reset()
    fs.search_device(Q, K)
    pq.search_device(Q, K)
    torch.cuda.synchronize()
    prof = _ffi.profile_read()
    _ffi.profile_enable(False)
    names = ("pqfs_tables", "pqfs_stage", "pqfs_scan", "pqfs_select_groups", "pqfs_keys", "pqfs_select_rows", "pqfs_finish", "pq_scan")
    kern = ", ".join(f"{n} {prof[n]['ms']:.4f}" for n in names if n in prof)
    scan = prof.get("pqfs_scan", {"ms": 0.0})["ms"]
    asked = -(-nq // P) * code_bytes
    print(f"## M = {M}, nq = {nq}: flat {t_flat:.4f} ms; pqfs {t_fs:.4f} ms = {t_fs / t_flat:.2f} x flat = {t_fs / t_pq:.3f} x pq, recall@{K} "
          f"{r_fs:.4f}; pq (M = {M // 2}) {t_pq:.4f} ms, recall {r_pq:.4f}; sq {t_sq:.4f} ms, recall {r_sq:.4f}; kernels of one profiled "
          f"call (ms): {kern}; the scan asks for {asked / 1e6:.1f} MB = {asked / max(scan, 1e-6) / 1e9:.3f} TB/s", flush=True)
    print("base    | k_factor |   kc | whole ms | whole / flat | recall@10", flush=True)
    for kf in KFS:
        t = event_ms(lambda: index.search_device(Q, K, k_factor=kf))
        r = recall(index.search_device(Q, K, k_factor=kf)[1].cpu().numpy(), If)
        print(f"pqfs{M:<3d} | {kf:8d} | {K * kf:4d} | {t:8.4f} | {t / t_flat:12.3f} | {r:9.4f}", flush=True)
