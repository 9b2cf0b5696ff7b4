#!/usr/bin/env python3
"""Exact range search (FlatIPIndex.range_search_device) on 1M x 512 unit rows with 10 and 64 queries, at radii that give about
10, 1,000 and 100,000 hits per query, next to search(k=50) on the same rows and queries.  Device-resident calls with a fixed
capacity (no host sync inside a call); each figure is the median over warmed repeats of one call timed with HIP events.

    python tools/bench_range_search.py [rows=1048576] [repeats=20]
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "intelligent-video-analysis-retrieval-system_amd"))
import torch  # noqa: E402

from ivr_amd.index import FlatIPIndex  # noqa: E402

rows = int(sys.argv[1]) if len(sys.argv) > 1 else 1 << 20
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
d = 512


def timed(fn, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return ts[len(ts) // 2], ts[0], ts[-1]


g = torch.Generator(device="cuda").manual_seed(31)
idx = FlatIPIndex(d, capacity=rows)
for i in range(0, rows, 1 << 18):
    idx.add(torch.randn((min(1 << 18, rows - i), d), generator=g, device="cuda"), normalize=True)
print(f"index {rows} x {d}, bf16 scan copy: {idx.scan_stats()[0]}, {reps} timed repeats after 3 warm-up calls", flush=True)
for nq in (10, 64):
    Q = torch.randn((nq, d), generator=g, device="cuda")
    Q /= Q.norm(dim=1, keepdim=True)
    D50, I50 = idx.search_device(Q, 50)
    tk = timed(lambda: idx.search_device(Q, 50, out=(D50, I50)))
    print(f"nq={nq:3d}  search k=50                      median {tk[0]:8.3f} ms  (min {tk[1]:.3f}, max {tk[2]:.3f})", flush=True)
    # radii from the exact scores of query 0: its 11th, 1001st best (top-k) and the 100,001st (a range count)
    Dk, _ = idx.search_device(Q[:1], 2048)
    targets = [(10, float(Dk[0, 10])), (1000, float(Dk[0, 1000]))]
    lo, hi = 0.0, float(Dk[0, 2047])
    for _ in range(30):                                  # bisection on the count of query 0 for ~100,000 hits
        mid = 0.5 * (lo + hi)
        _, _, _, tot = idx.range_search_device(Q[:1], mid, cap=0)
        lo, hi = (mid, hi) if int(tot.item()) > 100_000 else (lo, mid)
    targets.append((100_000, hi))
    for want, radius in targets:
        lims, _, _, total = idx.range_search_device(Q, radius)
        cap = int(total.item())
        out = idx.range_search_device(Q, radius, cap=cap)
        tr = timed(lambda: idx.range_search_device(Q, radius, cap=cap))
        hits = (lims[1:] - lims[:-1]).float()
        print(f"nq={nq:3d}  range ~{want:>7d}/query radius {radius:.5f}  hits/query mean {hits.mean().item():10.1f} "
              f"(min {int(hits.min().item())}, max {int(hits.max().item())})  median {tr[0]:8.3f} ms  (min {tr[1]:.3f}, max {tr[2]:.3f})"
              f"  = {tr[0] / tk[0]:5.2f} x search(k=50)", flush=True)
        del out
idx.close()
