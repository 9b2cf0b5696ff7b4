#!/usr/bin/env python3
"""Filtered search (FlatIPIndex.search_device(..., sel=IDSelector...)) on 1M x 512 unit rows with 10 and 1000 queries, k = 10 and 50:
no selector, bitmaps allowing 100 % / 10 % / 0.1 % of the rows, a 10,000-row IDSelectorRange and 1,000 ids in 10 clusters
(IDSelectorBatch).  Each filtered call is timed alternately with the unfiltered search of the same queries (one filtered, one
unfiltered, repeated), with HIP events around each device-resident call; figures are medians over the warmed repeats.

    python tools/bench_filtered_search.py [rows=1048576] [repeats=25]
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "intelligent-video-analysis-retrieval-system_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from ivr_amd.index import FlatIPIndex, IDSelectorBatch, IDSelectorBitmap, IDSelectorRange  # noqa: E402

rows = int(sys.argv[1]) if len(sys.argv) > 1 else 1 << 20
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 25
d = 512


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def alternate(fa, fb, warm=3):
    """medians of fa and fb, timed alternately"""
    for _ in range(warm):
        fa()
        fb()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(reps):
        ta.append(event_ms(fa))
        tb.append(event_ms(fb))
    return float(np.median(ta)), float(np.median(tb))


g = torch.Generator(device="cuda").manual_seed(31)
idx = FlatIPIndex(d, capacity=rows)
for i in range(0, rows, 1 << 18):
    idx.add(torch.randn((min(1 << 18, rows - i), d), generator=g, device="cuda"), normalize=True)
rng = np.random.default_rng(5)


def bitmap(frac):
    return IDSelectorBitmap(np.packbits(rng.random(rows) < frac, bitorder="little"))


clusters = np.concatenate([c + np.arange(100) for c in rng.choice(rows - 100, 10, replace=False)])
selectors = [("none", None), ("bitmap 100%", bitmap(1.0)), ("bitmap 10%", bitmap(0.1)), ("bitmap 0.1%", bitmap(0.001)),
             ("range 10,000 rows", IDSelectorRange(rows // 2, rows // 2 + 10_000)), ("batch 1,000 ids / 10 clusters", IDSelectorBatch(clusters))]
print(f"index {rows} x {d}, bf16 scan copy: {idx.scan_stats()[0]}, median of {reps} alternating repeats after 3 warm-up pairs", flush=True)
for nq in (10, 1000):
    Q = torch.randn((nq, d), generator=g, device="cuda")
    Q /= Q.norm(dim=1, keepdim=True)
    for k in (10, 50):
        D0, I0 = idx.search_device(Q, k)
        D1, I1 = idx.search_device(Q, k)
        for name, sel in selectors:
            if sel is None:
                f = lambda: idx.search_device(Q, k, out=(D1, I1))          # noqa: E731
            else:
                f = lambda: idx.search_device(Q, k, out=(D1, I1), sel=sel)  # noqa: E731
            tf, tu = alternate(f, lambda: idx.search_device(Q, k, out=(D0, I0)))
            f()
            torch.cuda.synchronize()
            redone = idx.scan_stats()[1]
            print(f"nq={nq:4d} k={k:2d}  {name:30s} filtered {tf:8.3f} ms  unfiltered {tu:8.3f} ms  ratio {tf / tu:5.2f}"
                  f"  (queries of the last chunk redone by the exact scan: {redone})", flush=True)
idx.close()
