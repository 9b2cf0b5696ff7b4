#!/usr/bin/env python3
"""Stable external ids (FlatIPIndex.add_with_ids) against the plain index, both over the same 1M x 512 unit rows in one process.
Labels are a random sample of [0, 10 rows): not monotone, with gaps.

  1. unfiltered search: 1 query / k = 50 and 1,000 queries / k = 10.  The id-mapped index reads one 8-byte label per result.
  2. filtered search: a bitmap over the label span that allows 10 % of the labels on the id-mapped index, against the same rows as a
     positional bitmap over the whole plain index (lo = 0, so that it scans every row too).  The difference is the row-mask pass.
  3. the row-mask pass alone: HIP-event time of the launch from the library's profile hooks, with its bytes (8 per stored row read,
     one bit per row written).
  4. remove_ids of the first, the middle and the last 1 % of the rows: by their stored ids (IDSelectorBatch) on the id-mapped index,
     by IDSelectorRange on the plain one.

Searches are device-resident calls between HIP events, the two indexes timed alternately; remove_ids waits for its count on the
host, so it is timed by the wall clock between two device synchronisations, with the index refilled before every repeat (not
timed).  Figures are medians after warm-up.

    python tools/bench_id_map.py [rows=1048576] [remove_repeats=7]
"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "intelligent-video-analysis-retrieval-system_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from ivr_amd import _ffi  # noqa: E402
from ivr_amd.index import FlatIPIndex, IDSelectorBatch, IDSelectorBitmap, IDSelectorRange  # noqa: E402

rows = int(sys.argv[1]) if len(sys.argv) > 1 else 1 << 20
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 7
d = 512

g = torch.Generator(device="cuda").manual_seed(31)
master = torch.randn((rows, d), generator=g, device="cuda")
master /= master.norm(dim=1, keepdim=True)
rng = np.random.default_rng(5)
ids = rng.permutation(10 * rows)[:rows].astype(np.int64)
ids_dev = torch.from_numpy(ids).cuda()
P = FlatIPIndex(d, capacity=rows)
M = FlatIPIndex(d, capacity=rows)


def refill(idx):
    idx.reset()
    if idx is M:
        idx._add_device(master, False, ids)
    else:
        idx._add_device(master, False)
    torch.cuda.synchronize()


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def alternate(fa, fb, n, warm=5):
    """medians of fa and fb, timed alternately"""
    for _ in range(warm):
        fa()
        fb()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(n):
        ta.append(event_ms(fa))
        tb.append(event_ms(fb))
    return float(np.median(ta)), float(np.median(tb))


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


refill(P)
refill(M)
print(f"index {rows} x {d}, labels: a random sample of [0, {10 * rows}), bf16 scan copy: {M.scan_stats()[0]}", flush=True)

# 1 + 2: searches
allowed_label = rng.random(10 * rows) < 0.1
sel_m = IDSelectorBitmap(np.packbits(allowed_label, bitorder="little"))
sel_p = IDSelectorBitmap(np.packbits(allowed_label[ids], bitorder="little"))
for s, idx in ((sel_m, M), (sel_p, P)):
    s._filter(idx.device)                                   # the bitmap upload is not part of a call
for nq, k, n in ((1, 50, 200), (1000, 10, 20)):
    Q = torch.randn((nq, d), generator=g, device="cuda")
    Q /= Q.norm(dim=1, keepdim=True)
    outs = [(torch.empty((nq, k), dtype=torch.float32, device="cuda"), torch.empty((nq, k), dtype=torch.int64, device="cuda")) for _ in range(2)]
    for name, sp, sm in (("unfiltered", None, None), ("filtered 10 %", sel_p, sel_m)):
        tm, tp = alternate(lambda: M.search_device(Q, k, out=outs[0], sel=sm), lambda: P.search_device(Q, k, out=outs[1], sel=sp), n)
        torch.cuda.synchronize()
        same = torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], torch.where(outs[1][1] >= 0, ids_dev[outs[1][1].clamp(min=0)], -1))
        print(f"search {name:14s} nq={nq:4d} k={k:2d}  id-mapped {tm:8.4f} ms  plain {tp:8.4f} ms  ratio {tm / tp:6.3f}  "
              f"(median of {n} alternating calls; same scores, labels = ids[rows]: {same})", flush=True)

# 3: the row-mask pass from the profile hooks
dev = M.device.index
Q = master[:10].contiguous()
_ffi.profile_enable(2, dev)
_ffi.profile_reset(dev)
for _ in range(20):
    M.search_device(Q, 10, sel=sel_m)
torch.cuda.synchronize()
prof = _ffi.profile_read(dev)
_ffi.profile_enable(0, dev)
v = prof["ids_row_mask"]
per = v["ms"] / v["launches"]
print(f"ids_row_mask: {v['launches']} launches, {per * 1e3:7.2f} us each, {v['work'] / v['launches'] / 1e6:6.2f} MB read + written = "
      f"{v['work'] / v['ms'] / 1e9:6.3f} TB/s; the same calls' scan16_groupmax: "
      f"{prof['scan16_groupmax']['ms'] / prof['scan16_groupmax']['launches'] * 1e3:7.2f} us", flush=True)

# 4: removal
one = rows // 100
print(f"remove_ids of {one} rows, wall clock, median of {reps} repeats after 2 warm-ups", flush=True)
for name, lo in (("first 1 %", 0), ("middle 1 %", rows // 2), ("last 1 %", rows - one)):
    by_id, by_row = IDSelectorBatch(ids[lo:lo + one]), IDSelectorRange(lo, lo + one)
    by_id._filter(M.device)
    tm, tp = [], []
    for r in range(reps + 2):
        refill(M)
        t = wall_ms(lambda: M.remove_ids(by_id))
        refill(P)
        u = wall_ms(lambda: P.remove_ids(by_row))
        assert M.ntotal == P.ntotal == rows - one
        if r >= 2:
            tm.append(t)
            tp.append(u)
    ok = bool(np.array_equal(M.id_map, np.delete(ids, np.arange(lo, lo + one))))
    a, b = float(np.median(tm)), float(np.median(tp))
    print(f"remove {name:11s} id-mapped {a:8.3f} ms  plain {b:8.3f} ms  difference {a - b:7.3f} ms  (id table follows: {ok})", flush=True)
P.close()
M.close()
