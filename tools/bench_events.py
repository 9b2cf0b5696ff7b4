#!/usr/bin/env python3
"""Event search (ivr_amd/temporal.py: event_search_device) against the flat search of the same frames, which is its floor, and against
the host route a caller without it has to take: m flat searches at k = 2048 and a join in numpy.

    python tools/bench_events.py [--rows 1000000] [--segment 500] [--timeout 900] [--quick]

Rows are those of tools/bench_temporal.py: `--rows` x 512 unit-norm float32 around 1000 random unit centres, drawn on the device by
torch.Generator(device="cuda").manual_seed(1234) in blocks of 250,000 rows.  The index is cut into segments of `--segment` rows, and is
taken as one segment.  A chain of m events is planted per query: a random segment, m rows of it in ascending order with gaps drawn
uniformly from 1 .. min(max_gap, what the segment leaves), each event normalize(row + 0.5 g / sqrt(d)) (manual_seed(4321)).

Grid: B in {1, 16} chains, m in {2, 4, 8} events, max_gap in {8, 64, 1024, 4096}, min_gap = 1, k = 10.  The measurement is one child
process under `timeout`.  Per grid point it reports
    call       median ms of event_search_device between two device events after 3 warm-up calls (events and offsets on the device)
    score / steps / tail   the passes of one profiled call (event pairs around the passes lengthen the call: compare them with each
               other, not with the median); tail = selection + backtrack
    step GB/s  the bytes the m - 1 step launches must move (26 per chain, row and step: previous key 8, frame score 4, segment start 4,
               new key 8, distance 2) over the profiled step time
    flat       FlatIPIndex.search_device of the B m frames as one batch, k = 10: the score pass alone is that work
    host       m searches at k = 2048 (one batch), the results copied to the host, and a numpy join per chain by row order, gap and
               segment; `share` = the part of the true top-10 chains (end row and path) the join finds
and whether the best chain of query 0 is the planted one."""
import argparse
import os
import subprocess
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=1_000_000)
ap.add_argument("--segment", type=int, default=500)
ap.add_argument("--timeout", type=int, default=900, help="seconds for the measuring process")
ap.add_argument("--quick", action="store_true", help="B = 1 and 16, m = 4, max_gap = 64 and 4096 only")
ap.add_argument("--step", default=None, help="internal: measure")
args = ap.parse_args()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D, NCENT, K, KHOST, NOISE = 512, 1000, 10, 2048, 0.5

if args.step is None:
    cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--rows", str(args.rows), "--segment",
           str(args.segment), "--step", "measure"] + (["--quick"] if args.quick else [])
    rc = subprocess.run(cmd).returncode
    if rc != 0:
        print(f"the measuring process ended with status {rc}", flush=True)
    sys.exit(rc)

sys.path.insert(0, os.path.join(ROOT, "intelligent-video-analysis-retrieval-system_amd"))
import time  # noqa: E402

import numpy as np  # noqa: E402
import torch  # noqa: E402

from ivr_amd import _ffi  # noqa: E402
from ivr_amd.index import FlatIPIndex  # noqa: E402
from ivr_amd.temporal import event_search_device  # noqa: E402

assert torch.cuda.is_available(), "bench_events.py needs a GPU"
N, SEG = args.rows, args.segment
assert N % SEG == 0 and SEG >= 8


def draw(g, centres, n):
    j = torch.randint(0, len(centres), (n,), generator=g, device="cuda")
    x = centres[j] + torch.randn((n, D), generator=g, device="cuda") / D ** 0.5
    return x / x.norm(dim=1, keepdim=True)


def event_ms(fn, budget_s=0.2):
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


def profiled(fn):
    torch.cuda.synchronize()
    _ffi.profile_enable(2)
    _ffi.profile_reset()
    fn()
    torch.cuda.synchronize()
    prof = _ffi.profile_read()
    _ffi.profile_enable(False)
    return {name: v["ms"] for name, v in prof.items()}


def host_join(Dh, Ih, m, min_gap, max_gap, seg_len):
    """The join of one chain's m result lists (Dh float32 [m,KHOST], Ih int64 [m,KHOST]) in numpy: the dynamic programme of the
    definition over the listed rows only -> the 10 best (score, path) by (score descending, end row ascending)."""
    rows, val, back = [], [], []
    for j in range(m):
        keep = Ih[j] >= 0
        order = np.argsort(Ih[j][keep], kind="stable")
        r, s = Ih[j][keep][order], Dh[j][keep][order]
        if j == 0:
            c, p = s.copy(), np.full(len(r), -1, np.int64)
        else:
            lo = np.maximum(r - max_gap, (r // seg_len) * seg_len if seg_len else 0)
            a, b = np.searchsorted(rows[-1], lo, side="left"), np.searchsorted(rows[-1], r - min_gap, side="right")
            c, p = np.full(len(r), -np.inf, np.float32), np.full(len(r), -1, np.int64)
            prev = val[-1]
            for i in np.flatnonzero(b > a):
                t = a[i] + int(np.argmax(prev[a[i]:b[i]]))
                if prev[t] > -np.inf:
                    c[i], p[i] = np.float32(prev[t] + s[i]), t
        rows.append(r)
        val.append(c)
        back.append(p)
    ends = np.flatnonzero(val[-1] > -np.inf)
    ends = ends[np.lexsort((rows[-1][ends], -val[-1][ends].astype(np.float64)))][:K]
    out = []
    for e in ends:
        path, t = [], int(e)
        for j in range(m - 1, -1, -1):
            path.append(int(rows[j][t]))
            t = int(back[j][t])
        out.append(tuple(path[::-1]))
    return out


g = torch.Generator(device="cuda").manual_seed(1234)
centres = torch.randn((NCENT, D), generator=g, device="cuda")
centres = centres / centres.norm(dim=1, keepdim=True)
index = FlatIPIndex(D)
for i in range(0, N, 250_000):
    index.add(draw(g, centres, min(250_000, N - i)))
seg = torch.arange(0, N + 1, SEG, dtype=torch.int64, device="cuda").contiguous()
print(f"# bench_events: {N} x {D} rows around {NCENT} centres ({N * D * 4 / 1e6:.1f} MB float32), segments of {SEG} rows "
      f"({N // SEG}) and one segment, min_gap = 1, k = {K}, host route at k = {KHOST}", flush=True)
print("segments |  B | m | max_gap |  call ms | score ms | steps ms | tail ms | step GB/s | flat ms | call/flat | host ms | share | planted first",
      flush=True)
gq = torch.Generator(device="cuda").manual_seed(4321)
grid_B, grid_m, grid_gap = ((1, 16), (4,), (64, 4096)) if args.quick else ((1, 16), (2, 4, 8), (8, 64, 1024, 4096))
for name, s, seg_len in ((str(N // SEG), seg, SEG), ("one", None, 0)):
    for B in grid_B:
        for m in grid_m:
            for max_gap in grid_gap:
                # the planted chains: inside one segment of SEG rows in both cases, so that both cases answer the same queries
                first = torch.randint(0, N // SEG, (B,), generator=gq, device="cuda") * SEG
                gaps = torch.randint(1, min(max_gap, (SEG - 1) // (m - 1)) + 1, (B, m), generator=gq, device="cuda")
                gaps[:, 0] = 0
                planted = first[:, None] + gaps.cumsum(1)
                Q = index.gather_device(planted.reshape(-1).contiguous()) + NOISE * torch.randn((B * m, D), generator=gq, device="cuda") / D ** 0.5
                Q = (Q / Q.norm(dim=1, keepdim=True)).reshape(B, m, D).contiguous()
                call = lambda: event_search_device(index, Q, K, max_gap, 1, seg_off=s)      # noqa: E731
                t_call = event_ms(call)
                prof = profiled(call)
                t_score, t_steps, t_tail = prof.get("seq_score", 0.0), prof.get("event_step", 0.0), prof.get("event_tail", 0.0)
                gbs = B * N * (m - 1) * 26.0 / (t_steps * 1e-3) / 1e9 if t_steps else 0.0
                flat = Q.reshape(B * m, D)
                t_flat = event_ms(lambda: index.search_device(flat, K))
                I = event_search_device(index, Q, K, max_gap, 1, seg_off=s)[1].cpu().numpy()

                def host_route():
                    Dh, Ih = index.search_device(flat, KHOST)
                    Dh, Ih = Dh.cpu().numpy().reshape(B, m, KHOST), Ih.cpu().numpy().reshape(B, m, KHOST)
                    return [host_join(Dh[b], Ih[b], m, 1, max_gap, seg_len) for b in range(B)]

                host_route()
                ts = []
                for _ in range(3):
                    t0 = time.perf_counter()
                    found = host_route()
                    ts.append((time.perf_counter() - t0) * 1e3)
                true = [[tuple(int(r) for r in p) for p in I[b] if p[0] >= 0] for b in range(B)]
                share = sum(len(set(true[b]) & set(found[b])) for b in range(B)) / max(1, sum(len(t) for t in true))
                ok = sum(tuple(planted[b].tolist()) == true[b][0] for b in range(B))
                print(f"{name:>8} | {B:2d} | {m} | {max_gap:7d} | {t_call:8.4f} | {t_score:8.4f} | {t_steps:8.4f} | {t_tail:7.4f} | {gbs:9.1f} | "
                      f"{t_flat:7.4f} | {t_call / t_flat:9.2f} | {sorted(ts)[1]:7.2f} | {share:5.2f} | {ok}/{B}", flush=True)
