#!/usr/bin/env python3
"""Moment search (ivr_amd/moments.py: moment_search_device, moment_range_search_device) against the flat search of the same batch,
which answers a different question with the parent's code, and against the route a caller without it has to take: range_search at
the threshold, the hits copied to the host and merged there into intervals with numpy.

    python tools/bench_moments.py [--rows 1000000] [--segment 500] [--shot 100] [--centres 1000] [--timeout 900] [--quick]

Rows: `--rows` x 512 unit-norm float32 in videos of `--segment` rows (2,000 videos by default); a video is cut into shots of `--shot`
rows, a shot is one of `--centres` random unit centres plus 0.3 g / sqrt(d) per row: adjacent keyframes of a shot are near-duplicates,
and a centre returns in about rows / shot / centres shots (10 by default), so the rows of a query's shots are about 0.1 % of the
index.  Drawn on the device by torch.Generator(device="cuda").manual_seed(1234).  A query is normalize(centre + 0.5 g / sqrt(d))
(manual_seed(4321)).  Two thresholds: "clean" = 0.5, far below the rows of the query's shots and far above every other row, so a moment
is a whole shot; "ragged" = the median score of the query batch's own shots, so about every other row of a shot is cold, max_gap = 1
bridges most of the holes and the moments are many and short.

Grid: nq in {1, 64, 1000} x {clean, ragged}, max_gap = 1, k = 10.  The measurement is one child process under `timeout`.  Per point:
    hot        the share of (query, row) pairs at or above the threshold; moments = moments per query
    topk       median ms of moment_search_device (rank peak) between two device events after 3 warm-up calls
    range      the same of moment_range_search_device at cap = the exact total (no host synchronisation)
    score / runs / tail   the passes of one profiled top-k call (event pairs around the passes lengthen the call: compare them with
               each other, not with the median): the score pass of the clip search, the count / prefix / totals / fill / write passes
               together, the selection and the gather; score % = its share of the three
    flat       FlatIPIndex.search_device of the batch at k = 10
    host       range_search_device(cap=None) at the threshold, lims / D / I copied to the host, the rows merged into moments with
               numpy (diff, reduceat); median of 3"""
import argparse
import os
import subprocess
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=1_000_000)
ap.add_argument("--segment", type=int, default=500)
ap.add_argument("--shot", type=int, default=100)
ap.add_argument("--centres", type=int, default=1000)
ap.add_argument("--timeout", type=int, default=900, help="seconds for the measuring process")
ap.add_argument("--quick", action="store_true", help="nq = 1 and 64 only")
ap.add_argument("--step", default=None, help="internal: measure")
args = ap.parse_args()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D, NCENT, SHOT, K, GAP = 512, args.centres, args.shot, 10, 1

if args.step is None:
    cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--rows", str(args.rows), "--segment",
           str(args.segment), "--shot", str(args.shot), "--centres", str(args.centres), "--step", "measure"] + (["--quick"] if args.quick else [])
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
from ivr_amd.moments import moment_range_search_device, moment_search_device  # noqa: E402

assert torch.cuda.is_available(), "bench_moments.py needs a GPU"
N, SEG = args.rows, args.segment
assert N % SEG == 0 and 250_000 % SHOT == 0 and N % SHOT == 0


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


def host_merge(lims, Dh, Ih, seg_rows, max_gap):
    """The moments of range_search hits on the host: rows ascend within a query; a hit starts a moment at the start of its query, in
    another video than its predecessor, or more than max_gap rows behind it.  -> (lo, hi, cnt, peak row, peak score)"""
    if len(Ih) == 0:
        return (np.zeros(0, np.int64),) * 4 + (np.zeros(0, np.float32),)
    head = np.ones(len(Ih), bool)
    head[1:] = (Ih[1:] - Ih[:-1] > max_gap + 1) | (Ih[1:] // seg_rows != Ih[:-1] // seg_rows)
    head[lims[:-1][lims[:-1] < len(Ih)]] = True
    starts = np.flatnonzero(head)
    ends = np.append(starts[1:], len(Ih))
    best = np.maximum.reduceat(Dh, starts)
    first_best = np.minimum.reduceat(np.where(Dh == np.repeat(best, ends - starts), np.arange(len(Ih)), len(Ih)), starts)
    return Ih[starts], Ih[ends - 1], ends - starts, Ih[first_best], best


g = torch.Generator(device="cuda").manual_seed(1234)
centres = torch.randn((NCENT, D), generator=g, device="cuda")
centres = centres / centres.norm(dim=1, keepdim=True)
index = FlatIPIndex(D)
for i in range(0, N, 250_000):
    n = min(250_000, N - i)
    shot = torch.randint(0, NCENT, (n // SHOT,), generator=g, device="cuda").repeat_interleave(SHOT)
    x = centres[shot] + 0.3 * torch.randn((n, D), generator=g, device="cuda") / D ** 0.5
    index.add(x / x.norm(dim=1, keepdim=True))
seg = torch.arange(0, N + 1, SEG, dtype=torch.int64, device="cuda")
print(f"# bench_moments: {N} x {D} rows ({N * D * 4 / 1e6:.1f} MB float32) in {N // SEG} videos of {SEG} rows, shots of {SHOT} rows around "
      f"{NCENT} centres, max_gap = {GAP}, k = {K}", flush=True)
print("  nq | threshold |   hot % | moments | topk ms | range ms | score ms | runs ms | tail ms | score % | flat ms | topk/flat | host ms | "
      "host/range", flush=True)
gq = torch.Generator(device="cuda").manual_seed(4321)
for nq in ((1, 64) if args.quick else (1, 64, 1000)):
    j = torch.randint(0, NCENT, (nq,), generator=gq, device="cuda")
    Q = centres[j] + 0.5 * torch.randn((nq, D), generator=gq, device="cuda") / D ** 0.5
    Q = (Q / Q.norm(dim=1, keepdim=True)).contiguous()
    # the scores of the batch's own shots, for the ragged threshold: every hit of a range search at 0.5
    own = index.range_search_device(Q, 0.5)[1]
    for name, thr in (("clean", 0.5), ("ragged", float(own.median().item()))):
        lims, Dm, Im, Lo, Hi, Cnt, total = moment_range_search_device(index, Q, thr, GAP, seg)
        total = int(total.item())
        hot = int(Cnt.sum().item()) / (nq * N)
        t_topk = event_ms(lambda: moment_search_device(index, Q, K, thr, GAP, seg_off=seg))
        t_range = event_ms(lambda: moment_range_search_device(index, Q, thr, GAP, seg, cap=total))
        prof = profiled(lambda: moment_search_device(index, Q, K, thr, GAP, seg_off=seg))
        score, runs, tail = prof.get("seq_score", 0.0), prof.get("mom_runs", 0.0), prof.get("mom_tail", 0.0)
        t_flat = event_ms(lambda: index.search_device(Q, K))

        # range_search tests > where the moment search tests >=: the float32 just below the threshold as radius gives the same rows
        radius = float(np.nextafter(np.float32(thr), np.float32(-np.inf)))

        def host_route():
            hl, hd, hi_, _ = index.range_search_device(Q, radius)
            return host_merge(hl.cpu().numpy(), hd.cpu().numpy(), hi_.cpu().numpy(), SEG, GAP)

        host_route()
        ts = []
        for _ in range(3):
            t0 = time.perf_counter()
            found = host_route()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        agree = len(found[0]) == total and np.array_equal(found[0], Lo.cpu().numpy()) and np.array_equal(found[3], Im.cpu().numpy())
        print(f"{nq:4d} | {name:6s} {thr:.2f} | {100 * hot:7.4f} | {total / nq:7.1f} | {t_topk:7.4f} | {t_range:8.4f} | {score:8.4f} | {runs:7.4f} | "
              f"{tail:7.4f} | {100 * score / max(score + runs + tail, 1e-9):7.1f} | {t_flat:7.4f} | {t_topk / t_flat:9.2f} | {sorted(ts)[1]:7.2f} | "
              f"{sorted(ts)[1] / t_range:10.2f}{'' if agree else '   (host route differs)'}", flush=True)
