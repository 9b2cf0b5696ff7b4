#!/usr/bin/env python3
"""Diversified search (ivr_amd/diversify.py: mmr_search_device, dedup_search_device) against what the parent commit offers: the flat
search at fetch_k alone, which is the price of the candidates, and the only route to a diversified list there: search_and_reconstruct
at fetch_k, fetch_k x d floats per query copied to the host, and a numpy greedy loop.

    python tools/bench_diverse.py [--rows 1000000] [--segment 500] [--shot 20] [--centres 1000] [--timeout 900] [--quick]

Rows: `--rows` x 512 unit-norm float32 in videos of `--segment` rows; a video is cut into shots of `--shot` rows.  A shot has a centre
of its own, one of `--centres` random unit scene centres plus 0.5 g / sqrt(d), and its rows are that centre plus 0.15 g / sqrt(d)
each: the rows of one shot lie at a cosine of about 0.98 to each other (near-duplicates above the 0.95 of dedup_search), two shots of
one scene at about 0.8.  Drawn on the device by torch.Generator(device="cuda").manual_seed(1234).  A query is normalize(scene centre +
0.5 g / sqrt(d)) (manual_seed(4321)).

Grid: nq in {1, 64, 1000} x (k, fetch_k) in {(10, 50), (10, 200), (50, 1000)} x {MMR at lambda 0.5, suppress at 0.95}.  The
measurement is one child process under `timeout`.  Per grid point:
    call     median ms of the whole call (search + re-ranking) between two device events after 3 warm-up calls, queries on the device
    score / select   the two launches of the re-ranking from one profiled call (event pairs lengthen the call: compare them with
             each other, not with the median)
    flat     baseline (a): FlatIPIndex.search_device of the batch at fetch_k
    host     baseline (b): search_and_reconstruct_device at fetch_k, D, I and the rows copied to the host, the greedy loop in numpy;
             host clock, median of 3 (one run at nq = 1000)
    shots    distinct shots among the first k hits, mean over the queries: of the plain search at k, and of this call
"""
import argparse
import os
import subprocess
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=1_000_000)
ap.add_argument("--segment", type=int, default=500)
ap.add_argument("--shot", type=int, default=20)
ap.add_argument("--centres", type=int, default=1000)
ap.add_argument("--timeout", type=int, default=900, help="seconds for the measuring process")
ap.add_argument("--quick", action="store_true", help="nq = 1 and 64, the first two (k, fetch_k) only")
ap.add_argument("--step", default=None, help="internal: measure")
args = ap.parse_args()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D, NCENT, SHOT, LAMBDA, THRESHOLD = 512, args.centres, args.shot, 0.5, 0.95

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
from ivr_amd.diversify import dedup_search_device, mmr_search_device  # noqa: E402
from ivr_amd.index import FlatIPIndex  # noqa: E402

assert torch.cuda.is_available(), "bench_diverse.py needs a GPU"
N, SEG = args.rows, args.segment
assert N % SEG == 0 and SEG % SHOT == 0 and 250_000 % SHOT == 0


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


def host_greedy(Dh, Ih, Rh, k, mode):
    """The greedy loop a caller of the parent commit writes: scores against the chosen row by a matrix-vector product per step."""
    out = np.full((len(Dh), k), -1, np.int64)
    for q in range(len(Dh)):
        rel, rows = Dh[q], Rh[q]
        live = Ih[q] >= 0
        m = np.full(len(rel), -np.inf, np.float32)
        for t in range(k):
            if not live.any():
                break
            value = rel if (mode == "suppress" or t == 0) else LAMBDA * rel - (1.0 - LAMBDA) * m
            s = int(np.argmax(np.where(live, value, -np.inf)))
            out[q, t] = Ih[q, s]
            live[s] = False
            m = np.maximum(m, rows @ rows[s])
            if mode == "suppress":
                live &= m < THRESHOLD
    return out


def shots_in(I):
    I = I.cpu().numpy() if isinstance(I, torch.Tensor) else I
    return float(np.mean([len({int(r) // SHOT for r in row if r >= 0}) for row in I]))


g = torch.Generator(device="cuda").manual_seed(1234)
centres = torch.randn((NCENT, D), generator=g, device="cuda")
centres = centres / centres.norm(dim=1, keepdim=True)
index = FlatIPIndex(D)
for i in range(0, N, 250_000):
    n = min(250_000, N - i)
    scene = torch.randint(0, NCENT, (n // SHOT,), generator=g, device="cuda")
    shot = centres[scene] + 0.5 * torch.randn((n // SHOT, D), generator=g, device="cuda") / D ** 0.5
    x = shot.repeat_interleave(SHOT, dim=0) + 0.15 * torch.randn((n, D), generator=g, device="cuda") / D ** 0.5
    index.add(x / x.norm(dim=1, keepdim=True))
print(f"# bench_diverse: {N} x {D} rows ({N * D * 4 / 1e6:.1f} MB float32) in {N // SEG} videos of {SEG} rows, shots of {SHOT} near-duplicate "
      f"rows, {NCENT} scene centres; MMR at lambda {LAMBDA}, suppress at {THRESHOLD}", flush=True)
print("  nq |  k | fetch_k | mode     |  call ms | score ms | select ms | flat ms | call/flat |  host ms | host/call | shots plain | shots here",
      flush=True)
gq = torch.Generator(device="cuda").manual_seed(4321)
grid_nq = (1, 64) if args.quick else (1, 64, 1000)
grid_k = ((10, 50), (10, 200)) if args.quick else ((10, 50), (10, 200), (50, 1000))
for nq in grid_nq:
    j = torch.randint(0, NCENT, (nq,), generator=gq, device="cuda")
    Q = centres[j] + 0.5 * torch.randn((nq, D), generator=gq, device="cuda") / D ** 0.5
    Q = (Q / Q.norm(dim=1, keepdim=True)).contiguous()
    for k, fetch_k in grid_k:
        t_flat = event_ms(lambda: index.search_device(Q, fetch_k))
        plain = shots_in(index.search_device(Q, k)[1])
        for mode in ("mmr", "suppress"):
            if mode == "mmr":
                call = lambda: mmr_search_device(index, Q, k, fetch_k, LAMBDA)              # noqa: E731
            else:
                call = lambda: dedup_search_device(index, Q, k, fetch_k, THRESHOLD)        # noqa: E731
            t_call = event_ms(call)
            prof = profiled(call)
            here = shots_in(call()[1])

            def host_route():
                Dh, Ih, Rh = (t.cpu().numpy() for t in index.search_and_reconstruct_device(Q, fetch_k))
                return host_greedy(Dh, Ih, Rh, k, mode)

            ts = []
            for _ in range(3 if nq <= 64 else 1):
                t0 = time.perf_counter()
                host_route()
                ts.append((time.perf_counter() - t0) * 1e3)
            t_host = sorted(ts)[len(ts) // 2]
            print(f"{nq:4d} | {k:2d} | {fetch_k:7d} | {mode:8s} | {t_call:8.4f} | {prof.get('refine_score', 0.0):8.4f} | "
                  f"{prof.get('diverse_select', 0.0):9.4f} | {t_flat:7.4f} | {t_call / t_flat:9.2f} | {t_host:8.2f} | {t_host / t_call:9.1f} | "
                  f"{plain:11.2f} | {here:10.2f}", flush=True)
