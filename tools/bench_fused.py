#!/usr/bin/env python3
"""Fused search (ivr_amd/fusion.py: fused_search_device) against the flat search of the same nq m vectors, which does the same
multiply-adds and answers m questions instead of one, and against the route a caller without it has to take: m searches at k = 2048,
the hits copied to the host and joined there in a dictionary per fused query, a row that misses a list counting as score 0 there (the
reference's _combine_search_results).

    python tools/bench_fused.py [--rows 1000000] [--shot 100] [--centres 1000] [--timeout 1100] [--quick]

Rows: `--rows` x 512 unit-norm float32 in shots of `--shot` rows; a shot is one of `--centres` random unit centres plus
0.3 g / sqrt(d) per row.  Drawn on the device by torch.Generator(device="cuda").manual_seed(1234).  The m members of a fused query are
normalize(centre + 0.5 g / sqrt(d)) for m different centres (manual_seed(4321)): m concepts, each with its own near rows.

Grid: m in {2, 4, 8}, nq in {1, 64, 1000} fused queries, k = 10; the first cell is measured again behind the grid, on the same members
(the last line).  The measurement is one child process under `timeout`.  Before the
grid, singleton sets are checked against search_device at the full size, bit for bit.  Per grid point:
    call       median ms of fused_search_device (fold = max) between two device events after 3 warm-up calls, members on the device; the
               call stages its tables from the host and waits for the stream once
    score / select   the two passes of one profiled call (event pairs lengthen the call: compare them with each other, not with the
               median)
    flat       FlatIPIndex.search_device of the nq m member vectors at k = 10
    host       m search_device calls at k = 2048, the hits copied to the host and joined per fused query; wall clock, the median of 3
               runs (one run at nq = 1000)
    max / min  the share of the true fused top-10 (fused_search_device, fold = max / min) that the join finds under that fold"""
import argparse
import os
import subprocess
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=1_000_000)
ap.add_argument("--shot", type=int, default=100)
ap.add_argument("--centres", type=int, default=1000)
ap.add_argument("--timeout", type=int, default=1100, help="seconds for the measuring process")
ap.add_argument("--quick", action="store_true", help="m = 2 and 8, nq = 1 and 64 only")
ap.add_argument("--step", default=None, help="internal: measure")
args = ap.parse_args()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D, NCENT, SHOT, K, KHOST = 512, args.centres, args.shot, 10, 2048

if args.step is None:
    cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--rows", str(args.rows), "--shot", str(args.shot),
           "--centres", str(args.centres), "--step", "measure"] + (["--quick"] if args.quick else [])
    rc = subprocess.run(cmd).returncode
    if rc != 0:
        print(f"the measuring process ended with status {rc}", flush=True)
    sys.exit(rc)

sys.path.insert(0, os.path.join(ROOT, "intelligent-video-analysis-retrieval-system_amd"))
import time  # noqa: E402

import numpy as np  # noqa: E402
import torch  # noqa: E402

from ivr_amd import _ffi  # noqa: E402
from ivr_amd.fusion import fused_search_device  # noqa: E402
from ivr_amd.index import FlatIPIndex  # noqa: E402

assert torch.cuda.is_available(), "bench_fused.py needs a GPU"
N = args.rows
assert N % SHOT == 0 and 250_000 % SHOT == 0


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
    return {name: (v["ms"], v["launches"]) for name, v in prof.items()}


def join(Dh, Ih, fold):
    """The host join of one fused query: Dh, Ih [m,KHOST] -> its K best rows by the fold of the list scores, 0 for a missing one."""
    m = len(Ih)
    seen = {}
    for j in range(m):
        for s, r in zip(Dh[j].tolist(), Ih[j].tolist()):
            if r >= 0:
                seen.setdefault(r, [0.0] * m)[j] = s
    f = max if fold == "max" else min
    return [r for _, r in sorted((-f(v), r) for r, v in seen.items())[:K]]


g = torch.Generator(device="cuda").manual_seed(1234)
centres = torch.randn((NCENT, D), generator=g, device="cuda")
centres = centres / centres.norm(dim=1, keepdim=True)
index = FlatIPIndex(D)
for i in range(0, N, 250_000):
    n = min(250_000, N - i)
    shot = torch.randint(0, NCENT, (n // SHOT,), generator=g, device="cuda").repeat_interleave(SHOT)
    x = centres[shot] + 0.3 * torch.randn((n, D), generator=g, device="cuda") / D ** 0.5
    index.add(x / x.norm(dim=1, keepdim=True))
print(f"# bench_fused: {N} x {D} rows ({N * D * 4 / 1e6:.1f} MB float32), shots of {SHOT} rows around {NCENT} centres, k = {K}, "
      f"host route at k = {KHOST}", flush=True)
gq = torch.Generator(device="cuda").manual_seed(4321)


def members(nq, m):
    j = torch.stack([torch.randperm(NCENT, generator=gq, device="cuda")[:m] for _ in range(nq)])
    Q = centres[j] + 0.5 * torch.randn((nq, m, D), generator=gq, device="cuda") / D ** 0.5
    return (Q / Q.norm(dim=2, keepdim=True)).contiguous()


# singleton sets with weight 1 are the flat search, at the size that is timed
Q1 = members(17, 1)
Ds, Is = index.search_device(Q1[:, 0].contiguous(), K)
for fold in ("max", "min", "sum"):
    Df, If = fused_search_device(index, Q1, K, fold=fold)
    assert torch.equal(If, Is) and torch.equal(Df.view(torch.int32), Ds.view(torch.int32)), f"singleton sets differ from search ({fold})"
print("# singleton sets: rows and score bits equal to search_device for 17 queries, every fold", flush=True)
print("  m |   nq |   call ms | score ms | select ms |  flat ms | call/flat |   host ms | host/call | join max | join min", flush=True)
grid_m, grid_nq = ((2, 8), (1, 64)) if args.quick else ((2, 4, 8), (1, 64, 1000))


def measure(m, nq, Q):
    """one line of the table: nq fused queries of m members, Q [nq,m,D] on the device"""
    flatq = Q.reshape(nq * m, D).contiguous()
    call = lambda: fused_search_device(index, Q, K, fold="max")          # noqa: E731
    t_call = event_ms(call)
    prof = {k: v[0] for k, v in profiled(call).items()}
    t_flat = event_ms(lambda: index.search_device(flatq, K))
    true = {fold: fused_search_device(index, Q, K, fold=fold)[1].cpu().numpy() for fold in ("max", "min")}

    def host_route():
        Dh, Ih = [], []
        for j in range(m):
            Dj, Ij = index.search_device(Q[:, j].contiguous(), KHOST)
            Dh.append(Dj.cpu().numpy())
            Ih.append(Ij.cpu().numpy())
        Dh, Ih = np.stack(Dh, axis=1), np.stack(Ih, axis=1)             # [nq,m,KHOST]
        return {fold: [join(Dh[q], Ih[q], fold) for q in range(nq)] for fold in ("max",)}, Dh, Ih

    ts = []
    for _ in range(1 if nq >= 1000 else 3):
        t0 = time.perf_counter()
        found, Dh, Ih = host_route()
        ts.append((time.perf_counter() - t0) * 1e3)
    t_host = sorted(ts)[len(ts) // 2]
    found["min"] = [join(Dh[q], Ih[q], "min") for q in range(nq)]
    share = {fold: sum(len(set(found[fold][q]) & set(true[fold][q].tolist())) for q in range(nq)) / (nq * K) for fold in ("max", "min")}
    print(f"{m:3d} | {nq:4d} | {t_call:9.4f} | {prof.get('fused_score', 0.0):8.4f} | {prof.get('select_final', 0.0):9.4f} | {t_flat:8.4f} | "
          f"{t_call / t_flat:9.2f} | {t_host:9.2f} | {t_host / t_call:9.2f} | {share['max']:8.3f} | {share['min']:8.3f}", flush=True)


# the first cell is measured once more behind the grid, on the same members (the last line of the table): what only the first cell of
# a process pays shows as a difference between the two lines
cells = [(m, nq) for m in grid_m for nq in grid_nq]
first_Q = members(cells[0][1], cells[0][0])
for i, (m, nq) in enumerate(cells):
    measure(m, nq, first_Q if i == 0 else members(nq, m))
measure(cells[0][0], cells[0][1], first_Q)
