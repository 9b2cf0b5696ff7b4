#!/usr/bin/env python3
"""Grouped search (ivr_amd/grouping.py: group_search_device) against the flat search of the same batch at k = G g, which answers a
different question with the parent's code, and against the route a caller without it has to take: search(k = 2048), the hits copied
to the host and grouped there by video.

    python tools/bench_groups.py [--rows 1000000] [--segment 500] [--shot 100] [--centres 1000] [--timeout 900] [--quick]

Rows: `--rows` x 512 unit-norm float32 in videos of `--segment` rows; a video is cut into shots of `--shot` rows, a shot is one of
`--centres` random unit centres plus 0.3 g / sqrt(d) per row: adjacent keyframes of a shot sit close to each other, and a centre
returns in about rows / shot / centres shots of other videos.  The host route loses groups once the rows close to a query outnumber
its 2,048 hits while lying in fewer than G videos (--shot 500 --centres 400: five videos of 500 such rows).  Drawn on the device by
torch.Generator(device="cuda").manual_seed(1234).  A query is normalize(centre + 0.5 g / sqrt(d)) (manual_seed(4321)).

Grid: nq in {1, 10, 64, 1000}, G = 10, g in {1, 3, 10}.  The measurement is one child process under `timeout`.  Per grid point:
    call       median ms of group_search_device between two device events after 3 warm-up calls (queries and offsets on the device)
    best / select / rows / merge   the passes of one profiled call (event pairs around the passes lengthen the call: compare them
               with each other, not with the median); best = the segment-best pass, select = top-G selection + labels
    score      the clip search's score pass (seq_score) per 16-query tile, from a profiled sequence_search_device at L = 1 over the
               same queries, beside best per 16-query tile: the same bytes read, the first writes every score, the second none
    flat       FlatIPIndex.search_device of the batch at k = G g
    host       search_device at k = 2048, the hits copied to the host, a dict per query keyed by video; `all G` = the share of the
               queries for which that finds all G true groups
and once per layout the atomics the segment-best pass issues per (query, 16-row tile), counted from the segment layout by walking the
tiles as the kernel's waves do."""
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
ap.add_argument("--quick", action="store_true", help="nq = 1 and 64, g = 1 and 3 only")
ap.add_argument("--step", default=None, help="internal: measure")
args = ap.parse_args()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D, NCENT, SHOT, G, KHOST = 512, args.centres, args.shot, 10, 2048

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
from ivr_amd.grouping import group_search_device  # noqa: E402
from ivr_amd.index import FlatIPIndex  # noqa: E402
from ivr_amd.temporal import sequence_search_device  # noqa: E402

assert torch.cuda.is_available(), "bench_groups.py needs a GPU"
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
    return {name: (v["ms"], v["launches"]) for name, v in prof.items()}


def atomics_per_tile(n, seg_off):
    """Atomics per (query column, 16-row tile) of the segment-best pass, by walking the tiles as its waves do: a workgroup owns 64
    tiles, wave w the tiles w, w + 4, ...; a wave issues one atomic per column when its running segment changes, one per further
    segment inside a tile, and one at the end of its walk."""
    rows = np.arange((n + 15) // 16 * 16)
    sg = np.searchsorted(seg_off, rows, side="right") - 1
    sg[rows >= n] = len(seg_off) - 1
    nseg = len(seg_off) - 1
    sg = sg.reshape(-1, 16)
    first, last = sg[:, 0], sg[:, 15]
    inner = np.array([len(np.unique(t)) - 1 for t in sg[first != last]]).sum() if (first != last).any() else 0      # segments in front of a tile's last
    count = int(inner)
    ntiles = len(sg)
    for b0 in range(0, ntiles, 64):
        for w in range(4):
            t = np.arange(b0 + w, min(b0 + 64, ntiles), 4)
            if len(t) == 0:
                continue
            # the running segment is flushed when the next tile starts in another one, and at the end
            runs = last[t]
            nxt = first[t]
            valid = (runs >= 0) & (runs < nseg)
            count += int((valid[:-1] & (runs[:-1] != nxt[1:])).sum()) + int(valid[-1])
    return count / ntiles


g = torch.Generator(device="cuda").manual_seed(1234)
centres = torch.randn((NCENT, D), generator=g, device="cuda")
centres = centres / centres.norm(dim=1, keepdim=True)
index = FlatIPIndex(D)
for i in range(0, N, 250_000):
    n = min(250_000, N - i)
    shot = torch.randint(0, NCENT, (n // SHOT,), generator=g, device="cuda").repeat_interleave(SHOT)
    x = centres[shot] + 0.3 * torch.randn((n, D), generator=g, device="cuda") / D ** 0.5
    index.add(x / x.norm(dim=1, keepdim=True))
seg_host = np.arange(0, N + 1, SEG, dtype=np.int64)
seg = torch.from_numpy(seg_host).cuda()
print(f"# bench_groups: {N} x {D} rows ({N * D * 4 / 1e6:.1f} MB float32) in {N // SEG} videos of {SEG} rows, shots of {SHOT} rows around "
      f"{NCENT} centres, G = {G}, host route at k = {KHOST}", flush=True)
print(f"# atomics of the segment-best pass per (query, 16-row tile): {atomics_per_tile(N, seg_host):.4f} "
      f"(one per row would be 16; every row its own segment: {atomics_per_tile(4096, np.arange(4097)):.1f})", flush=True)
print("  nq |  g |  call ms | best ms | select ms | rows ms | merge ms | best/tile | score/tile | flat ms | call/flat | host ms | all G", flush=True)
gq = torch.Generator(device="cuda").manual_seed(4321)
grid_nq, grid_g = ((1, 64), (1, 3)) if args.quick else ((1, 10, 64, 1000), (1, 3, 10))
for nq in grid_nq:
    j = torch.randint(0, NCENT, (nq,), generator=gq, device="cuda")
    Q = centres[j] + 0.5 * torch.randn((nq, D), generator=gq, device="cuda") / D ** 0.5
    Q = (Q / Q.norm(dim=1, keepdim=True)).contiguous()
    true = group_search_device(index, Q, G, 1, seg_off=seg)[0].cpu().numpy()

    def host_route():
        Ih = index.search_device(Q, KHOST)[1].cpu().numpy()
        out = []
        for q in range(nq):
            seen = {}
            for r in Ih[q]:
                if r >= 0:
                    seen.setdefault(int(r) // SEG, len(seen))
                    if len(seen) == G:
                        break
            out.append(list(seen))
        return out

    host_route()
    ts = []
    for _ in range(3):
        t0 = time.perf_counter()
        found = host_route()
        ts.append((time.perf_counter() - t0) * 1e3)
    all_g = sum(found[q] == [int(s) for s in true[q] if s >= 0] for q in range(nq)) / nq
    # the score pass alone: a clip search at L = 1 scores the same queries in chunks; per 16-query tile it launched
    sp = profiled(lambda: sequence_search_device(index, Q, 1, G))
    wc = max(1, min(nq, (1 << 25) // N, 4096))
    seq_tiles = sum(((w0 + min(wc, nq - w0) - 1) >> 4) - (w0 >> 4) + 1 for w0 in range(0, nq, wc))
    score_tile = sp.get("seq_score", (0.0, 0))[0] / seq_tiles
    for gsz in grid_g:
        call = lambda: group_search_device(index, Q, G, gsz, seg_off=seg)      # noqa: E731
        t_call = event_ms(call)
        prof = {k: v[0] for k, v in profiled(call).items()}
        t_flat = event_ms(lambda: index.search_device(Q, G * gsz))
        print(f"{nq:4d} | {gsz:2d} | {t_call:8.4f} | {prof.get('grp_segbest', 0.0):7.4f} | {prof.get('grp_select', 0.0):9.4f} | "
              f"{prof.get('grp_rows', 0.0):7.4f} | {prof.get('grp_merge', 0.0):8.4f} | {prof.get('grp_segbest', 0.0) / ((nq + 15) // 16):9.4f} | "
              f"{score_tile:10.4f} | {t_flat:7.4f} | {t_call / t_flat:9.2f} | {sorted(ts)[1]:7.2f} | {all_g:5.2f}", flush=True)
