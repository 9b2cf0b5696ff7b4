#!/usr/bin/env python3
"""Clip search (ivr_amd/temporal.py) against the flat searches it would otherwise be assembled from: 64 target frames, window length
L = 5, over `--rows` x 512 stored rows.

    python tools/bench_temporal.py [--rows 1000000] [--frames 64] [--length 5] [--timeout 600]

Rows are those of tools/bench_refine.py: `--rows` x 512 unit-norm float32 around 1000 random unit centres, row = normalize(centre[j] +
g / sqrt(d)), drawn on the device by torch.Generator(device="cuda").manual_seed(1234) in blocks of 250,000 rows.  The target clip is a
noisy copy of `--frames` consecutive stored rows from the middle of the index (normalize(row + 0.3 g / sqrt(d)), manual_seed(4321)), so
that one run of starts scores high and the rest do not.  The index is one segment, and again 1000 equal segments.

The measurement is one child process under `timeout`.  It reports, each as the median time between two device events after 3 warm-up
calls (frames and offsets resident on the device):
    top-k      sequence_search_device(index, Q, L, 10)
    range      sequence_range_search_device(index, Q, L, 0.8, cap = 65536): one pass, no host synchronisation
    flat       FlatIPIndex.search_device(Q, 10): the T single-frame searches as one batch, which answers a different question (the
               best rows per frame, not per window) and is what a caller without clip search has to start from
then the kernels of one profiled top-k and one profiled range call (event pairs around every kernel, which lengthen the call: compare
them with each other, not with the medians), and whether the best start of the middle window is the planted one."""
import argparse
import os
import subprocess
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=1_000_000)
ap.add_argument("--frames", type=int, default=64)
ap.add_argument("--length", type=int, default=5)
ap.add_argument("--timeout", type=int, default=600, help="seconds for the measuring process")
ap.add_argument("--step", default=None, help="internal: measure")
args = ap.parse_args()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D, NCENT, K, THRESHOLD, CAP, NSEG = 512, 1000, 10, 0.8, 65536, 1000

if args.step is None:
    rc = subprocess.run(["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--rows", str(args.rows),
                         "--frames", str(args.frames), "--length", str(args.length), "--step", "measure"]).returncode
    if rc != 0:
        print(f"the measuring process ended with status {rc}", flush=True)
    sys.exit(rc)

sys.path.insert(0, os.path.join(ROOT, "intelligent-video-analysis-retrieval-system_amd"))
import torch  # noqa: E402

from ivr_amd import _ffi  # noqa: E402
from ivr_amd.index import FlatIPIndex  # noqa: E402
from ivr_amd.temporal import sequence_range_search_device, sequence_search_device  # noqa: E402

assert torch.cuda.is_available(), "bench_temporal.py needs a GPU"
N, T, L = args.rows, args.frames, args.length
assert N >= 4 * T and T >= L


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


def profiled(fn):
    torch.cuda.synchronize()
    _ffi.profile_enable(2)
    _ffi.profile_reset()
    fn()
    torch.cuda.synchronize()
    prof = _ffi.profile_read()
    _ffi.profile_enable(False)
    return " ".join(f"{name} {v['ms']:.4f} ms x{v['launches']}" for name, v in sorted(prof.items()))


g = torch.Generator(device="cuda").manual_seed(1234)
centres = torch.randn((NCENT, D), generator=g, device="cuda")
centres = centres / centres.norm(dim=1, keepdim=True)
index = FlatIPIndex(D)
planted = N // 2
clip = None
for i in range(0, N, 250_000):
    block = draw(g, centres, min(250_000, N - i))
    if i <= planted and planted + T <= i + len(block):
        clip = block[planted - i:planted - i + T].clone()
    index.add(block)
assert clip is not None, "the planted clip must lie inside one block of 250,000 rows"
gq = torch.Generator(device="cuda").manual_seed(4321)
Q = clip + 0.3 * torch.randn((T, D), generator=gq, device="cuda") / D ** 0.5
Q = (Q / Q.norm(dim=1, keepdim=True)).contiguous()
seg = torch.linspace(0, N, NSEG + 1, device="cuda").to(torch.int64).contiguous()
print(f"# bench_temporal: {N} x {D} rows around {NCENT} centres ({N * D * 4 / 1e6:.1f} MB float32), {T} target frames, L = {L}: "
      f"{T - L + 1} windows x {N - L + 1} starts, k = {K}, threshold = {THRESHOLD}, cap = {CAP}", flush=True)
t_flat = event_ms(lambda: index.search_device(Q, K))
print(f"flat search of the {T} frames as one batch, k = {K}: {t_flat:.4f} ms", flush=True)
print("segments | top-k ms | range ms | top-k / flat | results >= threshold | best start of the middle window (planted)", flush=True)
for name, s in (("one", None), (str(NSEG), seg)):
    t_top = event_ms(lambda: sequence_search_device(index, Q, L, K, seg_off=s))
    t_rng = event_ms(lambda: sequence_range_search_device(index, Q, L, THRESHOLD, seg_off=s, cap=CAP))
    I = sequence_search_device(index, Q, L, K, seg_off=s)[1]
    total = int(sequence_range_search_device(index, Q, L, THRESHOLD, seg_off=s, cap=CAP)[3].item())
    w = (T - L + 1) // 2
    print(f"{name:>8} | {t_top:8.4f} | {t_rng:8.4f} | {t_top / t_flat:12.3f} | {total:20d} | {int(I[w, 0])} ({planted + w})", flush=True)
print("kernels of one profiled top-k call: " + profiled(lambda: sequence_search_device(index, Q, L, K)), flush=True)
print("kernels of one profiled range call: " + profiled(lambda: sequence_range_search_device(index, Q, L, THRESHOLD, cap=CAP)), flush=True)
