#!/usr/bin/env python3
"""Zero-shot tagging (ivr_amd/tagging.py) against the two routes to the same answer that exist without it.

    python tools/bench_tags.py [--rows 1000000] [--videos 2000] [--labels 100,1000,4096] [--top 5] [--timeout 600]

Rows: 512-d unit-norm float32 drawn on the device by torch.Generator(device="cuda").manual_seed(1234), cut into `videos` equal
segments; labels: unit-norm rows from the same generator; scale 100.

Every label count is measured by one child process under `timeout`, one after the other; the first one that fails ends the run.  It
reports
    tag_rows      tag_rows_device(index, labels, top): median time between two device events over at least 5 calls after 2 warm-up
                  calls, labels resident on the device
    tag_segments  tag_segments_device(index, labels, seg_off, 5, "mass", top) likewise, then the kernels of one profiled call (the
                  score pass, the aggregation and the selection; event pairs lengthen the call: read them as shares)
    (a)           a FlatIPIndex holding the labels, searched with the reconstructed rows in chunks of 65,536: cosines only
    (b)           torch.softmax(scale * X @ L.T, 1).topk(top) in chunks of 65,536 rows through rocBLAS
and, once, whether index.rescore_device(labels, rows) (the label as the query) gives the bits of the tagging's scores (the row as the
query) on the first 2,048 rows: an observation, nothing rests on it."""
import argparse
import os
import subprocess
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=1_000_000)
ap.add_argument("--videos", type=int, default=2000)
ap.add_argument("--labels", default="100,1000,4096")
ap.add_argument("--top", type=int, default=5)
ap.add_argument("--timeout", type=int, default=600, help="seconds for each measuring process")
ap.add_argument("--step", type=int, default=None, help="internal: the label count of the measuring process")
args = ap.parse_args()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D, SCALE, BLOCK = 512, 100.0, 1 << 16

if args.step is None:
    for C in args.labels.split(","):
        cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--step", C, "--rows", str(args.rows),
               "--videos", str(args.videos), "--top", str(args.top)]
        rc = subprocess.run(cmd).returncode
        if rc != 0:
            print(f"the measuring process of C = {C} ended with status {rc}: nothing more is started", flush=True)
            sys.exit(rc)
    sys.exit(0)

sys.path.insert(0, os.path.join(ROOT, "intelligent-video-analysis-retrieval-system_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from ivr_amd import _ffi  # noqa: E402
from ivr_amd.index import FlatIPIndex  # noqa: E402
from ivr_amd.tagging import tag_rows_device, tag_segments_device  # noqa: E402

assert torch.cuda.is_available(), "bench_tags.py needs a GPU"
N, NSEG, C, T = args.rows, args.videos, args.step, args.top


def event_ms(fn, budget_s=1.0):
    """median ms between two device events around fn(), after 2 warm-up calls; enough repeats to fill budget_s, 5 to 50"""
    for _ in range(2):
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
            reps = int(min(50, max(5, budget_s * 1e3 / max(ts[0], 1e-3))))
    ts.sort()
    return ts[len(ts) // 2], len(ts)


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
X = torch.randn((N, D), generator=g, device="cuda")
X = (X / X.norm(dim=1, keepdim=True)).contiguous()
L = torch.randn((C, D), generator=g, device="cuda")
L = (L / L.norm(dim=1, keepdim=True)).contiguous()
index = FlatIPIndex(D, capacity=N)
index.add(X)
seg = torch.from_numpy(np.linspace(0, N, NSEG + 1).astype(np.int64)).cuda()
flop = 2.0 * N * C * D
name = f"{N} x {D} rows in {NSEG} videos, C = {C}, top {T}"
print(f"# bench_tags: {name}; {flop / 1e12:.2f} TFLOP of float32 multiply-adds, labels {C * D * 4 / 1e6:.1f} MB", flush=True)

ms, reps = event_ms(lambda: tag_rows_device(index, L, T, SCALE))
print(f"{name}: tag_rows_device: {ms:.3f} ms (device events, median of {reps}), {flop / ms / 1e9:.1f} TFLOP/s", flush=True)
ms, reps = event_ms(lambda: tag_segments_device(index, L, seg, 5, "mass", T, SCALE))
print(f"{name}: tag_segments_device: {ms:.3f} ms (device events, median of {reps})", flush=True)
print(f"{name}: kernels of one profiled tag_segments call: " + profiled(lambda: tag_segments_device(index, L, seg, 5, "mass", T, SCALE)),
      flush=True)

lab_index = FlatIPIndex(D, capacity=C)
lab_index.add(L)
allrows = torch.arange(N, dtype=torch.int64, device="cuda")


def route_a():
    return [lab_index.search_device(index.gather_device(allrows[i:i + BLOCK]), T) for i in range(0, N, BLOCK)]


def route_b():
    out = []
    for i in range(0, N, BLOCK):
        out.append(torch.softmax(SCALE * (X[i:i + BLOCK] @ L.T), 1).topk(min(T, C)))
    return out


ms, reps = event_ms(route_a)
print(f"{name}: (a) label index searched with the gathered rows in blocks of {BLOCK} (cosines only): {ms:.3f} ms (median of {reps})",
      flush=True)
ms, reps = event_ms(route_b)
print(f"{name}: (b) torch.softmax(scale X L^T).topk in blocks of {BLOCK}: {ms:.3f} ms (median of {reps}), {flop / ms / 1e9:.1f} TFLOP/s",
      flush=True)

# agreement with the routes, and the observation on the direction of the score
D_own, P_own, J_own, _, _ = tag_rows_device(index, L, T, SCALE)
J_a = torch.cat([r[1] for r in route_a()])
J_b = torch.cat([r[1] for r in route_b()])
P_b = torch.cat([r[0] for r in route_b()])
k = min(T, C)
print(f"{name}: rows whose first label agrees with (a): {int((J_a[:, 0] == J_own[:, 0]).sum())}, with (b): "
      f"{int((J_b[:, 0] == J_own[:, 0]).sum())} of {N}; largest |P - P of (b)| on the first label: "
      f"{float((P_b[:, 0] - P_own[:, 0]).abs().max()):.3e}", flush=True)
m = min(N, 2048)
S_own = tag_rows_device(index, L, min(C, 64), SCALE, row1=m)
cand = torch.arange(m, dtype=torch.int64, device="cuda").repeat(C, 1).contiguous()
S_rev = index.rescore_device(L, cand)[0]                                       # [C, m]: the label as the query
picked = torch.gather(S_rev.t().contiguous(), 1, S_own[2][:m].clamp(min=0))
equal = (picked.view(torch.int32) == S_own[0][:m].view(torch.int32)) | (S_own[2][:m] < 0)
print(f"{name}: scores with the label as the query (index.rescore_device(labels, rows)) equal to the bit on {int(equal.sum())} of "
      f"{equal.numel()} listed (row, label) pairs of the first {m} rows", flush=True)
