#!/usr/bin/env python3
"""IndexLSH (256 sign bits, Hamming top-k by counting) against FlatIPIndex on the same rows: time of add, of search with its encode
share, and the share of the flat top-10 that the LSH top-100 contains.

    python tools/bench_lsh.py [--rows 1000000] [--nbits 256] [--timeout 600]

Rows: `--rows` x 512 unit-norm float32 around 1000 random unit centres, row = normalize(centre[j] + g / sqrt(d)) with j uniform and g
standard normal, drawn on the device by torch.Generator(device="cuda").manual_seed(1234) in blocks of 250,000 rows: centres first,
then per block j and g (the rows of tools/bench_ivf.py).  Queries: 1000 more rows of the same distribution from manual_seed(4321),
the first nq of them.

The run is a chain of steps, each a child process of its own under `timeout`; a step that fails ends the chain.
    add            generate; median device-event time of IndexLSH.add (encode + store, rows resident on the device, the index reset
                   before every call) and of the encoder alone
    measure NQ     generate, add to both indexes, and per k in (10, 100): 3 warm-up calls, then the median over repeated calls
                   (queries resident on the device) of the time between two device events around IndexLSH.search_device, around the
                   query encoder alone, and around FlatIPIndex.search_device; then one profiled search per k (event pairs around
                   every kernel, which lengthen the call: read the shares, not the sum) to show which pass the time goes to
Recall: |flat top-10  &  LSH top-100| / 10, averaged over the nq queries."""
import argparse
import os
import subprocess
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=1_000_000)
ap.add_argument("--nbits", type=int, default=256)
ap.add_argument("--timeout", type=int, default=600, help="seconds per step")
ap.add_argument("--step", default=None, help="internal: add | measure")
ap.add_argument("--nq", type=int, default=1)
args = ap.parse_args()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D, NCENT, NQS, KS = 512, 1000, (1, 10, 1000), (10, 100)

if args.step is None:
    base = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--rows", str(args.rows), "--nbits", str(args.nbits)]
    for step in [["--step", "add"]] + [["--step", "measure", "--nq", str(nq)] for nq in NQS]:
        rc = subprocess.run(base + step).returncode
        if rc != 0:
            print(f"step {' '.join(step)} ended with status {rc}: stopping", flush=True)
            sys.exit(rc)
    sys.exit(0)

sys.path.insert(0, os.path.join(ROOT, "intelligent-video-analysis-retrieval-system_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from ivr_amd import _ffi  # noqa: E402
from ivr_amd.binary import IndexLSH  # noqa: E402
from ivr_amd.index import FlatIPIndex  # noqa: E402

assert torch.cuda.is_available(), "bench_lsh.py needs a GPU"
N, NBITS = args.rows, args.nbits


def draw(g, centres, n):
    j = torch.randint(0, len(centres), (n,), generator=g, device="cuda")
    x = centres[j] + torch.randn((n, D), generator=g, device="cuda") / D ** 0.5
    return x / x.norm(dim=1, keepdim=True)


def rows():
    g = torch.Generator(device="cuda").manual_seed(1234)
    c = torch.randn((NCENT, D), generator=g, device="cuda")
    c = c / c.norm(dim=1, keepdim=True)
    return c, torch.cat([draw(g, c, min(250_000, N - i)) for i in range(0, N, 250_000)])


def event_ms(fn, budget_s=1.0, before=None):
    """median ms between two device events around fn(), after 3 warm-up calls; enough repeats to fill budget_s, 5 to 100"""
    for _ in range(3):
        if before:
            before()
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ts = []
    reps = 5
    while len(ts) < reps:
        if before:
            before()
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
        if len(ts) == 1:
            reps = int(min(100, max(5, budget_s * 1e3 / max(ts[0], 1e-3))))
    ts.sort()
    return ts[len(ts) // 2], len(ts)


centres, X = rows()
lsh = IndexLSH(D, NBITS)
if args.step == "add":
    print(f"# bench_lsh: {N} x {D} rows around {NCENT} centres, nbits = {NBITS}; codes {N * lsh.code_size / 1e6:.1f} MB, "
          f"float32 rows {N * D * 4 / 1e6:.1f} MB", flush=True)
    t_add, reps = event_ms(lambda: lsh.add(X), before=lsh.reset)
    t_enc, reps_e = event_ms(lambda: lsh.sa_encode_device(X))
    print(f"add ({N} rows, one call, encode included): {t_add:.3f} ms (median of {reps}); the encoder alone: {t_enc:.3f} ms (median of {reps_e}), "
          f"{2.0 * N * D * NBITS / t_enc / 1e9:.1f} TFLOP/s float32", flush=True)
    sys.exit(0)

nq = args.nq
lsh.add(X)
flat = FlatIPIndex(D, capacity=N)
flat.add(X)
Q = draw(torch.Generator(device="cuda").manual_seed(4321), centres, 1000)[:nq].contiguous()
del X
t_enc, _ = event_ms(lambda: lsh.sa_encode_device(Q))
print(f"## nq = {nq}: query encode {t_enc:.4f} ms", flush=True)
print("  k | LSH search ms (reps) | of which encode | per query | flat search ms (reps) | per query | LSH / flat", flush=True)
for k in KS:
    t_lsh, reps = event_ms(lambda: lsh.search_device(Q, k))
    t_flat, reps_f = event_ms(lambda: flat.search_device(Q, k))
    print(f"{k:3d} | {t_lsh:13.4f} ({reps:3d}) | {t_enc:15.4f} | {t_lsh / nq:9.5f} | {t_flat:14.4f} ({reps_f:3d}) | {t_flat / nq:9.5f} | {t_lsh / t_flat:8.3f}",
          flush=True)
If = flat.search_device(Q, 10)[1].cpu().numpy()
Il = lsh.search_device(Q, 100)[1].cpu().numpy()
recall = float(np.mean([len(set(If[i]) & set(Il[i])) / 10 for i in range(nq)]))
print(f"recall: {recall:.4f} of the flat top-10 inside the LSH top-100", flush=True)
for k in KS:
    torch.cuda.synchronize()
    _ffi.profile_enable(2)
    _ffi.profile_reset()
    lsh.search_device(Q, k)
    torch.cuda.synchronize()
    prof = _ffi.profile_read()
    _ffi.profile_enable(False)
    line = ", ".join(f"{name} {v['ms']:.4f} ms x{v['launches']}" for name, v in sorted(prof.items()) if name.startswith(("bin_", "sign_")))
    print(f"passes of one search, k = {k}: {line}", flush=True)
