#!/usr/bin/env python3
"""IVFFlatIndex against FlatIPIndex on the same rows: time, index bytes read per second and recall@10 per (nprobe, nq) cell, plus the
wall time of train and add.

    python tools/bench_ivf.py [--rows 1000000] [--nlist 1000] [--timeout 600]

Rows: `--rows` x 512 unit-norm float32 around `--nlist` random unit centres, row = normalize(centre[j] + g / sqrt(d)) with j uniform
and g standard normal (noise as long as the centre itself: cos(row, centre) is about 0.7, so lists overlap), drawn on the device by
torch.Generator(device="cuda").manual_seed(1234) in blocks of 250,000 rows: centres first, then per block j and g.  Queries: 1000 more
rows of the same distribution from manual_seed(4321), the first nq of them.  k = 10.

The run is a chain of steps, each a child process of its own under `timeout`; a step that fails ends the chain.
    build          generate, train (k-means defaults: niter=10, seed=1234, 256 points per centroid, spherical), add; wall times; the
                   centroids go to --workdir so that the other steps add the same lists without training again
    measure NQ     generate, add to both indexes, and per nprobe: 3 warm-up calls, then the median over repeated search_device calls
                   (queries resident on the device) of the time between two device events around one call
Index bytes read are counted from shapes, not measured: for the flat search ntotal x 512 x 2 (one pass over the bf16 scan copy, which
holds for nq <= 1024), for the IVF search sum over lists of ceil(queries probing the list / 16) x rows x 512 x 4 (a list's float32
tiles once per 16 queries that probe it; the coarse search over nlist centroids is left out).  GB/s = those bytes over the median
time."""
import argparse
import os
import subprocess
import sys
import tempfile
import time

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=1_000_000)
ap.add_argument("--nlist", type=int, default=1000)
ap.add_argument("--timeout", type=int, default=600, help="seconds per step")
ap.add_argument("--workdir", default=None, help="where the build step leaves the centroids (default: a temporary directory)")
ap.add_argument("--step", default=None, help="internal: build | measure")
ap.add_argument("--nq", type=int, default=1)
args = ap.parse_args()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D, K, NQS = 512, 10, (1, 10, 1000)

if args.step is None:
    work = args.workdir or tempfile.mkdtemp(prefix="bench_ivf_")
    os.makedirs(work, exist_ok=True)
    base = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--rows", str(args.rows), "--nlist", str(args.nlist),
            "--workdir", work]
    for step in [["--step", "build"]] + [["--step", "measure", "--nq", str(nq)] for nq in NQS]:
        rc = subprocess.run(base + step).returncode
        if rc != 0:
            print(f"step {' '.join(step)} ended with status {rc}: stopping", flush=True)
            sys.exit(rc)
    sys.exit(0)

sys.path.insert(0, os.path.join(ROOT, "intelligent-video-analysis-retrieval-system_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from ivr_amd.index import FlatIPIndex  # noqa: E402
from ivr_amd.ivf import IndexIVFFlat, IVFFlatIndex  # noqa: E402

assert torch.cuda.is_available(), "bench_ivf.py needs a GPU"
N, NLIST = args.rows, args.nlist
CENT = os.path.join(args.workdir, "centroids.npy")


def draw(g, centres, n):
    j = torch.randint(0, len(centres), (n,), generator=g, device="cuda")
    x = centres[j] + torch.randn((n, D), generator=g, device="cuda") / D ** 0.5
    return x / x.norm(dim=1, keepdim=True)


def rows():
    g = torch.Generator(device="cuda").manual_seed(1234)
    c = torch.randn((NLIST, D), generator=g, device="cuda")
    c = c / c.norm(dim=1, keepdim=True)
    return c, torch.cat([draw(g, c, min(250_000, N - i)) for i in range(0, N, 250_000)])


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def event_ms(fn, budget_s=1.0):
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
    return ts[len(ts) // 2], len(ts)


centres, X = rows()
if args.step == "build":
    print(f"# bench_ivf: {N} x {D} rows around {NLIST} centres, nlist = {NLIST}, k = {K}", flush=True)
    ivf = IVFFlatIndex(D, NLIST)
    t_train = wall(lambda: ivf.train(X))
    t_add = wall(lambda: ivf.add(X))
    sizes = ivf.list_sizes()
    print(f"train (k-means on {min(N, 256 * NLIST)} sampled rows, 10 iterations): {t_train:.3f} s wall", flush=True)
    print(f"add ({N} rows, one call): {t_add:.3f} s wall; list sizes min {sizes.min()} median {int(np.median(sizes))} max {sizes.max()}", flush=True)
    np.save(CENT, ivf.centroids)
    sys.exit(0)

nq = args.nq
quant = FlatIPIndex(D)
quant.add(np.load(CENT))
ivf = IndexIVFFlat(quant, D, NLIST)
ivf.train(None)
ivf.add(X)
flat = FlatIPIndex(D, capacity=N)
flat.add(X)
Q = draw(torch.Generator(device="cuda").manual_seed(4321), centres, 1000)[:nq].contiguous()
del X
sizes = ivf.list_sizes()
Df, If = flat.search_device(Q, K)
t_flat, reps = event_ms(lambda: flat.search_device(Q, K))
flat_bytes = N * D * 2
print(f"## nq = {nq}: FlatIPIndex.search {t_flat:.4f} ms (median of {reps}), {flat_bytes / t_flat / 1e6:.0f} GB/s of index read, recall@10 1.0000 (the comparator)",
      flush=True)
print("nprobe |     ms (reps) |   GB/s | recall@10 | ms / flat ms", flush=True)
If_h = If.cpu().numpy()
for nprobe in (1, 8, 32, NLIST):
    Di, Ii = ivf.search_device(Q, K, nprobe=nprobe)
    Ii_h = Ii.cpu().numpy()
    recall = float(np.mean([len(set(Ii_h[i]) & set(If_h[i])) / K for i in range(nq)]))
    if nprobe >= NLIST:
        assert recall == 1.0, f"recall at nprobe = nlist is {recall}"
        assert torch.equal(Di.view(torch.int32), Df.view(torch.int32)), "scores at nprobe = nlist differ from the flat search"
        probes = np.full(NLIST, nq)
    else:
        probes = np.bincount(quant.search_device(Q, nprobe)[1].cpu().numpy().ravel(), minlength=NLIST)
    ivf_bytes = float((-(-probes // 16) * sizes).sum()) * D * 4
    t, reps = event_ms(lambda: ivf.search_device(Q, K, nprobe=nprobe))
    print(f"{nprobe:6d} | {t:9.4f} ({reps:3d}) | {ivf_bytes / t / 1e6:6.0f} | {recall:9.4f} | {t / t_flat:8.3f}", flush=True)
