#!/usr/bin/env python3
"""IndexIVFPQ (inverted lists over M-byte codes) alone and as the base of IndexRefineFlat, against FlatIPIndex, IndexPQ and
IndexIVFFlat at the same nprobe on the same rows: what training, adding and searching cost and what recall the probed codes keep.

    python tools/bench_ivfpq.py [--rows 1000000] [--nlist 1024] [--timeout 900] [--ab]

Rows and queries are those of tools/bench_pq.py: `--rows` x 512 unit-norm float32 around 1000 random unit centres, row =
normalize(centre[j] + g / sqrt(d)), drawn on the device by torch.Generator(device="cuda").manual_seed(1234) in blocks of 250,000 rows;
queries: 1000 more rows of the same distribution from manual_seed(4321), the first nq of them.  k = 10.

The run is a chain of steps, one per M in (32, 64), each a child process of its own under `timeout`; a step that fails ends the chain.
A step generates the rows, trains IndexIVFFlat(nlist) on the first block, gives IndexIVFPQ(nlist, M) a quantizer holding the same
centroids (so both probe the same lists), trains its codebooks on the residuals of the first block and an IndexPQ(512, M) on the block
itself (wall clock around a device synchronisation), adds every block to all of them (IndexIVFPQ through IndexRefineFlat, whose
refine_index is the FlatIPIndex the comparison uses) and then reports, per nq in (1, 64, 1000):
    flat, pq    FlatIPIndex.search_device(Q, 10) and IndexPQ.search_device(Q, 10)
and per nprobe in (1, 16, 64):
    ivfpq       IndexIVFPQ.search_device(Q, 10, nprobe), with the kernels of one profiled call (event pairs around every kernel
                lengthen the call: compare them with each other, not with the medians)
    ivfflat     IndexIVFFlat.search_device(Q, 10, nprobe=nprobe)
    refine      IndexRefineFlat(IndexIVFPQ).search_device(Q, 10, k_factor) at k_factor 1, 4 and 16
each as the median time between two device events after 3 warm-up calls (queries resident on the device), with recall@10 =
|top-10 & flat top-10| / 10 averaged over the queries.

--ab (M = 64 only) repeats the ivfpq timings on indexes made with IVR_IVFPQ_GROUPS_PER_WG = 8, 32 and 512 beside the default 128: the
64-row groups a scan workgroup takes per copy of a query's table."""
import argparse
import os
import subprocess
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=1_000_000)
ap.add_argument("--nlist", type=int, default=1024)
ap.add_argument("--timeout", type=int, default=900, help="seconds per step")
ap.add_argument("--ab", action="store_true", help="also time other shares of the scan (M = 64)")
ap.add_argument("--step", default=None, help="internal: measure")
ap.add_argument("--M", type=int, default=64)
args = ap.parse_args()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D, NCENT, NQS, K, KFS, MS, NPROBES, AB = 512, 1000, (1, 64, 1000), 10, (1, 4, 16), (32, 64), (1, 16, 64), (8, 32, 512)

if args.step is None:
    base = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--rows", str(args.rows), "--nlist",
            str(args.nlist)] + (["--ab"] if args.ab else [])
    for step in [["--step", "measure", "--M", str(m)] for m in MS]:
        rc = subprocess.run(base + step).returncode
        if rc != 0:
            print(f"step {' '.join(step)} ended with status {rc}: stopping", flush=True)
            sys.exit(rc)
    sys.exit(0)

sys.path.insert(0, os.path.join(ROOT, "intelligent-video-analysis-retrieval-system_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from ivr_amd import _ffi  # noqa: E402
from ivr_amd.index import FlatIPIndex  # noqa: E402
from ivr_amd.ivf import IndexIVFFlat  # noqa: E402
from ivr_amd.ivfpq import IndexIVFPQ  # noqa: E402
from ivr_amd.pq import IndexPQ  # noqa: E402
from ivr_amd.refine import IndexRefineFlat  # noqa: E402

assert torch.cuda.is_available(), "bench_ivfpq.py needs a GPU"
N, M, NLIST = args.rows, args.M, args.nlist


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


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def recall(I, If):
    return float(np.mean([len(set(If[i]) & set(I[i])) / K for i in range(len(If))]))


def blocks():
    g = torch.Generator(device="cuda").manual_seed(1234)
    centres = torch.randn((NCENT, D), generator=g, device="cuda")
    centres = centres / centres.norm(dim=1, keepdim=True)
    for i in range(0, N, 250_000):
        yield i, draw(g, centres, min(250_000, N - i)), centres


def same_quantizer(ivf):
    q = FlatIPIndex(D)
    q.add(ivf.centroids)
    return q


ivfflat = IndexIVFFlat(FlatIPIndex(D), D, NLIST)
pq = IndexPQ(D, M)
ivfpq = index = None
t = {"coarse": 0.0, "fine": 0.0, "pq": 0.0, "add": 0.0, "add_flat": 0.0}
for i, x, centres in blocks():
    if i == 0:
        t["coarse"] = wall_ms(lambda: ivfflat.train(x))
        ivfpq = IndexIVFPQ(same_quantizer(ivfflat), D, NLIST, M)
        index = IndexRefineFlat(ivfpq)
        t["fine"] = wall_ms(lambda: ivfpq.train(x))
        t["pq"] = wall_ms(lambda: pq.train(x))
    t["add"] += wall_ms(lambda: ivfpq.add(x))
    t["add_flat"] += wall_ms(lambda: ivfflat.add(x))
    index.refine_index.add(x)
    pq.add(x)
    del x
flat = index.refine_index
Qall = draw(torch.Generator(device="cuda").manual_seed(4321), centres, 1000)
sizes = ivfpq.list_sizes()
print(f"# bench_ivfpq: {N} x {D} rows around {NCENT} centres, nlist = {NLIST}, M = {M} (dsub = {D // M}), k = {K}; codes "
      f"{N * M / 1e6:.1f} MB ({int(((sizes + 63) // 64).sum()) * 64 * M / 1e6:.1f} MB padded), float32 rows {N * D * 4 / 1e6:.1f} MB; lists of "
      f"{sizes.min()} .. {sizes.max()} rows; coarse k-means {t['coarse']:.1f} ms, codebooks on residuals {t['fine']:.1f} ms (IndexPQ on rows "
      f"{t['pq']:.1f} ms); add {t['add']:.1f} ms = {t['add'] / N * 1e3:.3f} us per row (IndexIVFFlat {t['add_flat']:.1f} ms)", flush=True)


def profiled(fn):
    torch.cuda.synchronize()
    _ffi.profile_enable(2)
    _ffi.profile_reset()
    fn()
    torch.cuda.synchronize()
    prof = _ffi.profile_read()
    _ffi.profile_enable(False)
    return ", ".join(f"{n} {v['ms']:.4f}" for n, v in prof.items())


for nq in NQS:
    Q = Qall[:nq].contiguous()
    t_flat = event_ms(lambda: flat.search_device(Q, K))
    If = flat.search_device(Q, K)[1].cpu().numpy()
    t_pq = event_ms(lambda: pq.search_device(Q, K))
    r_pq = recall(pq.search_device(Q, K)[1].cpu().numpy(), If)
    print(f"## M = {M}, nq = {nq}: flat {t_flat:.4f} ms; pq alone {t_pq:.4f} ms = {t_pq / t_flat:.2f} x flat, recall@{K} {r_pq:.4f}", flush=True)
    print("index   | nprobe | k_factor | whole ms | whole / flat | whole / pq | recall@10", flush=True)
    for nprobe in NPROBES:
        t_i = event_ms(lambda: ivfpq.search_device(Q, K, nprobe=nprobe))
        r_i = recall(ivfpq.search_device(Q, K, nprobe=nprobe)[1].cpu().numpy(), If)
        print(f"ivfpq{M:<2d} | {nprobe:6d} | {'-':>8s} | {t_i:8.4f} | {t_i / t_flat:12.3f} | {t_i / t_pq:10.3f} | {r_i:9.4f}", flush=True)
        t_f = event_ms(lambda: ivfflat.search_device(Q, K, nprobe=nprobe))
        r_f = recall(ivfflat.search_device(Q, K, nprobe=nprobe)[1].cpu().numpy(), If)
        print(f"ivfflat | {nprobe:6d} | {'-':>8s} | {t_f:8.4f} | {t_f / t_flat:12.3f} | {t_f / t_pq:10.3f} | {r_f:9.4f}", flush=True)
        ivfpq.nprobe = nprobe
        for kf in KFS:
            t_r = event_ms(lambda: index.search_device(Q, K, k_factor=kf))
            r_r = recall(index.search_device(Q, K, k_factor=kf)[1].cpu().numpy(), If)
            print(f"refine  | {nprobe:6d} | {kf:8d} | {t_r:8.4f} | {t_r / t_flat:12.3f} | {t_r / t_pq:10.3f} | {r_r:9.4f}", flush=True)
        print(f"   kernels of one profiled ivfpq call, nq = {nq}, nprobe = {nprobe} (ms): "
              f"{profiled(lambda: ivfpq.search_device(Q, K, nprobe=nprobe))}", flush=True)

if args.ab and M == 64:
    for share in AB:
        os.environ["IVR_IVFPQ_GROUPS_PER_WG"] = str(share)
        other = IndexIVFPQ(same_quantizer(ivfflat), D, NLIST, M)
        other.pq.centroids = ivfpq.pq.centroids
        for _, x, _ in blocks():
            other.add(x)
            del x
        for nq in NQS:
            Q = Qall[:nq].contiguous()
            line = []
            for nprobe in NPROBES:
                a, b = other.search_device(Q, K, nprobe=nprobe), ivfpq.search_device(Q, K, nprobe=nprobe)
                assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), "the share of the scan must not change a result"
                t_o, t_i = event_ms(lambda: other.search_device(Q, K, nprobe=nprobe)), event_ms(lambda: ivfpq.search_device(Q, K, nprobe=nprobe))
                line.append(f"nprobe {nprobe}: {t_o:.4f} ms against {t_i:.4f} ms")
            print(f"## A/B, {share} groups per scan workgroup against 128, nq = {nq}: {'; '.join(line)}", flush=True)
        other.close()
