#!/usr/bin/env python3
"""Row access by id on an id-mapped rows x 512 index: find() through the scan and through the hash table, gather against a contiguous
reconstruct, scatter against single-row writes, and (with --ab-lib) the unfiltered 10-query search against another build of the
library, interleaved in one process.  Warm-up, then the median (and p90) of the wall-clock time of each call including the stream
synchronisation that ends it; the inputs are resident on the device.

    python tools/bench_row_access.py [--rows 1000000] [--ab-lib PATH/libivr_hip.so]
    python tools/bench_row_access.py --search-tree CHECKOUT     the 10-query search alone with CHECKOUT's package and library (a process
                                                                per tree, alternated by the caller): wall clock and per-launch event times
"""
import argparse
import ctypes as C
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=1_000_000)
ap.add_argument("--ab-lib", default=None, help="another build of libivr_hip.so (the parent commit's) for the search A/B")
ap.add_argument("--search-tree", default=None, help="a checkout: time only the 10-query search with its package and library")
args = ap.parse_args()
ROOT = os.path.abspath(args.search_tree) if args.search_tree else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "intelligent-video-analysis-retrieval-system_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from ivr_amd import _ffi  # noqa: E402
from ivr_amd.index import FlatIPIndex  # noqa: E402

N, D, BASE = args.rows, 512, 3 * 10**12


def timed(fn, n=50, warm=5, before=None):
    """median and p90 in ms of fn() + stream synchronisation; before() runs untimed in front of every call"""
    ts = []
    for it in range(warm + n):
        if before:
            before()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if it >= warm:
            ts.append((time.perf_counter() - t0) * 1e3)
    ts.sort()
    return ts[len(ts) // 2], ts[int(len(ts) * 0.9)]


def build(env):
    os.environ.update(env)
    try:
        idx = FlatIPIndex(D, capacity=N)
    finally:
        for k in env:
            del os.environ[k]
    g = torch.Generator(device="cuda").manual_seed(5678)
    ids = torch.from_numpy(BASE + np.random.default_rng(1).permutation(10 * N)[:N]).to(torch.int64)
    for i in range(0, N, 250_000):
        n = min(250_000, N - i)
        idx.add_with_ids(torch.randn((n, D), generator=g, device="cuda"), ids[i:i + n], normalize=True)
    return idx, ids


if args.search_tree:
    g = torch.Generator(device="cuda").manual_seed(5678)
    idx = FlatIPIndex(D, capacity=N)
    for i in range(0, N, 250_000):
        idx.add(torch.randn((min(250_000, N - i), D), generator=g, device="cuda"), normalize=True)
    q = torch.randn((10, D), generator=g, device="cuda")
    out = (torch.empty((10, 10), device="cuda"), torch.empty((10, 10), dtype=torch.int64, device="cuda"))
    w = timed(lambda: idx.search_device(q, 10, normalize=True, out=out), n=300, warm=50)
    _ffi.profile_enable(2)
    _ffi.profile_reset()
    for _ in range(200):
        idx.search_device(q, 10, normalize=True, out=out)
    torch.cuda.synchronize()
    per = {k: round(v["ms"] / v["launches"] * 1e3, 3) for k, v in sorted(_ffi.profile_read().items())}
    print(f"{args.search_tree}: search 10 x {N} x {D}, k = 10: {w[0]:.4f} ms ({w[1]:.4f}); us per launch with events: {per}", flush=True)
    sys.exit(0)

print(f"# id-mapped index {N} x {D}, labels {BASE} + a permutation sample; ms per call, median (p90)", flush=True)
scan, ids = build({"IVR_FIND_TABLE_MIN_KEYS": str(1 << 62)})
table, _ = build({"IVR_FIND_TABLE_MIN_KEYS": "0"})
empty_x, empty_i = torch.empty((0, D), device="cuda"), np.zeros(0, np.int64)
rng = np.random.default_rng(2)
print("## find: keys | scan (the only path before) | table, built | table + one rebuild", flush=True)
crossover = None
for nk in (1, 16, 256, 512, 1024, 2048, 4096, 65536):
    keys = ids[torch.from_numpy(rng.integers(0, N, nk))].cuda()
    keys[::7] += 10 * N                                     # some absent keys
    assert torch.equal(scan._find_device(keys), table._find_device(keys))
    s = timed(lambda: scan._find_device(keys), n=50 if nk <= 4096 else 5, warm=5 if nk <= 4096 else 1)
    t = timed(lambda: table._find_device(keys))
    # add_with_ids of no rows marks the table stale: the next lookup rebuilds it
    r = timed(lambda: table._find_device(keys), before=lambda: table._add_device(empty_x, False, empty_i))
    if crossover is None and r[0] < s[0]:
        crossover = nk
    print(f"{nk:6d} keys | {s[0]:9.3f} ({s[1]:9.3f}) | {t[0]:7.3f} ({t[1]:7.3f}) | {r[0]:7.3f} ({r[1]:7.3f})", flush=True)
print(f"smallest measured key count at which table + rebuild beats the scan: {crossover}", flush=True)

print("## gather: 4096 random rows against ivr_index_reconstruct of 4096 contiguous rows", flush=True)
rows = torch.from_numpy(rng.integers(0, N, 4096)).cuda()
out = torch.empty((4096, D), device="cuda")
lib = _ffi.load()


def contiguous():
    _ffi.check(lib.ivr_index_reconstruct(table._h, N // 3, 4096, C.c_void_p(out.data_ptr()), _ffi.stream_ptr()))


ga, co = timed(lambda: table.gather_device(rows), n=200, warm=20), timed(contiguous, n=200, warm=20)
print(f"gather {ga[0]:.4f} ({ga[1]:.4f})   contiguous {co[0]:.4f} ({co[1]:.4f})   ratio {ga[0] / co[0]:.2f}   "
      f"(layout: a random row touches all {D * 4 // 16} 64-byte lines of its tile = 16x its bytes on the index side, the contiguous read 1x)", flush=True)

print("## scatter: 4096 rows in one call against 4096 single-row ivr_index_write calls (write_device: enqueue only, one sync at the end)", flush=True)
srows = torch.from_numpy(rng.permutation(N)[:4096]).cuda()
srows_h = srows.cpu().tolist()
x = torch.randn((4096, D), device="cuda")


def single():
    for i, r in enumerate(srows_h):
        table.write_device(r, x[i:i + 1], normalize=True)


sc, si = timed(lambda: table.scatter_device(srows, x, normalize=True), n=200, warm=20), timed(single, n=5, warm=1)
print(f"scatter {sc[0]:.4f} ({sc[1]:.4f})   4096 x write {si[0]:.3f} ({si[1]:.3f})   ratio {si[0] / sc[0]:.0f}x", flush=True)

if args.ab_lib:
    print(f"## unfiltered search, 10 queries x {N} rows, k = 10: this build (new) against {os.path.basename(args.ab_lib)} (old), interleaved", flush=True)
    old = C.CDLL(args.ab_lib)
    for name, (res, at) in _ffi._SIGS.items():
        if hasattr(old, name):
            getattr(old, name).restype, getattr(old, name).argtypes = res, at
    print(f"api versions: new {lib.ivr_api_version()}, old {old.ivr_api_version()}", flush=True)
    ctx, h = C.c_void_p(), C.c_void_p()
    _ffi.check(old.ivr_init(0, C.byref(ctx)))
    _ffi.check(old.ivr_index_create(ctx, D, N, C.byref(h)))
    new = FlatIPIndex(D, capacity=N)
    g = torch.Generator(device="cuda").manual_seed(5678)
    for i in range(0, N, 250_000):
        t = torch.randn((min(250_000, N - i), D), generator=g, device="cuda")
        new.add(t, normalize=True)
        _ffi.check(old.ivr_index_add(h, C.c_void_p(t.data_ptr()), t.shape[0], 1, _ffi.stream_ptr()))
        torch.cuda.synchronize()
    q = torch.randn((10, D), generator=g, device="cuda")
    Dn, In = torch.empty((10, 10), device="cuda"), torch.empty((10, 10), dtype=torch.int64, device="cuda")
    Do, Io = torch.empty_like(Dn), torch.empty_like(In)

    def search(which, handle, Dx, Ix):                     # the same host path for both builds: the bare C call
        return lambda: _ffi.check(which.ivr_index_search(handle, C.c_void_p(q.data_ptr()), 10, 10, 1, 0, C.c_void_p(Dx.data_ptr()),
                                                         C.c_void_p(Ix.data_ptr()), _ffi.stream_ptr()))

    run_new, run_old = search(lib, new._h, Dn, In), search(old, h, Do, Io)

    for rnd in range(6):
        a, b = (timed(run_old, n=200, warm=20), timed(run_new, n=200, warm=20)) if rnd % 2 == 0 else \
            (timed(run_new, n=200, warm=20), timed(run_old, n=200, warm=20))[::-1]
        print(f"round {rnd}: old {a[0]:.4f} ({a[1]:.4f})   new {b[0]:.4f} ({b[1]:.4f})   new / old {b[0] / a[0]:.4f}", flush=True)
    assert torch.equal(In, Io) and torch.equal(Dn.view(torch.int32), Do.view(torch.int32)), "the two builds disagree"
    print("results of the two builds are bit-identical", flush=True)
    old.ivr_index_destroy(h)
