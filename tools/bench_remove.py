#!/usr/bin/env python3
"""Row removal (FlatIPIndex.remove_ids) on 1M x 512 unit rows: a contiguous 1 % in the middle, a random 1 % given as a bitmap, the last
1 % and the first half.  Each case is timed against the only alternative the index offered before: ivr_index_reconstruct of the
surviving rows into a device buffer, ivr_index_reset, ivr_index_add.  (Contiguous cases reconstruct the surviving runs straight into
the buffer; the random case reconstructs everything and gathers the survivors with one torch index_select, which is kinder to the
alternative than one reconstruct call per run.)

Both are wall-clock times between two device synchronisations, because remove_ids waits for its count on the host; the index is
refilled from a device-resident master copy before every repeat (not timed).  Figures are medians.  "moved" is the payload: the
surviving rows behind the first removed row in both layouts (float32 tiles + bf16 scan copy), counted once; a step through the
bounce buffer reads and writes each of them twice (index -> bounce -> index), a direct step once.  The per-kernel lines at the end are
HIP-event times of one call (profile level 2) with the bytes each launch reads + writes, next to the append kernel.

    python tools/bench_remove.py [rows=1048576] [repeats=7]
"""
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "intelligent-video-analysis-retrieval-system_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from ivr_amd import _ffi  # noqa: E402
from ivr_amd.index import FlatIPIndex, IDSelectorBitmap, IDSelectorRange  # noqa: E402

rows = int(sys.argv[1]) if len(sys.argv) > 1 else 1 << 20
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 7
d = 512
lib = _ffi.load()

g = torch.Generator(device="cuda").manual_seed(31)
master = torch.randn((rows, d), generator=g, device="cuda")
master /= master.norm(dim=1, keepdim=True)
idx = FlatIPIndex(d, capacity=rows)
buf = torch.empty((rows, d), dtype=torch.float32, device="cuda")
rng = np.random.default_rng(5)


def refill():
    idx.reset()
    idx._add_device(master, False)
    torch.cuda.synchronize()


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def reconstruct_into(start, n, out):
    _ffi.check(lib.ivr_index_reconstruct(idx._h, int(start), int(n), C.c_void_p(out.data_ptr()), _ffi.stream_ptr()), "ivr_index_reconstruct")


def rebuild(removed):
    """reconstruct the survivors, reset, add"""
    keep = ~removed
    n_keep = int(keep.sum())
    edges = np.flatnonzero(np.diff(np.concatenate([[0], keep.view(np.int8), [0]])))
    runs = list(zip(edges[::2], edges[1::2]))
    if len(runs) <= 4:
        at = 0
        for a, b in runs:
            reconstruct_into(a, b - a, buf[at:at + (b - a)])
            at += b - a
        left = buf[:n_keep]
    else:
        reconstruct_into(0, rows, buf)
        left = buf.index_select(0, torch.from_numpy(np.flatnonzero(keep)).cuda())
    idx.reset()
    idx._add_device(left, False)


def bitmap_case(frac):
    m = rng.random(rows) < frac
    return IDSelectorBitmap(np.packbits(m, bitorder="little")), m


def range_case(lo, hi):
    m = np.zeros(rows, bool)
    m[lo:hi] = True
    return IDSelectorRange(lo, hi), m


one = rows // 100
cases = [("contiguous 1 % in the middle", *range_case(rows // 2, rows // 2 + one)), ("random 1 % (bitmap)", *bitmap_case(0.01)),
         ("last 1 %", *range_case(rows - one, rows)), ("first half", *range_case(0, rows // 2))]
row_bytes = 4 * ((d + 15) // 16 * 16) + 64 * (((d + 15) // 16 + 1) // 2)
print(f"index {rows} x {d}, {row_bytes} bytes per row in both layouts, bf16 scan copy: {idx.scan_stats()[0]}, "
      f"median of {reps} repeats after 2 warm-ups, chunk rows: {os.environ.get('IVR_REMOVE_CHUNK_ROWS', 'default')}", flush=True)
for name, sel, removed in cases:
    sel._filter(idx.device)                                 # the bitmap upload is not part of the call
    t_remove, t_rebuild = [], []
    for r in range(reps + 2):
        refill()
        t = wall_ms(lambda: idx.remove_ids(sel))
        assert idx.ntotal == rows - int(removed.sum())
        refill()
        u = wall_ms(lambda: rebuild(removed))
        assert idx.ntotal == rows - int(removed.sum())
        if r >= 2:
            t_remove.append(t)
            t_rebuild.append(u)
    tr, tb = float(np.median(t_remove)), float(np.median(t_rebuild))
    first = int(np.flatnonzero(removed)[0])
    moved = int((~removed[first:]).sum()) * row_bytes
    print(f"{name:30s} removed {int(removed.sum()):7d}  remove_ids {tr:8.3f} ms  moved {moved / 1e9:6.3f} GB = {moved / tr / 1e6:7.1f} GB/s "
          f" rebuild {tb:8.3f} ms  rebuild / remove_ids {tb / tr:6.2f}", flush=True)

# per-kernel event times of one call each (ivr_profile level 2), next to the append kernel that writes the same layouts
dev = idx.device.index
print("per-kernel HIP-event times of one call (bytes read + written per launch / time):", flush=True)
for name, sel, removed in cases[:2] + cases[3:]:
    refill()
    _ffi.profile_enable(2, dev)
    _ffi.profile_reset(dev)
    idx.remove_ids(sel)
    torch.cuda.synchronize()
    if name.startswith("contiguous"):
        refill()
    prof = _ffi.profile_read(dev)
    _ffi.profile_enable(0, dev)
    for kernel in ("remove_gather", "remove_place", "remove_gather_direct", "tile_rows"):
        if kernel in prof and prof[kernel]["ms"] > 0:
            v = prof[kernel]
            print(f"{name:30s} {kernel:22s} {v['launches']:3d} launches {v['ms']:8.3f} ms  {v['work'] / v['ms'] / 1e9:6.2f} TB/s", flush=True)
idx.close()
