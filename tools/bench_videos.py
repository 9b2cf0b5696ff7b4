#!/usr/bin/env python3
"""Video search (ivr_amd/videos.py: video_search_device, related_videos) against the two routes a caller without it has to take.

    python tools/bench_videos.py [--rows 1000000] [--segment 500] [--related-rows 100000] [--timeout 1100] [--quick]

Rows: `--rows` x 512 unit-norm float32 in videos of `--segment` rows; a video is cut into shots of 100 rows, a shot is one of 1,000
random unit centres plus 0.3 g / sqrt(d) per row, as in tools/bench_groups.py.  Drawn on the device by
torch.Generator(device="cuda").manual_seed(1234).  A query video is a run of stored rows of one video plus 0.1 g / sqrt(d) per row,
normalised (manual_seed(4321)): a re-encoded copy of a stretch of a stored video.

Cells: one query video of 16, 64 and 500 frames, 16 query videos of 64 frames, each mode="symmetric" and k = 10; and related_videos
(k = 10, symmetric) over an index of `--related-rows` rows in videos of `--segment` rows.  The measurement is one child process under
`timeout`.  Per cell:
    call       median ms of the call between two device events after 3 warm-up calls (members and offsets on the device; the call
               holds its one read-back of set_off)
    score / reduce / select   the passes of one profiled call (event pairs around the passes lengthen the call: compare them with
               each other, not with the median); select = finish + top-k
    segbest    grp_segbest of best_per_segment_device over the same members, from a profiled call: the pass whose cost the score
               pass is expected to match
    parent     the route of the parent commit: best_per_segment_device over every member (one direction), tag_rows_device(top=1) per
               set with its members as the labels (the other direction; at most 4,096 labels), and a torch reduction per video and
               set (index_add_ / mean) with a topk; `-` where a set exceeds the label cap
    torch      (X @ Q.T) in blocks of 65,536 rows through rocBLAS with amax over the members and torch.segment_reduce over the rows,
               on a row-major float32 copy of the rows, and a topk
    same       whether the parent route and the torch route name the same k videos as the call for every set (their float32
               sums are not the call's integer sums: the order of near ties may differ)"""
import argparse
import os
import subprocess
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=1_000_000)
ap.add_argument("--segment", type=int, default=500)
ap.add_argument("--related-rows", type=int, default=100_000)
ap.add_argument("--timeout", type=int, default=1100, help="seconds for the measuring process")
ap.add_argument("--quick", action="store_true", help="the cells of 16 and 64 frames and related_videos on a tenth of the rows")
ap.add_argument("--step", default=None, help="internal: measure")
args = ap.parse_args()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D, NCENT, SHOT, K = 512, 1000, 100, 10

if args.step is None:
    cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--rows", str(args.rows), "--segment",
           str(args.segment), "--related-rows", str(args.related_rows), "--step", "measure"] + (["--quick"] if args.quick else [])
    rc = subprocess.run(cmd).returncode
    if rc != 0:
        print(f"the measuring process ended with status {rc}", flush=True)
    sys.exit(rc)

sys.path.insert(0, os.path.join(ROOT, "intelligent-video-analysis-retrieval-system_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from ivr_amd import _ffi  # noqa: E402
from ivr_amd.grouping import best_per_segment_device  # noqa: E402
from ivr_amd.index import FlatIPIndex  # noqa: E402
from ivr_amd.tagging import tag_rows_device  # noqa: E402
from ivr_amd.videos import related_videos, video_search_device  # noqa: E402

assert torch.cuda.is_available(), "bench_videos.py needs a GPU"
SEG = args.segment
assert args.rows % SEG == 0 and args.related_rows % SEG == 0 and SEG % SHOT == 0 and args.rows % SHOT == 0


def event_ms(fn, budget_s=0.3, warm=3):
    """median ms between two device events around fn(), after `warm` warm-up calls; enough repeats to fill budget_s, 3 to 50"""
    for _ in range(warm):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ts = []
    reps = 3
    while len(ts) < reps:
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
        if len(ts) == 1:
            reps = int(min(50, max(3, budget_s * 1e3 / max(ts[0], 1e-3))))
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


def build(n, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    centres = torch.randn((NCENT, D), generator=g, device="cuda")
    centres = centres / centres.norm(dim=1, keepdim=True)
    index = FlatIPIndex(D)
    for i in range(0, n, 250_000):
        c = min(250_000, n - i)
        shot = torch.randint(0, NCENT, (c // SHOT,), generator=g, device="cuda").repeat_interleave(SHOT)
        x = centres[shot] + 0.3 * torch.randn((c, D), generator=g, device="cuda") / D ** 0.5
        index.add(x / x.norm(dim=1, keepdim=True))
    return index


def parent_route(index, Q, sets, seg, nseg, lengths, k):
    """best_per_segment over every member, tag_rows(top=1) per set, a torch reduction per video -> Vseg [nsets,k]; None past the cap"""
    if int(np.diff(sets).max()) > _ffi.IVR_TAG_MAX_LABELS:
        return None
    nsets = len(sets) - 1
    Df = torch.cat([best_per_segment_device(index, Q[i:i + 4096], seg)[0] for i in range(0, Q.shape[0], 4096)])
    video_of_row = torch.repeat_interleave(torch.arange(nseg, device="cuda"), lengths)
    V = torch.empty((nsets, nseg), device="cuda")
    for s in range(nsets):
        fwd = Df[sets[s]:sets[s + 1]].mean(dim=0)
        Db = tag_rows_device(index, Q[sets[s]:sets[s + 1]], top=1)[0][:, 0]
        bwd = torch.zeros(nseg, device="cuda").index_add_(0, video_of_row, Db) / lengths
        V[s] = (fwd + bwd) * 0.5
    return V.topk(k, dim=1)[1]


def torch_route(X, Q, sets, lengths, k):
    """(X @ Q.T) in row blocks through rocBLAS, amax over the members of each set, segment_reduce over the rows -> Vseg [nsets,k]"""
    nsets = len(sets) - 1
    fwd = torch.empty((nsets, len(lengths)), device="cuda")
    bwd = torch.empty((nsets, len(lengths)), device="cuda")
    rowmax = torch.empty((nsets, X.shape[0]), device="cuda")
    membest = [[] for _ in range(nsets)]
    block = 65_536 // SEG * SEG                                    # whole videos
    for r0 in range(0, X.shape[0], block):
        S = X[r0:r0 + block] @ Q.T                                 # [rows of the block, members]
        for s in range(nsets):
            Ss = S[:, sets[s]:sets[s + 1]].contiguous()
            rowmax[s, r0:r0 + block] = Ss.amax(dim=1)
            membest[s].append(torch.segment_reduce(Ss, "max", lengths=lengths[r0 // SEG:(r0 + S.shape[0]) // SEG], axis=0))
    for s in range(nsets):
        fwd[s] = torch.cat(membest[s]).mean(dim=1)
        bwd[s] = torch.segment_reduce(rowmax[s], "mean", lengths=lengths)
    return ((fwd + bwd) * 0.5).topk(k, dim=1)[1]


def same(a, b):
    return "-" if b is None else "yes" if torch.equal(a.sort(dim=1)[0], b.sort(dim=1)[0]) else "no"


def fmt(t):
    return "       -" if t is None else f"{t:8.3f}"


name = torch.cuda.get_device_name(0)
index = build(args.rows, 1234)
N = index.ntotal
nseg = N // SEG
seg = torch.arange(0, N + 1, SEG, dtype=torch.int64, device="cuda")
lengths = torch.full((nseg,), SEG, dtype=torch.int64, device="cuda")
X = torch.cat([index.gather_device(torch.arange(i, min(i + 250_000, N), device="cuda")) for i in range(0, N, 250_000)])
print(f"# bench_videos on {name}: {N} x {D} rows ({N * D * 4 / 1e6:.1f} MB float32) in {nseg} videos of {SEG} rows, mode = symmetric, k = {K}",
      flush=True)
print("  sets x frames |  call ms | score ms | reduce ms | select ms | segbest ms | parent ms | parent/call | torch ms | torch/call | same parent / torch",
      flush=True)
gq = torch.Generator(device="cuda").manual_seed(4321)
cells = [(1, 16), (1, 64)] if args.quick else [(1, 16), (1, 64), (1, min(500, SEG)), (16, 64)]
for nsets, m in cells:
    starts = torch.randint(0, nseg, (nsets,), generator=gq, device="cuda") * SEG
    rows = (starts[:, None] + torch.arange(m, device="cuda")[None, :]).reshape(-1)
    Q = index.gather_device(rows) + 0.1 * torch.randn((nsets * m, D), generator=gq, device="cuda") / D ** 0.5
    Q = (Q / Q.norm(dim=1, keepdim=True)).contiguous()
    sets = np.arange(0, nsets * m + 1, m, dtype=np.int64)
    call = lambda: video_search_device(index, Q, K, seg, sets)     # noqa: E731
    t_call = event_ms(call)
    prof = profiled(call)
    ours = call()[0]
    segbest = profiled(lambda: best_per_segment_device(index, Q, seg)).get("grp_segbest", 0.0)
    par = parent_route(index, Q, sets, seg, nseg, lengths, K)
    t_par = None if par is None else event_ms(lambda: parent_route(index, Q, sets, seg, nseg, lengths, K), warm=1)
    tor = torch_route(X, Q, sets, lengths, K)
    t_tor = event_ms(lambda: torch_route(X, Q, sets, lengths, K), warm=1)
    print(f"{nsets:6d} x {m:6d} | {t_call:8.3f} | {prof.get('vid_score', 0.0):8.3f} | {prof.get('vid_reduce', 0.0):9.3f} | "
          f"{prof.get('vid_select', 0.0):9.3f} | {segbest:10.3f} | {fmt(t_par)}  | {'-' if t_par is None else f'{t_par / t_call:11.2f}'} | "
          f"{fmt(t_tor)} | {t_tor / t_call:10.2f} | {same(ours, par)} / {same(ours, tor)}", flush=True)
del X, index
torch.cuda.empty_cache()

# related videos: every video of a smaller index against every video
NR = args.related_rows // 10 if args.quick else args.related_rows
index = build(NR, 99)
nseg = NR // SEG
seg = torch.arange(0, NR + 1, SEG, dtype=torch.int64, device="cuda")
lengths = torch.full((nseg,), SEG, dtype=torch.int64, device="cuda")
X = index.gather_device(torch.arange(NR, device="cuda"))
sets = np.arange(0, NR + 1, SEG, dtype=np.int64)
own = torch.arange(nseg, device="cuda")[:, None]


def without_own(V, k):
    return V.masked_fill(torch.eye(V.shape[0], dtype=torch.bool, device="cuda"), float("-inf")).topk(k, dim=1)[1]


def related_parent():
    Df = torch.cat([best_per_segment_device(index, X[i:i + 4096], seg)[0] for i in range(0, NR, 4096)])
    video_of_row = torch.repeat_interleave(torch.arange(nseg, device="cuda"), lengths)
    V = torch.empty((nseg, nseg), device="cuda")
    for s in range(nseg):
        Db = tag_rows_device(index, X[sets[s]:sets[s + 1]], top=1)[0][:, 0]
        V[s] = (Df[sets[s]:sets[s + 1]].mean(dim=0) + torch.zeros(nseg, device="cuda").index_add_(0, video_of_row, Db) / lengths) * 0.5
    return without_own(V, K)


def related_torch_blocks():
    V = torch.empty((nseg, nseg), device="cuda")
    step = max(1, 16_384 // SEG)                                   # query videos per block
    for s0 in range(0, nseg, step):
        s1 = min(nseg, s0 + step)
        S = X @ X[sets[s0]:sets[s1]].T                             # [rows, members of the block]
        S = S.reshape(NR, s1 - s0, SEG)
        bwd = torch.segment_reduce(S.amax(dim=2), "mean", lengths=lengths, axis=0)          # [videos, sets of the block]
        fwd = torch.segment_reduce(S.reshape(NR, -1), "max", lengths=lengths, axis=0).reshape(nseg, s1 - s0, SEG).mean(dim=2)
        V[s0:s1] = ((fwd + bwd) * 0.5).T
    return without_own(V, K)


call = lambda: related_videos(index, seg, K)                       # noqa: E731
t0 = event_ms(call, warm=1)
prof = profiled(call)
ours = torch.from_numpy(call()[0]).cuda()
par = related_parent()
t_par = event_ms(related_parent, warm=0, budget_s=0.0)
tor = related_torch_blocks()
t_tor = event_ms(related_torch_blocks, warm=1)
print(f"# related_videos on {name}: {NR} x {D} rows in {nseg} videos of {SEG} rows, k = {K}: every video against every video, host copies "
      f"of the results included", flush=True)
print("  call ms | score ms | reduce ms | select ms | parent ms | parent/call | torch ms | torch/call | same parent / torch", flush=True)
print(f"{t0:9.2f} | {prof.get('vid_score', 0.0):8.2f} | {prof.get('vid_reduce', 0.0):9.2f} | {prof.get('vid_select', 0.0):9.2f} | {t_par:9.2f} | "
      f"{t_par / t0:11.2f} | {t_tor:8.2f} | {t_tor / t0:10.2f} | {same(ours, par)} / {same(ours, tor)}", flush=True)
