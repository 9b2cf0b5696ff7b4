#!/usr/bin/env python3
"""A/B in one process, interleaved rounds: the last encoder block on every row (IVR_PRUNE_LAST=0) vs on the pooled token-0 rows only
(=1), inside the ViT-B/32 tower at 4,096 frames (the bench step's tower part).  Prints ms per encode per round, the medians, and
one profiled pass per arm (per-tag ms per encode).   python tools/ab_prune_last.py [frames] [rounds]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "intelligent-video-analysis-retrieval-system_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from ivr_amd import _ffi  # noqa: E402
from ivr_amd import config as C  # noqa: E402
from ivr_amd.tower import Tower  # noqa: E402
from ivr_amd.weights import make_weights  # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
ROUNDS = int(sys.argv[2]) if len(sys.argv) > 2 else 7
REPS = 5
cfg = C.CLIP_VIT_B32
tw = Tower(cfg, make_weights(cfg, 12), max_batch=B)
px = (torch.randn((B * 49, 3072), device="cuda") * 0.5).to(torch.bfloat16)
out = {m: torch.empty((B, 512), device="cuda") for m in ("0", "1")}
ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
res = {"0": [], "1": []}
for rd in range(ROUNDS + 1):
    for mode in ("0", "1"):
        os.environ["IVR_PRUNE_LAST"] = mode
        tw.encode_patches(px, B, out=out[mode])
        torch.cuda.synchronize()
        ev[0].record()
        for _ in range(REPS):
            tw.encode_patches(px, B, out=out[mode])
        ev[1].record()
        torch.cuda.synchronize()
        if rd:                                   # round 0 warms up
            res[mode].append(ev[0].elapsed_time(ev[1]) / REPS)
            print(f"round {rd} IVR_PRUNE_LAST={mode}: {res[mode][-1]:.3f} ms per encode of {B} frames", flush=True)
print("embeddings bit-identical:", bool(torch.equal(out["0"], out["1"])))
for mode, t in res.items():
    print(f"IVR_PRUNE_LAST={mode}: median {np.median(t):.3f} ms, min {min(t):.3f}, spread (max - min) {max(t) - min(t):.3f} ms")
m0, m1 = np.median(res["0"]), np.median(res["1"])
print(f"pruned: {m0 - m1:.3f} ms per encode less ({100.0 * (m0 / m1 - 1.0):.2f} % more frames/s)")
for mode in ("0", "1"):
    os.environ["IVR_PRUNE_LAST"] = mode
    torch.cuda.synchronize()
    _ffi.profile_reset()
    _ffi.profile_enable(1)
    for _ in range(REPS):
        tw.encode_patches(px, B, out=out[mode])
    torch.cuda.synchronize()
    _ffi.profile_enable(False)
    prof = _ffi.profile_read()
    print(f"IVR_PRUNE_LAST={mode} per encode: " + ", ".join(f"{k} {v['ms'] / REPS:.3f}" for k, v in sorted(prof.items())))
