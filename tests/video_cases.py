"""Seeded inputs shared by the CPU and the GPU suite of the video search (ivr_amd/videos.py, csrc/search_videos.hip), and the brute
force the numpy definition is checked against.  Nothing here calls the code under test."""
import numpy as np

from group_cases import ordered

FLT_MAX = np.finfo(np.float32).max
MODES = ("forward", "backward", "symmetric")
# stored rows of the issue's grid: around one 16-row tile, four tiles, a 1,024-row workgroup of the reduction, a 2,048-row piece of
# the score pass, and one size past two pieces
SIZES = [1, 15, 16, 17, 63, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049, 4099]
# members of a set: around one 16-member tile, around the one-block limit of 64 (plain stores below, atomic maxima above), three blocks
SET_SIZES = [1, 15, 16, 17, 63, 64, 65, 130]


def set_offsets(sizes):
    return np.concatenate(([0], np.cumsum(sizes))).astype(np.int64)


def make_members(d, m, seed):
    return np.random.default_rng([seed, d, m, 77]).standard_normal((m, d)).astype(np.float32)


def fix(t):
    """float32 -> Python int: rint(float32(t * 2^24)), written out here with Python's round (half to even) on the exact product."""
    p = np.float32(t) * np.float32(16777216.0)
    return int(round(float(p)))


def brute_videos(S, seg_off=None, set_off=None):
    """The definition by enumeration in Python: {mode: V float32 [nsets,nseg]}, Fsum and Bsum as Python ints, the divisions in
    float64."""
    M, N = S.shape
    soff = [0, M] if set_off is None else [int(v) for v in set_off]
    off = [0, N] if seg_off is None else [int(v) for v in seg_off]
    nsets, nseg = len(soff) - 1, len(off) - 1
    V = {mode: np.full((nsets, nseg), -FLT_MAX, np.float32) for mode in MODES}
    for s in range(nsets):
        members = range(soff[s], soff[s + 1])
        for j in range(nseg):
            rows = range(min(max(off[j], 0), N), min(max(off[j + 1], 0), N))
            if len(rows) == 0:
                continue
            zero = np.float32(0.0)
            fsum = sum(fix(max(float(S[i, r] + zero) for r in rows)) for i in members)
            bsum = sum(fix(max(float(S[i, r] + zero) for i in members)) for r in rows)
            f64 = float(fsum) / (len(members) * 16777216.0)
            b64 = float(bsum) / (len(rows) * 16777216.0)
            V["forward"][s, j] = np.float32(f64)
            V["backward"][s, j] = np.float32(b64)
            V["symmetric"][s, j] = np.float32((f64 + b64) * 0.5)
    return V


def brute_search(V, k, nrows, exclude=None):
    """(Vseg, D) by `sorted` on (-ordered score, video) over the videos that hold rows; nrows [nseg]."""
    nsets, nseg = V.shape
    Vseg = np.full((nsets, k), -1, np.int64)
    D = np.full((nsets, k), -FLT_MAX, np.float32)
    for s in range(nsets):
        cand = sorted((-ordered(V[s, j]), j) for j in range(nseg) if nrows[j] > 0 and not (exclude is not None and int(exclude[s]) == j))
        for slot, (_, j) in enumerate(cand[:k]):
            Vseg[s, slot] = j
            D[s, slot] = V[s, j] + np.float32(0.0)
    return Vseg, D


def row_counts(N, seg_off):
    off = [0, N] if seg_off is None else [int(v) for v in seg_off]
    return [max(min(max(b, 0), N) - min(max(a, 0), N), 0) for a, b in zip(off[:-1], off[1:])]


def small_scores(count=90, seed=11):
    """(S float32 [members,N], seg_off or None, set_off or None): N <= 20, members <= 9; a third with scores on a coarse grid, so
    that maxima tie inside a video and video scores tie across videos, and -0.0 among them."""
    rng = np.random.default_rng(seed)
    for i in range(count):
        N = int(rng.integers(1, 21))
        M = int(rng.integers(1, 10))
        if i % 3 == 1:
            S = (rng.integers(-2, 3, size=(M, N)) / 2.0).astype(np.float32)
            S[S == 0] = np.float32(-0.0) if i % 2 else np.float32(0.0)
        else:
            S = rng.standard_normal((M, N)).astype(np.float32)
        kind = i % 5
        if kind == 0:
            seg = None
        elif kind == 1:
            seg = np.arange(N + 1, dtype=np.int64)
        elif kind == 2:
            seg = np.sort(rng.integers(0, N + 1, size=int(rng.integers(2, 8)))).astype(np.int64)      # empty videos, rows outside at both ends
        elif kind == 3:
            seg = np.sort(rng.integers(-3, N + 6, size=int(rng.integers(2, 8)))).astype(np.int64)     # offsets below 0 and past N
        else:
            seg = np.repeat(np.arange(0, N + 1, 2, dtype=np.int64), 2)                                # every other video empty
        if i % 2:
            sets = None
        else:
            cuts = np.sort(rng.choice(np.arange(1, M), size=min(M - 1, int(rng.integers(0, 3))), replace=False)) if M > 1 else []
            sets = np.concatenate(([0], cuts, [M])).astype(np.int64)
        yield S, seg, sets
