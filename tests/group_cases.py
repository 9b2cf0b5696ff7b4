"""Seeded inputs shared by the CPU and the GPU suite of the grouped search (ivr_amd/grouping.py, csrc/search_groups.hip), and the brute
force the numpy definition is checked against.  Nothing here calls the code under test."""
import numpy as np

FLT_MAX = np.finfo(np.float32).max
# (G, g) of the issue's grid
SIZES = [(1, 1), (1, 64), (10, 1), (10, 3), (32, 64), (2048, 1)]


def ordered(x):
    """float32 -> int that orders like the value with -0.0 equal to +0.0 (written out here, not imported from the package)."""
    u = int((np.float32(x) + np.float32(0.0)).view(np.uint32))
    return 0xFFFFFFFF - u if u & 0x80000000 else u | 0x80000000


def layouts(N, P):
    """{name: seg_off or None}: no segments; one segment; every row its own; boundaries at 1, 15, 16, 17, 1024 +- 1 and P +- 1 with
    two empty segments among them, once as they are (offsets past N: clipped) and once cut so that rows stay outside at both ends;
    more segments than rows (every other one empty)."""
    marks = np.array([1, 15, 16, 17, 17, 1023, 1024, 1025, 1025, P - 1, P, P + 1, 2 * P + 1], np.int64)
    return {"none": None,
            "one": np.array([0, N], np.int64),
            "each": np.arange(N + 1, dtype=np.int64),
            "marks": marks,
            "inside": np.minimum(marks, max(N - 2, 0)),
            "many": np.repeat(np.arange(N + 1, dtype=np.int64), 2)}


def brute_groups(S, G, g, seg_off=None, ids=None):
    """The definition by sorting in Python: per segment `sorted` on (-score, row), groups sorted on their first entry."""
    nq, N = S.shape
    off = [0, N] if seg_off is None else [int(v) for v in seg_off]
    Gseg = np.full((nq, G), -1, np.int64)
    D = np.full((nq, G, g), -FLT_MAX, np.float32)
    I = np.full((nq, G, g), -1, np.int64)
    for q in range(nq):
        groups = []
        for j in range(len(off) - 1):
            rows = sorted(((-ordered(S[q, r]), r) for r in range(max(off[j], 0), min(off[j + 1], N))))
            if rows:
                groups.append((rows[0], j, rows[:g]))
        groups.sort()
        for slot, (_, j, rows) in enumerate(groups[:G]):
            Gseg[q, slot] = j
            for e, (_, r) in enumerate(rows):
                D[q, slot, e] = S[q, r] + np.float32(0.0)
                I[q, slot, e] = r if ids is None else ids[r]
    return Gseg, D, I


def brute_best(S, seg_off=None, ids=None):
    nq, N = S.shape
    off = [0, N] if seg_off is None else [int(v) for v in seg_off]
    nseg = len(off) - 1
    D = np.full((nq, nseg), -FLT_MAX, np.float32)
    I = np.full((nq, nseg), -1, np.int64)
    for q in range(nq):
        for j in range(nseg):
            rows = sorted(((-ordered(S[q, r]), r) for r in range(max(off[j], 0), min(off[j + 1], N))))
            if rows:
                r = rows[0][1]
                D[q, j] = S[q, r] + np.float32(0.0)
                I[q, j] = r if ids is None else ids[r]
    return D, I


def small_scores(count=120, seed=5):
    """(S float32 [nq,N], seg_off or None): N <= 24; half of them with half-integer scores, so that equal scores occur inside a
    segment and equal best scores across segments."""
    rng = np.random.default_rng(seed)
    for i in range(count):
        N = int(rng.integers(1, 25))
        nq = int(rng.integers(1, 4))
        if i % 2:
            S = (rng.integers(-3, 4, size=(nq, N)) / 2.0).astype(np.float32)
            S[S == 0] = np.float32(-0.0) if i % 4 == 1 else np.float32(0.0)
        else:
            S = rng.standard_normal((nq, N)).astype(np.float32)
        kind = i % 6
        if kind == 0:
            seg = None
        elif kind == 1:
            seg = np.arange(N + 1, dtype=np.int64)                                   # one-row segments
        elif kind == 2:
            seg = np.sort(rng.integers(0, N + 1, size=int(rng.integers(2, 9)))).astype(np.int64)     # empty segments, rows outside at both ends
        elif kind == 3:
            seg = np.sort(rng.integers(-3, N + 6, size=int(rng.integers(2, 9)))).astype(np.int64)    # offsets below 0 and past N
        elif kind == 4:
            seg = np.array([0, N], np.int64)
        else:
            seg = np.repeat(np.arange(N + 1, dtype=np.int64), 2)                     # more segments than rows
        yield S, seg
