"""Seeded inputs shared by the CPU and the GPU suite of the event search (ivr_amd/temporal.py, csrc/search_events.hip), and the
brute-force enumerator the numpy definition is checked against.  Nothing here calls the code under test."""
import numpy as np

SEGMENTS_SMALL = np.array([1, 1, 6, 8, 13], np.int64)      # N = 14: row 0 in front, an empty segment, [6, 8) shorter than m, row 13 past the end
# the segment array of test_temporal_gpu.py::test_segments: boundaries at 15 / 16 / 17 and 64 / 65, an empty segment [17, 17), short
# segments, row 0 in front of the first offset and rows 90 .. 99 past the last
SEGMENTS_100 = np.array([1, 15, 16, 17, 17, 19, 64, 65, 90], np.int64)


def ordered(x):
    """float32 -> int64 that orders like the value with -0.0 equal to +0.0 (written out here, not imported from the package)."""
    u = (np.asarray(x, np.float32) + np.float32(0.0)).view(np.uint32).astype(np.int64)
    return np.where(u & 0x80000000, 0xFFFFFFFF - u, u | 0x80000000)


def segment_of(r, N, seg_off):
    """(lo, hi) of the segment that holds row r, or None."""
    if seg_off is None:
        return (0, N)
    for s in range(len(seg_off) - 1):
        if seg_off[s] <= r < seg_off[s + 1]:
            return (max(int(seg_off[s]), 0), min(int(seg_off[s + 1]), N))
    return None


def chain_sum(S, path):
    """The left-to-right float32 sum of a chain with the + 0.0 step of the definition."""
    acc = np.float32(S[0, path[0]])
    for j in range(1, len(path)):
        acc = np.float32(np.float32(acc + np.float32(0.0)) + S[j, path[j]])
    return acc


def admissible(path, N, seg_off, min_gap, max_gap):
    seg = segment_of(path[-1], N, seg_off)
    if seg is None:
        return False
    if any(not seg[0] <= r < seg[1] for r in path):
        return False
    return all(min_gap <= b - a <= max_gap for a, b in zip(path[:-1], path[1:]))


def enumerate_chains(S, min_gap, max_gap, seg_off=None):
    """Every admissible chain, one by one: (best float32 [N], ok bool [N]) = per end row the greatest chain sum (in the order of
    `ordered`) and whether any chain ends there."""
    m, N = S.shape
    best = np.zeros(N, np.float32)
    ok = np.zeros(N, bool)

    def extend(path):
        if len(path) == m:
            if not admissible(path, N, seg_off, min_gap, max_gap):
                return
            r, v = path[-1], chain_sum(S, path)
            if not ok[r] or ordered(v) > ordered(best[r]):
                best[r], ok[r] = v, True
            return
        first = 0 if not path else path[-1] + min_gap
        last = N - 1 if not path else min(N - 1, path[-1] + max_gap)
        for r in range(first, last + 1):
            extend(path + [r])

    extend([])
    return best, ok


def small_cases(count=300, seed=11):
    """(S float32 [m,N], min_gap, max_gap, seg_off or None): N <= 14, m in 1 .. 4, half of them with half-integer scores (ties)."""
    rng = np.random.default_rng(seed)
    for i in range(count):
        m = int(rng.integers(1, 5))
        with_seg = bool(i % 2)
        N = 14 if with_seg else int(rng.integers(1, 15))
        min_gap = int(rng.integers(1, 4))
        max_gap = int(rng.integers(min_gap, 7))
        if i % 4 < 2:
            S = (rng.integers(-4, 5, size=(m, N)) / 2.0).astype(np.float32)
        else:
            S = rng.standard_normal((m, N)).astype(np.float32)
        yield S, min_gap, max_gap, (SEGMENTS_SMALL if with_seg else None)


def make_rows(d, N, seed, period=None):
    rng = np.random.default_rng([seed, d, N])
    X = rng.standard_normal((N, d)).astype(np.float32)
    if period:
        X = X[np.arange(N) % period].copy()           # duplicate rows: equal chain scores and equal predecessors
    return X


def make_chains(d, B, m, seed):
    return np.random.default_rng([seed, d, B, m]).standard_normal((B, m, d)).astype(np.float32)
