"""Seeded inputs shared by the CPU and the GPU suite of the moment search (ivr_amd/moments.py, csrc/search_moments.hip), and the brute
force the numpy definition is checked against.  Nothing here calls the code under test."""
import numpy as np

from group_cases import ordered, small_scores

FLT_MAX = np.finfo(np.float32).max


def brute_moments(s, threshold, max_gap, seg_off=None):
    """The moments of one query's scores s [N] as [(lo, hi, cnt, peak)], by walking the rows of every segment in turn with a counter
    of the cold rows since the last hot one.  Knows nothing of heads or blocks."""
    N = len(s)
    threshold = np.float32(threshold)
    off = [0, N] if seg_off is None else [int(v) for v in seg_off]
    out = []
    for j in range(len(off) - 1):
        rows, cold = [], 0
        for r in range(max(off[j], 0), min(off[j + 1], N)):
            if s[r] >= threshold:                                  # False for NaN
                if rows and cold > max_gap:
                    out.append(rows)
                    rows = []
                rows.append(r)
                cold = 0
            else:
                cold += 1
        if rows:
            out.append(rows)
    return [(rows[0], rows[-1], len(rows), sorted((-ordered(s[r]), r) for r in rows)[0][1]) for rows in out]


def brute_range(S, threshold, max_gap, seg_off=None, ids=None):
    lims, D, I, Lo, Hi, Cnt = [0], [], [], [], [], []
    for q in range(S.shape[0]):
        for lo, hi, cnt, peak in brute_moments(S[q], threshold, max_gap, seg_off):
            D.append(S[q, peak] + np.float32(0.0))
            I.append(peak if ids is None else ids[peak])
            Lo.append(lo), Hi.append(hi), Cnt.append(cnt)
        lims.append(len(D))
    i64 = lambda v: np.asarray(v, np.int64).reshape(-1)            # noqa: E731
    return i64(lims), np.asarray(D, np.float32).reshape(-1), i64(I), i64(Lo), i64(Hi), i64(Cnt)


def brute_topk(S, k, threshold, max_gap, min_count=1, rank="peak", seg_off=None, ids=None):
    nq = S.shape[0]
    D = np.full((nq, k), -FLT_MAX, np.float32)
    I, Lo, Hi = (np.full((nq, k), -1, np.int64) for _ in range(3))
    Cnt = np.zeros((nq, k), np.int64)
    for q in range(nq):
        ms = [m for m in brute_moments(S[q], threshold, max_gap, seg_off) if m[2] >= min_count]
        ms.sort(key=(lambda m: (-m[2], m[0])) if rank == "count" else (lambda m: (-ordered(S[q, m[3]]), m[3])))
        for slot, (lo, hi, cnt, peak) in enumerate(ms[:k]):
            D[q, slot] = S[q, peak] + np.float32(0.0)
            I[q, slot] = peak if ids is None else ids[peak]
            Lo[q, slot], Hi[q, slot], Cnt[q, slot] = lo, hi, cnt
    return D, I, Lo, Hi, Cnt


def small_cases(count=240, seed=17):
    """(S float32 [nq,N], threshold, max_gap, seg_off or None): the scores and segment layouts of group_cases.small_scores (N <= 24,
    half of them half-integer scores), the threshold one of the scores (so that equality occurs), max_gap in 0 .. 3."""
    rng = np.random.default_rng(seed)
    for S, seg in small_scores(count, seed):
        yield S, float(S.reshape(-1)[int(rng.integers(S.size))]), int(rng.integers(0, 4)), seg


def pattern_rows(C, d=20):
    """C float32 [N,P], P <= d -> (rows X float32 [N,d], queries float32 [P,d]) with <query j, row r> = C[r, j] exactly: row r is
    sum_j C[r, j] e_j and query j is e_j, so every product but one is a zero and no sum rounds."""
    C = np.asarray(C, np.float32)
    N, P = C.shape
    X = np.zeros((N, d), np.float32)
    X[:, :P] = C
    return X, np.eye(P, d, dtype=np.float32)
