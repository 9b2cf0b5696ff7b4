"""Seeded inputs shared by the CPU and the GPU suite of the diversified search (ivr_amd/diversify.py, csrc/search_diverse.hip), the
brute-force statement of the rule that the numpy definition is checked against, and the checks that keep the cases from passing
vacuously.  Nothing here calls the code under test."""
import numpy as np

from event_cases import make_rows

FLT_MAX = np.float32(3.4028234663852886e38)
ABSENT = (-1, None, 2**40)                     # None stands for ntotal


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(got, want):
    return all(a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(got, want))


# -- the rule, once more, without numpy's sorting ----------------------------------------------------------------------------------
def order_key(v):
    """float32 -> int that orders like the value with -0.0 equal to +0.0 (written out here, not imported from the package)."""
    u = int((np.float32(v) + np.float32(0.0)).view(np.uint32))
    return 0xFFFFFFFF - u if u & 0x80000000 else u | 0x80000000


def brute(R, P, cand, k, mode, param, ntotal=None, ids=None):
    """The rule as a loop over sets: mode "mmr" (param = lambda) or "suppress" (param = threshold).  Ties are resolved by sorting the
    tuples (value descending, row, position)."""
    R, P = np.asarray(R, np.float32), np.asarray(P, np.float32)
    nq, kc = R.shape
    zero = np.float32(0.0)
    lam = np.float32(param)
    mu = np.float32(1.0) - lam
    D = np.full((nq, k), -FLT_MAX, np.float32)
    I = np.full((nq, k), -1, np.int64)
    M = np.full((nq, k), -FLT_MAX, np.float32)
    for q in range(nq):
        rows = [int(c) for c in cand[q]]
        left = {j for j in range(kc) if rows[j] >= 0 and (ntotal is None or rows[j] < ntotal)}
        chosen = []

        def redundancy(j):
            best = -FLT_MAX
            for s in chosen:
                p = P[q, s, j] + zero
                if p > best:
                    best = p
            return best

        def value(j):
            r = R[q, j] + zero
            if mode == "suppress" or not chosen:
                return r
            return np.float32(np.float32(lam * r) - np.float32(mu * redundancy(j)))

        while len(chosen) < k and left:
            s = sorted((-order_key(value(j)), rows[j], j) for j in left)[0][2]
            t = len(chosen)
            D[q, t], M[q, t] = R[q, s] + zero, redundancy(s)
            I[q, t] = rows[s] if ids is None else ids[rows[s]]
            left.remove(s)
            chosen.append(s)
            if mode == "suppress":
                left = {j for j in left if not redundancy(j) >= np.float32(param)}
    return D, I, M


def small_cases(count=120, seed=5):
    """(R float32 [2,kc], P float32 [2,kc,kc], cand int64 [2,kc], ntotal): kc <= 9 over at most 6 rows, so rows are named twice;
    half-integer scores that are a function of the row in every second case (ties on the row and on the position), -0.0 entries,
    absent entries of all three kinds."""
    rng = np.random.default_rng(seed)
    for i in range(count):
        kc = int(rng.integers(1, 10))
        ntotal = int(rng.integers(1, 7))
        cand = rng.integers(0, ntotal, size=(2, kc)).astype(np.int64)
        if i % 2:
            rel = (rng.integers(-3, 4, size=(2, ntotal)) / 2.0).astype(np.float32)
            pair = (rng.integers(-3, 4, size=(ntotal, ntotal)) / 2.0).astype(np.float32)
            rel[rel == 0] = -0.0 if i % 4 == 1 else 0.0
            pair[pair == 0] = -0.0
            R = np.take_along_axis(rel, cand, axis=1)
            P = pair[cand[:, :, None], cand[:, None, :]]
        else:
            R = rng.standard_normal((2, kc)).astype(np.float32)
            P = rng.standard_normal((2, kc, kc)).astype(np.float32)
        for a in ABSENT:
            if rng.random() < 0.4:
                cand[int(rng.integers(0, 2)), int(rng.integers(0, kc))] = ntotal if a is None else a
        yield R, P, cand, ntotal


# -- rows, queries and candidate lists of the larger cases ----------------------------------------------------------------------------
def unit_rows(d, N, seed, period=None):
    """make_rows scaled to unit length: duplicates (period) stay duplicates to the bit, and a pair score is a cosine."""
    X = make_rows(d, N, seed, period)
    return (X / np.linalg.norm(X, axis=1, keepdims=True)).astype(np.float32)


def shot_rows(d, shots, per, seed, noise=1e-3):
    """`shots` runs of `per` near-duplicates: a unit row plus noise * a normal vector, scaled back to unit length."""
    rng = np.random.default_rng([seed, d, shots, per])
    base = np.repeat(rng.standard_normal((shots, d)), per, axis=0)
    X = base / np.linalg.norm(base, axis=1, keepdims=True) + noise * rng.standard_normal((shots * per, d))
    return (X / np.linalg.norm(X, axis=1, keepdims=True)).astype(np.float32)


def make_queries(d, nq, seed):
    return np.random.default_rng([seed, d, nq]).standard_normal((nq, d)).astype(np.float32)


def make_cand(nq, kc, N, seed, absent=False):
    """int64 [nq,kc] rows of an index of N rows: distinct per query while kc <= N, repeating beyond; with `absent` one entry of each
    kind of ABSENT in query 0 (kc >= 3)."""
    rng = np.random.default_rng([seed, nq, kc, N])
    if kc <= N:
        cand = np.stack([rng.permutation(N)[:kc] for _ in range(nq)]).astype(np.int64)
    else:
        cand = rng.integers(0, N, size=(nq, kc)).astype(np.int64)
    if absent and kc >= 3:
        at = rng.permutation(kc)[:3]
        cand[0, at] = [-1, N, 2**40]
    return cand


def k_values(kc):
    return sorted({1, min(2, kc), min(kc, 10), kc})


def host_scores(X, x):
    """(R [nq,N], P [N,N]) float32 stand-ins computed on the host, for the CPU checks that the cases hold what they are there for."""
    X64 = X.astype(np.float64)
    return (x.astype(np.float64) @ X64.T).astype(np.float32), (X64 @ X64.T).astype(np.float32)


def lists_of(Rfull, Pfull, cand):
    """R [nq,kc] and P [nq,kc,kc] of the candidate lists from the full tables; absent entries read row 0 and are never looked at."""
    N = Pfull.shape[0]
    c = np.where((cand >= 0) & (cand < N), cand, 0)
    return np.take_along_axis(Rfull, c, axis=1), Pfull[c[:, :, None], c[:, None, :]]


def row_tie_decides(I, D):
    """Two consecutive results with the same score bits and ascending rows: the row broke the tie."""
    return bool(((bits(D[:, 1:]) == bits(D[:, :-1])) & (I[:, 1:] > I[:, :-1]) & (I[:, :-1] >= 0)).any())


def ends_early(I):
    return bool(((I[:, 0] >= 0) & (I[:, -1] == -1)).any())
