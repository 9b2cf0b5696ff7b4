"""Seeded inputs shared by the CPU and the GPU suite of the fused search (ivr_amd/fusion.py, csrc/search_fused.hip), and the brute
force the numpy definition is checked against: Python loops over rows with np.float32 scalars, the pairwise tree spelled out.  Nothing
here calls the code under test."""
import numpy as np

from event_cases import make_rows, ordered  # noqa: F401  (make_rows is re-exported to both suites)

FLT_MAX = np.float32(3.4028234663852886e38)
FOLDS = ("max", "min", "sum")
COMBINES = ("margin", "veto")
f32 = np.float32


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def make_members(d, nq, m, seed):
    return np.random.default_rng([seed, d, nq, m]).standard_normal((nq, m, d)).astype(np.float32)


def make_weights(nq, m, seed):
    """Random weights in [-2, 2) with a few exact -1 and 1."""
    rng = np.random.default_rng([seed, nq, m, 7])
    w = (rng.random((nq, m)) * 4 - 2).astype(np.float32)
    w[rng.random((nq, m)) < 0.2] = -1.0
    w[rng.random((nq, m)) < 0.2] = 1.0
    return w


def make_mask(nq, m, seed):
    """bool [nq,m] with absent slots first (set 0), last (set 1), in the middle (set 2) and at random beyond; every set keeps a member."""
    rng = np.random.default_rng([seed, nq, m, 11])
    mask = rng.random((nq, m)) < 0.7
    if m >= 2:
        for q, hole in zip(range(nq), (0, m - 1, m // 2)):
            mask[q] = True
            mask[q, hole] = False
    mask[~mask.any(axis=1), 0] = True
    return mask


def pad_pow2(n):
    p = 1
    while p < n:
        p *= 2
    return p


def tree_sum(t):
    """The balanced pairwise float32 sum of the 1, 2, 4, 8 or 16 terms t, written out."""
    t = [f32(v) for v in t]
    if len(t) == 1:
        return t[0]
    if len(t) == 2:
        return f32(t[0] + t[1])
    if len(t) == 4:
        return f32(f32(t[0] + t[1]) + f32(t[2] + t[3]))
    if len(t) == 8:
        return f32(f32(f32(t[0] + t[1]) + f32(t[2] + t[3])) + f32(f32(t[4] + t[5]) + f32(t[6] + t[7])))
    assert len(t) == 16
    return f32(tree_sum(t[:8]) + tree_sum(t[8:]))


def brute_one(s, w, r, fold, combine):
    """F of one row: s, w, r = the member scores, weights and roles of the set, slot by slot."""
    slots = len(s)
    T = [f32(f32(w[j]) * f32(f32(s[j]) + f32(0.0))) for j in range(slots)]
    pos = [T[j] for j in range(slots) if r[j] > 0]
    neg = [T[j] for j in range(slots) if r[j] < 0]
    if fold == "max":
        P = max(pos)
    elif fold == "min":
        P = min(pos)
    else:
        terms = [T[j] if r[j] > 0 else f32(0.0) for j in range(slots)] + [f32(0.0)] * (pad_pow2(slots) - slots)
        P = tree_sum(terms)
    if not neg:
        return f32(P)
    Nn = max(neg)
    if combine == "margin":
        return f32(f32(P) - f32(Nn))
    return f32(P) if P > Nn else f32(-f32(f32(Nn) * f32(Nn)))


def brute_scores(S, W, R, fold, combine):
    """F float32 [nq,N] of S [nq,slots,N], W and R [nq,slots], row by row."""
    nq, slots, N = S.shape
    F = np.empty((nq, N), np.float32)
    with np.errstate(all="ignore"):
        for q in range(nq):
            for n in range(N):
                F[q, n] = brute_one(S[q, :, n], W[q], R[q], fold, combine)
    return F


def brute_topk(F, k, ids=None):
    nq, N = F.shape
    D = np.full((nq, k), -FLT_MAX, np.float32)
    I = np.full((nq, k), -1, np.int64)
    for q in range(nq):
        o = ordered(F[q])
        best = sorted(range(N), key=lambda n: (-int(o[n]), n))[:k]
        for j, n in enumerate(best):
            D[q, j] = F[q, n] + f32(0.0)
            I[q, j] = n if ids is None else ids[n]
    return D, I


def brute_range(F, threshold, ids=None):
    lims, D, I = [0], [], []
    for q in range(F.shape[0]):
        for n in range(F.shape[1]):
            v = f32(F[q, n] + f32(0.0))
            if v >= f32(threshold):
                D.append(v)
                I.append(n if ids is None else ids[n])
        lims.append(len(D))
    return np.asarray(lims, np.int64), np.asarray(D, np.float32), np.asarray(I, np.int64)


def small_scores(nq, slots, N, seed, halves=False):
    """S float32 [nq,slots,N]; halves: half-integer scores (ties, exact sums) with +0.0 and -0.0 among them."""
    rng = np.random.default_rng([seed, nq, slots, N])
    if halves:
        S = (rng.integers(-4, 5, size=(nq, slots, N)) / 2.0).astype(np.float32)
        S[rng.random(S.shape) < 0.1] = -0.0
        return S
    return rng.standard_normal((nq, slots, N)).astype(np.float32)


def small_roles(nq, slots, seed, negatives=True):
    """int8 [nq,slots]: 1, 0 and (with negatives) -1, with a positive member in every set and an absent slot in the middle of set 0."""
    rng = np.random.default_rng([seed, nq, slots, 3])
    R = rng.choice(np.array([1, 1, 0, -1] if negatives else [1, 1, 0], np.int8), size=(nq, slots))
    if slots >= 3:
        R[0, 0], R[0, 1], R[0, 2] = 1, 0, 1
    for q in range(nq):
        if not (R[q] > 0).any():
            R[q, rng.integers(slots)] = 1
    return R.astype(np.int8)
