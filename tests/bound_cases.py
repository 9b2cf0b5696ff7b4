"""Worst-case rows for the error bounds of the bf16 candidate scan, and a numpy model of that scan: shared by test_scan_bound_cpu.py
(which proves on the model alone that every case does what it claims) and test_scan_bound_gpu.py (which runs the cases through
FlatIPIndex).  A plain module, not a conftest: it builds inputs and models, it asserts nothing and touches no GPU.

The search is exact only because of a check on the device: the first excluded group's approximate maximum + e < the k-th exact score
(select_topk_kernel), with
    small batches (<= 64 queries, 64-row groups,  approx = bf16(row) . (q_hi + q_lo)):  e >= E_small = (2^-8 + 2^-15 + dp 2^-23) |q| max|row|
    large batches (>  64 queries, 16-row tiles,   approx = bf16(row) . q_hi):           e >= E_big = (|q| + |dq|) max|dr| + |dq| max|r| + dp 2^-23 |q| max|r|
(dq = q - bf16(q), dr = row - bf16(row), norms in float64, dp = d rounded up to 16).  The cases below put a row's true error at 0.95 ..
1.0 of these bounds, so that an e a few per cent too small returns a wrong neighbour and an e a quarter too large fails `safe`.

Layout of every case: N = 256 (kp + 1) + 356 rows (not a multiple of 64; just enough groups for the candidate scan to engage, kp =
fast_groups(k)) of filler 0.05 N(0, 1), with the special rows stored unnormalised, one per 128-row block (hence one per group and per
tile), the hidden rows in the highest blocks.  All special scores are sums of a few distinct products, so they can be stated exactly.

hidden (k = 1 and k = 10; both batch sizes).  Query: all ones.  H: k rows of constant h = 1 + 2^-8 - 2^-16, which rounds DOWN to 1.0, so
  approx(H) = d understates exact(H) = d h by 0.98 E_small / 0.998 E_big (d = 64).  Decoys, all bf16-exact (approx = exact): `top` rows
  of ones with n7 elements at 1 + 2^-7, n7 the smallest count that puts them at >= approx(H) + 0.955 E_small, still below exact(H);
  `low` rows of ones, scoring exactly approx(H).  40 decoys in all:
    sharp  kp top + (40 - kp) low.  The kp re-scored groups are the top decoys, the k-th exact score is a top decoy's, the first
           excluded group scores approx(H) = d: the check must fire, and does so iff e >= 0.956 E.  An e 5 % short accepts the decoys.
    tied   all 40 at the top level: the first excluded group ties the k-th score, so the strict check fires whatever e is.  Pins the
           strict inequality and the exact pass, not the size of e (which is why `sharp` exists).
    safe   k winners at the top level, everything else lowered by at least 1.25 E: 40 - k low decoys of ones with j elements at
           1 - 2^-8, and the hidden rows on top of a low decoy (each element half a bf16 step above it, rounding down), whose exact
           score stays below the winners'.  The true top-k are the winners, they are re-scored, and the check must PASS: a bound more
           than a quarter too large (or a maximum that counts rows it should not) shows as a redone query.
qrem (large batch only).  Query: h on the first half of the coordinates, 1 on the second; bf16(q) = ones, so the large-batch scan, which
  uses q_hi only, understates the winner W (2.0 on the first half, 0 on the second: bf16-exact) by |dq| |W|: the `|dq| max|r|` term alone.
  Decoys are 0 on the first half and 2 + 2^-6 / 2 - 2^-7 / 2 on the second: bf16-exact, approx = exact; kp top + (40 - kp) low as above.
  The filler rows are rounded to bf16 here, so max|dr| = 0 and a bound without the dq term is ~0.
prune (large batch, k = 1).  The best tile holds P: ones with m elements at 1 + 2^-8 + 2^-16, which round UP, so approx(P) overstates.
  H sits in the second-best tile, approx(P) - approx(H) = 0.96 .. 0.97 of 2 E_big, exact(H) > exact(P).  The pruned re-score must
  still fetch H's tile; pruning at 1 e drops it, and the verification then passes (every other tile is filler), so P is returned.
nonfinite.  Gaussian rows; a few hold 3.4e38 at coordinates where every query is 0 (bf16 image +inf, approximate score NaN), a few
  have norm ~1e30.  No bound exists: every query must be redone and the result must be the exact scan's."""
import numpy as np

H_ELEM = np.float32(1 + 2.0 ** -8 - 2.0 ** -16)       # rounds down to 1.0 in bf16: just below the midpoint of [1, 1 + 2^-7]
UP_ELEM = np.float32(1 + 2.0 ** -8 + 2.0 ** -16)      # rounds up to 1 + 2^-7
N_DECOYS = 40
DIMS = (64, 512)                                      # d = 512: 16 pieces, the LDS-ring kernel for <= 16 queries
SCALES = (1.0, 2.0, 0.5)                              # powers of two: every score, approximation and bound scales exactly
SMALL_NQ = (1, 10, 64)
BIG_NQ = (65, 300)


def fast_groups(k):
    """ivr_index::fast_groups: groups (tiles) re-scored behind the candidate scan."""
    return k + max(22, k)


def n_rows(k):
    """4 (kp + 1) groups is where the candidate scan engages (ivr_index::fast_scan); five groups and 36 rows more."""
    return 256 * (fast_groups(k) + 1) + 356


def dp_of(d):
    return (d + 15) // 16 * 16


# ---------------------------------------------------------------------------------------------------------------------------------
# the model: bf16 rounding, the two approximate scores, maxima, the analytic bounds
# ---------------------------------------------------------------------------------------------------------------------------------
def bf16_round(x):
    """float32 -> the float32 value of its bf16 image: round to nearest even on the upper 16 bits (overflow goes to inf)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    u = x.view(np.uint32).astype(np.uint64)
    r = ((u + np.uint64(0x7FFF) + ((u >> np.uint64(16)) & np.uint64(1))) >> np.uint64(16)) << np.uint64(16)
    out = (r & np.uint64(0xFFFFFFFF)).astype(np.uint32).view(np.float32).reshape(x.shape)
    return np.where(np.isnan(x), x, out)


def split_q(Q):
    """(q_hi, q_lo) of the small-batch scan: hi = bf16(q), lo = bf16(q - hi) (the subtraction is exact in float32)."""
    Q = np.ascontiguousarray(Q, dtype=np.float32)
    hi = bf16_round(Q)
    with np.errstate(invalid="ignore"):
        lo = bf16_round(Q - hi)
    return hi, lo


def exact_scores(X, Q):
    return np.asarray(Q, np.float64) @ np.asarray(X, np.float64).T


def approx_small(X, Q):
    """bf16(row) . (q_hi + q_lo) in float64, [nq, N]."""
    hi, lo = split_q(Q)
    with np.errstate(invalid="ignore", over="ignore"):
        return (hi.astype(np.float64) + lo.astype(np.float64)) @ bf16_round(X).astype(np.float64).T


def approx_big(X, Q):
    """bf16(row) . q_hi in float64, [nq, N]."""
    with np.errstate(invalid="ignore", over="ignore"):
        return bf16_round(Q).astype(np.float64) @ bf16_round(X).astype(np.float64).T


def group_max(S, rows):
    """[nq, N] scores -> [nq, ceil(N / rows)] maxima of consecutive `rows` rows (64: groups, 16: tiles, 128: blocks); NaN never wins,
    as with fmaxf."""
    nq, n = S.shape
    pad = (-n) % rows
    S = np.where(np.isnan(S), -np.inf, S)
    S = np.concatenate([S, np.full((nq, pad), -np.inf)], axis=1)
    return S.reshape(nq, -1, rows).max(axis=2)


def ranked(m):
    """positions of one query's maxima in selection order: maximum descending, equal maxima the lower position first."""
    return np.lexsort((np.arange(len(m)), -m))


def selected_small(X, q, kp):
    """Small batch: (the kp re-scored groups in order, the first excluded group or -1, the approximate group maxima)."""
    gm = group_max(approx_small(X, q[None, :]), 64)[0]
    order = ranked(gm)
    return order[:kp], (int(order[kp]) if len(order) > kp else -1), gm


def selected_big(X, q, kp):
    """Large batch, two levels as search_big does it: the kp + 1 best 128-row blocks, then the kp + 1 best 16-row tiles among their
    tiles.  Returns (the kp re-scored tiles in order, the first excluded tile or -1, the approximate tile maxima)."""
    S = approx_big(X, q[None, :])
    tm, bm = group_max(S, 16)[0], group_max(S, 128)[0]
    blocks = ranked(bm)[:kp + 1]
    tiles = np.concatenate([np.arange(8 * b, min(8 * b + 8, len(tm))) for b in blocks])
    order = tiles[np.lexsort((tiles, -tm[tiles]))]
    return order[:kp], (int(order[kp]) if len(order) > kp else -1), tm


def _norms(A):
    with np.errstate(over="ignore", invalid="ignore"):
        return np.sqrt((np.asarray(A, np.float64) ** 2).sum(axis=-1))


def e_small(X, Q, d):
    """E_small per query, from the mathematics: bf16 keeps 8 significant bits of a row element (2^-8 relative), hi + lo of the query
    leaves 2^-16 relative per element (2^-15 covers it against the rounded row), dp float32 accumulation steps."""
    return (2.0 ** -8 + 2.0 ** -15 + dp_of(d) * 2.0 ** -23) * _norms(Q) * _norms(X).max()


def e_big(X, Q, d):
    """E_big per query: |bf16(r).bf16(q) - r.q| = |dr.q_hi + r.dq| <= |dr| (|q| + |dq|) + |r| |dq|, plus the accumulation term."""
    X, Q = np.asarray(X, np.float32), np.asarray(Q, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        dr, dq = _norms(X - bf16_round(X)).max(), _norms(Q - bf16_round(Q))
    qn, rn = _norms(Q), _norms(X).max()
    return (qn + dq) * dr + dq * rn + dp_of(d) * 2.0 ** -23 * qn * rn


def f32_sum_bound(x, q):
    """Bound of the float32 score of one (row, query) pair against the float64 one, sequential accumulation: (d + 8) 2^-24 sum|q_i x_i|
    (oracle/search_ref.py flat_ip_bound) - or 0 when every product is a multiple of one power of two g and sum|q_i x_i| <= 2^24 g, so
    that every partial sum, in any order, is a float32 and nothing is ever rounded."""
    p = np.asarray(x, np.float64) * np.asarray(q, np.float64)
    a = np.abs(p).sum()
    nz = p[p != 0]
    if len(nz) == 0:
        return 0.0
    g = 2.0 ** -40
    while g < 1 and np.all(nz / (2 * g) == np.round(nz / (2 * g))):
        g *= 2
    if np.all(nz / g == np.round(nz / g)) and a <= 2.0 ** 24 * g:
        return 0.0
    return (len(p) + 8) * 2.0 ** -24 * a


# ---------------------------------------------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------------------------------------------
def _filler(rng, n, d):
    return (0.05 * rng.standard_normal((n, d))).astype(np.float32)


def _places(rng, n, count):
    """`count` rows in `count` different whole 128-row blocks, ascending: one special row per block, group and tile.  Block 0 stays
    filler, so that an overwrite of the special rows can start at an unaligned row in front of them."""
    nblk = n // 128
    assert count <= nblk - 1, (count, nblk)
    blocks = 1 + np.sort(rng.choice(nblk - 1, count, replace=False))
    return blocks * 128 + rng.integers(0, 128, count)


def _case(kind, d, k, X, F, q, hidden, top, low, winners, paths):
    """hidden: the rows the approximate ranking must lose; winners: the float64 top-k, in result order; top / low: the decoys; F: the
    filler rows alone (what an index holds before the special rows are stored); paths: `small`, `big` or both."""
    return dict(kind=kind, d=d, k=k, kp=fast_groups(k), N=len(X), X=X, F=F, q=q.astype(np.float32), hidden=np.asarray(hidden, np.int64),
                top=np.asarray(top, np.int64), low=np.asarray(low, np.int64), winners=np.asarray(winners, np.int64), paths=paths)


def hidden_case(d, k=1, variant="sharp"):
    rng = np.random.default_rng(1000 + d + 7 * k)
    n, kp = n_rows(k), fast_groups(k)
    F = _filler(rng, n, d)
    q = np.ones(d, np.float32)
    H = np.full(d, H_ELEM, np.float32)
    E = max(e_small(H[None, :], q[None, :], d)[0], e_big(H[None, :], q[None, :], d)[0])       # max|row| and max|dr| are H's
    n7 = int(np.ceil(0.955 * E * 128))
    top_row = np.ones(d, np.float32)
    top_row[:n7] = 1 + 2.0 ** -7
    low_row = np.ones(d, np.float32)
    hid_row = H
    n_top = {"sharp": kp, "tied": N_DECOYS, "safe": k}[variant]
    if variant == "safe":
        # everything but the winners at least 1.25 E below them: ones with j elements one bf16 step (2^-8) below 1
        j = int(np.ceil((1.25 * E * 1.002 - n7 / 128) * 256))
        low_row[d - j:] = 1 - 2.0 ** -8
        hid_row = np.where(low_row == 1, H_ELEM, np.float32(1 - 2.0 ** -9 - 2.0 ** -17)).astype(np.float32)
    rows = _places(rng, n, N_DECOYS + k)
    # the hidden rows take the highest blocks: among equal approximate maxima they rank last
    dec, hid = rng.permutation(rows[:N_DECOYS]), rows[N_DECOYS:]
    top, low = np.sort(dec[:n_top]), np.sort(dec[n_top:])
    X = F.copy()
    X[top], X[low], X[hid] = top_row, low_row, hid_row
    winners = top[:k] if variant == "safe" else hid
    return _case("hidden_" + variant, d, k, X, F, q, hid, top, low, winners, ("small", "big"))


def qrem_case(d):
    k, rng = 1, np.random.default_rng(2000 + d)
    n, kp, h = n_rows(k), fast_groups(k), d // 2
    F = bf16_round(_filler(rng, n, d))
    q = np.ones(d, np.float32)
    q[:h] = H_ELEM
    W = np.zeros(d, np.float32)
    W[:h] = 2.0
    low_row = np.zeros(d, np.float32)
    low_row[h:] = 2.0
    E = e_big(np.stack([W, low_row]), q[None, :], d)[0]
    # the top decoys' score above approx(W) = d, in steps of 2^-7: m = 2 up - down, `up` elements at 2 + 2^-6, `down` at 2 - 2^-7
    m = int(np.ceil(0.955 * E * 128))
    up = (m + 1) // 2
    down = 2 * up - m
    top_row = low_row.copy()
    top_row[h:h + up] = 2 + 2.0 ** -6
    top_row[h + up:h + up + down] = 2 - 2.0 ** -7
    rows = _places(rng, n, N_DECOYS + 1)
    dec = rng.permutation(rows[:-1])
    top, low, hid = np.sort(dec[:kp]), np.sort(dec[kp:]), rows[-1:]
    X = F.copy()
    X[top], X[low], X[hid] = top_row, low_row, W
    return _case("qrem", d, k, X, F, q, hid, top, low, hid, ("big",))


def prune_case(d):
    k, rng = 1, np.random.default_rng(3000 + d)
    n = n_rows(k)
    F = _filler(rng, n, d)
    q = np.ones(d, np.float32)
    H = np.full(d, H_ELEM, np.float32)
    E = e_big(H[None, :], q[None, :], d)[0]
    # the largest m with an approximate gap m 2^-7 <= 0.97 * 2 E whose exact order is firm in float32: exact(H) - exact(P) above the
    # accumulation bounds of both scores
    m = int(np.floor(0.97 * 2 * E * 128))
    while True:
        P = np.ones(d, np.float32)
        P[:m] = UP_ELEM
        if float(H.astype(np.float64).sum() - P.astype(np.float64).sum()) > 1.05 * (f32_sum_bound(H, q) + f32_sum_bound(P, q)):
            break
        m -= 1
    rows = _places(rng, n, 2)
    X = F.copy()
    X[rows[0]], X[rows[1]] = P, H
    return _case("prune", d, k, X, F, q, rows[1:], rows[:1], [], rows[1:], ("big",))


NONFINITE_ZERO_COORDS = (0, 5, 33)       # every nonfinite-case query is 0 here; the huge elements sit here


def nonfinite_case(d):
    k, rng = 10, np.random.default_rng(4000 + d)
    n = n_rows(k)
    X = rng.standard_normal((n, d)).astype(np.float32)
    rows = _places(rng, n, 8)
    for i, r in enumerate(rows[:4]):
        X[r, NONFINITE_ZERO_COORDS[i % 3]] = np.float32(3.4e38 if i % 2 == 0 else -3.4e38)
    for r in rows[4:]:
        X[r] *= np.float32(1e30 / np.sqrt(d))
    q = rng.standard_normal(d).astype(np.float32)
    q[list(NONFINITE_ZERO_COORDS)] = 0
    return _case("nonfinite", d, k, X, X, q, rows[:4], rows[4:], [], [], ("small", "big"))


def queries(case, nq, fillers=True, seed=0):
    """(Q float32 [nq, d], adv bool [nq]).  Small batches (nq <= 64): the case's query at the scales 1, 2, 0.5 in turn, all adversarial.
    Large batches: the same for the first two thirds, then Gaussian fillers (unless fillers=False: `safe` asks that NO query is redone,
    which nothing guarantees for a Gaussian query against these rows).  nonfinite: Gaussian queries that are 0 at the huge coordinates."""
    d = case["d"]
    rng = np.random.default_rng(5000 + d + nq + seed)
    if case["kind"] == "nonfinite":
        Q = rng.standard_normal((nq, d)).astype(np.float32)
        Q[0] = case["q"]
        Q[:, list(NONFINITE_ZERO_COORDS)] = 0
        return Q, np.ones(nq, bool)
    nadv = nq if (nq <= 64 or not fillers) else (2 * nq) // 3
    Q = rng.standard_normal((nq, d)).astype(np.float32)
    for i in range(nadv):
        Q[i] = case["q"] * np.float32(SCALES[i % len(SCALES)])
    adv = np.arange(nq) < nadv
    return Q, adv


def topk_f64(X, Q, k):
    """float64 top-k ids [nq, k]: score descending, equal scores the lower id first."""
    S = exact_scores(X, Q)
    return np.stack([np.lexsort((np.arange(S.shape[1]), -s))[:k] for s in S]).astype(np.int64)


def range_radii(case):
    """Radii for the hidden_sharp data and the query at scale 1, with the float64 result each must give:
    a quarter of the way from the top decoys (whose float32 score is exact) to exact(H): H alone (its group's approximate maximum is
    0.96 E below the radius);
    between the low and the top decoys: H and the top decoys;  below the low decoys: H and all 40 decoys."""
    X, q = case["X"], case["q"]
    s = exact_scores(X, q[None, :])[0]
    sH, sT, sL = s[case["hidden"]].min(), s[case["top"]].max(), s[case["low"]].max()
    out = []
    for r in (sT + 0.25 * (sH - sT), 0.5 * (sT + sL), sL - 2.0 ** -4):
        r = float(np.float32(r))
        out.append((r, np.nonzero(s > r)[0].astype(np.int64)))
    return out


CASE_NAMES = ("sharp_k1", "sharp_k10", "tied_k1", "safe_k1", "safe_k10", "qrem", "prune", "nonfinite")
_CACHE = {}


def make(name, d):
    """The case `name` at dimension d, built once per process (the arrays are shared: leave them unchanged)."""
    if (name, d) not in _CACHE:
        if name == "qrem":
            c = qrem_case(d)
        elif name == "prune":
            c = prune_case(d)
        elif name == "nonfinite":
            c = nonfinite_case(d)
        else:
            variant, k = name.split("_k")
            c = hidden_case(d, int(k), variant)
        for a in c.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _CACHE[(name, d)] = c
    return _CACHE[(name, d)]
