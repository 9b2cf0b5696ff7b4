"""The inputs and the checks of the row-reduction suites (cosine, keep / drop chains, row normalisation, segment mean), shared by
the GPU suites (test_cosine_gpu.py, test_dedup_gpu.py, test_filters_gpu.py, test_keyframe_pipeline_gpu.py, test_normalize_gpu.py,
test_segment_mean_gpu.py) and by test_reduce_ref_cpu.py, which runs the very same checks on a numpy emulation of the kernels - the
correct one must pass them all, a faulty one must fail.  A plain module, not a conftest: it builds inputs and asserts.

Every check takes a backend `B`: numpy in, numpy out, one method per entry point (class Gpu below binds them to ivr_amd).  Every
tolerance comes from oracle/reduce_ref.py.  A check returns the largest error / bound ratio it saw where it compares with a bound."""
import numpy as np

from oracle import reduce_ref as R

COSINE_D = (1, 3, 63, 64, 65, 100, 384, 1025, 2048, 4099)
COSINE_N = (1, 4, 5, 103)
NORMALIZE_D = (1, 3, 33, 64, 65, 512, 2048, 4099)
NORMALIZE_N = (1, 4, 5, 1027)
WALK_CASES = ((1, 0.98), (63, 0.9), (65, 0.98), (100, 0.95), (1024, 0.98), (1025, 0.995), (1500, 0.9), (2048, 0.98))
TIE_D = (16, 1025, 2048)
SCENE_CASES = [(d, n) for d in (2048, 1000) for n in (2, 5, 50)]
SCENE_DIST = (1, 3, 5, 9)
WINDOW_CASES = ((3, 1, 2), (65, 63, 64), (65, 65, 65), (130, 1025, 7), (40, 2048, 40), (40, 2048, 1000))
SEGMENT_D = (1, 8, 255, 256, 257, 768, 1000)
SEGMENT_SIZES = (0, 1, 2, 63, 1000, 0, 5, 0)
KMEANS_CASES = ((4096, 64, 16), (2000, 300, 7))
SCALES = (-40, -17, -1, 0, 3, 22, 40)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _ratio(err, bound):
    """max err / bound; an element with bound 0 must have err 0."""
    err, bound = np.asarray(err, np.float64), np.asarray(bound, np.float64)
    assert err.shape == bound.shape
    assert not np.isnan(err).any(), "NaN in the output"
    zero = bound == 0
    assert (err[zero] == 0).all(), f"error {err[zero].max()} where the bound is 0"
    r = float((err[~zero] / bound[~zero]).max(initial=0.0))
    assert r <= 1.0, f"error / bound = {r:.3f}"
    return r


# ---------------------------------------------------------------------------------------------------------------------------------
# cosine
# ---------------------------------------------------------------------------------------------------------------------------------
def cosine_rows(kind, n, d, seed):
    rng = np.random.default_rng(seed)
    a = rng.standard_normal((n, d))
    b = rng.standard_normal((n, d))
    if kind == "near1":                      # mean 5, spread 0.1: cos near 1, every product positive
        a, b = 5 + 0.1 * a, 5 + 0.1 * b
    elif kind == "orth":                     # b made orthogonal to a in float64: cos is what the float32 rounding of b leaves
        a32 = a.astype(np.float32).astype(np.float64)
        b = b - a32 * ((a32 * b).sum(1) / (a32 * a32).sum(1))[:, None]
    elif kind != "gauss":
        raise ValueError(kind)
    return a.astype(np.float32), b.astype(np.float32)


def check_cosine_bound(B, d):
    worst = 0.0
    for n in COSINE_N:
        for kind in ("gauss", "near1", "orth"):
            a, b = cosine_rows(kind, n, d, 1000 * d + n)
            out = B.rowwise_cosine(a, b)
            assert out.dtype == np.float32 and out.shape == (n,)
            worst = max(worst, _ratio(np.abs(out.astype(np.float64) - R.cosine_ref(a, b)), R.cosine_bound(a, b)))
    return worst


def support(d, count=16):
    """`count` distinct columns of a row of d floats: 0, d - 1, 63 and 64 where they exist, the rest spread evenly."""
    cols = [c for c in (0, d - 1, 63, 64) if 0 <= c < d]
    cols += [int(c) for c in np.linspace(0, d - 1, 4 * count).round()]
    out = list(dict.fromkeys(cols))[:count]
    assert len(out) == count, (d, count)
    return out


def exact_rows(d):
    """{0, 1} rows whose sums are exact in any order: `a` sixteen ones (norm 4), `b` four of them (0, d - 1 and 63, 64 where they
    exist; norm 2), `c` sixteen ones off a's support when the row is wide enough (else None).  cos(a, b) = 4 / (4 * 2) = 0.5."""
    cols = support(d)
    a, b = np.zeros(d, np.float32), np.zeros(d, np.float32)
    a[cols] = 1
    b[cols[:4]] = 1
    c = None
    if d >= 32:
        c = np.zeros(d, np.float32)
        c[[k for k in range(d) if k not in cols][-16:]] = 1
    return a, b, c


def check_cosine_exact(B, d):
    a, b, c = exact_rows(d)
    assert a[0] == a[63] == a[64] == a[d - 1] == 1 and b[0] == b[63] == b[64] == b[d - 1] == 1 and c.sum() == 16 and not (a * c).any()
    A = np.stack([a, a, a, b, c, a])
    Bm = np.stack([b, a, c, b, c, np.zeros(d, np.float32)])
    want = np.array([0.5, 1.0, 0.0, 1.0, 1.0, 0.0], np.float32)
    assert np.array_equal(bits(B.rowwise_cosine(A, Bm)), bits(want))
    assert np.array_equal(bits(B.rowwise_cosine(Bm, A)), bits(want))


def square_rows():
    """Integer rows whose sum of squares is a perfect square (dot = ss exactly, the root exact, ss / ss = 1)."""
    rows = []
    for d in (1, 3, 65, 100, 1025):
        x = np.zeros((4, d), np.float32)
        x[0, d - 1] = 3                                           # 9
        x[1, d - 1] = -7                                          # 49
        x[2, d - 1] = 5
        x[3, d - 1] = -12
        if d >= 3:
            x[1, 0], x[1, d - 1] = 3, -4                          # 25
            x[3, [0, 1]] = (3, 4)                                 # 169
        if d >= 65:
            x[2, support(d)] = 2                                  # 64, columns 0, 63, 64 and d - 1 among the sixteen
        rows.append(x)
    return rows


def check_cosine_special(B):
    rng = np.random.default_rng(77)
    for d in (1, 3, 65, 1025):
        x = rng.standard_normal((5, d)).astype(np.float32)
        z = np.zeros_like(x)
        for a, b in ((x, z), (z, x), (z, z)):
            assert np.array_equal(bits(B.rowwise_cosine(a, b)), np.zeros(5, np.uint32)), d       # +0.0, not -0.0 and not NaN
    for x in square_rows():
        assert np.array_equal(bits(B.rowwise_cosine(x, x)), bits(np.ones(len(x)))), x.shape
    # powers of two scale every product, every partial sum and both roots exactly: no output bit may move
    for d in (1, 3, 65, 384, 1025):
        sign = np.where(rng.random((len(SCALES) ** 2, d)) < 0.5, -1.0, 1.0)
        a = (sign * rng.uniform(0.5, 1.0, sign.shape)).astype(np.float32)        # entries away from 0: no square near the denormals
        b = (a + 0.5 * rng.uniform(-1.0, 1.0, sign.shape)).astype(np.float32)
        b = np.where(np.abs(b) < 0.25, np.float32(0.25), b).astype(np.float32)
        a[:], b[:] = a[:1], b[:1]
        s = np.repeat(SCALES, len(SCALES))
        t = np.tile(SCALES, len(SCALES))
        base = B.rowwise_cosine(a, b)
        assert np.all(bits(base) == bits(base)[0])
        got = B.rowwise_cosine(np.ldexp(a, s[:, None]), np.ldexp(b, t[:, None]))
        assert np.array_equal(bits(got), bits(base)), (d, got, base)


def check_calculate_similarities(B):
    rng = np.random.default_rng(5)
    for n, d in ((2, 3), (7, 3), (6, 1), (9, 65), (5, 1025)):
        E = rng.standard_normal((n, d)).astype(np.float32)
        got = B.calculate_similarities(E)
        assert got.shape == (n - 1,)
        assert np.array_equal(bits(got), bits(B.rowwise_cosine(E[:-1].copy(), E[1:].copy()))), (n, d)
    assert len(B.calculate_similarities(E[:1])) == 0


# ---------------------------------------------------------------------------------------------------------------------------------
# the carried keep / drop chain (dedup_kernel through DedupState)
# ---------------------------------------------------------------------------------------------------------------------------------
def random_walk(d, thr, n=300):
    """The sequence of test_random_walk for the first seed in d .. d + 49 whose decisions all clear the threshold by more than four
    times the bound of their cosine.  Returns (E, mask, Comparisons)."""
    for seed in range(d, d + 50):
        rng = np.random.default_rng(seed)
        E = (np.cumsum(rng.standard_normal((n, d)) * 0.2, axis=0) + 2.0).astype(np.float32)
        mask, cmp, _ = R.keep_chain_ref(E, thr)
        if cmp.clear_of(thr):
            return E, mask, cmp
    raise AssertionError(f"d={d} thr={thr}: no seed in {d}..{d + 49} keeps every decision clear of the threshold")


def chunk_rows(d):
    return max(1, 8192 // d)


def check_random_walk(B, d, thr):
    E, mask, cmp = random_walk(d, thr)
    n = len(E)
    gap, need = cmp.margin(thr)
    assert gap > need
    assert 1 < mask.sum() < n
    rc = chunk_rows(d)
    split = 2 * rc + 1 if 2 * rc + 1 < n else 137                 # not a multiple of the chunk length
    assert 0 < split < n and split % rc
    for batches in ([(0, n)], [(0, 1), (1, n)], [(0, split), (split, n)], [(0, split), (split, split + 1), (split + 1, n)]):
        st = B.dedup_state(d)
        got = np.concatenate([st.keep_mask(E[a:b], thr) for a, b in batches])
        assert np.array_equal(got, mask), (d, thr, batches, np.flatnonzero(got != mask)[:8])
        assert np.array_equal(st.bits(), np.concatenate([bits(np.ones(1)), bits(E[np.flatnonzero(mask)[-1]])]))
    return int(mask.sum())


def small_chain(d=2048, n=9):
    """Nine frames in chunks of four: orthogonal directions u_k and their near copies.  Kept: 0, 3 (last row of chunk 0), 5 and 7
    (last row of chunk 1); the frame after a kept one resembles IT and not the frame kept before, so it is dropped only if the
    kept frame really became the one to compare with."""
    u = np.zeros((6, d), np.float32)
    for k in range(6):
        u[k, support(d, 64)[k::6]] = 1 + k
    near = lambda x, k: (x + np.float32(0.01) * u[k]).astype(np.float32)      # noqa: E731
    E = np.stack([u[0], near(u[0], 1), near(u[0], 2), u[1], near(u[1], 0), u[2], near(u[2], 1), u[3], near(u[3], 4)])[:n]
    return E, 0.9


def check_small_chain_splits(B):
    E, thr = small_chain()
    d, n = E.shape[1], len(E)
    mask, cmp, _ = R.keep_chain_ref(E, thr)
    assert cmp.clear_of(thr) and list(np.flatnonzero(mask)) == [0, 3, 5, 7]
    for k in range(n + 1):
        st = B.dedup_state(d)
        got = []
        for a, b in ((0, k), (k, n)):
            got.append(st.keep_mask(E[a:b], thr))
            assert got[-1].shape == (b - a,)
            if b == 0:
                assert not st.bits().any()                                    # an empty first batch leaves the fresh state
                continue
            want, _, last = R.keep_chain_ref(E[:b], thr)
            assert np.array_equal(st.bits(), np.concatenate([bits(np.ones(1)), bits(E[last])])), (k, b)
        assert np.array_equal(np.concatenate(got), mask), (k, np.concatenate(got))


def check_carried_state(B):
    """A batch that keeps nothing leaves every bit of the state alone, and the next batch is judged against the older frame."""
    rng = np.random.default_rng(3)
    for d in (65, 1025, 2048):
        first = rng.standard_normal((3, d)).astype(np.float32)
        first[1] = first[0]
        first[2] = first[0] * np.float32(2)                       # cos = 1 exactly: kept is row 0 only
        st = B.dedup_state(d)
        assert list(st.keep_mask(first, 0.98)) == [True, False, False]
        st.poke0(2.0)                                             # any non-zero flag means "a frame is carried": it must survive too
        before = st.bits().copy()
        assert np.array_equal(before[1:], bits(first[0])) and before[0] == bits(np.float32(2.0))
        same = np.repeat(first[:1], 2 * chunk_rows(d) + 1, axis=0)
        assert not st.keep_mask(same, 0.98).any()
        assert np.array_equal(st.bits(), before), d
        nxt = np.stack([first[0] * np.float32(0.5), -first[0], first[0]])
        want, cmp, last = R.keep_chain_ref(nxt, 0.98, prev=first[0])
        assert list(want) == [False, True, True] and cmp.clear_of(0.98)
        assert np.array_equal(st.keep_mask(nxt, 0.98), want)
        assert np.array_equal(st.bits(), np.concatenate([bits(np.ones(1)), bits(nxt[last])]))
        st.reset()
        assert not st.bits().any()
        assert list(st.keep_mask(nxt[2:], 0.98)) == [True]        # a new chain: its first frame is kept whatever came before
        assert np.array_equal(st.bits(), np.concatenate([bits(np.ones(1)), bits(nxt[2])]))


def check_zero_rows(B):
    rng = np.random.default_rng(4)
    for d in (3, 100, 2048):
        x = rng.standard_normal((4, d)).astype(np.float32)
        z = np.zeros(d, np.float32)
        for pos, E in (("first", np.stack([z, x[0], x[0]])), ("middle", np.stack([x[0], z, x[0], z, z])), ("last", np.stack([x[0], x[0], z]))):
            for thr in (0.5, 0.0, -0.5):
                want, cmp, _ = R.keep_chain_ref(E, thr)
                assert cmp.clear_of(thr) or thr == 0.0            # sim = 0 against thr = 0 is an exact tie: bound 0 on a zero row
                st = B.dedup_state(d)
                got = st.keep_mask(E, thr)
                assert np.array_equal(got, want), (d, pos, thr, got, want)
                # sim = 0 (zero norm -> 1): kept below thr = 0.5, dropped at 0.0 (>=) and at -0.5
                zr = np.flatnonzero(~E.any(axis=1))
                assert all(got[i] == (thr == 0.5) for i in zr if i > 0)
        # a kept zero row is what the next frames are compared with: every one has sim = 0 < 0.5 and is kept, and carried
        E = np.stack([x[0], z, x[0], x[0], z])
        st = B.dedup_state(d)
        assert list(st.keep_mask(E, 0.5)) == [True, True, True, False, True]
        assert np.array_equal(st.bits(), np.concatenate([bits(np.ones(1)), np.zeros(d, np.uint32)]))
        assert list(st.keep_mask(np.stack([z, x[1]]), 0.5)) == [True, True]
        assert list(st.keep_mask(np.stack([x[1], z, z]), 0.0)) == [False, False, False]


def tie_rows(d):
    """(a, b): cos(a, b) = 0.5 and cos(a, a) = 1 exactly in float32 in any summation order, non-zeros in the last column."""
    if d >= 32:
        a, b, _ = exact_rows(d)
        return a, b
    a, b = np.ones(d, np.float32), np.zeros(d, np.float32)
    assert d == 16
    b[[0, 5, 10, d - 1]] = 1
    return a, b


def check_exact_ties(B, d):
    a, b = tie_rows(d)
    assert a[d - 1] == 1 and b[d - 1] == 1 and float(R.cosine_ref(a, b)) == 0.5 and float(R.cosine_ref(a, a)) == 1.0
    up = lambda v, to: float(np.nextafter(np.float32(v), np.float32(to)))      # noqa: E731
    for E, thr, keep in ((np.stack([a, a]), 1.0, False), (np.stack([a, a]), up(1, 2), True),
                         (np.stack([a, b]), 0.5, False), (np.stack([a, b]), up(0.5, 1), True),
                         (np.stack([b, a]), 0.5, False), (np.stack([b, a]), up(0.5, 1), True)):
        got = B.dedup_state(d).keep_mask(E, thr)
        assert list(got) == [True, keep], (d, thr, list(got))
        cfg = {"enable_similarity_filtering": True, "similarity_threshold": thr, "min_frame_distance": 1, "similarity_window_size": 2}
        E3 = np.concatenate([E, E[:1]])
        wmask, _ = R.keep_window_ref(E3, thr, 2)
        assert wmask[1] == keep
        assert B.filter_advanced(E3, [0, 1, 2], cfg) == np.flatnonzero(wmask).tolist(), (d, thr)


# ---------------------------------------------------------------------------------------------------------------------------------
# the in-scene filters
# ---------------------------------------------------------------------------------------------------------------------------------
def scene_walk(seed, n, d, thr, min_distance=1, window=None):
    """A drifting scene (cosines of neighbours around the threshold) whose decisions are all clear of it; seeds seed .. seed + 49."""
    for s in range(seed, seed + 50):
        rng = np.random.default_rng(s)
        step = np.sqrt(2 * (1 - thr)) * 0.6
        e = [rng.standard_normal(d)]
        for _ in range(1, n):
            v = e[-1] / np.linalg.norm(e[-1]) + step * rng.uniform(0.2, 1.8) * rng.standard_normal(d) / np.sqrt(d)
            e.append(v * rng.uniform(0.5, 2.0))
        E = np.asarray(e, np.float32)
        if window is None:
            mask, cmp, _ = R.keep_chain_ref(E, thr, min_distance)
        else:
            mask, cmp = R.keep_window_ref(E, thr, window)
        if cmp.clear_of(thr):
            return E, mask, cmp
    raise AssertionError(f"n={n} d={d}: no seed keeps every decision clear of the threshold")


def _cfg(thr, dist=1, window=5):
    return {"enable_similarity_filtering": True, "similarity_threshold": thr, "min_frame_distance": dist, "similarity_window_size": window}


def check_scene_filter(B, d, n):
    kept_counts = []
    for dist in SCENE_DIST:
        for thr in (0.95, 0.8):
            E, mask, cmp = scene_walk(100 * dist + n, n, d, thr, dist)
            gap, need = cmp.margin(thr)
            assert gap > need
            idx = list(range(100, 100 + n))
            want = sorted(set(np.flatnonzero(mask).tolist()) | {n - 1})              # filter.py: the scene's last frame always stays
            got = B.filter_in_scene(E, idx, _cfg(thr, dist))
            assert got == [idx[i] for i in want], (d, n, dist, thr, got, want)
            kept_counts.append(int(mask.sum()))
    if n == 50:
        assert max(kept_counts) > 5 and min(kept_counts) < 45, kept_counts
    return kept_counts


def check_window_filter(B, n, d, window):
    thr = 0.9
    E, mask, cmp = scene_walk(n + d + window, n, d, thr, window=window)
    gap, need = cmp.margin(thr)
    assert gap > need
    idx = list(range(100, 100 + n))
    got = B.filter_advanced(E, idx, _cfg(thr, window=window))
    assert got == [idx[i] for i in np.flatnonzero(mask)], (n, d, window)
    assert mask[0] and (n <= 3 or 1 < mask.sum() < n), (n, d, window, int(mask.sum()))
    # zero rows inside the window: sim = 0 to everything, so they are kept at thr > 0 and block nobody
    Z = E.copy()
    Z[1::4] = 0
    zmask, zcmp = R.keep_window_ref(Z, thr, window)
    assert zcmp.clear_of(thr)
    assert B.filter_advanced(Z, idx, _cfg(thr, window=window)) == [idx[i] for i in np.flatnonzero(zmask)]
    assert zmask[1::4].all()
    return int(mask.sum())


def check_window_dropped_blocker(B):
    """Frame 2 resembles only frame 1, frame 1 was dropped for resembling frame 0: frame 2 stays (only KEPT frames block).  With
    window = 1 frame 0 is out of reach of frame 2 as well; with window = 2 it is in reach and does not resemble it."""
    for d in (1025, 2048, 65):
        u = np.zeros((3, d), np.float32)
        for k in range(3):
            u[k, support(d, 48)[k::3]] = 1
        E = np.stack([u[0], u[0] + np.float32(0.7) * u[1], np.float32(0.45) * u[0] + u[1], u[2], u[2] + np.float32(0.3) * u[1]]).astype(np.float32)
        thr = 0.8
        for window in (1, 2, 5):
            mask, cmp = R.keep_window_ref(E, thr, window)
            assert cmp.clear_of(thr)
            assert list(mask) == [True, False, True, True, False], (window, list(mask))
            assert float(R.cosine_ref(E[2], E[1])) > thr > float(R.cosine_ref(E[2], E[0]))
            assert B.filter_advanced(E, list(range(5)), _cfg(thr, window=window)) == [0, 2, 3], (d, window)


# ---------------------------------------------------------------------------------------------------------------------------------
# row normalisation
# ---------------------------------------------------------------------------------------------------------------------------------
def check_normalize_bound(B, d):
    worst = 0.0
    for n in NORMALIZE_N:
        rng = np.random.default_rng(10 * d + n)
        x = (rng.standard_normal((n, d)) * rng.uniform(0.01, 100.0, (n, 1))).astype(np.float32)
        out = B.normalize(x)
        assert out.dtype == np.float32 and out.shape == x.shape
        worst = max(worst, _ratio(np.abs(out.astype(np.float64) - R.l2_normalize_ref(x)), R.l2_normalize_bound(x)))
        nz = x.any(axis=1)
        nrm = np.sqrt((out.astype(np.float64) ** 2).sum(axis=1))
        assert np.abs(nrm[nz] - 1).max(initial=0.0) <= R.unit_norm_bound(d), (d, n)
    return worst


def check_normalize_special(B):
    rng = np.random.default_rng(8)
    for d in (1, 3, 65, 512):
        x = rng.standard_normal((6, d)).astype(np.float32)
        x[1] = 0.0
        x[4] = -0.0
        x[5, ::2] = 0.0
        x[5, 1::2] = -0.0
        out = B.normalize(x)
        assert np.array_equal(bits(out[[1, 4, 5]]), bits(x[[1, 4, 5]])), d                  # zero rows keep their sign bits
        _ratio(np.abs(out.astype(np.float64) - R.l2_normalize_ref(x)), R.l2_normalize_bound(x))
        sign = np.where(rng.random((1, d)) < 0.5, -1.0, 1.0)
        row = (sign * rng.uniform(0.5, 1.0, (1, d))).astype(np.float32)                     # entries away from 0, norm of d = 1 below 1
        scaled = np.ldexp(np.repeat(row, 81, axis=0), np.arange(-40, 41)[:, None])
        got = B.normalize(scaled)
        assert np.all(bits(got) == bits(got)[40]), d


def check_nonfinite_count(B):
    rng = np.random.default_rng(9)
    n, d = 1027, 33
    x = rng.standard_normal((n, d)).astype(np.float32)
    clean = x.copy()
    x[2, [0, 32]] = np.nan                                          # two in one row
    x[5, 7] = np.inf                                                # one in another: 3 elements in 2 rows
    out, count = B.normalize(x, count=True)
    assert count == 3
    ok = np.isfinite(x).all(axis=1)
    _ratio(np.abs(out[ok].astype(np.float64) - R.l2_normalize_ref(clean[ok])), R.l2_normalize_bound(clean[ok]))
    assert np.array_equal(bits(out[ok]), bits(B.normalize(clean)[ok]))                      # the counter changes no output bit
    # one per row in rows that different waves and workgroups handle (4 rows per workgroup), the last row among them
    y = clean.copy()
    bad_rows = np.array([0, 1, 3, 4, 255, 256, 511, 1023, 1024, 1026])
    y[bad_rows, rng.integers(0, d, len(bad_rows))] = -np.inf
    y[1026, 0] = np.nan
    y[1026, 32] = np.nan
    want = int((~np.isfinite(y)).sum())
    out, count = B.normalize(y, count=True)
    assert count == want and want >= len(bad_rows) + 1
    ok = np.isfinite(y).all(axis=1)
    assert np.array_equal(bits(out[ok]), bits(B.normalize(clean)[ok]))
    out, count = B.normalize(clean, count=True)
    assert count == 0 and np.array_equal(bits(out), bits(B.normalize(clean)))


# ---------------------------------------------------------------------------------------------------------------------------------
# segment mean
# ---------------------------------------------------------------------------------------------------------------------------------
def segment_rows(d, sizes=SEGMENT_SIZES, seed=0):
    rng = np.random.default_rng(31 * d + seed)
    n = int(sum(sizes))
    rows = (rng.standard_normal((n, d)) + 0.25 * rng.standard_normal(d)).astype(np.float32)
    return rows, np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def _check_segments(out, rows, off, normalize):
    ref, bound = R.segment_mean_ref_bound(rows, off, normalize)
    empty = np.isnan(ref[:, 0])
    assert out.dtype == np.float32 and out.shape == ref.shape
    assert np.isnan(out[empty]).all() and not np.isnan(out[~empty]).any(), "NaN rows exactly where a segment is empty"
    return _ratio(np.abs(out[~empty].astype(np.float64) - ref[~empty]), bound[~empty])


def check_segment_mean(B, d):
    worst = 0.0
    rows, off = segment_rows(d)
    sizes = np.diff(off)
    for normalize in (False, True):
        out = B.segment_mean(rows, off, normalize)
        worst = max(worst, _check_segments(out, rows, off, normalize))
        if not normalize:
            one = int(np.flatnonzero(sizes == 1)[0])
            assert np.array_equal(bits(out[one]), bits(rows[off[one]])), "a one-row segment is that row"
        # the same rows as one segment (nseg = 1), and every segment on its own: no neighbour is disturbed
        whole = B.segment_mean(rows, np.array([0, len(rows)], np.int64), normalize)
        worst = max(worst, _check_segments(whole, rows, np.array([0, len(rows)]), normalize))
        for s in (1, 3, 6):
            alone = B.segment_mean(rows, off[s:s + 2], normalize)
            assert np.array_equal(bits(alone[0]), bits(out[s])), (d, s)
    return worst


def check_segment_offsets(B):
    """seg_off below 0 and above n is clipped to [0, n]."""
    rows, _ = segment_rows(257, (40,))
    n = len(rows)
    off = np.array([-5, 7, 7, 25, n + 9, n + 20], np.int64)
    clipped = np.array([0, 7, 7, 25, n, n], np.int64)
    worst = 0.0
    for normalize in (False, True):
        out = B.segment_mean(rows, off, normalize)
        assert np.array_equal(bits(out), bits(B.segment_mean(rows, clipped, normalize)))
        worst = max(worst, _check_segments(out, rows, clipped, normalize))
        assert np.isnan(out[[1, 4]]).all()
        # every offset out of range: all segments empty but the one that spans everything
        out = B.segment_mean(rows, np.array([-9, -3, n + 1, n + 2], np.int64), normalize)
        assert np.isnan(out[[0, 2]]).all()
        worst = max(worst, _check_segments(out[1:2], rows, np.array([0, n]), normalize))
    return worst


def check_segment_zero_mean(B):
    rng = np.random.default_rng(12)
    for d in (1, 257, 1000):
        x = rng.standard_normal((3, d)).astype(np.float32)
        rows = np.concatenate([x[:1], x, -x, x[:2]])                     # segment 1 = x and -x: mean exactly zero
        off = np.array([0, 1, 7, 9], np.int64)
        for normalize in (False, True):
            out = B.segment_mean(rows, off, normalize)
            assert np.array_equal(bits(out[1]), np.zeros(d, np.uint32)), (d, normalize)      # +0.0 everywhere, not NaN
            _check_segments(out, rows, off, normalize)


def check_segment_double_sum(B):
    """2^24 followed by 999 ones: a float32 running sum stays at 2^24 (mean 16777.216), the double sum gives (2^24 + 999) / 1000."""
    for d in (3, 300):
        rows = np.ones((1000, d), np.float32)
        rows[0, d - 1] = 2.0 ** 24
        out = B.segment_mean(rows, np.array([0, 1000], np.int64), False)
        want = np.ones(d, np.float32)
        want[d - 1] = np.float32((2.0 ** 24 + 999) / 1000)
        assert np.array_equal(bits(out[0]), bits(want)), (d, out[0, d - 1], want[d - 1])
        _check_segments(out, rows, np.array([0, 1000]), False)
        _check_segments(B.segment_mean(rows, np.array([0, 1000], np.int64), True), rows, np.array([0, 1000]), True)


def check_segment_means_wrapper(B):
    """_kmeans.segment_means: a column slice of a wider matrix, order given and omitted, an unsorted assignment."""
    rng = np.random.default_rng(13)
    n, k = 700, 9
    base = rng.standard_normal((n, 40)).astype(np.float32)
    a = rng.integers(0, k - 1, n).astype(np.int64)
    a[a == 3] = 4                                                       # clusters 3 and k - 1 are empty
    assert (np.diff(a) < 0).any()
    order = np.argsort(a, kind="stable")
    counts = np.bincount(a, minlength=k)
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    worst = 0.0
    for c0, c1 in ((8, 16), (0, 40), (39, 40), (3, 20)):
        rows = np.ascontiguousarray(base[:, c0:c1][order])
        for spherical in (False, True):
            direct = B.segment_mean(rows, off, spherical)
            worst = max(worst, _check_segments(direct, rows, off, spherical))
            for use_order in (False, True):
                out, cnt = B.segment_means(base, c0, c1, a, k, spherical, order if use_order else None)
                assert np.array_equal(cnt, counts) and cnt.dtype == np.int64
                assert np.array_equal(bits(out), bits(direct)), (c0, c1, spherical, use_order)
    return worst


def kmeans_rows(n, d, seed=21):
    """Unit-norm rows around 2 * nlist-ish loose centres: no cluster of the first k-means step comes out empty."""
    rng = np.random.default_rng(seed + d)
    centres = rng.standard_normal((24, d))
    x = centres[rng.integers(0, 24, n)] + 1.5 * rng.standard_normal((n, d))
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


def check_kmeans_step(xs, cent0, D, I, trained, spherical, min_count):
    """One k-means step: xs the sampled rows, cent0 the centroids before it, (D, I) the library's own nearest-centroid search of xs,
    trained the centroids after the step.  The assignment is the library's, checked to be a best one within the index's stated
    error; the centroids must then be the segment means of exactly that assignment."""
    nlist, d = cent0.shape
    s64 = xs.astype(np.float64) @ cent0.astype(np.float64).T
    a = I[:, 0].astype(np.int64)
    assert a.min() >= 0 and a.max() < nlist
    tol = R.flat_score_bound(d, np.sqrt((cent0.astype(np.float64) ** 2).sum(axis=1))[a])
    chosen = s64[np.arange(len(xs)), a]
    assert (np.abs(D[:, 0].astype(np.float64) - chosen) <= tol).all()
    assert (chosen >= s64.max(axis=1) - tol).all()
    counts = np.bincount(a, minlength=nlist)
    assert counts.min() >= max(1, min_count), counts                             # nothing empty: the repair path stays out of it
    order = np.argsort(a, kind="stable")
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    return _check_segments(trained, np.ascontiguousarray(xs[order]), off, spherical)


# ---------------------------------------------------------------------------------------------------------------------------------
# the GPU backend
# ---------------------------------------------------------------------------------------------------------------------------------
class _GpuDedup:
    def __init__(self, d):
        from ivr_amd.dedup import DedupState
        self.st = DedupState(d)

    def keep_mask(self, E, thr):
        import torch
        return self.st.keep_mask(torch.from_numpy(np.ascontiguousarray(E)).cuda(), thr).cpu().numpy().astype(bool)

    def bits(self):
        return self.st.state.cpu().numpy().view(np.uint32)

    def poke0(self, v):
        self.st.state[0] = v

    def reset(self):
        self.st.reset()


class Gpu:
    """The entry points of ivr_amd as the checks call them."""
    dedup_state = staticmethod(_GpuDedup)

    @staticmethod
    def rowwise_cosine(a, b):
        from ivr_amd.filters import rowwise_cosine
        return rowwise_cosine(a, b).cpu().numpy()

    @staticmethod
    def calculate_similarities(E):
        from ivr_amd.filters import calculate_similarities
        return np.asarray(calculate_similarities(E), dtype=np.float32)

    @staticmethod
    def filter_in_scene(E, idx, cfg):
        from ivr_amd.filters import filter_similar_frames_in_scene
        return filter_similar_frames_in_scene(E, idx, cfg)

    @staticmethod
    def filter_advanced(E, idx, cfg):
        from ivr_amd.filters import filter_similar_frames_advanced
        return filter_similar_frames_advanced(E, idx, cfg)

    @staticmethod
    def normalize(x, count=False):
        import torch
        from ivr_amd.index import count_nonfinite_and_normalize, normalize_L2
        t = torch.from_numpy(x.copy()).cuda()
        if count:
            c = count_nonfinite_and_normalize(t)
            return t.cpu().numpy(), c
        normalize_L2(t)
        return t.cpu().numpy()

    @staticmethod
    def segment_mean(rows, seg_off, normalize):
        import torch
        from ivr_amd import _ffi
        r = torch.from_numpy(np.ascontiguousarray(rows)).cuda()
        off = torch.from_numpy(np.ascontiguousarray(seg_off, dtype=np.int64)).cuda()
        nseg = len(seg_off) - 1
        out = torch.full((nseg + 1, rows.shape[1]), 7.0, dtype=torch.float32, device="cuda")
        _ffi.call("ivr_segment_mean", _ffi.CTX, r, len(rows), off, nseg, rows.shape[1], bool(normalize), out, device=r.device)
        out = out.cpu().numpy()
        assert (out[nseg] == 7.0).all(), "a write past the last segment's row"
        return out[:nseg]

    @staticmethod
    def segment_means(base, c0, c1, a, k, spherical, order):
        import torch
        from ivr_amd import _kmeans
        x = torch.from_numpy(base).cuda()[:, c0:c1]
        assert c1 - c0 == base.shape[1] or not x.is_contiguous()
        out = torch.empty((k, c1 - c0), dtype=torch.float32, device="cuda")
        cnt = _kmeans.segment_means(x, torch.from_numpy(a).cuda(), k, out, spherical,
                                    order=None if order is None else torch.from_numpy(order).cuda())
        return out.cpu().numpy(), cnt.cpu().numpy()
