"""What keeps tests/test_scan_bound_gpu.py honest, checked on the numpy model of tests/bound_cases.py alone (no GPU): every case's
float64 top-k is the intended rows by a margin float32 scoring cannot cross, the modelled approximate ranking loses exactly those rows,
the hidden row's true error is 0.95 .. 1.0 of the analytic bound of its path, and the decoys' approximate scores are exact.  The GPU
file compares for equality only, so it asks nothing looser than what is established here.

Margins.  A relative margin of 2^-13 is out of reach for these cases: a decoy must clear approx(H) + 0.95 E while exact(H) is only
0.97 .. 0.98 E above approx(H), which leaves at most 0.03 * 2^-8 = 2^-13.1 of the score (2^-14.4 at d = 512; 31 elements at 1 + 2^-7
against H at d = 64 is 6.8e-3 / 64.25 = 2^-13.2).  What the margin is for is a firm order under float32 scoring, so that is what is
asserted: the gap between the k-th and the (k+1)-th float64 score exceeds the sum of the two rows' sequential-accumulation bounds
(d + 8) 2^-24 sum|q_i x_i|, where a row whose partial sums are all float32 numbers (the bf16-exact decoys) has bound 0."""
import numpy as np
import pytest
import torch

import bound_cases as B

ADVERSARIAL = [n for n in B.CASE_NAMES if n.startswith(("sharp", "tied")) or n == "qrem"]
SAFE = [n for n in B.CASE_NAMES if n.startswith("safe")]


def _path(path):
    return (B.selected_small, B.approx_small, B.e_small, 64) if path == "small" else (B.selected_big, B.approx_big, B.e_big, 16)


def _rescored_kth(case, sel, rows_per):
    """the k-th float64 score among the rows of the re-scored groups / tiles: what the device check compares against"""
    X, q, k = case["X"], case["q"], case["k"]
    rows = np.concatenate([np.arange(g * rows_per, min((g + 1) * rows_per, len(X))) for g in sel])
    return np.sort(B.exact_scores(X[rows], q[None, :])[0])[::-1][k - 1]


def test_bf16_model_rounds_to_nearest_even():
    one = np.float32(1)
    vals = np.array([B.H_ELEM, B.UP_ELEM, 1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 3.4e38, -3.4e38, 0.0, 1 - 2.0 ** -9 - 2.0 ** -17], np.float32)
    want = np.array([one, 1 + 2.0 ** -7, 1.0, 1 + 2.0 ** -6, np.inf, -np.inf, 0.0, 1 - 2.0 ** -8], np.float32)
    assert np.array_equal(B.bf16_round(vals), want)
    x = (np.random.default_rng(0).standard_normal(100_000) * 10.0 ** np.random.default_rng(1).integers(-30, 30, 100_000)).astype(np.float32)
    assert np.array_equal(B.bf16_round(x), torch.from_numpy(x).to(torch.bfloat16).to(torch.float32).numpy())
    hi, lo = B.split_q(x)
    assert np.abs(x.astype(np.float64) - hi - lo).max() <= 2.0 ** -16 * np.abs(x).max()


@pytest.mark.parametrize("d", B.DIMS)
@pytest.mark.parametrize("name", [n for n in B.CASE_NAMES if n != "nonfinite"])
def test_layout_and_float64_topk(name, d):
    c = B.make(name, d)
    X, q, k, kp, N = c["X"], c["q"], c["k"], c["kp"], c["N"]
    assert N % 64 != 0 and N % 16 != 0
    assert (N + 63) // 64 >= 4 * (kp + 1)                        # ivr_index::fast_scan: the candidate scan engages
    special = np.concatenate([c["hidden"], c["top"], c["low"]])
    assert len(np.unique(special // 128)) == len(special)         # one per 128-row block: one per group and per tile too
    assert (special // 128).max() < N // 128                      # whole blocks only
    if name != "prune":
        assert len(c["top"]) + len(c["low"]) == B.N_DECOYS and len(c["hidden"]) == k
    s = B.exact_scores(X, q[None, :])[0]
    order = np.lexsort((np.arange(N), -s))
    assert np.array_equal(order[:k], c["winners"]) and np.array_equal(B.topk_f64(X, q[None, :], k)[0], c["winners"])
    a, b = order[k - 1], order[k]
    margin, need = s[a] - s[b], B.f32_sum_bound(X[a], q) + B.f32_sum_bound(X[b], q)
    print(f"{name} d={d}: margin {margin:.3e} = 2^{np.log2(margin / s[a]):.1f} relative, float32 bounds {need:.3e}")
    assert margin > need
    # the fillers are far below: nothing but the special rows competes
    fill = np.setdiff1d(np.arange(N), special)
    assert s[fill].max() < 0.1 * s[special].min()


@pytest.mark.parametrize("d", B.DIMS)
@pytest.mark.parametrize("name", [n for n in B.CASE_NAMES if n != "nonfinite"])
def test_decoys_are_bf16_exact(name, d):
    c = B.make(name, d)
    X, q = c["X"], c["q"]
    dec = np.concatenate([c["top"], c["low"]]) if name != "prune" else np.zeros(0, np.int64)
    assert np.array_equal(B.bf16_round(X[dec]), X[dec])
    s = B.exact_scores(X, q[None, :])[0]
    for path in c["paths"]:
        ap = _path(path)[1](X, q[None, :])[0]
        assert np.array_equal(ap[dec], s[dec])
        assert B.f32_sum_bound(X[dec[0]], q) == 0 if len(dec) else True


@pytest.mark.parametrize("d", B.DIMS)
@pytest.mark.parametrize("name", ADVERSARIAL)
def test_hidden_rows_are_lost_at_the_edge_of_the_bound(name, d):
    c = B.make(name, d)
    X, k, kp = c["X"], c["k"], c["kp"]
    for scale in B.SCALES:
        q = c["q"] * np.float32(scale)
        s = B.exact_scores(X, q[None, :])[0]
        for path in c["paths"]:
            select, approx, bound, rows_per = _path(path)
            sel, excl, m = select(X, q, kp)
            E = bound(X, q[None, :], d)[0]
            ap = approx(X, q[None, :])[0]
            assert not np.isin(c["hidden"] // rows_per, sel).any()            # outside the kp re-scored groups / tiles
            assert np.array_equal(np.sort(sel), np.sort(c["top"][:kp] // rows_per) if name.startswith("tied") else np.sort(c["top"] // rows_per))
            err = s[c["hidden"]] - ap[c["hidden"]]
            print(f"{name} d={d} {path} x{scale}: true error / E = {err.min() / E:.4f}")
            assert 0.95 * E <= err.min() and err.max() <= E
            kth = _rescored_kth(dict(c, q=q), sel, rows_per)
            assert kth < s[c["hidden"]].min()                                  # accepting the fast result returns a decoy
            assert m[excl] + E >= kth                                          # so every valid e makes the check fire
            if name.startswith("tied"):
                assert m[excl] == kth                                          # ... here even e = 0, by the strict inequality
            else:
                assert m[excl] + 0.95 * E < kth                                # ... and an e 5 % short does not


@pytest.mark.parametrize("d", B.DIMS)
@pytest.mark.parametrize("name", SAFE)
def test_safe_variant_clears_the_bound_by_a_quarter(name, d):
    c = B.make(name, d)
    X, q, k, kp = c["X"], c["q"], c["k"], c["kp"]
    s = B.exact_scores(X, q[None, :])[0]
    assert s[c["top"]].min() > s[c["hidden"]].max()                            # the decoys beat H's exact score too
    for path in c["paths"]:
        select, approx, bound, rows_per = _path(path)
        sel, excl, m = select(X, q, kp)
        E = bound(X, q[None, :], d)[0]
        ap = approx(X, q[None, :])[0]
        assert np.isin(c["winners"] // rows_per, sel[:k]).all()
        kth = _rescored_kth(c, sel, rows_per)
        assert kth == s[c["winners"]].min()
        print(f"{name} d={d} {path}: (k-th exact - first excluded) / E = {(kth - m[excl]) / E:.3f}")
        assert m[excl] + 1.25 * E <= kth
        assert ap[c["hidden"]].max() + 1.25 * E <= s[c["top"]].min()
        assert ap[c["hidden"]].max() <= m[excl]


@pytest.mark.parametrize("d", B.DIMS)
def test_qrem_is_harmless_with_hi_plus_lo_but_cannot_be_verified(d):
    """At most 64 queries: q_hi + q_lo carries the query's remainder, so W's group has the best approximate maximum and is re-scored.
    The check still cannot pass on these rows: the first excluded group holds a top decoy within E_small of W."""
    c = B.make("qrem", d)
    X, q, kp = c["X"], c["q"], c["kp"]
    sel, excl, m = B.selected_small(X, q, kp)
    assert sel[0] == c["hidden"][0] // 64
    assert m[excl] + B.e_small(X, q[None, :], d)[0] >= _rescored_kth(c, sel, 64)


@pytest.mark.parametrize("d", B.DIMS)
def test_prune_case_sits_just_inside_twice_the_bound(d):
    c = B.make("prune", d)
    X, q, kp = c["X"], c["q"], c["kp"]
    P, H = int(c["top"][0]), int(c["hidden"][0])
    s, ap = B.exact_scores(X, q[None, :])[0], B.approx_big(X, q[None, :])[0]
    E = B.e_big(X, q[None, :], d)[0]
    sel, excl, tm = B.selected_big(X, q, kp)
    assert sel[0] == P // 16 and sel[1] == H // 16                             # H's tile is selected, past position k = 1
    gap = tm[P // 16] - tm[H // 16]
    print(f"prune d={d}: approximate gap / 2 E = {gap / (2 * E):.4f}, H error / E = {(s[H] - ap[H]) / E:.4f}")
    assert 0.95 * 2 * E <= gap < 2 * E                                         # inside 2 E (kept), far outside 1 E (dropped by a 1 e rule)
    assert 0.95 * E <= s[H] - ap[H] <= E
    assert ap[P] > s[P] and s[H] > s[P]
    # with H's tile dropped the verification passes, so the wrong row would be returned, not redone: nothing masks the fault
    assert tm[excl] + 1.25 * E < s[P]


@pytest.mark.parametrize("d", B.DIMS)
def test_range_radii_split_the_hidden_row_from_the_decoys(d):
    c = B.make("sharp_k1", d)
    X, q = c["X"], c["q"]
    H = int(c["hidden"][0])
    gm = B.group_max(B.approx_small(X, q[None, :]), 64)[0]
    E = B.e_small(X, q[None, :], d)[0]
    (r1, ids1), (r2, ids2), (r3, ids3) = B.range_radii(c)
    assert np.array_equal(ids1, [H])
    assert np.array_equal(ids2, np.sort(np.concatenate([c["top"], c["hidden"]])))
    assert np.array_equal(ids3, np.sort(np.concatenate([c["top"], c["low"], c["hidden"]])))
    assert gm[H // 64] + 0.95 * E < r1 <= gm[H // 64] + E                      # H's group survives only with (nearly) the whole bound
    s = B.exact_scores(X, q[None, :])[0]
    special = np.concatenate([c["top"], c["low"], c["hidden"]])
    for r in (r1, r2, r3):                                                     # no float32 score can land on the other side of a radius
        assert all(abs(s[i] - r) > B.f32_sum_bound(X[i], q) for i in special)
        assert np.abs(np.delete(s, special)).max() < 0.1 * r


@pytest.mark.parametrize("d", B.DIMS)
def test_filler_rows_alone_leave_the_bound_many_times_too_small(d):
    """The row-writing test starts from the fillers: a path that does not raise maxnorm / maxdelta leaves e at their level."""
    c = B.make("sharp_k1", d)
    q = c["q"][None, :]
    assert B.e_small(c["F"], q, d)[0] < 0.2 * B.e_small(c["X"], q, d)[0]
    assert B.e_big(c["F"], q, d)[0] < 0.2 * B.e_big(c["X"], q, d)[0]


@pytest.mark.parametrize("d", B.DIMS)
def test_nonfinite_case_has_no_bound(d):
    c = B.make("nonfinite", d)
    X, N, kp = c["X"], c["N"], c["kp"]
    assert (N + 63) // 64 >= 4 * (kp + 1)
    assert np.isinf(B.bf16_round(X[c["hidden"]])).sum() == len(c["hidden"]) and np.isfinite(X).all()
    for nq in (10, 65):
        Q, _ = B.queries(c, nq)
        assert (Q[:, list(B.NONFINITE_ZERO_COORDS)] == 0).all()
        assert np.isnan(B.approx_small(X, Q)[:, c["hidden"]]).all() and np.isnan(B.approx_big(X, Q)[:, c["hidden"]]).all()
        assert np.isfinite(B.exact_scores(X, Q)).all() and np.abs(Q @ X[c["top"]].T).max() > 1e28
        # no usable bound on either path: E_big is infinite (dr is), E_small exceeds every score by orders of magnitude (and is
        # infinite once |row| is taken in float32), so no check can pass
        assert not np.isfinite(B.e_big(X, Q, d)).any()
        assert (B.e_small(X, Q, d) > 1e3 * np.abs(B.exact_scores(X, Q)).max(axis=1)).all()


def test_query_batches():
    c = B.make("sharp_k1", 64)
    for nq in B.SMALL_NQ:
        Q, adv = B.queries(c, nq)
        assert Q.shape == (nq, 64) and adv.all()
    for nq in B.BIG_NQ:
        Q, adv = B.queries(c, nq)
        assert 0 < adv.sum() < nq and all(np.array_equal(Q[i], c["q"] * np.float32(B.SCALES[i % 3])) for i in np.nonzero(adv)[0])
        assert B.queries(c, nq, fillers=False)[1].all()
