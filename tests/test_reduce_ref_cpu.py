"""CPU suite: the float64 references and derived bounds of oracle/reduce_ref.py are neither too loose nor too tight.  A numpy float32
emulation of the reducing kernels as written (csrc/dedup.hip, l2_normalize_kernel, segment_mean_kernel) runs every check the GPU
suites make (tests/reduce_cases.py, at the same shapes) and passes; the same emulation with one typical kernel fault fails at least
one of them.  The largest error / bound ratio per kernel is printed (pytest -s shows it).

The emulation follows the kernels operation by operation: lane l of the wave runs an fma chain over the columns l, l + 64, ...,
ivr_wave_sum adds lane pairs (l, l ^ 1), (l, l ^ 2), ... (its six levels pair equal partial sums, so the order inside a pair does
not matter); sqrtf, the product of the norms and the quotient are single float32 operations.  An fma is the exact float64 product
plus the accumulator rounded to float64 and then to float32: the double rounding differs from a hardware fma by one ulp in about one
operation in 2^29, which no check here can see except as an error far inside its bound."""
import numpy as np
import pytest

import reduce_cases as C

F32 = np.float32
FAULTS = ("drop_last_col", "tail_read", "seg_drop_last_row", "seg_start_next", "seg_f32_sum", "clamp_norm", "gt_threshold",
          "prev_chunk_end", "dist_no_r0", "state_always", "band_shift")


def _wave_sum(v):
    """ivr_wave_sum of float32 [n, 64] lane values -> float32 [n]."""
    for _ in range(6):
        v = v[:, 0::2] + v[:, 1::2]
    return v[:, 0]


class Emu:
    def __init__(self, fault=None):
        assert fault is None or fault in FAULTS
        self.fault = fault

    # -- the wave's view of a row -------------------------------------------------------------------------------------------
    def _regs(self, X):
        """Rows as the lanes hold them: float32 [n, 64 * ceil(d / 64)] and which columns enter a sum.  A correct kernel zeroes the
        columns from d on; with tail_read the last register holds whatever follows the row in memory (the next row; ones after
        the last), with drop_last_col the loop stops one column early."""
        n, d = X.shape
        w = -(-d // 64) * 64
        if self.fault == "tail_read":
            flat = np.concatenate([X.ravel(), np.ones(w, F32)])
            R = np.stack([flat[i * d:i * d + w] for i in range(n)]) if n else np.zeros((0, w), F32)
            valid = np.ones(w, bool)
        else:
            R = np.zeros((n, w), F32)
            R[:, :d] = X
            valid = np.arange(w) < (d - 1 if self.fault == "drop_last_col" else d)
        return R, valid

    @staticmethod
    def _dot(Ra, Rb, valid):
        """The fma chains and the wave tree: float32 [n]."""
        acc = np.zeros((Ra.shape[0], 64), F32)
        for j in range(Ra.shape[1] // 64):
            s = slice(64 * j, 64 * j + 64)
            new = (Ra[:, s].astype(np.float64) * Rb[:, s].astype(np.float64) + acc.astype(np.float64)).astype(F32)
            acc = np.where(valid[s], new, acc)
        return _wave_sum(acc)

    def _norm(self, ss):
        with np.errstate(invalid="ignore"):
            if self.fault == "clamp_norm":
                return np.maximum(np.sqrt(ss), F32(1e-12)).astype(F32)
            return np.where(ss > 0, np.sqrt(ss), F32(1)).astype(F32)

    def _cos(self, Ra, Rb, valid):
        dot, sa, sb = self._dot(Ra, Rb, valid), self._dot(Ra, Ra, valid), self._dot(Rb, Rb, valid)
        return (dot / (self._norm(sa) * self._norm(sb))).astype(F32)

    # -- rowwise_cosine_kernel ----------------------------------------------------------------------------------------------
    def rowwise_cosine(self, a, b):
        (Ra, valid), (Rb, _) = self._regs(a), self._regs(b)
        return self._cos(Ra, Rb, valid)

    def calculate_similarities(self, E):
        return self.rowwise_cosine(E[:-1], E[1:]) if len(E) > 1 else np.zeros(0, F32)

    # -- dedup_kernel -------------------------------------------------------------------------------------------------------
    def _chain(self, E, thr, state, min_distance):
        """dedup_kernel<PER>: chunks of rc rows, the last kept frame in registers, `state` (float32 [d + 1] or None) read at the
        start and written at the end."""
        n, d = E.shape
        thr = F32(thr)
        rc = max(1, 8192 // d)
        R, valid = self._regs(E)
        SS = self._dot(R, R, valid)
        keep = np.zeros(n, bool)
        has_prev = state is not None and state[0] != 0
        prev = np.zeros((1, R.shape[1]), F32)
        prev_ss = F32(0)
        if has_prev:
            prev[0, :d] = state[1:]
            prev_ss = self._dot(prev, prev, valid)[0]
        last_kept = -1
        for r0 in range(0, n, rc):
            rows = min(rc, n - r0)
            for r in range(rows):
                i = r0 + r
                uniq = True
                if has_prev:
                    dot = self._dot(R[i:i + 1], prev, valid)[0]
                    sim = F32(dot / F32(self._norm(SS[i]) * self._norm(prev_ss)))
                    if (sim > thr) if self.fault == "gt_threshold" else (sim >= thr):
                        uniq = False
                    pos = r if self.fault == "dist_no_r0" else i
                    if min_distance > 1 and last_kept >= 0 and pos - last_kept < min_distance:
                        uniq = False
                if uniq:
                    has_prev = True
                    prev_ss = SS[i]
                    last_kept = i
                    if not (self.fault == "prev_chunk_end" and r == rc - 1):
                        prev = R[i:i + 1].copy()
                keep[i] = uniq
        if state is not None and (last_kept >= 0 or self.fault == "state_always"):
            state[1:] = prev[0, :d]
            state[0] = 1
        return keep

    def dedup_state(self, d):
        emu = self

        class State:
            def __init__(self):
                self.s = np.zeros(d + 1, F32)

            def keep_mask(self, E, thr):
                assert E.shape[1] == d and E.dtype == F32
                return emu._chain(E, thr, self.s, 1) if len(E) else np.zeros(0, bool)       # n = 0: no launch

            def bits(self):
                return self.s.view(np.uint32)

            def poke0(self, v):
                self.s[0] = v

            def reset(self):
                self.s[:] = 0
        return State()

    def filter_in_scene(self, E, idx, cfg):
        n = len(E)
        if not cfg["enable_similarity_filtering"] or n <= 1:
            return idx
        kept = np.flatnonzero(self._chain(E, cfg["similarity_threshold"], None, max(1, int(cfg["min_frame_distance"])))).tolist()
        if kept[-1] != n - 1:
            kept.append(n - 1)
        return [idx[j] for j in kept]

    # -- band_cosine_kernel + window_chain_kernel ---------------------------------------------------------------------------
    def filter_advanced(self, E, idx, cfg):
        n = len(E)
        if not cfg["enable_similarity_filtering"] or n <= 1:
            return idx
        thr, window = F32(cfg["similarity_threshold"]), min(max(1, int(cfg["similarity_window_size"])), n)
        R, valid = self._regs(E)
        band = np.zeros(n * window + 1, F32)                           # pairs with i - t < 0 are never written (nor read)
        for t in range(1, window + 1):
            if t < n:
                band[np.arange(t, n) * window + t - 1] = self._cos(R[t:], R[:-t], valid)
        keep = np.zeros(n, bool)
        shift = 1 if self.fault == "band_shift" else 0
        for i in range(n):
            k = True
            for t in range(1, min(window, i) + 1):
                if keep[i - t] and band[i * window + t - 1 + shift] >= thr:
                    k = False
                    break
            keep[i] = k
        return [idx[j] for j in np.flatnonzero(keep)]

    # -- l2_normalize_kernel ------------------------------------------------------------------------------------------------
    def normalize(self, x, count=False):
        R, valid = self._regs(x)
        with np.errstate(invalid="ignore", over="ignore"):
            out = (x / self._norm(self._dot(R, R, valid))[:, None]).astype(F32)
        return (out, int((~np.isfinite(x)).sum())) if count else out

    # -- segment_mean_kernel ------------------------------------------------------------------------------------------------
    def segment_mean(self, rows, seg_off, normalize):
        n, d = rows.shape
        nseg = len(seg_off) - 1
        out = np.empty((nseg, d), F32)
        acc = F32 if self.fault == "seg_f32_sum" else np.float64
        for s in range(nseg):
            s0 = min(max(int(seg_off[s + 1 if self.fault == "seg_start_next" else s]), 0), n)
            s1 = min(max(int(seg_off[s + 1]), s0), n)
            if s1 <= s0:
                out[s] = np.nan
                continue
            inv = 1.0 / float(s1 - s0)
            body = rows[s0:s1 - 1 if self.fault == "seg_drop_last_row" else s1]
            total = np.cumsum(body.astype(acc), axis=0)[-1].astype(np.float64) if len(body) else np.zeros(d)   # ascending row order
            mean = (total * inv).astype(F32)
            if normalize:
                sq = np.zeros(-(-d // 256) * 256)
                sq[:d] = mean.astype(np.float64) ** 2
                red = np.cumsum(sq.reshape(-1, 256), axis=0)[-1]                   # thread t: its columns t, t + 256, ... in order
                o2 = 128
                while o2:
                    red = red[:o2] + red[o2:2 * o2]
                    o2 >>= 1
                nrm = F32(np.sqrt(red[0])) if red[0] > 0 else F32(1)
                mean = (mean / nrm).astype(F32)
            out[s] = mean
        return out

    def segment_means(self, base, c0, c1, a, k, spherical, order):
        x = base[:, c0:c1]
        rows = np.ascontiguousarray(x[np.argsort(a, kind="stable") if order is None else order])
        counts = np.bincount(a, minlength=k).astype(np.int64)
        off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        return self.segment_mean(rows, off, spherical), counts

    # -- one k-means step (the search is float64 on the host: only the centroid update is emulated) -------------------------
    def kmeans_step(self, x, nlist, spherical):
        perm = np.random.RandomState(1234).permutation(len(x))[:min(len(x), 256 * nlist)]
        xs = x[perm]
        cent0 = self.normalize(xs[:nlist]) if spherical else xs[:nlist].copy()
        s = xs.astype(np.float64) @ cent0.astype(np.float64).T
        I = s.argmax(axis=1)[:, None]
        D = s.max(axis=1).astype(F32)[:, None]
        trained, _ = self.segment_means(xs, 0, xs.shape[1], I[:, 0], nlist, spherical, None)
        return xs, cent0, D, I, trained


# -- every check of the GPU suites, by kernel ---------------------------------------------------------------------------------------
def _kmeans(B, case, spherical):
    n, d, nlist = case
    xs, cent0, D, I, trained = B.kmeans_step(C.kmeans_rows(n, d), nlist, spherical)
    return C.check_kmeans_step(xs, cent0, D, I, trained, spherical, 1)


CHECKS = {
    "cosine": [(C.check_cosine_bound, d) for d in C.COSINE_D] + [(C.check_cosine_exact, 1025), (C.check_cosine_exact, 2048),
                                                                 (C.check_cosine_special,), (C.check_calculate_similarities,)],
    "dedup": [(C.check_random_walk, d, thr) for d, thr in C.WALK_CASES] + [(C.check_small_chain_splits,), (C.check_carried_state,),
                                                                           (C.check_zero_rows,)] + [(C.check_exact_ties, d) for d in C.TIE_D],
    "scene": [(C.check_scene_filter, d, n) for d, n in C.SCENE_CASES],
    "window": [(C.check_window_filter, *c) for c in C.WINDOW_CASES] + [(C.check_window_dropped_blocker,)],
    "normalize": [(C.check_normalize_bound, d) for d in C.NORMALIZE_D] + [(C.check_normalize_special,), (C.check_nonfinite_count,)],
    "segment_mean": [(C.check_segment_mean, d) for d in C.SEGMENT_D] + [(C.check_segment_offsets,), (C.check_segment_zero_mean,),
                                                                        (C.check_segment_double_sum,), (C.check_segment_means_wrapper,)]
                    + [(_kmeans, c, s) for c in C.KMEANS_CASES for s in (True, False)],
}
# the checks each fault is expected to fail (a subset keeps the suite quick; any one failing is enough)
EXPECT = {
    "drop_last_col": [(C.check_cosine_exact, 1025), (C.check_exact_ties, 16), (C.check_normalize_bound, 65)],
    "tail_read": [(C.check_cosine_bound, 65), (C.check_normalize_bound, 33), (C.check_random_walk, 100, 0.95)],
    "seg_drop_last_row": [(C.check_segment_mean, 8), (_kmeans, C.KMEANS_CASES[0], True)],
    "seg_start_next": [(C.check_segment_mean, 8), (C.check_segment_offsets,)],
    "seg_f32_sum": [(C.check_segment_double_sum,)],
    "clamp_norm": [(C.check_cosine_special,), (C.check_normalize_special,)],
    "gt_threshold": [(C.check_exact_ties, 16), (C.check_exact_ties, 2048), (C.check_zero_rows,)],
    "prev_chunk_end": [(C.check_small_chain_splits,), (C.check_random_walk, 2048, 0.98)],
    "dist_no_r0": [(C.check_scene_filter, 2048, 50), (C.check_scene_filter, 1000, 50)],
    "state_always": [(C.check_carried_state,)],
    "band_shift": [(C.check_window_filter, 65, 63, 64), (C.check_window_filter, 130, 1025, 7), (C.check_window_dropped_blocker,)],
}


def _name(check):
    return f"{check[0].__name__.replace('check_', '')}{check[1:]}"


@pytest.mark.parametrize("kernel", list(CHECKS))
def test_correct_emulation_passes_every_gpu_check(kernel):
    B = Emu()
    worst = 0.0
    for check in CHECKS[kernel]:
        r = check[0](B, *check[1:])
        if isinstance(r, float):
            worst = max(worst, r)
    print(f"\n{kernel}: largest error / bound of the correct emulation = {worst:.3f}")
    assert worst <= 1.0


def test_the_bounds_are_not_loose():
    """The correct emulation comes close to the bounds it is held to.  The cosine bound is a worst case over three float32 sums whose
    roundings mostly cancel on random rows, so the emulation uses a tenth of it; the other two are within a factor of two or three."""
    B = Emu()
    assert max(C.check_cosine_bound(B, d) for d in (3, 65, 384)) > 0.1
    assert max(C.check_normalize_bound(B, d) for d in (3, 65, 512)) > 0.3
    assert C.check_segment_mean(B, 257) > 0.5


@pytest.mark.parametrize("fault", FAULTS)
def test_faulty_emulation_fails_a_gpu_check(fault):
    B = Emu(fault)
    failed = []
    for check in EXPECT[fault]:
        try:
            check[0](B, *check[1:])
        except AssertionError:
            failed.append(_name(check))
    print(f"\n{fault}: caught by {failed}")
    assert failed, f"{fault} passes {[_name(c) for c in EXPECT[fault]]}"


def test_reference_conventions():
    from oracle import reduce_ref as R
    z, x = np.zeros((1, 5), F32), np.arange(5, dtype=F32)[None]
    assert R.cosine_ref(z, x)[0] == 0 and R.cosine_bound(z, x)[0] == 0 and R.cosine_ref(x, x)[0] == 1
    assert not R.l2_normalize_ref(z).any() and R.m(64) == 7 and R.m(65) == 8 and R.m(2048) == 38
    rows = np.array([[1, 2], [3, 4], [5, 9]], F32)
    ref = R.segment_mean_ref(rows, [-3, 2, 2, 7], False)
    assert np.array_equal(ref[0], [2, 3]) and np.isnan(ref[1]).all() and np.array_equal(ref[2], [5, 9])
    assert not R.segment_mean_ref(np.array([[1, -2], [-1, 2]], F32), [0, 2], True).any()
    with pytest.raises(TypeError):
        R.cosine_ref(x.astype(np.float64), x)
    E = np.array([[1, 0], [1, 0.01], [0, 1], [0, 1]], F32)
    mask, cmp, last = R.keep_chain_ref(E, 0.9)
    assert list(mask) == [True, False, True, False] and last == 2 and len(cmp.sim) == 3 and cmp.clear_of(0.9)
    mask, cmp, last = R.keep_chain_ref(E, 0.9, min_distance=3)
    assert list(mask) == [True, False, False, True] and len(cmp.sim) == 1
    mask, cmp, last = R.keep_chain_ref(E[:2], 0.9, prev=E[0])
    assert not mask.any() and last is None and cmp.j == [-1, -1]
    mask, cmp = R.keep_window_ref(E, 0.9, 1)
    assert list(mask) == [True, False, True, False]
