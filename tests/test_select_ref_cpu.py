"""CPU side of the top-k selector tests: the reference select_ref against the project's other merges, the CPU model select_path
against the constants of csrc/search_select.h, and the proof that the case table (tests/select_cases.py) that
test_select_paths_gpu.py runs reaches every branch of select_topk_kernel."""
import collections
import os
import re

import numpy as np
import pytest
import torch

import select_cases as T
from oracle import search_ref as S

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "intelligent-video-analysis-retrieval-system_amd", "csrc",
                      "search_select.h")


def _ascending(I_parts):
    """The launch's ids replaced by ids that ascend with the candidate position (absent stays -1): where id order = position order
    the id-ordered merges must agree with the position-ordered reference."""
    parts, nq, k = I_parts.shape
    p = (np.arange(parts)[:, None, None] * k + np.arange(k)[None, None, :]) * 3 + (1 << 33)
    return np.where(I_parts >= 0, np.broadcast_to(p, I_parts.shape), -1).astype(np.int64)


def _same(Da, Ia, Db, Ib):
    assert np.array_equal(Ia, Ib)
    assert np.array_equal(Da, Db)                       # by value: -0.0 == +0.0, and there is no NaN


@pytest.mark.parametrize("la", T.LAUNCHES + T.sweep_launches(40), ids=repr)
def test_select_ref_equals_merge_shards_and_merge_host(la):
    from ivr_amd.sharded import merge_host
    D_parts, I_parts = la.arrays()
    I_asc = _ascending(I_parts)
    Dr, Ir = S.select_ref(D_parts, I_asc, la.k)
    _same(Dr, Ir, *S.merge_shards(D_parts, I_asc, la.k))
    Dh, Ih = merge_host(torch.from_numpy(D_parts.copy()), torch.from_numpy(I_asc), la.k)
    _same(Dr, Ir, Dh.numpy(), Ih.numpy())
    # the reference on the launch's own ids: the same candidates, by position
    D2, I2 = S.select_ref(D_parts, I_parts, la.k)
    flat = I_parts.transpose(1, 0, 2).reshape(la.nq, -1)
    pos = np.where(Ir >= 0, (Ir - (1 << 33)) // 3, 0)
    assert np.array_equal(np.where(Ir >= 0, np.take_along_axis(flat, pos, 1), -1), I2)
    assert np.array_equal(Dr.view(np.uint32), D2.view(np.uint32))


def test_select_ref_equals_float64_argsort_without_ties():
    rng = np.random.default_rng(5)
    parts, nq, k = 37, 4, 23
    D_parts = rng.standard_normal((parts, nq, k)).astype(np.float32)
    I_parts = rng.permutation(parts * nq * k).reshape(parts, nq, k).astype(np.int64)
    D, I = S.select_ref(D_parts, I_parts, k)
    for q in range(nq):
        d, i = D_parts[:, q].reshape(-1), I_parts[:, q].reshape(-1)
        assert len(np.unique(d)) == len(d)
        order = np.argsort(-d.astype(np.float64))[:k]
        assert np.array_equal(I[q], i[order]) and np.array_equal(D[q], d[order])


def test_select_ref_conventions():
    """-0.0 ties with +0.0 and the position decides; -FLT_MAX with a valid id keeps its id and is not an unused slot; an absent
    slot's score never counts; unused slots are (-FLT_MAX, -1)."""
    D_parts = np.array([[[-0.0, -np.inf, 5.0]], [[0.0, S.NEG_FLT_MAX, 7.0]]], dtype=np.float32)       # [2 parts, 1 query, 3]
    I_parts = np.array([[[40, 30, -1]], [[10, 20, -1]]], dtype=np.int64)
    D, I = S.select_ref(D_parts, I_parts, 5)
    assert I.tolist() == [[40, 10, 20, 30, -1]]
    assert D[0, :2].tolist() == [0.0, 0.0] and np.signbit(D[0, 0]) and not np.signbit(D[0, 1])
    assert D[0, 2] == S.NEG_FLT_MAX and D[0, 3] == -np.inf and D[0, 4] == S.NEG_FLT_MAX


def test_select_ord_is_monotone_and_folds_the_zeros():
    v = np.sort(np.unique(np.concatenate([T.SPECIAL, np.random.default_rng(1).standard_normal(500).astype(np.float32)])))
    o = S.select_ord(v).astype(np.int64)
    strictly = np.diff(v.astype(np.float64)) > 0                                  # the two zeros compare equal
    assert (np.diff(o)[strictly] > 0).all() and (np.diff(o)[~strictly] == 0).all() and (o != 0).all()
    assert S.select_ord(np.float32(-0.0)) == S.select_ord(np.float32(0.0))
    assert S.select_ord(np.float32(1e-40)) < S.select_ord(np.float32(2e-40))


def test_model_constants_match_the_kernel():
    """Drift guard: the five constants select_path copies from search_select.h."""
    src = open(HEADER).read()

    def one(pattern):
        m = re.findall(pattern, src)
        assert len(m) == 1, f"search_select.h: expected exactly one match of {pattern!r}, found {len(m)}: the selector's dispatch " \
                            "changed - update oracle/search_ref.py select_path together with the kernel"
        return m[0]

    got = {
        "SEL_THREADS": int(one(r"constexpr int kSelThreads = (\d+);")),
        "SEL_REG_KEYS": int(one(r"constexpr int kRegKeys = (\d+);")),
        "SEL_FAST_ROUNDS": int(one(r"keff >= 1 && rounds <= (\d+)\)")),
        "SEL_EXTRACT_KEFF": int(one(r"cached && keff <= (\d+)\)")),
    }
    a, b, c = (int(x) for x in one(r"int sel_threads\(int64_t n\) \{ return n <= (\d+) \* (\d+) \? (\d+) : kSelThreads; \}"))
    got["SEL_SHORT_THREADS"] = c
    want = {name: getattr(S, name) for name in got}
    assert got == want and a * b == S.SEL_REG_KEYS * S.SEL_SHORT_THREADS, \
        f"search_select.h has {got} (short lists: n <= {a} * {b}), select_path has {want}: update oracle/search_ref.py select_path " \
        "together with the kernel"
    assert (S.SEL_THREADS, S.SEL_REG_KEYS, S.SEL_SHORT_THREADS, S.SEL_FAST_ROUNDS, S.SEL_EXTRACT_KEFF) == (1024, 16, 256, 16, 64)


def test_select_path_on_hand_made_lists():
    ones = np.ones(4096, dtype=bool)
    s = np.random.default_rng(2).standard_normal(4096).astype(np.float32)
    assert S.select_path(s, ones, 64) == ("fast", 256, True)
    assert S.select_path(s, ones, 65) == ("radix/bigk", 256, True)
    assert S.select_path(s[:30], ones[:30], 10) == ("extract/short", 256, True)          # waves 1 .. 3 hold no key
    assert S.select_path(s, ~ones, 10) == ("extract/empty", 256, True)
    assert S.select_path(np.ones(4097, np.float32), np.ones(4097, bool), 16) == ("extract/ties", 1024, True)
    assert S.select_path(np.ones(16385, np.float32), np.ones(16385, bool), 16) == ("radix/ties", 1024, False)
    assert S.select_path(np.ones(16385, np.float32), np.ones(16385, bool), 17) == ("radix/short", 1024, False)   # 2 rounds, 1 level


def test_case_table_reaches_every_class():
    """A condition on the inputs of test_select_paths_gpu.py: every query takes the branch the table declares for it, and each
    of the 17 reachable classes (3 fast + 6 extract + 3 radix/bigk + 3 more radix without cached keys + 2 more radix with 1024
    threads and cached keys) is taken by at least two queries."""
    hits = collections.Counter()
    for la in T.LAUNCHES:
        assert la.n == la.parts * la.k and 1 <= la.nq <= 7 and la.k <= 2048
        for q, (kind, arg, want) in enumerate(la.queries):
            got = S.select_path(*la.query_keys(q), la.k)
            hits[got] += 1
            assert got[1:] == want[1:], (la, q, got, want)
            if want[0] is not None:
                assert got == want, (la, q, got, want)
    assert len(T.REACHABLE) == 17 and len(set(T.REACHABLE)) == 17
    assert set(hits) <= set(T.REACHABLE), set(hits) - set(T.REACHABLE)
    short = {c: hits[c] for c in T.REACHABLE if hits[c] < 2}
    assert not short, f"classes reached by fewer than two queries: {short}"
    print(sorted(hits.items()))


def test_sweep_is_seeded_and_within_bounds():
    a, b = T.sweep_launches(), T.sweep_launches()
    assert len(a) == 200 and [x.name for x in a] == [x.name for x in b]
    assert all(x.n <= 24000 and x.k <= 2048 and 1 <= x.nq <= 3 for x in a)
    classes = {S.select_path(*x.query_keys(0), x.k) for x in a}
    assert len(classes) >= 12, classes                    # the sweep is broad, the table is what guarantees coverage


def test_score_value_cases_carry_every_special_value_into_the_result():
    """Again a condition on the inputs: in each block-size class some expected result holds every value of SPECIAL under a valid
    id (-FLT_MAX with its id, not as an unused slot) followed by unused slots, and -0.0 next to +0.0."""
    seen = collections.defaultdict(set)
    for la in T.LAUNCHES:
        if la.queries[0][0] != "special":
            continue
        D, I = S.select_ref(*la.arrays(), la.k)
        for q in range(la.nq):
            bits = set(D[q][I[q] >= 0].view(np.uint32).tolist())
            if set(T.SPECIAL.view(np.uint32).tolist()) <= bits and (I[q] < 0).any():
                seen[la.queries[q][2][1:]].add(la.name)
    assert set(seen) == {T.C256, T.C1K, T.U1K}, dict(seen)
