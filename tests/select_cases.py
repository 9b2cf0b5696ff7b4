"""The case table of the top-k selector tests (select_topk_kernel, csrc/search_select.h), shared by test_select_ref_cpu.py (which
proves with the CPU model oracle.search_ref.select_path that every branch of the kernel is reached) and test_select_paths_gpu.py
(which runs every case through both merge entry points).  A plain module, not a conftest: it only builds inputs.

A LAUNCH is one call of topk_merge: `parts` candidate lists of `k` entries for each of its queries, so the kernel sees
n = parts * k keys per query and one block per query.  Every query of a launch names how its keys are made and the class
(path, block threads, keys cached) the model must give it; queries of different classes share launches on purpose."""
import functools
import zlib

import numpy as np

FLT_MAX = np.float32(3.4028234663852886e38)
TIE = np.float32(9.0)                  # the tied score of the bulk-tie cases, above every background score
ABSENT_SCORE = np.float32(1e30)        # what an absent slot (id -1) carries as its score: must never show in a result
# +-inf, +-FLT_MAX, the two zeros (they tie), denormals with their order (1e-40 < 2e-40), ordinary values
SPECIAL = np.array([np.inf, -np.inf, FLT_MAX, -FLT_MAX, 0.0, -0.0, 1e-40, 2e-40, -1e-40, -2e-40, 1.0, -1.0, 0.5, 3.25, -7.5, 1e-3],
                   dtype=np.float32)

C256, C1K, U1K = (256, True), (1024, True), (1024, False)      # (block threads, keys cached)


def _scores(rng, n, kind, arg):
    """(scores float32 [n], valid bool [n]) of one query."""
    valid = np.ones(n, dtype=bool)
    if kind == "gauss":
        s = rng.standard_normal(n)
    elif kind == "valid":                    # arg keys valid, at random positions: absent slots interleaved with valid ones
        s = rng.standard_normal(n)
        valid[:] = False
        valid[rng.choice(n, arg, replace=False)] = True
    elif kind == "ties_at":                  # arg random positions hold the tied score
        s = rng.standard_normal(n)
        s[rng.choice(n, arg, replace=False)] = TIE
    elif kind == "ties_first":               # positions 0 .. arg-1 hold it, one per thread before wrapping; uniform background
        s = rng.uniform(-0.999, 0.999, n)
        s[:arg] = TIE
    elif kind == "equal":
        s = np.full(n, 1.5)
    elif kind == "empty":
        s = rng.standard_normal(n)
        valid[:] = False
    elif kind == "levels":                   # arg = (distinct score levels, valid fraction)
        levels, frac = arg
        s = rng.standard_normal(levels)[rng.integers(0, levels, n)]
        valid = rng.random(n) < frac
    elif kind == "special":                  # arg = (fraction of the keys drawn from SPECIAL, the rest ordinary; valid fraction)
        frac, vfrac = arg
        s = rng.standard_normal(n).astype(np.float32)
        pick = rng.random(n) < frac
        s[pick] = SPECIAL[rng.integers(0, len(SPECIAL), int(pick.sum()))]
        valid = rng.random(n) < vfrac
    elif kind == "denorm":                   # multiples of the smallest denormal in +-2000 steps, both zeros among them
        m = rng.integers(-2000, 2001, n)
        s = m.astype(np.float32) * np.float32(1.4e-45)
        s[(m == 0) & (rng.random(n) < 0.5)] = np.float32(-0.0)
        valid = rng.random(n) < 0.95
    else:
        raise ValueError(kind)
    s = np.asarray(s, dtype=np.float32)
    return np.where(valid, s, ABSENT_SCORE), valid


def _ids(rng, n, scheme):
    """int64 ids of the n candidate positions.  pos: the position itself (a valid id 0); big: ascending above 2^32; perm: a
    permutation above 2^32, NOT monotone in the position, so the result must carry I_parts[p] and not p."""
    p = np.arange(n, dtype=np.int64)
    if scheme == "pos":
        return p
    if scheme == "big":
        return (1 << 33) + 7 * p
    if scheme == "perm":
        return (1 << 40) + rng.permutation(n).astype(np.int64)
    raise ValueError(scheme)


class Launch:
    def __init__(self, name, parts, k, ids, queries):
        self.name, self.parts, self.k, self.ids, self.queries = name, parts, k, ids, queries
        self.n, self.nq = parts * k, len(queries)

    def __repr__(self):
        return self.name

    @functools.lru_cache(maxsize=None)
    def arrays(self):
        """(D_parts float32 [parts,nq,k], I_parts int64 [parts,nq,k]), seeded by the launch's name; never modified."""
        rng = np.random.default_rng(zlib.crc32(self.name.encode()))
        D = np.empty((self.nq, self.n), dtype=np.float32)
        I = np.empty((self.nq, self.n), dtype=np.int64)
        for q, (kind, arg, _) in enumerate(self.queries):
            s, valid = _scores(rng, self.n, kind, arg)
            D[q] = s
            I[q] = np.where(valid, _ids(rng, self.n, self.ids), -1)
        D = np.ascontiguousarray(D.reshape(self.nq, self.parts, self.k).transpose(1, 0, 2))
        I = np.ascontiguousarray(I.reshape(self.nq, self.parts, self.k).transpose(1, 0, 2))
        D.setflags(write=False)
        I.setflags(write=False)
        return D, I

    def query_keys(self, q):
        """(scores [n], valid [n]) of query q in candidate order, as select_path takes them."""
        D, I = self.arrays()
        return D[:, q, :].reshape(-1), I[:, q, :].reshape(-1) >= 0


def _L(parts, k, ids, *queries):
    name = f"{parts}x{k}-{ids}-" + "+".join(f"{kind}{'' if arg is None else arg}".replace(" ", "") for kind, arg, _ in queries)
    return Launch(name, parts, k, ids, queries)


def _q(kind, arg, path, cls):
    return (kind, arg, (path,) + cls)


# every query: (how its keys are made, argument, the class select_path must report)
LAUNCHES = [
    # ---- survivor path
    _L(8, 64, "big", _q("gauss", None, "fast", C256)),
    _L(64, 64, "perm", _q("gauss", None, "fast", C256), _q("gauss", None, "fast", C256)),          # keff 64 at n = 4096 ...
    _L(63, 65, "big", _q("gauss", None, "radix/bigk", C256)),                                       # ... against keff 65 at n = 4095
    _L(409, 10, "big", _q("gauss", None, "fast", C256)),                                            # n = 4090 ...
    _L(410, 10, "perm",                                                                             # ... against n = 4100
       _q("gauss", None, "fast", C1K), _q("valid", 5, "extract/short", C1K), _q("equal", None, "extract/ties", C1K),
       _q("empty", None, "extract/empty", C1K), _q("valid", 12, "extract/short", C1K), _q("gauss", None, "fast", C1K)),
    _L(64, 256, "big", _q("gauss", None, "fast", C1K), _q("empty", None, "extract/empty", C1K)),    # keff 256 at n = 16384 ...
    _L(1638, 10, "big", _q("gauss", None, "fast", C1K)),                                            # n = 16380 ...
    _L(1639, 10, "perm", _q("gauss", None, "fast", U1K)),                                           # ... against n = 16390
    _L(65, 256, "big", _q("gauss", None, "fast", U1K)),                                             # keff 256 at n = 16640 ...
    _L(64, 260, "big",                                                                              # ... against keff 257 there
       _q("valid", 257, "radix/bigk", U1K), _q("valid", 256, "radix/short", U1K)),
    # ---- a wave runs out of keys
    _L(3, 10, "big", _q("gauss", None, "extract/short", C256), _q("empty", None, "extract/empty", C256)),
    _L(1, 1, "pos", _q("gauss", None, "extract/short", C256)),
    _L(30, 100, "perm", _q("valid", 64, "extract/short", C256)),
    _L(8, 2048, "big",
       _q("valid", 100, "radix/short", C1K), _q("gauss", None, "radix/bigk", C1K), _q("valid", 256, "radix/short", C1K),
       _q("valid", 257, "radix/bigk", C1K)),                                                        # ... against keff 257 at n = 16384
    _L(200, 100, "perm", _q("valid", 70, "radix/short", U1K)),
    _L(9, 2048, "big",
       _q("valid", 3, "radix/short", U1K), _q("gauss", None, "radix/bigk", U1K), _q("empty", None, "radix/empty", U1K)),
    # ---- bulk ties
    _L(400, 10, "big", _q("ties_at", 600, "extract/ties", C256),
       _q("equal", None, "extract/short", C256)),              # all equal: every wave is empty after one round
    _L(100, 100, "perm", _q("ties_at", 1100, "radix/ties", C1K), _q("levels", (50, 1.0), "radix/ties", C1K),
       _q("ties_at", 600, "fast", C1K)),                       # 600 ties and the few keys above T still fit the 1024 survivor slots
    _L(1700, 10, "big",
       _q("equal", None, "radix/ties", U1K), _q("empty", None, "radix/empty", U1K), _q("gauss", None, "fast", U1K),
       _q("levels", (3, 0.7), "radix/ties", U1K)),
    # ---- large k
    _L(4, 65, "perm", _q("gauss", None, "radix/bigk", C256)),
    _L(16, 256, "big", _q("gauss", None, "radix/bigk", C256), _q("empty", None, "extract/empty", C256)),
    _L(2, 2048, "big", _q("gauss", None, "radix/bigk", C256)),
    _L(20, 257, "big", _q("gauss", None, "radix/bigk", C1K)),
    _L(40, 500, "perm", _q("gauss", None, "radix/bigk", U1K)),
    # ---- blockDim against blockDim + 1 survivors: k <= waves so one round, exactly m keys at 9.0 in threads 0 .. m-1 (mod blockDim)
    _L(512, 4, "pos", _q("ties_first", 256, "fast", C256), _q("ties_first", 257, "extract/ties", C256)),
    _L(512, 16, "pos", _q("ties_first", 1024, "fast", C1K), _q("ties_first", 1025, "extract/ties", C1K)),
    _L(1280, 16, "pos", _q("ties_first", 1024, "fast", U1K), _q("ties_first", 1025, "radix/ties", U1K)),
    # ---- score values, per block-size class; the path is whatever the draw gives (None: not declared).  Fewer valid keys than k:
    # the result is the whole sorted list, every special value in it; small k: the specials and denormals on the other paths
    _L(2, 128, "big", _q("special", (1.0, 0.45), None, C256), _q("special", (0.3, 0.45), None, C256), _q("special", (1.0, 0.9), None, C256)),
    _L(3, 2048, "perm", _q("special", (1.0, 0.3), None, C1K), _q("special", (0.3, 0.3), None, C1K)),
    _L(9, 2048, "big", _q("special", (1.0, 0.1), None, U1K), _q("special", (0.3, 0.1), None, U1K)),
    _L(64, 8, "big", _q("special", (1.0, 0.9), None, C256), _q("special", (0.05, 0.9), None, C256), _q("denorm", None, None, C256)),
    _L(512, 10, "perm", _q("special", (1.0, 0.9), None, C1K), _q("special", (0.05, 0.9), None, C1K), _q("denorm", None, None, C1K)),
    _L(1650, 10, "big", _q("special", (1.0, 0.9), None, U1K), _q("special", (0.05, 0.9), None, U1K), _q("denorm", None, None, U1K)),
]

# The 17 classes that can be reached at all; each must be hit by at least two queries of LAUNCHES.  Not reachable: extraction
# without cached keys; extract/bigk (more than 16 rounds means keff > 64); radix/short and radix/ties with 256 threads (they need
# 64 < keff <= 16 * 4); radix/empty with cached keys (keff = 0 <= 64 extracts nothing).
REACHABLE = ([("fast",) + c for c in (C256, C1K, U1K)]
             + [("extract/" + w,) + c for w in ("short", "ties", "empty") for c in (C256, C1K)]
             + [("radix/bigk",) + c for c in (C256, C1K, U1K)]
             + [("radix/" + w,) + U1K for w in ("short", "ties", "empty")]
             + [("radix/" + w,) + C1K for w in ("short", "ties")])


def sweep_launches(count=200, seed=20240607):
    """The seeded random sweep: (parts, k, valid fraction, distinct score levels) with parts * k <= 24000."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(count):
        k = int(rng.choice([1, 2, 5, 10, 16, 17, 50, 64, 65, 100, 256, 257, 700, 2048]))
        n_max = int(rng.choice([300, 4096, 4200, 16384, 16500, 24000]))
        parts = int(rng.integers(1, max(1, n_max // k) + 1))
        frac = float(rng.choice([1.0, 0.9, 0.3, 0.01]))
        levels = int(rng.choice([1, 3, 50, 0]))                                   # 0: all distinct
        kind = ("valid", max(1, int(frac * parts * k))) if levels == 0 else ("levels", (levels, frac))
        ids = ("pos", "big", "perm")[i % 3]
        la = Launch(f"sweep{i}-{parts}x{k}-{ids}-{kind[0]}{kind[1]}".replace(" ", ""), parts, k, ids,
                    [(kind[0], kind[1], None)] * int(rng.integers(1, 4)))
        out.append(la)
    return out
