"""CPU check of oracle/gemm_ref.py: a numpy emulation of a correct tower GEMM (one fp32 accumulator over 32-wide bf16, 4-wide f32 or
128-wide e4m3 K chunks in ascending order, the fast activation formulas of act_fn<true> in float32, round to nearest even) stays inside
the per-element bound with margin and reaches a stated fraction of it on bf16 output; every typical kernel fault leaves it."""
import numpy as np
import pytest
import torch

from oracle import gemm_ref as G

CHUNK = {"bf16": 32, "f32": 4, "e4m3": 128}
# A correct kernel's bf16 output reaches at least this fraction of the bound: the output rounding term 2^-8 |ref| is the unit roundoff,
# which round to nearest even attains (half an ulp) just above a power of two; every other term is a small worst case on top.
BF16_FRACTION = 0.9


def f32(a):
    return np.asarray(a, np.float32)


def to_bf16(a, trunc=False):
    """float32 -> bf16 value (as float32): round to nearest even, or truncation (a fault)."""
    b = f32(a).view(np.uint32).astype(np.uint64)
    if not trunc:
        b = b + 0x7FFF + ((b >> 16) & 1)
    return ((b >> 16) << 16).astype(np.uint32).view(np.float32)


def to_e4m3(a):
    return torch.from_numpy(f32(np.clip(a, -448, 448))).to(torch.float8_e4m3fn).to(torch.float32).numpy()


def act_fast(v, act):
    """act_fn<true> / act4_fast of tower_kernels.hip in float32."""
    v = f32(v)
    with np.errstate(over="ignore"):
        if act == G.QUICK:
            e = np.exp2(v * np.float32(-2.4554669595930157))
            return f32(v * f32(np.float32(1) / f32(np.float32(1) + e)))
        z = f32(np.abs(v) * np.float32(0.70710678118654752))
        t = f32(np.float32(1) / f32(np.float32(0.3275911) * z + np.float32(1)))
        p = f32(np.float32(1.061405429) * t - np.float32(1.453152027))
        p = f32(p * t + np.float32(1.421413741))
        p = f32(p * t - np.float32(0.284496736))
        p = f32(p * t + np.float32(0.254829592))
        e = np.exp2(f32(f32(-z * z) * np.float32(1.4426950408889634)))
        ea = f32(np.float32(1) - f32(p * t) * e)
        return f32(np.float32(0.5) * v * f32(np.float32(1) + np.copysign(ea, v)))


def accumulate(x, w, dtype, drop_last=False):
    """One fp32 accumulator per output, K chunks in ascending order, each chunk's products summed exactly and added with one rounding
    (bf16 / e4m3 products are exact in fp32; f32 products are rounded first)."""
    M, K = x.shape
    c = CHUNK[dtype]
    acc = np.zeros((M, w.shape[0]), np.float32)
    for k0 in range(0, K - c if drop_last else K, c):
        xs, ws = x[:, k0:k0 + c].astype(np.float64), w[:, k0:k0 + c].astype(np.float64)
        if dtype == "f32":
            prod = f32(xs[:, None, :] * ws[None, :, :]).astype(np.float64)
            part = prod.sum(-1)
        else:
            part = xs @ ws.T
        acc = f32(acc.astype(np.float64) + part)
    return acc


def emulate(before, x, w, *, dtype, out_kind, epi, act=-1, bias=None, colscale=None, pos=None, T=0, G2=0, skip_mod=0, fault=None):
    """The kernel's write into the output buffer `before` (numpy, float32 values; returns a new array).  `fault` injects one bug."""
    M, N = x.shape[0], w.shape[0]
    acc = accumulate(x, w, dtype, drop_last=fault == "drop_last_chunk")
    if colscale is not None:
        s = colscale.copy()
        if fault == "colscale_neighbour":
            s[:-1] = s[1:]
        acc = f32(acc * s)
    out = before.copy()
    b = np.zeros(N, np.float32) if bias is None else bias
    if epi in (G.STORE, G.F32):
        if fault == "bias_after_rounding":
            v = f32(to_bf16(acc) + b)
        else:
            v = f32(acc + b)
        if act >= 0:
            v = act_fast(to_bf16(v) if fault == "act_on_rounded" else v, act) if out_kind != "f32" else v
        if out_kind == "bf16":
            v = to_bf16(v, trunc=fault == "truncate")
        elif out_kind == "e4m3":
            v = to_e4m3(v)
        if fault == "transpose_fragment":
            v[16:32, 32:48] = v[16:32, 32:48].T.copy()
        if fault == "tail_shift":
            v[:, N - 4:] = v[:, N - 8:N - 4]
        out[:M, :N] = v
        return out
    v = f32(acc + b)
    if epi == G.RESID:
        rows = np.arange(M)
        if skip_mod:
            skip = (rows % skip_mod == (1 if fault == "skip_wrong_row" else 0)) if fault != "skip_ignored" else np.zeros(M, bool)
        else:
            skip = np.zeros(M, bool)
        base = np.zeros_like(v) if fault == "resid_overwrite" else out[:M, :N]
        new = f32(base + v)
        out[:M, :N] = np.where(skip[:, None], out[:M, :N], new)
        return out
    m = np.arange(M)
    p = m % G2
    img = m // G2
    if fault == "image_off_by_one":
        for edge in (128, 256):                       # the image that straddles a tile edge: rows past the edge take img + 1
            if edge < M and edge % G2:
                straddle = (m >= edge) & (img == edge // G2)
                img = np.where(straddle, img + 1, img)
    prow = pos[p] if fault == "pos_off_by_one" else pos[1 + p]
    dst = img * T + 1 + p
    keep = dst < out.shape[0]
    out[dst[keep], :N] = f32(prow + v)[keep]
    if fault == "token0_written":
        out[img * T, :N] = f32(prow + v)
    return out


def check(after, before, x8, w8, dtype, out_kind, epi, **kw):
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)) if a is not None else None   # noqa: E731
    exp = G.expect(t(before), t(x8), t(w8), dtype=dtype, out_kind=out_kind, epi=epi, N=w8.shape[0], K=x8.shape[1],
                   **{k: t(v) if isinstance(v, np.ndarray) else v for k, v in kw.items()})
    return G.verify(t(after), t(before), exp)


def operands(rng, M, N, K, dtype, tail=False, bias_scale=1.0):
    """Gaussian operands exact in the operand dtype; bias of the size of the products (so that bias and product cancel somewhere);
    tail=True adds rows whose pre-activations sit in [-12, -3] and near 0 (small products, the bias carries the value)."""
    x = f32(rng.standard_normal((M, K)))
    w = f32(rng.standard_normal((N, K)) * K ** -0.5)
    if dtype == "bf16":
        x, w = to_bf16(x), to_bf16(w)
    elif dtype == "e4m3":
        x, w = to_e4m3(x * 2), to_e4m3(w * 64)
    b = f32(rng.standard_normal(N) * bias_scale)
    if tail:
        x[: M // 2] = x[: M // 2] * np.float32(2.0 ** -6)
        if dtype == "bf16":
            x = to_bf16(x)
        elif dtype == "e4m3":
            x = to_e4m3(x)
        b = f32(np.where(np.arange(N) % 2 == 0, rng.uniform(-12, -3, N), rng.uniform(-0.05, 0.05, N)))
    return x, w, b


CASES = [("bf16", "bf16", -1), ("bf16", "bf16", G.QUICK), ("bf16", "bf16", G.GELU), ("f32", "f32", -1), ("e4m3", "bf16", -1),
         ("e4m3", "bf16", G.GELU), ("e4m3", "e4m3", -1), ("e4m3", "e4m3", G.QUICK)]


@pytest.mark.parametrize("dtype,out_kind,act", CASES)
@pytest.mark.parametrize("tail", [False, True])
def test_correct_kernel_passes_with_margin(dtype, out_kind, act, tail):
    rng = np.random.default_rng(CASES.index((dtype, out_kind, act)) * 2 + int(tail))
    M, N, K = 160, 132, 768
    x, w, b = operands(rng, M, N, K, dtype, tail)
    s = f32(rng.uniform(0.5, 2, N) / 64) if dtype == "e4m3" else None
    before = np.full((M, N + 4), np.nan, np.float32)
    after = emulate(before, x, w, dtype=dtype, out_kind=out_kind, epi=G.STORE, act=act, bias=b, colscale=s)
    ratio, changed = check(after, before, x, w, dtype, out_kind, G.STORE, act=act, bias=b, colscale=s)
    print(f"{dtype} -> {out_kind} act={act} tail={tail}: largest err / bound = {ratio:.3f}")
    assert changed == 0
    # margin: the terms in front of the output rounding are worst cases that a correct kernel stays far inside (float32 output: only
    # those terms); a rounded output can take the whole rounding term
    assert ratio <= (0.5 if out_kind == "f32" else 1.0), ratio
    if out_kind == "bf16" and not tail:
        assert ratio >= BF16_FRACTION, ratio          # not vacuous: the output rounding term is reached


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_correct_residual_and_patch_epilogues_pass(dtype):
    rng = np.random.default_rng(3)
    M, N, K, T = 300, 68, 192, 50
    x, w, b = operands(rng, M, N, K, dtype)
    before = f32(rng.standard_normal((M, N + 4)) * 8 + 100)       # residual rows of large mean
    after = emulate(before, x, w, dtype=dtype, out_kind="f32", epi=G.RESID, bias=b, skip_mod=T)
    ratio, changed = check(after, before, x, w, dtype, "f32", G.RESID, bias=b, skip_mod=T)
    assert changed == 0 and ratio <= 0.5, ratio
    G2 = 49
    M = 6 * G2
    x, w, b = operands(rng, M, N, K, dtype)
    pos = f32(rng.standard_normal((T, N)))
    before = np.full((6 * T, N), np.nan, np.float32)
    after = emulate(before, x, w, dtype=dtype, out_kind="f32", epi=G.PATCH, bias=b, pos=pos, T=T, G2=G2)
    ratio, changed = check(after, before, x, w, dtype, "f32", G.PATCH, bias=b, pos=pos, T=T, G2=G2)
    assert changed == 0 and ratio <= 0.5, ratio


STORE_FAULTS = [("truncate", "bf16", "bf16", -1, False), ("bias_after_rounding", "bf16", "bf16", -1, False),
                ("act_on_rounded", "bf16", "bf16", G.GELU, True), ("act_on_rounded", "bf16", "bf16", G.QUICK, True),
                ("drop_last_chunk", "bf16", "bf16", -1, False), ("drop_last_chunk", "f32", "f32", -1, False),
                ("drop_last_chunk", "e4m3", "bf16", -1, False), ("transpose_fragment", "bf16", "bf16", -1, False),
                ("transpose_fragment", "f32", "f32", -1, False), ("tail_shift", "bf16", "bf16", -1, False),
                ("tail_shift", "e4m3", "e4m3", -1, False), ("colscale_neighbour", "e4m3", "bf16", -1, False)]


@pytest.mark.parametrize("fault,dtype,out_kind,act,tail", STORE_FAULTS)
def test_store_fault_is_rejected(fault, dtype, out_kind, act, tail):
    rng = np.random.default_rng(11)
    M, N, K = 160, 68 if fault == "tail_shift" else 132, 768
    x, w, b = operands(rng, M, N, K, dtype, tail, bias_scale=4.0 if fault == "bias_after_rounding" else 1.0)
    s = f32(rng.uniform(0.5, 2, N) / 64) if dtype == "e4m3" else None
    before = np.full((M, N + 4), np.nan, np.float32)
    kw = dict(act=act, bias=b, colscale=s)
    good = emulate(before, x, w, dtype=dtype, out_kind=out_kind, epi=G.STORE, **kw)
    bad = emulate(before, x, w, dtype=dtype, out_kind=out_kind, epi=G.STORE, fault=fault, **kw)
    r_good, _ = check(good, before, x, w, dtype, out_kind, G.STORE, **kw)
    r_bad, changed = check(bad, before, x, w, dtype, out_kind, G.STORE, **kw)
    print(f"{fault} ({dtype} -> {out_kind}, act {act}): err / bound {r_good:.3f} correct, {r_bad:.3g} with the fault")
    assert r_good <= 1 and (r_bad > 1 or changed), (r_good, r_bad)


@pytest.mark.parametrize("fault", ["skip_ignored", "skip_wrong_row", "resid_overwrite"])
@pytest.mark.parametrize("dtype", ["bf16", "e4m3"])
def test_residual_fault_is_rejected(fault, dtype):
    rng = np.random.default_rng(12)
    M, N, K, T = 300, 128, 256, 50
    x, w, b = operands(rng, M, N, K, dtype)
    before = f32(rng.standard_normal((M, N + 4)) + 3)
    kw = dict(bias=b, skip_mod=T)
    bad = emulate(before, x, w, dtype=dtype, out_kind="f32", epi=G.RESID, fault=fault, **kw)
    r_bad, changed = check(bad, before, x, w, dtype, "f32", G.RESID, **kw)
    assert r_bad > 1 or changed, (r_bad, changed)


@pytest.mark.parametrize("fault,G2", [("pos_off_by_one", 49), ("image_off_by_one", 49), ("image_off_by_one", 196),
                                      ("token0_written", 49)])
@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_patch_fault_is_rejected(fault, G2, dtype):
    rng = np.random.default_rng(13)
    T, n, N, K = G2 + 1, 6 if G2 == 49 else 2, 64, 64
    M = n * G2
    x, w, b = operands(rng, M, N, K, dtype)
    pos = f32(rng.standard_normal((T, N)))
    before = np.full((n * T, N), np.nan, np.float32)
    kw = dict(bias=b, pos=pos, T=T, G2=G2)
    bad = emulate(before, x, w, dtype=dtype, out_kind="f32", epi=G.PATCH, fault=fault, **kw)
    r_bad, changed = check(bad, before, x, w, dtype, "f32", G.PATCH, **kw)
    assert r_bad > 1 or changed, (r_bad, changed)
