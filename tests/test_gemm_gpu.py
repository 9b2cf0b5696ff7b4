"""GPU: every GEMM instantiation of tower_kernels.hip per element against the float64 reference of oracle/gemm_ref.py, through
ivr_gemm (the towers' GemmArgs: strided operands and outputs, the patch epilogue, skipped residual rows, reversed row order).

Three kinds of data:
  * exact operands (small integers, dyadic bias / pos / residual, power-of-two colscale): every value before the output rounding is
    exact in fp32, so F32 / RESID / PATCH outputs equal float64 bit for bit, bf16 / e4m3 stores equal the round-to-nearest-even of
    the float64 value, and activations are within one output ulp.  Any slip of layout, tile walk, ragged edge, stride, skip or
    position row is a mismatch;
  * Gaussian operands, pre-activations pushed into [-12, -3] and next to 0, residual rows of large mean: err / bound <= 1 per element;
  * bit identities where the code claims them (skinny vs tiled, wide vs narrow epilogue, persistent vs one tile per workgroup,
    reverse_m, the group size of the tile order, 128 x 128 vs 256 x 256).
Outputs are filled with NaN before each call; canary columns, canary rows, skipped rows, token-0 rows and everything beyond M and N
must keep their bits.  Lines starting with RATIO (pytest -s) feed profiles/r09a_gemm_error_ratios.log."""
import pytest
import torch

from oracle import gemm_ref as G

pytestmark = pytest.mark.gpu

QG, GE = G.QUICK, G.GELU
STORE, RESID, PATCH, F32 = G.STORE, G.RESID, G.PATCH, G.F32
ENV = ("IVR_GEMM", "IVR_GEMM_SKINNY", "IVR_GEMM_WIDE_EPI", "IVR_GEMM_PERS", "IVR_GEMM_STAGGER", "IVR_GEMM_GROUP_M")
# kernel selection through the launcher's switches (ivr_launch_gemm reads them on every call)
MODES = {
    "tiled": {"IVR_GEMM": "0"},                                                  # gemm_kernel (128 x 128)
    "big_narrow": {"IVR_GEMM": "4", "IVR_GEMM_WIDE_EPI": "0", "IVR_GEMM_PERS": "0"},  # gemm_big_kernel, narrow epilogue
    "big_wide": {"IVR_GEMM": "4", "IVR_GEMM_PERS": "0"},                         # gemm_big_kernel, row-wide epilogue where N % 64 == 0
    "pers": {"IVR_GEMM": "4", "IVR_GEMM_PERS": "2", "IVR_GEMM_STAGGER": "3"},    # gemm_pers_kernel (bf16 STORE / RESID, N % 64 == 0)
    "skinny": {},                                                                # default selection at M <= 128: gemm_skinny_kernel
    "fp8": {},                                                                   # gemm_big8_kernel (the only e4m3 kernel)
}

# Every (kernel, template arguments) instantiation in libivr_hip.so and the runs of this file that launch it.  The symbol guard
# (tests/test_gemm_symbols_cpu.py) fails when the library holds one that is not listed here.
COVERAGE = {}
for _t in ("bf16", "f32"):
    for _e, _a in (("STORE", "none"), ("STORE", "QUICK"), ("STORE", "GELU"), ("RESID", "none"), ("PATCH", "none"), ("F32", "none")):
        COVERAGE[f"gemm_kernel<{_t},{_e},{_a}>"] = "tiled"
        COVERAGE[f"gemm_big_kernel<{_t},{_e},{_a}>"] = "big_narrow, big_wide (bf16 STORE / RESID)"
        COVERAGE[f"gemm_skinny_kernel<{_t},{_e},{_a},1>"] = "skinny"
    COVERAGE[f"gemm_big_kernel<{_t},RESID,none,SKIP>"] = "big_narrow / big_wide with skip_mod"
for _e, _a in (("STORE", "none"), ("STORE", "QUICK"), ("STORE", "GELU"), ("RESID", "none")):
    COVERAGE[f"gemm_pers_kernel<{_e},{_a}>"] = "pers"
for _a in ("none", "QUICK", "GELU"):
    COVERAGE[f"gemm_big8_kernel<STORE,{_a}>"] = "fp8, bf16 output"
    COVERAGE[f"gemm_big8_kernel<STORE,{_a},OUT8>"] = "fp8, e4m3 output"
COVERAGE["gemm_big8_kernel<RESID,none>"] = "fp8 RESID"
COVERAGE["gemm_big8_kernel<RESID,none,SKIP>"] = "fp8 RESID with skip_mod"

TDT = {"bf16": torch.bfloat16, "f32": torch.float32, "e4m3": torch.float8_e4m3fn}
KSTEP = {"bf16": 64, "f32": 32, "e4m3": 128}
RATIOS = {}


def _set_mode(monkeypatch, mode, **extra):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in {**MODES[mode], **extra}.items():
        monkeypatch.setenv(k, str(v))


def _nan(shape, dtype):
    if dtype == torch.float8_e4m3fn:
        return torch.full(shape, 0x7F, dtype=torch.uint8, device="cuda").view(torch.float8_e4m3fn)
    return torch.full(shape, float("nan"), dtype=dtype, device="cuda")


def _operands(gen, M, N, K, dtype, data, pad_k=0, act=-1):
    """A [M, K + pad_k], W [N, K + pad_k] in the operand dtype (NaN in the padding: a kernel that reads it poisons its outputs),
    bias [N], colscale [N] (e4m3) or None."""
    cuda = dict(device="cuda", generator=gen)
    if data == "exact":
        lo = 0 if act >= 0 else -3                      # activations: pre-activations >= -3.5, away from the erf tail (1-ulp check)
        x = torch.randint(lo, 4, (M, K), **cuda).float()
        w = torch.randint(lo, 4, (N, K), **cuda).float()
        b = torch.randint(-14, 15, (N,), **cuda).float() / 4 if act >= 0 else torch.randint(-64, 65, (N,), **cuda).float() / 4
        s = 2.0 ** torch.randint(-6, -2, (N,), **cuda).float() if dtype == "e4m3" else None
    else:
        x = torch.randn((M, K), **cuda) * (2.0 if dtype == "e4m3" else 0.7)
        w = torch.randn((N, K), **cuda) * K ** -0.5
        b = torch.randn((N,), **cuda)
        s = None
        if dtype == "e4m3":
            from ivr_amd.linear import quantize_rows_e4m3
            w, s = quantize_rows_e4m3(w)
            w = w.view(torch.float8_e4m3fn).float()
        if data == "tail":                              # half the rows: small products, the bias carries the pre-activation
            x[: M // 2] *= 2.0 ** -6
            even = torch.arange(N, device="cuda") % 2 == 0
            b = torch.where(even, torch.rand((N,), **cuda) * -9 - 3, (torch.rand((N,), **cuda) - 0.5) * 0.1)
    dt = TDT[dtype]
    A = _nan((M, K + pad_k), dt)
    W = _nan((N, K + pad_k), dt)
    A[:, :K] = x.to(dt)
    W[:, :K] = w.to(dt)
    return A, W, b.contiguous(), s


def _out_kind(dtype, epi, out8):
    if epi != STORE:
        return "f32"
    return "e4m3" if out8 else ("f32" if dtype == "f32" else "bf16")


def _ulps_ok(out, ref, kind):
    """|out - round(ref)| <= one ulp of the output dtype at the larger magnitude (ref exact in float64)."""
    r = G.round_to(ref, kind)
    o = G.decode(out)
    mant, emin = {"bf16": (7, -126), "e4m3": (3, -6), "f32": (23, -126)}[kind]
    mag = torch.maximum(r.abs(), o.abs())
    e = torch.floor(torch.log2(torch.where(mag > 0, mag, torch.ones_like(mag))))
    ulp = torch.exp2(torch.clamp(e, min=emin) - mant)
    return (o - r).abs() <= ulp


def run(mode, dtype, epi, M, N, K, *, act=-1, data="gauss", seed=0, out8=False, skip_mod=0, pad_k=0, pad_n=0, cls_T=0, G2=0,
        reverse_m=0, monkeypatch=None, label=None, env=None):
    """One ivr_gemm call on NaN-filled outputs, checked per element (exact data: bit for bit / one ulp; else err / bound <= 1) and for
    untouched sentinels.  Returns the output buffer."""
    from ivr_amd.linear import gemm
    if monkeypatch is not None:
        _set_mode(monkeypatch, mode, **(env or {}))
    gen = torch.Generator(device="cuda").manual_seed(seed * 7919 + M * 131 + N * 17 + K)
    A, W, bias, cs = _operands(gen, M, N, K, dtype, data, pad_k, act)
    kind = _out_kind(dtype, epi, out8)
    kw = dict(M=M, N=N, K=K, lda=K + pad_k, ldw=K + pad_k, epilogue=epi, act=act, bias=bias, colscale=cs, reverse_m=reverse_m)
    pos = None
    T = 0
    if epi in (STORE, F32):
        odt = torch.float8_e4m3fn if out8 else (torch.float32 if kind == "f32" else torch.bfloat16)
        ldo = N + pad_n
        buf = _nan((M + 3, ldo), odt)
        view = buf
        kw.update(out=buf.view(torch.uint8) if out8 else buf, ldo=ldo, out8=out8)
    elif epi == RESID:
        ldr = cls_T * N if cls_T else N + pad_n
        rows = M * cls_T if cls_T else M + 3
        buf = _nan((rows, N if cls_T else ldr), torch.float32)
        view = buf.view(M, ldr) if cls_T else buf
        if data == "exact":
            view[:M, :N] = torch.randint(-512, 513, (M, N), device="cuda", generator=gen).float() / 4
        else:
            view[:M, :N] = torch.randn((M, N), device="cuda", generator=gen) * 8 + 100     # rows of large mean
        kw.update(resid=buf, ldr=ldr, skip_mod=skip_mod)
    else:
        T = G2 + 1
        pos = torch.randn((T, N), device="cuda", generator=gen)
        if data == "exact":
            pos = torch.randint(-64, 65, (T, N), device="cuda", generator=gen).float() / 8
        buf = _nan(((M // G2) * T + 2, N + pad_n), torch.float32)
        view = buf
        kw.update(resid=buf, ldr=N + pad_n, pos=pos, T=T, G2=G2)
    before = view.clone()
    gemm(A, W, **kw)
    torch.cuda.synchronize()
    exp = G.expect(before, A, W, dtype=dtype, out_kind=kind, epi=epi, N=N, K=K, act=act, bias=bias, colscale=cs, pos=pos, T=T, G2=G2,
                   skip_mod=skip_mod)
    ratio, changed = G.verify(view, before, exp)
    tag = label or f"{mode} {dtype} epi={epi} act={act}{' out8' if out8 else ''}{' skip' if skip_mod else ''}"
    where = f"{tag} M={M} N={N} K={K} data={data}"
    assert changed == 0, f"{where}: {changed} sentinel / canary / skipped elements changed"
    assert ratio <= 1.0, f"{where}: err / bound = {ratio}"
    if data != "exact":
        RATIOS[tag] = max(RATIOS.get(tag, 0.0), ratio)
        print(f"RATIO {where}: {ratio:.4f}")
    else:
        ref, _, written = exp
        out = view.view(torch.uint8).view(torch.float8_e4m3fn) if out8 else view
        o, r = G.decode(out)[written], ref[written]
        if act < 0 and kind == "f32":
            assert torch.equal(o, r), f"{where}: not bit-exact ({int((o != r).sum())} elements)"
        elif act < 0:
            assert torch.equal(o, G.round_to(r, kind)), f"{where}: not the round to nearest even of the exact value"
        elif kind != "f32":           # (float32 activations: the bound above; __expf / erff are not correctly rounded)
            ok = _ulps_ok(o, r, kind)
            assert bool(ok.all()), f"{where}: {int((~ok).sum())} activation outputs beyond one ulp"
    return view


# ---- shapes -----------------------------------------------------------------------------------------------------------------------
MS = [1, 15, 16, 17, 127, 128, 129, 255, 256, 257, 513]


def _shapes(dtype, mode):
    """(M, N, K) list: every M of MS, ragged N (multiple of 4 not 16, multiple of 16 not 64) and whole ones, one K step, 192, 768,
    3072 and past the skinny kernel's 64-step LDS panel."""
    k1 = KSTEP[dtype]
    kbig = 4160 if dtype == "bf16" else 2080
    wide = mode in ("big_wide", "pers")
    ns = [64, 320, 768, 3072, 128] if wide else [68, 132, 80, 64, 320, 768, 3072]
    ks = [k1, 192, 768, 3072, kbig] if dtype != "f32" else [k1, 192, 768, 3072, kbig]
    ms = [m for m in MS if m <= 128] if mode == "skinny" else MS
    out = []
    for i, m in enumerate(ms):
        n = ns[i % len(ns)]
        if mode == "skinny" and n % 16:
            n = 80
        k = ks[i % len(ks)]
        if n * k > 768 * 3072:
            k = 768
        out.append((m, n, k))
    out.append((ms[-1], ns[3], kbig if mode != "pers" else 3072))
    return out


EPIS = [(STORE, -1), (STORE, QG), (STORE, GE), (RESID, -1), (F32, -1)]
# the row-wide epilogue exists for bf16 STORE / RESID only
RUNS = [(m, t, e, a) for m in ("tiled", "big_narrow", "big_wide", "skinny") for t in ("bf16", "f32") for e, a in EPIS
        if m != "big_wide" or (t == "bf16" and e != F32)]


@pytest.mark.parametrize("data", ["exact", "gauss"])
@pytest.mark.parametrize("mode,dtype,epi,act", RUNS)
def test_store_resid_f32_per_element(mode, dtype, epi, act, data, monkeypatch):
    for i, (M, N, K) in enumerate(_shapes(dtype, mode)):
        strided = i % 2 == 1
        run(mode, dtype, epi, M, N, K, act=act, data=data if act < 0 or data == "exact" else ("tail" if i % 2 else "gauss"), seed=i,
            pad_k=KSTEP[dtype] if strided else 0, pad_n=8 if strided else 0, monkeypatch=monkeypatch)
    if epi == RESID:          # skip_mod = T (the fp8 side path's layout), and the *_cls layout: ldr = T * N, other rows are canaries
        for M, N, K in ((513, 64 if mode == "big_wide" else 132, 768), (127, 64 if mode != "skinny" else 80, 192)):
            run(mode, dtype, RESID, M, N, K, data=data, skip_mod=50, monkeypatch=monkeypatch)
            run(mode, dtype, RESID, M, N, K, data=data, cls_T=7, monkeypatch=monkeypatch)


@pytest.mark.parametrize("data", ["exact", "gauss"])
@pytest.mark.parametrize("epi,act", [(STORE, -1), (STORE, QG), (STORE, GE), (RESID, -1)], ids=lambda v: str(v))
def test_persistent_per_element(epi, act, data, monkeypatch):
    for i, (M, N, K) in enumerate(_shapes("bf16", "pers")):
        for st in ("0", "3"):
            run("pers", "bf16", epi, M, N, K, act=act, data=data if act < 0 or data == "exact" else "tail", seed=i,
                pad_k=64 if i % 2 else 0, pad_n=8 if i % 2 else 0, monkeypatch=monkeypatch, env={"IVR_GEMM_STAGGER": st},
                reverse_m=i % 2)


@pytest.mark.parametrize("data", ["exact", "gauss"])
@pytest.mark.parametrize("dtype", ["bf16", "f32"])
@pytest.mark.parametrize("mode,G2", [("tiled", 49), ("tiled", 196), ("tiled", 256), ("big_narrow", 49), ("big_narrow", 196),
                                     ("big_narrow", 256), ("skinny", 49)])   # skinny: at most 128 rows, two images of 49 patches
def test_patch_epilogue_per_element(mode, dtype, G2, data, monkeypatch):
    """Images straddle the 128- and 256-row tile edges (G2 = 49: images 2 and 5; 196: image 0 / 1 at 128 / 256 ...)."""
    n_img = [2] if mode == "skinny" else ([1, 3, 11] if G2 == 49 else [1, 3])
    for i, n in enumerate(n_img):
        N = (768, 64, 132, 80)[i % 4] if mode != "skinny" else 80
        K = (192, KSTEP[dtype], 768)[i % 3]
        run(mode, dtype, PATCH, n * G2, N, K, data=data, G2=G2, seed=i, pad_n=4 * (i % 2), pad_k=KSTEP[dtype] * (i % 2),
            monkeypatch=monkeypatch)


@pytest.mark.parametrize("data", ["exact", "gauss"])
@pytest.mark.parametrize("act,out8", [(-1, False), (QG, False), (GE, False), (-1, True), (QG, True), (GE, True)])
def test_fp8_store_per_element(act, out8, data, monkeypatch):
    for i, (M, N, K) in enumerate([(1, 64, 128), (17, 192, 256), (129, 64, 768), (255, 320, 384), (257, 768, 128), (513, 128, 3072),
                                   (300, 3072, 256)]):
        run("fp8", "e4m3", STORE, M, N, K, act=act, out8=out8, data=data if act < 0 or data == "exact" else "tail", seed=i,
            pad_k=128 * (i % 2), pad_n=16 * (i % 2), monkeypatch=monkeypatch, reverse_m=i % 2)


@pytest.mark.parametrize("data", ["exact", "gauss"])
def test_fp8_resid_per_element(data, monkeypatch):
    for i, (M, N, K) in enumerate([(1, 64, 128), (129, 192, 768), (513, 768, 256), (300, 64, 3072)]):
        run("fp8", "e4m3", RESID, M, N, K, data=data, seed=i, pad_k=128 * (i % 2), pad_n=4 * (i % 2), monkeypatch=monkeypatch)
        run("fp8", "e4m3", RESID, M, N, K, data=data, seed=i, skip_mod=50, monkeypatch=monkeypatch)
        run("fp8", "e4m3", RESID, M, N, K, data=data, seed=i, cls_T=5, monkeypatch=monkeypatch)


# ---- bit identities ---------------------------------------------------------------------------------------------------------------
def _same(cfgs, call, monkeypatch):
    """Run `call` under each (mode, extra env) and assert the outputs are identical."""
    outs = []
    for mode, extra in cfgs:
        _set_mode(monkeypatch, mode, **extra)
        outs.append((mode, extra, call().clone()))
    for mode, extra, o in outs[1:]:
        assert torch.equal(G.bits(o), G.bits(outs[0][2])), (mode, extra, outs[0][:2])


def _call(dtype, epi, M, N, K, seed, **kw):
    from ivr_amd.linear import gemm
    gen = torch.Generator(device="cuda").manual_seed(seed)
    A, W, bias, cs = _operands(gen, M, N, K, dtype, "gauss", kw.pop("pad_k", 0))
    r0 = torch.randn((M * kw.get("cls_T", 1) + 2, N), device="cuda", generator=gen)
    G2 = kw.pop("G2", 0)
    pos = torch.randn((G2 + 1, N), device="cuda", generator=gen) if G2 else None
    act = kw.pop("act", -1)
    cls_T = kw.pop("cls_T", 0)

    def f():
        if epi == STORE:
            out = _nan((M, N), torch.float32 if dtype == "f32" else torch.bfloat16)
            return gemm(A, W, M=M, N=N, K=K, lda=A.stride(0), ldw=W.stride(0), act=act, bias=bias, colscale=cs, out=out, **kw)
        if epi == PATCH:
            r = _nan(((M // G2) * (G2 + 1), N), torch.float32)
            return gemm(A, W, M=M, N=N, K=K, lda=A.stride(0), ldw=W.stride(0), epilogue=PATCH, bias=bias, resid=r, pos=pos, T=G2 + 1, G2=G2,
                        **kw)
        r = r0.clone()
        return gemm(A, W, M=M, N=N, K=K, lda=A.stride(0), ldw=W.stride(0), epilogue=RESID, bias=bias, colscale=cs, resid=r,
                    ldr=(cls_T or 1) * N, **kw)
    return f


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_skinny_is_bit_identical_to_tiled_for_patch_skip_and_strides(dtype, monkeypatch):
    cfg = [("skinny", {}), ("tiled", {})]
    _same(cfg, _call(dtype, PATCH, 98, 768, 768, 1, G2=49), monkeypatch)
    _same(cfg, _call(dtype, RESID, 128, 512, 768, 2, skip_mod=50), monkeypatch)
    _same(cfg, _call(dtype, RESID, 100, 512, 4160 if dtype == "bf16" else 2080, 3, cls_T=50, pad_k=KSTEP[dtype]), monkeypatch)
    for act in (-1, QG, GE):
        _same(cfg, _call(dtype, STORE, 77, 1024, 768, 4, act=act, pad_k=KSTEP[dtype]), monkeypatch)


def test_wide_epilogue_is_bit_identical_to_narrow(monkeypatch):
    """act4_fast claims the same operations per element as act_fn<true>."""
    cfg = [("big_wide", {}), ("big_narrow", {})]
    for act in (-1, QG, GE):
        _same(cfg, _call("bf16", STORE, 600, 768, 768, 5 + act, act=act), monkeypatch)
    _same(cfg, _call("bf16", RESID, 600, 768, 768, 9), monkeypatch)
    _same(cfg, _call("bf16", RESID, 600, 768, 768, 10, skip_mod=50), monkeypatch)


@pytest.mark.parametrize("act", [-1, QG, GE])
def test_persistent_is_bit_identical_to_big(act, monkeypatch):
    cfg = [("big_wide", {}), ("pers", {"IVR_GEMM_STAGGER": "0"}), ("pers", {"IVR_GEMM_STAGGER": "3"})]
    _same(cfg, _call("bf16", STORE, 1300, 768, 768, 11, act=act, pad_k=64), monkeypatch)
    if act == -1:
        _same(cfg, _call("bf16", RESID, 1300, 768, 1536, 12), monkeypatch)


@pytest.mark.parametrize("mode", ["tiled", "big_narrow", "big_wide", "pers", "fp8"])
def test_reverse_m_and_group_m_give_the_same_bits(mode, monkeypatch):
    dtype = "e4m3" if mode == "fp8" else "bf16"
    for epi in (STORE, RESID):
        base = _call(dtype, epi, 1100, 768, 768, 13)
        cfg = [(mode, {})] + [(mode, {"IVR_GEMM_GROUP_M": g}) for g in (1, 2, 3, 8)]
        _same(cfg, base, monkeypatch)
        _set_mode(monkeypatch, mode)
        a = base().clone()
        b = _call(dtype, epi, 1100, 768, 768, 13, reverse_m=1)().clone()
        assert torch.equal(G.bits(a), G.bits(b)), (mode, epi)


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_128_and_256_tiles_give_the_same_bits(dtype, monkeypatch):
    """gemm_kernel and gemm_big_kernel: one fp32 accumulator per output, the same MFMA per 16-byte chunk, K ascending, the same
    epilogue expressions (narrow epilogue: act_fn<true> / float4 stores of acc + bias)."""
    cfg = [("tiled", {}), ("big_narrow", {})]
    for act in (-1, QG, GE):
        _same(cfg, _call(dtype, STORE, 513, 320, 768, 20 + act, act=act), monkeypatch)
    _same(cfg, _call(dtype, RESID, 513, 320, 768, 23, skip_mod=50), monkeypatch)
    _same(cfg, _call(dtype, PATCH, 5 * 49, 320, 768, 24, G2=49), monkeypatch)


# ---- invalid arguments ------------------------------------------------------------------------------------------------------------
def test_invalid_arguments_are_refused_before_any_launch():
    from ivr_amd import _ffi
    from ivr_amd.linear import gemm
    A = torch.zeros((256, 256), dtype=torch.bfloat16, device="cuda")
    W = torch.zeros((128, 256), dtype=torch.bfloat16, device="cuda")
    out = _nan((256, 128), torch.bfloat16)
    r = _nan((256 * 2, 128), torch.float32)
    pos = torch.zeros((50, 128), device="cuda")
    bad = [dict(lda=192), dict(ldw=128), dict(ldo=124), dict(epilogue=RESID, resid=r, ldr=64), dict(skip_mod=-1, epilogue=RESID, resid=r),
           dict(skip_mod=50), dict(epilogue=PATCH, resid=r, pos=pos, T=50, G2=49), dict(epilogue=PATCH, resid=r, pos=None, T=65, G2=64),
           dict(epilogue=PATCH, resid=r, pos=pos, T=64, G2=64), dict(K=100), dict(N=66), dict(act=3), dict(act=0, epilogue=RESID, resid=r),
           dict(reverse_m=2), dict(out8=True), dict(colscale=pos[0]), dict(lda=1 << 22), dict(M=-1), dict(out=None)]
    for b in bad:
        kw = dict(M=256, N=128, K=256, out=out)
        kw.update(b)
        with pytest.raises(ValueError, match="ivr_gemm"):
            gemm(A, W, **kw)
        assert b"ivr_gemm" in _ffi.load().ivr_last_error(None)
    A8 = torch.zeros((256, 256), dtype=torch.uint8, device="cuda")
    W8 = torch.zeros((128, 256), dtype=torch.uint8, device="cuda")
    for epi in (PATCH, F32):
        with pytest.raises(ValueError, match="ivr_gemm"):
            gemm(A8, W8, epilogue=epi, out=out, resid=r, pos=pos, T=65, G2=64)
    torch.cuda.synchronize()
    assert torch.isnan(out.float()).all() and torch.isnan(r).all(), "a refused call wrote its output"


# ---- row operands beyond 2 GiB (slabs) --------------------------------------------------------------------------------------------
def _slab_rows(M, quantum, row_bytes):
    most = 0x7FFFFFF0 // row_bytes
    slab = max(quantum, most // quantum * quantum)
    rows = {0, 1, M - 2, M - 1}
    for s in range(slab, M, slab):
        rows.update(range(max(0, s - 300), min(M, s + 300)))
    return torch.tensor(sorted(rows), device="cuda"), slab


def _tall(M, K, dtype, gen):
    dt = TDT[dtype]
    A = torch.empty((M, K), dtype=dt, device="cuda")
    for i in range(0, M, 8192):
        n = min(8192, M - i)
        if dtype == "e4m3":
            A[i:i + n] = torch.randint(-3, 4, (n, K), device="cuda", generator=gen).float().to(dt)
        else:
            A[i:i + n] = (torch.randn((n, K), device="cuda", generator=gen) * 0.7).to(dt)
    return A


def _checksum(out_sum, A, W, bias, cs, rowmask=None, extra=0.0):
    """Whole-output check: sum(out) against sum_m sum_n y[m, n] = (sum_m x_m) . w_n (* s_n) + M' bias_n, in float64; the tolerance is
    the sum of the per-element bounds' accumulation terms (chain * 2u * sum |x||w|) plus the output rounding of every element."""
    xs = torch.zeros(A.shape[1], dtype=torch.float64, device="cuda")
    xa = torch.zeros_like(xs)
    cnt = 0
    for i in range(0, A.shape[0], 16384):
        blk = G.decode(A[i:i + 16384])
        if rowmask is not None:
            blk = blk[rowmask[i:i + 16384]]
        xs += blk.sum(0)
        xa += blk.abs().sum(0)
        cnt += blk.shape[0]
    Wd = G.decode(W)
    y = Wd @ xs
    a = Wd.abs() @ xa
    if cs is not None:
        y, a = y * cs.double(), a * cs.double()
    if bias is not None:
        y = y + cnt * bias.double()
    return float(out_sum), float(y.sum()) + extra, float(a.sum()), cnt


def test_patch_beyond_2gib_runs_in_image_slabs():
    """G2 = 49, T = 50, K = 8192 bf16, 2700 images: a 2.17 GB row operand, slab boundary at image 2560 (256 * G2 rows per quantum)."""
    from ivr_amd.linear import gemm
    G2, T, K, N, n = 49, 50, 8192, 64, 2700
    M = n * G2
    assert M * K * 2 >= 2 ** 31
    gen = torch.Generator(device="cuda").manual_seed(31)
    A = _tall(M, K, "bf16", gen)
    W = (torch.randn((N, K), device="cuda", generator=gen) * K ** -0.5).to(torch.bfloat16)
    b = torch.randn(N, device="cuda", generator=gen)
    pos = torch.randn((T, N), device="cuda", generator=gen)
    r = _nan((n * T, N), torch.float32)
    gemm(A, W, epilogue=PATCH, bias=b, resid=r, pos=pos, T=T, G2=G2)
    torch.cuda.synchronize()
    rows, slab = _slab_rows(M, 256 * G2, K * 2)
    assert slab == 2560 * G2
    y, Ab, s, acc = G.gemm_ref(A[rows], W, K, None, b)
    ref, bnd = G.bound(y, Ab, s, acc, "bf16", K, "f32", -1, pos.double()[1 + rows % G2])
    out = r[G.patch_rows(M, T, G2).cuda()[rows]].double()
    assert float(((out - ref).abs() / bnd).max()) <= 1.0
    assert torch.isnan(r[0::T]).all(), "token-0 rows were written"
    tok = r.view(n, T, N)[:, 1:].double()
    got, want, asum, _ = _checksum(tok.sum(), A, W, b, None, extra=float(pos.double()[1:].sum()) * n)
    assert abs(got - want) <= G.acc_coef("bf16", K) * asum * 1.01 + 8 * G.U * float(tok.abs().sum()), (got, want)


def test_resid_with_skip_beyond_2gib():
    """bf16 RESID with skip_mod = 50: slabs of lcm(256, 50) rows, every skipped row untouched."""
    from ivr_amd.linear import gemm
    M, K, N, T = 140_000, 8192, 64, 50
    gen = torch.Generator(device="cuda").manual_seed(32)
    A = _tall(M, K, "bf16", gen)
    W = (torch.randn((N, K), device="cuda", generator=gen) * K ** -0.5).to(torch.bfloat16)
    b = torch.randn(N, device="cuda", generator=gen)
    r0 = torch.randn((M, N), device="cuda", generator=gen)
    r = r0.clone()
    gemm(A, W, epilogue=RESID, bias=b, resid=r, skip_mod=T)
    torch.cuda.synchronize()
    rows, slab = _slab_rows(M, 256 * 25, K * 2)
    assert slab % T == 0 and slab < M
    keep = rows[rows % T != 0]
    y, Ab, s, acc = G.gemm_ref(A[keep], W, K, None, b)
    ref, bnd = G.bound(y, Ab, s, acc, "bf16", K, "f32", -1, r0[keep].double())
    assert float(((r[keep].double() - ref).abs() / bnd).max()) <= 1.0
    assert torch.equal(G.bits(r[0::T]), G.bits(r0[0::T])), "skipped rows changed"
    mask = torch.arange(M, device="cuda") % T != 0
    got, want, asum, _ = _checksum((r - r0)[mask].double().sum(), A, W, b, None, rowmask=mask)
    assert abs(got - want) <= G.acc_coef("bf16", K) * asum * 1.01 + 2 * G.U * float(r.double().abs().sum()) * 2, (got, want)


@pytest.mark.parametrize("kind", ["bf16", "out8", "resid"])
def test_fp8_beyond_2gib(kind):
    """e4m3 row operand of 262,200 x 8192 (2.15 GB): whole 256-row slabs; bf16, e4m3 and residual outputs."""
    from ivr_amd.linear import gemm
    M, K, N = 262_200, 8192, 64
    gen = torch.Generator(device="cuda").manual_seed(33)
    A = _tall(M, K, "e4m3", gen)
    W = torch.randint(-3, 4, (N, K), device="cuda", generator=gen).float().to(torch.float8_e4m3fn)
    b = torch.randn(N, device="cuda", generator=gen)
    cs = 2.0 ** torch.randint(-12, -9, (N,), device="cuda", generator=gen).float()
    rows, slab = _slab_rows(M, 256, K)
    assert slab < M
    y, Ab, s, acc = G.gemm_ref(A[rows], W, K, cs, b)
    if kind == "resid":
        r0 = torch.randn((M, N), device="cuda", generator=gen)
        r = r0.clone()
        gemm(A, W, epilogue=RESID, bias=b, colscale=cs, resid=r)
        torch.cuda.synchronize()
        ref, bnd = G.bound(y, Ab, s, acc, "e4m3", K, "f32", -1, r0[rows].double())
        out = r[rows]
        total = (r - r0).double().sum()
    else:
        out8 = kind == "out8"
        o = _nan((M, N), torch.float8_e4m3fn if out8 else torch.bfloat16)
        gemm(A, W, bias=b, colscale=cs, out=o.view(torch.uint8) if out8 else o, out8=out8)
        torch.cuda.synchronize()
        ref, bnd = G.bound(y, Ab, s, acc, "e4m3", K, "e4m3" if out8 else "bf16")
        out = o[rows]
        total = G.decode(o).sum()
    assert float(((G.decode(out) - ref).abs() / bnd).max()) <= 1.0
    got, want, asum, cnt = _checksum(total, A, W, b, cs)
    rnd = {"bf16": 2.0 ** -8, "out8": 2.0 ** -4, "resid": 0.0}[kind]
    absout = float(G.decode(r if kind == "resid" else o).abs().sum())
    tol = (G.acc_coef("e4m3", K) * asum * 1.01 + (rnd * 1.07 + 8 * G.U) * absout + 4 * G.U * asum
           + (2.0 ** -10 * cnt * N if kind == "out8" else 0.0))
    assert got == got and abs(got - want) <= tol, (got, want, tol)


def test_f32_output_beyond_2gib():
    """float32 operands, EPI_F32: 70,000 x 8192 x 4 B = 2.3 GB row operand."""
    from ivr_amd.linear import gemm
    M, K, N = 70_000, 8192, 64
    gen = torch.Generator(device="cuda").manual_seed(34)
    A = _tall(M, K, "f32", gen)
    W = torch.randn((N, K), device="cuda", generator=gen) * K ** -0.5
    o = _nan((M, N), torch.float32)
    gemm(A, W, epilogue=F32, out=o)
    torch.cuda.synchronize()
    rows, slab = _slab_rows(M, 256, K * 4)
    assert slab < M
    y, Ab, s, acc = G.gemm_ref(A[rows], W, K)
    ref, bnd = G.bound(y, Ab, s, acc, "f32", K, "f32")
    assert float(((o[rows].double() - ref).abs() / bnd).max()) <= 1.0
    got, want, asum, _ = _checksum(o.double().sum(), A, W, None, None)
    assert abs(got - want) <= G.acc_coef("f32", K) * asum * 1.01 + 4 * G.U * float(o.double().abs().sum()), (got, want)


def test_zz_ratio_summary():
    """Largest err / bound per (kernel, epilogue, dtype) of the Gaussian runs above (printed for the records)."""
    for k in sorted(RATIOS):
        print(f"RATIO-MAX {k}: {RATIOS[k]:.4f}")
