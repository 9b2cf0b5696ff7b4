"""GPU numerics: every attention kernel, per element, through ivr_attention / ivr_qkv_attention, against the float64 reference of
oracle/attention_ref.py.  The launcher's switches (IVR_ATTN_QC, IVR_ATTN_HEAD, IVR_QKV_PERS) are read on every call, so each kernel is
reached on purpose: attention_mfma_short_kernel (bf16, T <= 64), attention_head_kernel<QC = 3/4/5> (64 < T <= 640),
attention_mfma_kernel (T > 640 or IVR_ATTN_HEAD=0), attention_f32_kernel<KS = 8/4/2/1>, qkv_attn_kernel / qkv_attn_pers_kernel.

Input designs: uniform scores (Q = 0: the output is the mean of V over the allowed keys, within 1 ulp), one-hot selection (the
output row is one V row, bit for bit), exact invariances (causality, batch independence, bitwise) and Gaussian operands against the
per-element bound."""
import ctypes

import numpy as np
import pytest
import torch

from ivr_amd import _ffi
from ivr_amd.attention import attention, qkv_attention
from ivr_amd.linear import linear
from oracle import attention_ref as A

pytestmark = pytest.mark.gpu

WORST = {}          # path -> worst error / bound ratio seen (printed at the end of the module)


def _note(path, ratio):
    WORST[path] = max(WORST.get(path, 0.0), ratio)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\nworst error / bound per attention path:")
    for k in sorted(WORST):
        print(f"  {k:28s} {WORST[k]:.3f}")


# ---- kernel paths ------------------------------------------------------------------------------------------------------------------
def set_path(monkeypatch, path):
    """path: short | head3 | head4 | head5 | headauto | generic | f32."""
    monkeypatch.delenv("IVR_ATTN_QC", raising=False)
    monkeypatch.delenv("IVR_ATTN_HEAD", raising=False)
    if path.startswith("head") and path != "headauto":
        monkeypatch.setenv("IVR_ATTN_QC", path[4:])
    if path == "generic":
        monkeypatch.setenv("IVR_ATTN_HEAD", "0")


def out_kinds(path):
    return ("f32",) if path == "f32" else ("bf16",) if path == "generic" else ("bf16", "e4m3")


SHORT_T = [1, 2, 15, 16, 17, 33, 50, 63, 64]
HEAD_T = [65, 77, 97, 197, 257, 288, 289, 577, 640]
GENERIC_T = [641, 785, 1024, 65, 77, 257]
F32_T = [1, 8, 64, 65, 128, 129, 256, 257, 301]       # 301: the longest whose K and V fit in LDS (KS = 1 from T = 257 on)
# (n, heads) with n * heads not a multiple of 4: the short and generic kernels pack 4 (image, head) items per workgroup
NH = [(3, 1), (1, 2), (5, 2), (3, 2), (5, 1)]

CASES = ([("short", T) for T in SHORT_T] + [(f"head{qc}", T) for qc in (3, 4, 5) for T in HEAD_T]
         + [("generic", T) for T in GENERIC_T] + [("f32", T) for T in F32_T])


def nh_for(T, i=0):
    return NH[(T + i) % len(NH)]


def to_dev(qkv_np, path):
    t = torch.from_numpy(qkv_np).cuda()
    return t if path == "f32" else t.to(torch.bfloat16)


def run(qkv, T, heads, causal, kind):
    return attention(qkv, T, heads, causal=causal, out_fp8=(kind == "e4m3"))


def decoded(att, n, T, H):
    return A.unpack(A.decode(att).cpu().numpy(), n, T, H)


def split_edges(T):
    """Query rows where the head kernel's work changes hands (per QC): the start of every split (16 * tiles-per-split) and, inside
    each split, the start of every wave's QC tiles."""
    ntiles = (T + 15) // 16
    edges = set()
    for qc in (3, 4, 5):
        nsplit = -(-ntiles // (6 * qc))
        tps = -(-ntiles // nsplit)
        for sp in range(nsplit):
            start = sp * tps
            edges.update(16 * t for t in range(start, min(ntiles, start + tps), qc) if 0 < 16 * t < T)
    return sorted(edges)


# ---- design 1 + 2: uniform scores and one-hot selection, every path x T x causal x output --------------------------------------
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("path,T", CASES)
def test_uniform_and_onehot(path, T, causal, monkeypatch):
    set_path(monkeypatch, path)
    n, H = nh_for(T)
    rng = np.random.default_rng(T * 4 + causal)
    uq, uk, uv = A.design_uniform(rng, n, H, T)
    oq, ok_, ov, pis = A.design_onehot(rng, n, H, T, causal, edges=split_edges(T))
    u_qkv, o_qkv = to_dev(A.pack(uq, uk, uv), path), to_dev(A.pack(oq, ok_, ov), path)
    want_u, want_o = A.uniform_expected(uv, causal), A.onehot_expected(ov, pis)
    for kind in out_kinds(path):
        got = decoded(run(u_qkv, T, H, causal, kind), n, T, H)
        good = A.within_ulps(got, want_u, kind, 2 if kind == "f32" else 1)
        bad = np.argwhere(~good)
        assert good.all(), f"{path} T={T} causal={causal} {kind}: uniform scores, {len(bad)} elements off, first [img,head,row,col] {bad[:4].tolist()}"
        got = decoded(run(o_qkv, T, H, causal, kind), n, T, H)
        wrong = np.argwhere((got != want_o).any(-1))
        assert len(wrong) == 0, (f"{path} T={T} causal={causal} {kind}: one-hot rows not selected exactly, first [img,head,row] "
                                 f"{wrong[:4].tolist()} (target keys {[int(pis[tuple(w)]) for w in wrong[:4]]})")


# ---- design 4: Gaussian operands against the bound ---------------------------------------------------------------------------------
GAUSS = [("gauss3", 3.0, 0.0)]
GAUSS_ALL = [("gauss0.3", 0.3, 0.0), ("gauss3", 3.0, 0.0), ("gauss10", 10.0, 0.0), ("near1e3", 3.0, 1000.0)]
BOUNDARY = {1, 16, 17, 64, 65, 289, 640, 641, 1024, 129, 257, 301}


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("path,T", CASES)
def test_gaussian_within_bound(path, T, causal, monkeypatch):
    set_path(monkeypatch, path)
    n, H = nh_for(T, 1)
    rng = np.random.default_rng(T * 8 + causal + 1)
    for name, std, off in (GAUSS_ALL if T in BOUNDARY else GAUSS):
        q, k, v = A.design_gaussian(rng, n, H, T, std, off)
        qkv = to_dev(A.pack(q, k, v), path)
        ref, absv, eps = A.attention_ref(qkv, T, H, causal)
        for kind in out_kinds(path):
            out = run(qkv, T, H, causal, kind)
            ratio = ((A.decode(out) - ref).abs() / A.attention_bound(ref, absv, eps, kind, T)).max().item()
            _note(f"{path}/{kind}", ratio)
            assert ratio <= 1.0, f"{path} T={T} causal={causal} {kind} {name}: error {ratio:.3f} x the bound"


# ---- design 3: exact invariances ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path,T", [("short", 64), ("short", 50), ("head3", 289), ("head4", 257), ("head5", 640), ("generic", 785),
                                    ("generic", 257), ("f32", 129), ("f32", 301)])
def test_causal_prefix_invariance(path, T, monkeypatch):
    """Rows <= p do not change, bit for bit, when every K / V row after p is replaced (p on tile, block and split edges)."""
    set_path(monkeypatch, path)
    n, H = 3, 1
    rng = np.random.default_rng(T)
    q, k, v = A.design_gaussian(rng, n, H, T, 3.0)
    base = to_dev(A.pack(q, k, v), path)
    ps = sorted({p for p in [0, 15, 16, 31, 32, 63, 64, 95, 127, 128, T - 2] + [e - 1 for e in split_edges(T)] + split_edges(T)
                 if 0 <= p < T - 1})
    for kind in out_kinds(path):
        ref_out = decoded(run(base, T, H, True, kind), n, T, H)
        for p in ps:
            q2, k2, v2 = q.copy(), k.copy(), v.copy()
            k2[:, :, p + 1:] = A.design_gaussian(rng, n, H, T - p - 1, 3.0)[1]
            v2[:, :, p + 1:] = -v[:, :, p + 1:] * 2
            got = decoded(run(to_dev(A.pack(q2, k2, v2), path), T, H, True, kind), n, T, H)
            assert np.array_equal(got[:, :, :p + 1], ref_out[:, :, :p + 1]), f"{path} T={T} {kind}: rows <= {p} saw keys after {p}"
            assert not np.array_equal(got[:, :, p + 1:], ref_out[:, :, p + 1:])


@pytest.mark.parametrize("path,T", [("short", 50), ("short", 17), ("headauto", 257), ("head3", 97), ("generic", 641), ("f32", 65)])
@pytest.mark.parametrize("causal", [False, True])
def test_batch_independence(path, T, causal, monkeypatch):
    """Image i's rows are the same, bit for bit, whether it is encoded alone or inside a batch of 37 (also no cross-image leak)."""
    set_path(monkeypatch, path)
    n, H = 37, 16 if path == "headauto" else 2               # headauto: 37 * 16 >= 512 (n.heads) -> the timed QC choice
    rng = np.random.default_rng(T + 100 * causal)
    q, k, v = A.design_gaussian(rng, n, H, T, 3.0)
    qkv = to_dev(A.pack(q, k, v), path)
    D = 64 * H
    for kind in out_kinds(path):
        full = run(qkv, T, H, causal, kind)
        for i in (0, 1, 17, 36):
            alone = run(qkv[i * T:(i + 1) * T].clone(), T, H, causal, kind)
            assert torch.equal(full[i * T:(i + 1) * T].view(torch.uint8), alone.view(torch.uint8)), f"{path} image {i} depends on its batch"
        assert full.shape == (n * T, D)


# ---- cross-kernel agreement --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [65, 97, 257, 289, 577, 640])
@pytest.mark.parametrize("causal", [False, True])
def test_query_chunks_bit_identical(T, causal, monkeypatch):
    """QC = 3 / 4 / 5 differ only in how query tiles are spread over waves: identical bits; the timed default (n.heads >= 512) too."""
    n, H = (37, 16) if T <= 289 else (33, 16)
    rng = np.random.default_rng(T + causal)
    qkv = to_dev(A.pack(*A.design_gaussian(rng, n, H, T, 3.0)), "head3")
    for kind in ("bf16", "e4m3"):
        outs = {}
        for path in ("head3", "head4", "head5", "headauto"):
            set_path(monkeypatch, path)
            outs[path] = run(qkv, T, H, causal, kind).view(torch.uint8)
        for path in ("head4", "head5", "headauto"):
            assert torch.equal(outs[path], outs["head3"]), f"{path} != head3 at T={T} causal={causal} {kind}"


@pytest.mark.parametrize("T", [65, 77, 257, 640])
@pytest.mark.parametrize("causal", [False, True])
def test_generic_agrees_with_head_kernel(T, causal, monkeypatch):
    n, H = 3, 2
    rng = np.random.default_rng(T * 3 + causal)
    qkv = to_dev(A.pack(*A.design_gaussian(rng, n, H, T, 3.0)), "head3")
    ref, absv, eps = A.attention_ref(qkv, T, H, causal)
    bound = A.attention_bound(ref, absv, eps, "bf16", T)
    set_path(monkeypatch, "head3")
    head = A.decode(run(qkv, T, H, causal, "bf16"))
    set_path(monkeypatch, "generic")
    gen = A.decode(run(qkv, T, H, causal, "bf16"))
    assert ((gen - head).abs() <= 2 * bound).all()


# ---- fused QKV projection + attention ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pers", ["0", "2"])
@pytest.mark.parametrize("D", [192, 768])
@pytest.mark.parametrize("T", [1, 17, 37, 50, 64])
def test_fused_qkv_attention_equals_linear_then_attention(T, D, pers, monkeypatch):
    monkeypatch.setenv("IVR_QKV_PERS", pers)
    H = D // 64
    G = 256 // T                                           # whole images per 256-row tile: the last tile is ragged
    n = 2 * G + 1 if T > 1 else 300
    g = torch.Generator(device="cuda").manual_seed(T * 7 + D)
    xn = torch.randn((n * T, D), generator=g, device="cuda").to(torch.bfloat16)
    w = (torch.randn((3 * D, D), generator=g, device="cuda") * (0.6 / D ** 0.5)).to(torch.bfloat16)
    b = torch.randn(3 * D, generator=g, device="cuda") * 0.1
    qkv = linear(xn, w, b)                                 # bf16 store epilogue
    ref, absv, eps = A.attention_ref(qkv, T, H, False)
    for kind in ("bf16", "e4m3"):
        fused = qkv_attention(xn, w, b, T, H, out_fp8=(kind == "e4m3"))
        unfused = run(qkv, T, H, False, kind)
        assert torch.equal(fused.view(torch.uint8), unfused.view(torch.uint8)), f"fused != linear + attention T={T} D={D} pers={pers} {kind}"
        ratio = ((A.decode(fused) - ref).abs() / A.attention_bound(ref, absv, eps, kind, T)).max().item()
        _note(f"fused_pers{pers}/{kind}", ratio)
        assert ratio <= 1.0


# ---- a batch past 2^31 bytes -------------------------------------------------------------------------------------------------------
def test_batch_past_2gib_offsets():
    """ViT-L/14 shape (T = 257, D = 1024, 16 heads): qkv of 1400 images is 2.2 GB; the images around the 2^31-byte offset and the
    last one match the reference."""
    T, H, n = 257, 16, 1400
    D = 64 * H
    img_bytes = T * 3 * D * 2
    assert n * img_bytes > 2 ** 31
    g = torch.Generator(device="cuda").manual_seed(11)
    qkv = torch.empty((n * T, 3 * D), device="cuda", dtype=torch.bfloat16)
    for i0 in range(0, n, 200):
        qkv[i0 * T:(i0 + 200) * T] = (torch.randn((min(200, n - i0) * T, 3 * D), generator=g, device="cuda") * 0.6).to(torch.bfloat16)
    out = run(qkv, T, H, False, "bf16")
    mid = 2 ** 31 // img_bytes
    for i in (mid - 1, mid, mid + 1, n - 1):
        rows = slice(i * T, (i + 1) * T)
        ref, absv, eps = A.attention_ref(qkv[rows], T, H, False)
        ratio = ((A.decode(out[rows]) - ref).abs() / A.attention_bound(ref, absv, eps, "bf16", T)).max().item()
        _note("head_2GiB/bf16", ratio)
        assert ratio <= 1.0, f"image {i}: error {ratio:.3f} x the bound"
    del qkv, out
    torch.cuda.empty_cache()


# ---- argument checks ---------------------------------------------------------------------------------------------------------------
def test_invalid_arguments_rejected(monkeypatch):
    bf = lambda r, c: torch.zeros((r, c), device="cuda", dtype=torch.bfloat16)      # noqa: E731
    f32 = lambda r, c: torch.zeros((r, c), device="cuda", dtype=torch.float32)      # noqa: E731
    with pytest.raises(ValueError):
        attention(bf(50, 3 * 128), 50, 3)                  # D != 64 * heads
    with pytest.raises(ValueError):
        attention(bf(1025, 3 * 64), 1025, 1)               # T > 1024
    with pytest.raises(ValueError):
        attention(bf(50, 3 * 64 * 33), 50, 33)             # D > 2048
    with pytest.raises(ValueError):
        attention(f32(513, 3 * 64), 513, 1)                # float32 mode: T <= 512
    with pytest.raises(ValueError):
        attention(f32(512, 3 * 64), 512, 1)                # ... and K / V must fit in LDS
    with pytest.raises(ValueError):
        attention(bf(641, 3 * 64), 641, 1, out_fp8=True)   # no e4m3 output from the generic kernel
    monkeypatch.setenv("IVR_ATTN_HEAD", "0")
    with pytest.raises(ValueError):
        attention(bf(257, 3 * 64), 257, 1, out_fp8=True)
    monkeypatch.delenv("IVR_ATTN_HEAD")
    buf = torch.zeros(50 * 3 * 64 + 8, device="cuda", dtype=torch.bfloat16)
    with pytest.raises(ValueError):
        attention(buf[1:1 + 50 * 3 * 64].view(50, 3 * 64), 50, 1)     # not 16-byte aligned
    with pytest.raises(ValueError):
        attention(f32(302, 3 * 64), 302, 1)                # float32 mode: K and V of a head fit in LDS up to T = 301
    with pytest.raises(ValueError):
        attention(bf(50, 3 * 64), 50, 2 ** 26 + 1)         # 64 * heads wraps to 64 = D in 32-bit arithmetic
    lib = _ffi.load()
    ctx = _ffi.context(0)
    q = bf(50, 3 * 64)
    s = _ffi.stream_ptr()
    assert lib.ivr_attention(ctx, 0, q.data_ptr(), 1, 50, 64, 2 ** 26 + 1, 0, 0, q.data_ptr(), s) == -1
    assert b"head_dim" in lib.ivr_last_error(None)
    assert lib.ivr_attention(ctx, 0, q.data_ptr(), 1, 50, 64, 0, 0, 0, q.data_ptr(), s) == -1
    assert lib.ivr_attention(ctx, 0, q.data_ptr(), 2 ** 26, 16, 2048, 32, 0, 0, q.data_ptr(), s) == -1    # grid past 2^31
    assert lib.ivr_attention(ctx, 1, q.data_ptr(), 1, 302, 64, 1, 0, 0, q.data_ptr(), s) == -1
    desc = _ffi.TowerDesc(kind=0, width=64, layers=1, heads=2 ** 26 + 1, mlp=256, tokens=50, out_dim=64, act=0, pool=0, image=224,
                          patch=32, pre_ln=1, patch_bias=0, compute=0, ln_eps=1e-5)
    h = _ffi._p()
    assert lib.ivr_tower_create(ctx, ctypes.byref(desc), ctypes.byref(h)) == -1
    assert b"head_dim" in lib.ivr_last_error(None)
    assert lib.ivr_attention(ctx, 0, None, 1, 50, 64, 1, 0, 0, q.data_ptr(), _ffi.stream_ptr()) == -1
    assert lib.ivr_attention(ctx, 0, q.data_ptr(), 1, 0, 64, 1, 0, 0, q.data_ptr(), _ffi.stream_ptr()) == -1
    assert lib.ivr_attention(ctx, 1, q.data_ptr(), 1, 50, 64, 1, 0, 1, q.data_ptr(), _ffi.stream_ptr()) == -1
    assert lib.ivr_attention(ctx, 0, q.data_ptr(), -1, 50, 64, 1, 0, 0, q.data_ptr(), _ffi.stream_ptr()) == -1
    # fused: the shape limits hold even when IVR_FUSED_QKV=1 forces the fused kernel
    for env in (None, "1"):
        if env:
            monkeypatch.setenv("IVR_FUSED_QKV", env)
        for T, D, H in ((65, 192, 3), (50, 128, 2), (50, 192, 2), (50, 200, 3)):
            xn, w, b = bf(2 * T, D), bf(3 * D, D), torch.zeros(3 * D, device="cuda")
            with pytest.raises(ValueError):
                qkv_attention(xn, w, b, T, H)
        xn, w, b = bf(100, 192), bf(3 * 192, 192), torch.zeros(3 * 192, device="cuda")
        assert lib.ivr_qkv_attention(ctx, xn.data_ptr(), w.data_ptr(), None, 2, 50, 192, 3, 0, xn.data_ptr(), s) == -1
        with pytest.raises(ValueError):
            qkv_attention(xn, w, b, 50, 2 ** 26 + 3)       # 64 * heads wraps to 192 = D
        assert lib.ivr_qkv_attention(ctx, xn.data_ptr(), w.data_ptr(), b.data_ptr(), 2, 50, 192, 2 ** 26 + 3, 0, xn.data_ptr(), s) == -1
        big = torch.zeros((3 * 2112, 2112), device="cuda", dtype=torch.bfloat16)
        assert lib.ivr_qkv_attention(ctx, xn.data_ptr(), big.data_ptr(), b.data_ptr(), 2, 50, 2112, 33, 0, xn.data_ptr(), s) == -1
    torch.cuda.synchronize()


def test_empty_batch():
    """n = 0 is a no-op that returns an empty result (the empty tensors' data pointers may be NULL)."""
    bf = lambda r, c: torch.zeros((r, c), device="cuda", dtype=torch.bfloat16)      # noqa: E731
    assert attention(bf(0, 3 * 128), 50, 2).shape == (0, 128)
    assert attention(torch.zeros((0, 3 * 64), device="cuda"), 50, 1).shape == (0, 64)
    assert attention(bf(0, 3 * 64), 50, 1, out_fp8=True).shape == (0, 64)
    att = qkv_attention(bf(0, 192), bf(3 * 192, 192), torch.zeros(3 * 192, device="cuda"), 50, 3)
    assert att.shape == (0, 192)
    lib = _ffi.load()
    assert lib.ivr_attention(_ffi.context(0), 0, None, 0, 50, 64, 1, 0, 0, None, _ffi.stream_ptr()) == 0
    torch.cuda.synchronize()
