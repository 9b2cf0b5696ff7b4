"""GPU numerics: the tower GEMM kernel with every epilogue vs a plain PyTorch fp32 reference of the same op
(this is the one floating-point kernel for which a torch reference is kept next to the oracle)."""
import numpy as np
import pytest
import torch

from oracle.gemm_ref import error_ratio

pytestmark = pytest.mark.gpu


def _ref(x, w, b, act):
    y = x.float().cpu() @ w.float().cpu().T + (b.cpu() if b is not None else 0)
    if act == 0:
        y = y * torch.sigmoid(1.702 * y)
    elif act == 1:
        y = torch.nn.functional.gelu(y)
    return y


@pytest.fixture(params=["auto", "128x128", "256x256", "256x256-narrow", "256x256-persistent"])
def kernel(request, monkeypatch):
    """The launcher picks the 256 x 256 kernels only for problems that fill the chip; the tests drive ALL of them (both epilogues of
    the one-tile-per-workgroup kernel, and the persistent kernel of round 3 wherever its alignment conditions hold) with every shape
    through the A/B switches the launcher reads on each call."""
    if request.param != "auto":
        monkeypatch.setenv("IVR_GEMM", "0" if request.param == "128x128" else "4")
    monkeypatch.setenv("IVR_GEMM_PERS", "2" if request.param == "256x256-persistent" else "0")
    if request.param == "256x256-narrow":
        monkeypatch.setenv("IVR_GEMM_WIDE_EPI", "0")
    return request.param


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("M,N,K", [(1, 64, 64), (50, 128, 128), (129, 260, 192), (400, 768, 768), (257, 2304, 768), (1000, 768, 3072),
                                   (700, 320, 384), (513, 1152, 128)])
def test_store_epilogue_with_activations(dtype, M, N, K, kernel):
    from ivr_amd.linear import linear
    g = torch.Generator(device="cuda").manual_seed(M * 31 + N)
    x = (torch.randn((M, K), generator=g, device="cuda") * 0.7).to(dtype)
    w = (torch.randn((N, K), generator=g, device="cuda") * K ** -0.5).to(dtype)
    b = torch.randn(N, generator=g, device="cuda") * 0.1
    for act in (-1, 0, 1):
        y = linear(x, w, b, act=act).float().cpu()
        ref = _ref(x, w, b, act)
        tol = 2e-5 if dtype == torch.float32 else 1.2e-2       # bf16 output rounding: 2^-8 relative
        assert (y - ref).abs().max() <= tol * max(1.0, ref.abs().max()), (act, (y - ref).abs().max())
        kind = "f32" if dtype == torch.float32 else "bf16"
        assert error_ratio(y, x, w, kind, kind, bias=b, act=act) <= 1.0, act     # per element (oracle/gemm_ref.py)
    y = linear(x, w, None)                                      # no bias
    assert (y.float().cpu() - _ref(x, w, None, -1)).abs().max() <= (2e-5 if dtype == torch.float32 else 1.2e-2) * 4
    assert error_ratio(y, x, w, kind, kind) <= 1.0


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("M,N,K", [(333, 512, 768), (600, 384, 256)])
def test_residual_and_f32_epilogues(dtype, M, N, K, kernel):
    from ivr_amd.linear import EPI_F32, EPI_RESID, linear
    g = torch.Generator(device="cuda").manual_seed(5)
    x = (torch.randn((M, K), generator=g, device="cuda") * 0.7).to(dtype)
    w = (torch.randn((N, K), generator=g, device="cuda") * K ** -0.5).to(dtype)
    b = torch.randn(N, generator=g, device="cuda") * 0.1
    r0 = torch.randn((M, N), generator=g, device="cuda")
    r = r0.clone()
    linear(x, w, b, epilogue=EPI_RESID, resid=r)
    ref = r0.cpu() + _ref(x, w, b, -1)
    assert (r.cpu() - ref).abs().max() < 2e-5 * 4               # accumulation and the residual stay in float32
    kind = "f32" if dtype == torch.float32 else "bf16"
    assert error_ratio(r, x, w, kind, "f32", bias=b, r=r0) <= 1.0
    y = linear(x, w, None, epilogue=EPI_F32)
    assert y.dtype == torch.float32 and (y.cpu() - _ref(x, w, None, -1)).abs().max() < 2e-5 * 4
    assert error_ratio(y, x, w, kind, "f32") <= 1.0


def test_exact_integer_operands_catch_layout_errors(kernel):
    """Small integers are exact in bf16 and f32 accumulation: any fragment / swizzle / transpose slip shows as != 0."""
    from ivr_amd.linear import EPI_F32, linear
    rng = np.random.default_rng(0)
    M, N, K = 192, 320, 256
    x = torch.from_numpy(rng.integers(-3, 4, (M, K)).astype(np.float32))
    w = torch.from_numpy(rng.integers(-3, 4, (N, K)).astype(np.float32))      # asymmetric, not identity
    ref = x @ w.T
    for dt in (torch.bfloat16, torch.float32):
        y = linear(x.cuda().to(dt), w.cuda().to(dt), None, epilogue=EPI_F32).cpu()
        assert torch.equal(y, ref)


def test_bad_shapes():
    from ivr_amd.linear import linear
    x = torch.zeros((4, 100), dtype=torch.bfloat16, device="cuda")
    w = torch.zeros((8, 100), dtype=torch.bfloat16, device="cuda")
    with pytest.raises(ValueError):
        linear(x, w)                                            # K not a multiple of 64


def test_row_operand_beyond_2gib_runs_in_slabs():
    """the kernels reach 2 GiB through their 32-bit buffer offsets; a taller row operand (here 1.1M x 1024 bf16
    = 2.25 GB, what ViT-B/32 reaches from ~6.8k frames per step) is run as slabs of whole 256-row tiles.  Store and residual
    epilogues, rows on both sides of every slab boundary and the last row checked against a float32 product."""
    from ivr_amd.linear import EPI_RESID, linear
    M, N, K = 1_100_003, 64, 1024
    assert M * K * 2 > 2 ** 31
    g = torch.Generator(device="cuda").manual_seed(9)
    x = torch.empty((M, K), dtype=torch.bfloat16, device="cuda")
    for i in range(0, M, 200_000):
        x[i:i + 200_000] = (torch.randn((min(200_000, M - i), K), generator=g, device="cuda") * 0.7).to(torch.bfloat16)
    w = (torch.randn((N, K), generator=g, device="cuda") * K ** -0.5).to(torch.bfloat16)
    b = torch.randn(N, generator=g, device="cuda") * 0.1
    y = linear(x, w, b)
    slab = (0x7ffffff0 // (K * 2)) // 256 * 256
    rows = torch.tensor(sorted({0, 1, 255, 256, slab - 1, slab, slab + 1, slab + 257, M - 2, M - 1} | set(range(slab - 300, slab + 300, 37))),
                        device="cuda")
    ref = x[rows].float() @ w.float().T + b
    assert (y[rows].float() - ref).abs().max() <= 1.2e-2 * max(1.0, float(ref.abs().max()))
    assert error_ratio(y[rows], x[rows], w, "bf16", "bf16", bias=b) <= 1.0
    # every row was written: an unwritten slab would leave torch.empty garbage, caught by a checksum against a chunked product
    tot = sum(float((x[i:i + 100_000].float() @ w.float().T + b).double().sum()) for i in range(0, M, 100_000))
    assert abs(float(y.double().sum()) - tot) <= 2e-3 * M ** 0.5 * N ** 0.5 + 1e-6 * abs(tot) + 50.0
    r = torch.zeros((M, N), dtype=torch.float32, device="cuda")
    linear(x, w, b, epilogue=EPI_RESID, resid=r)
    assert (r[rows] - ref).abs().max() < 2e-4 * max(1.0, float(ref.abs().max()))
    assert error_ratio(r[rows], x[rows], w, "bf16", "f32", bias=b, r=torch.zeros_like(r[rows])) <= 1.0


@pytest.mark.parametrize("M,N,K,act", [(40_000, 768, 768, -1), (11_003, 3072, 768, 0), (70_001, 768, 3072, -1), (131_072, 256, 128, 1),
                                       (300, 768, 768, -1)])
def test_persistent_kernel_is_bit_identical_to_the_tile_per_workgroup_kernel(M, N, K, act, monkeypatch):
    """gemm_pers_kernel walks several tiles per workgroup as one flattened stage sequence (DMA look-ahead across tile boundaries,
    LDS-free epilogues, staggered start): same K order and the same epilogue expressions as gemm_big_kernel, so store and residual
    outputs must be BIT-identical, ragged last panels and both zigzag directions included; small integers catch any layout slip."""
    from ivr_amd.linear import EPI_RESID, linear
    g = torch.Generator(device="cuda").manual_seed(M + N)
    x = (torch.randn((M, K), generator=g, device="cuda") * 0.7).to(torch.bfloat16)
    w = (torch.randn((N, K), generator=g, device="cuda") * K ** -0.5).to(torch.bfloat16)
    b = torch.randn(N, generator=g, device="cuda") * 0.1
    r0 = torch.randn((M, N), generator=g, device="cuda")
    outs = {}
    for mode, stagger in (("0", "0"), ("2", "0"), ("2", "3")):
        monkeypatch.setenv("IVR_GEMM", "4")
        monkeypatch.setenv("IVR_GEMM_PERS", mode)
        monkeypatch.setenv("IVR_GEMM_STAGGER", stagger)
        y = linear(x, w, b, act=act)
        r = r0.clone()
        linear(x, w, b, epilogue=EPI_RESID, resid=r)
        outs[(mode, stagger)] = (y, r)
    for key in (("2", "0"), ("2", "3")):
        assert torch.equal(outs[key][0], outs[("0", "0")][0]), key
        assert torch.equal(outs[key][1], outs[("0", "0")][1]), key
    rows = torch.tensor([0, 255, 256, M // 2, M - 1], device="cuda")
    ref = x[rows].float() @ w.float().T + b
    if act == 0:
        ref = ref * torch.sigmoid(1.702 * ref)
    elif act == 1:
        ref = torch.nn.functional.gelu(ref)
    assert (outs[("2", "3")][0][rows].float() - ref).abs().max() <= 1.2e-2 * max(1.0, float(ref.abs().max()))
    assert error_ratio(outs[("2", "3")][0][rows], x[rows], w, "bf16", "bf16", bias=b, act=act) <= 1.0
    assert error_ratio(outs[("2", "3")][1][rows], x[rows], w, "bf16", "f32", bias=b, r=r0[rows]) <= 1.0
    xi = torch.randint(-3, 4, (M, K), generator=g, device="cuda").to(torch.bfloat16)
    wi = torch.randint(-3, 4, (N, K), generator=g, device="cuda").to(torch.bfloat16)
    monkeypatch.setenv("IVR_GEMM_PERS", "2")
    ri = torch.zeros((M, N), device="cuda")
    linear(xi, wi, None, epilogue=EPI_RESID, resid=ri)
    pick = torch.tensor([0, 1, 257, M // 3, M - 1], device="cuda")
    assert torch.equal(ri[pick], xi[pick].float() @ wi.float().T)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("M,N,K", [(1, 64, 64), (16, 512, 512), (50, 768, 3072), (77, 2048, 512), (77, 512, 2048), (113, 2304, 768), (128, 3072, 1024),
                                   (49, 768, 3072), (127, 384, 1536), (128, 1152, 384), (129, 512, 512)])
def test_skinny_kernel_is_bit_identical_to_the_tiled_kernels(dtype, M, N, K, monkeypatch):
    """Up to 128 rows (one text query, one ViT-B/32 image) the launcher takes gemm_skinny_kernel: a wave per 16 x 16 output tile, the
    weight panel by LDS-DMA, activations from L2 straight into the MFMA fragments (129 rows: both runs take the tiled kernel).  Same accumulation order over K as the tiled kernels -> the same bits for every epilogue, so a
    row's embedding does not depend on the size of the batch it was encoded in."""
    from ivr_amd.linear import EPI_F32, EPI_RESID, linear
    g = torch.Generator(device="cuda").manual_seed(M * 7 + N + K)
    x = (torch.randn((M, K), generator=g, device="cuda") * 0.7).to(dtype)
    w = (torch.randn((N, K), generator=g, device="cuda") * K ** -0.5).to(dtype)
    b = torch.randn(N, generator=g, device="cuda") * 0.1
    r0 = torch.randn((M, N), generator=g, device="cuda")

    def run():
        return ([linear(x, w, b, act=a) for a in (-1, 0, 1)] + [linear(x, w, None), linear(x, w, b, epilogue=EPI_RESID, resid=r0.clone()),
                                                                linear(x, w, None, epilogue=EPI_F32)])
    monkeypatch.setenv("IVR_GEMM_SKINNY", "1")
    skinny = run()
    monkeypatch.setenv("IVR_GEMM_SKINNY", "0")
    tiled = run()
    for a, t in zip(skinny, tiled):
        assert torch.equal(a, t)
    ref = _ref(x, w, b, -1)
    assert (skinny[0].float().cpu() - ref).abs().max() <= (2e-5 if dtype == torch.float32 else 1.2e-2) * max(1.0, ref.abs().max())
    kind = "f32" if dtype == torch.float32 else "bf16"
    for a, out in zip((-1, 0, 1), skinny[:3]):
        assert error_ratio(out, x, w, kind, kind, bias=b, act=a) <= 1.0, a
    assert error_ratio(skinny[4], x, w, kind, "f32", bias=b, r=r0) <= 1.0
