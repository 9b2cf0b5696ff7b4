"""GPU numerics: the LayerNorm kernel of the towers (layernorm_kernel<float / bf16 / e4m3 out>) through ivr_layernorm, per element,
against float64 LayerNorm with the per-element bound of oracle/attention_ref.py."""
import numpy as np
import pytest
import torch

from ivr_amd import _ffi
from ivr_amd.attention import OUT_BF16, OUT_F32, OUT_FP8, layernorm
from oracle import attention_ref as A

pytestmark = pytest.mark.gpu

KINDS = {"bf16": OUT_BF16, "f32": OUT_F32, "e4m3": OUT_FP8}


def params(D, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return (1 + 0.3 * torch.randn(D, generator=g, device="cuda")), 0.2 * torch.randn(D, generator=g, device="cuda")


def check(out, x, g, b, eps, kind):
    ref, bound = A.layernorm_bound(x, g, b, eps, kind)
    ratio = ((A.decode(out) - ref).abs() / bound).max().item()
    assert ratio <= 1.0, f"{kind}: error {ratio:.3f} x the bound"
    return ratio


@pytest.mark.parametrize("kind", ["f32", "bf16", "e4m3"])
@pytest.mark.parametrize("rows", [1, 3, 5, 1027])
@pytest.mark.parametrize("D", [64, 128, 384, 512, 768, 1024, 1280, 2048])
def test_layernorm_matches_float64(D, rows, kind):
    gen = torch.Generator(device="cuda").manual_seed(D * 7 + rows)
    x = torch.randn((rows, D), generator=gen, device="cuda") * 2 + 0.5 * torch.randn((rows, 1), generator=gen, device="cuda")
    g, b = params(D, D)
    out = layernorm(x, g, b, 1e-5, KINDS[kind])
    check(out, x, g, b, 1e-5, kind)
    rev = layernorm(x, g, b, 1e-5, KINDS[kind], reverse=True)
    assert torch.equal(out.view(torch.uint8), rev.view(torch.uint8)), "reverse=1 differs from reverse=0"


@pytest.mark.parametrize("kind", ["f32", "bf16"])
@pytest.mark.parametrize("D", [768, 1024])
def test_pooling_gather(D, kind):
    """out row r = LN(x[r * row_mul + offs[r]]): the EOS / CLS gathers of the pooling."""
    T, n = 77, 37
    gen = torch.Generator(device="cuda").manual_seed(D)
    x = torch.randn((n * T, D), generator=gen, device="cuda")
    g, b = params(D, 3)
    offs = torch.randint(0, T, (n,), generator=gen, device="cuda", dtype=torch.int32)
    offs[0], offs[-1] = 0, T - 1
    src = x[torch.arange(n, device="cuda") * T + offs.long()]
    got = layernorm(x, g, b, 1e-5, KINDS[kind], row_mul=T, offs=offs)
    assert torch.equal(got.view(torch.uint8), layernorm(src, g, b, 1e-5, KINDS[kind]).view(torch.uint8))
    check(got, src, g, b, 1e-5, kind)
    cls = layernorm(x, g, b, 1e-5, KINDS[kind], row_mul=T)            # token-0 rows (no offsets)
    assert cls.shape == (n, D)
    assert torch.equal(cls.view(torch.uint8), layernorm(x[::T].contiguous(), g, b, 1e-5, KINDS[kind]).view(torch.uint8))


@pytest.mark.parametrize("kind", ["f32", "bf16", "e4m3"])
@pytest.mark.parametrize("D", [64, 768, 2048])
def test_large_mean_small_spread(D, kind):
    """Rows of mean 1e3 and standard deviation 1e-1: the two-pass statistics keep them accurate."""
    gen = torch.Generator(device="cuda").manual_seed(D + 1)
    x = 1000 + 0.1 * torch.randn((67, D), generator=gen, device="cuda")
    g, b = params(D, 5)
    out = layernorm(x, g, b, 1e-5, KINDS[kind])
    check(out, x, g, b, 1e-5, kind)
    if kind == "f32":
        ref, _, _ = A.layernorm_ref(x, g, b, 1e-5)
        assert (out.double() - ref).abs().max().item() < 1e-3


@pytest.mark.parametrize("eps", [1e-5, 1e-12])
@pytest.mark.parametrize("kind", ["f32", "bf16", "e4m3"])
@pytest.mark.parametrize("D", [64, 384, 768, 2048])
def test_constant_rows_give_b(D, kind, eps):
    gen = torch.Generator(device="cuda").manual_seed(D)
    c = torch.randn((257, 1), generator=gen, device="cuda") * torch.logspace(-3, 3, 257, device="cuda")[:, None]
    x = c.expand(257, D).contiguous()
    g, b = params(D, 9)
    out = A.decode(layernorm(x, g, b, eps, KINDS[kind]))
    want = torch.from_numpy(A.round_to(b.double().cpu().numpy(), kind)).cuda()
    bad = (out != want[None, :]).any(1).nonzero().flatten()
    assert len(bad) == 0, f"{len(bad)} constant rows do not give b, e.g. value {c[bad[:3], 0].tolist()}"


def test_invalid_arguments_rejected():
    x = torch.zeros((4, 66), device="cuda")
    g = torch.ones(66, device="cuda")
    with pytest.raises(ValueError):
        layernorm(x, g, g, 1e-5, OUT_F32)                 # D % 4 != 0
    x = torch.zeros((4, 2052), device="cuda")
    g = torch.ones(2052, device="cuda")
    with pytest.raises(ValueError):
        layernorm(x, g, g, 1e-5, OUT_BF16)                # D > 2048
    x = torch.zeros((4, 64), device="cuda")
    g = torch.ones(64, device="cuda")
    with pytest.raises(ValueError):
        layernorm(x, g, g, 1e-5, 3)
    with pytest.raises(ValueError):
        layernorm(torch.zeros((8, 64), device="cuda"), g, g, 1e-5, OUT_F32, row_mul=4,
                  offs=torch.tensor([0, 7], device="cuda", dtype=torch.int32))      # source row 4 + 7 lies outside x
    lib = _ffi.load()
    ctx = _ffi.context(0)
    out = torch.zeros((4, 64), device="cuda")
    s = _ffi.stream_ptr()
    assert lib.ivr_layernorm(ctx, 1, x.data_ptr(), 1, None, g.data_ptr(), g.data_ptr(), 1e-5, 4, 64, 0, None, s) == -1
    assert lib.ivr_layernorm(ctx, 3, x.data_ptr(), 1, None, g.data_ptr(), g.data_ptr(), 1e-5, 4, 64, 0, out.data_ptr(), s) == -1
    assert lib.ivr_layernorm(ctx, 1, x.data_ptr(), 1, None, g.data_ptr(), g.data_ptr(), 1e-5, 4, 66, 0, out.data_ptr(), s) == -1
    assert lib.ivr_layernorm(ctx, 1, x.data_ptr(), 1, None, g.data_ptr(), g.data_ptr(), -1.0, 4, 64, 0, out.data_ptr(), s) == -1
    assert lib.ivr_layernorm(ctx, 1, x.data_ptr() + 4, 1, None, g.data_ptr(), g.data_ptr(), 1e-5, 3, 64, 0, out.data_ptr(), s) == -1
    torch.cuda.synchronize()


def test_empty_rows():
    g = torch.ones(64, device="cuda")
    for kind in (OUT_F32, OUT_BF16, OUT_FP8):
        assert layernorm(torch.zeros((0, 64), device="cuda"), g, g, 1e-5, kind).shape == (0, 64)
    assert _ffi.load().ivr_layernorm(_ffi.context(0), 1, None, 1, None, g.data_ptr(), g.data_ptr(), 1e-5, 0, 64, 0, None,
                                     _ffi.stream_ptr()) == 0
