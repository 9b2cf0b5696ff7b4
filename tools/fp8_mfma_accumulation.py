"""Accumulation error of the e4m3 GEMM (gemm_big8_kernel, v_mfma_scale_f32_16x16x128_f8f6f4) on Gaussian operands, relative to
u * sum|x w| (u = 2^-24), next to the bf16 kernel on the same values; plus two probes of the instruction: a subnormal e4m3 product, and
one large product beside 127 small ones (rounding of the sum).  profiles/r09a_fp8_mfma_accumulation.log, oracle/gemm_ref.py."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "intelligent-video-analysis-retrieval-system_amd")]
import torch  # noqa: E402

from ivr_amd.linear import gemm, quantize_rows_e4m3  # noqa: E402
from oracle import gemm_ref as G  # noqa: E402

U = 2.0 ** -24
for K in (128, 256, 1024, 4096):
    for variant in ("gauss", "normal_only", "sub_zeroed", "bf16_same_values"):
        g = torch.Generator(device="cuda").manual_seed(K)
        x = (torch.randn((512, K), device="cuda", generator=g) * 2).to(torch.float8_e4m3fn)
        w8, s = quantize_rows_e4m3(torch.randn((64, K), device="cuda", generator=g))
        w = w8.view(torch.float8_e4m3fn)
        if variant == "normal_only":
            xf = x.float()
            xf = torch.where(xf.abs() < 2 ** -6, torch.sign(xf + 1e-30) * 2 ** -6, xf)
            x = xf.to(torch.float8_e4m3fn)
        if variant == "sub_zeroed":
            xf = x.float()
            x = torch.where(xf.abs() < 2 ** -6, torch.zeros_like(xf), xf).to(torch.float8_e4m3fn)
        r = torch.zeros((512, 64), device="cuda")
        if variant == "bf16_same_values":
            gemm(x.float().to(torch.bfloat16), w.float().to(torch.bfloat16), epilogue=1, resid=r)
        else:
            gemm(x, w, epilogue=1, resid=r)
        torch.cuda.synchronize()
        xd, wd = G.decode(x), G.decode(w)
        ref = xd @ wd.T
        A = xd.abs() @ wd.abs().T
        pm = (xd.abs()[:, None, :] * wd.abs()[None, :, :]).amax(-1)
        e = (r.double() - ref).abs()
        q = e / (U * A)
        print(f"K={K:5d} {variant:16s} max err/(u A) = {float(q.max()):8.2f}  p99 = {float(q.flatten().kthvalue(int(q.numel() * 0.99)).values):7.2f}"
              f"  median = {float(q.median()):6.2f}  max err/(u maxprod) = {float((e / (U * pm)).max()):8.2f}  exact frac = {float((e == 0).double().mean()):.3f}")
# subnormal flush check: one subnormal x times a large w
x = torch.zeros((256, 128), device="cuda"); x[:, 0] = 2.0 ** -9; x[:, 1] = 2.0 ** -7
w = torch.zeros((64, 128), device="cuda"); w[:, 0] = 256.0; w[:, 1] = 1.0
r = torch.zeros((256, 64), device="cuda")
gemm(x.to(torch.float8_e4m3fn), w.to(torch.float8_e4m3fn), epilogue=1, resid=r)
torch.cuda.synchronize()
print("subnormal product: got", float(r[0, 0]), "want", 2.0 ** -9 * 256 + 2.0 ** -7)
# one large and many small products: alignment / truncation inside the MFMA
x = torch.ones((256, 128), device="cuda") * 2.0 ** -5; x[:, 0] = 256.0
w = torch.ones((64, 128), device="cuda") * 2.0 ** -5; w[:, 0] = 256.0
r = torch.zeros((256, 64), device="cuda")
gemm(x.to(torch.float8_e4m3fn), w.to(torch.float8_e4m3fn), epilogue=1, resid=r)
torch.cuda.synchronize()
print("65536 + 127 * 2^-10: got", repr(float(r[0, 0])), "want", repr(65536 + 127 * 2.0 ** -10), "fp32 of want",
      float(torch.tensor(65536 + 127 * 2.0 ** -10, dtype=torch.float32)))
