"""ORACLE (test infrastructure, never shipped, never imported by the product path).

float64 restatement of the tower GEMMs (gemm_kernel, gemm_big_kernel, gemm_pers_kernel, gemm_skinny_kernel, gemm_big8_kernel behind
ivr_gemm / ivr_linear / ivr_linear_fp8) for the per-element tests (tests/test_gemm_gpu.py, tests/test_linear_gpu.py,
tests/test_fp8_gpu.py).  The operands are decoded exactly as the kernels read them (bf16 / float32 / e4m3 -> float64), then
    y = x w^T (* colscale[n]) + bias[n]
followed by the epilogue: act (none, QuickGELU x sigmoid(1.702 x), exact erf GELU) and STORE in the output dtype, EPI_F32, RESID
(r + y, rows m % skip_mod == 0 left as they were) or PATCH (row m -> residual row (m / G2) T + 1 + m % G2, plus pos[1 + m % G2]).
Everything is torch, so the references run on the GPU in float64.

Per-element error bound (u = 2^-24; one rounding of an fp32 adder is taken as one ulp, 2u relative, which also covers adders that
truncate inside the MFMA; A = sum_k |x_k w_k| in float64):

  * accumulation.  Every output has ONE fp32 accumulator and the K steps run in ascending order (all five kernels):
      bf16  v_mfma_f32_16x16x32_bf16: products exact in fp32 (8 x 8 significant bits); 32 products + the accumulator per issue are a
            sum tree of depth <= 6; K / 32 issues in a chain              -> chain c = K/32 + 6
      f32   four v_mfma_f32_16x16x4_f32 per 16-byte chunk: every product rounded once, 4 products + the accumulator a tree of depth
            <= 3, K / 4 issues in a chain                                  -> chain c = K/4 + 4
      e4m3  v_mfma_scale_f32_16x16x128_f8f6f4 (unit block scales): products exact, 128 products + the accumulator a tree of depth
            <= 8, K / 128 issues in a chain (gemm_big8_kernel)              -> chain c = K/128 + 8
    |acc - x.w| <= 2 c u A  (first order; the factor 1 + 2cu of the exact gamma_c is below 1.001 for every K the towers use).
    The e4m3 MFMA does NOT add like fp32 adders: measured on the MI355X (profiles/r09a_fp8_mfma_accumulation.log), one issue's sum of
    128 exact products is off by up to 255.5 u sum|p| (2^-16 of the block's absolute sum; results truncated toward zero), where the
    bf16 MFMA on the same values stays below 0.5 u A.  This is a property of the instruction, not of the kernel; the bound adds
    twice the largest value seen, 2^-15 A, to the chain term for e4m3 (acc_coef).
  * epilogue arithmetic: one rounding (2u of the result) for the colscale multiply (e4m3), the bias add, and the residual or
    position add (RESID, PATCH):  pre = |s| 2 c u A + 2u (|s acc| [e4m3] + |y| + |r + y| [RESID / PATCH]).
  * activation (STORE only), at the computed pre-activation v, |v - y| <= pre:
        |act_c(v) - act(y)| <= L pre + F(v),   L = |act'(y)| + pre max|act''|   (max|act''| = 0.851 QuickGELU, 0.798 GELU)
    F, the formula's own error, derived from the kernels' expressions (act_fn / act4_fast in tower_kernels.hip):
        fast (bf16 / e4m3 output) QuickGELU  x rcp(1 + exp2(x * -1.702 log2 e)): exp2 and rcp 1 ulp each, the exponent argument
                                  two roundings (constant + product, amplified by 1.702 |x|)          F = (3.5 |x| + 8) u |act|
        fast GELU  0.5 x (1 + sign(x) erf_AS(|x| / sqrt 2)): the Abramowitz & Stegun 7.1.26 erf (|err| <= 1.5e-7 absolute) with rcp
                   and exp2 1 ulp each, the 4-step Horner polynomial (sum |a_i| t^i <= 4.5) and the exponent argument z^2 log2 e
                   (z^2 erfc(z) <= 0.16) together <= 40 u absolute on erf, the final add and multiply 2u of the result:
                                                                              F = 0.5 |x| (1.5e-7 + 40 u) + 4 u |act|
        f32 QuickGELU  x / (1 + __expf(-1.702 x)): four roundings in the exponent, 1 ulp exp, IEEE division
                                                                              F = (8 |x| + 8) u |act|
        f32 GELU       0.5 x (1 + erff(x / sqrt 2)), erff within 2 ulp            F = 0.5 |x| 16 u + 4 u |act|
    The absolute terms matter in the negative tail: below x ~ -4 an erf error of 1.5e-7 is a large RELATIVE error of GELU(x), so a
    purely relative bound would be wrong there.  (Valid for x > -50: below that exp2 overflows to inf and the fast QuickGELU returns
    -0 against a reference of ~1e-37; no test input goes there.)
  * output rounding (|out| <= |ref| + pre'):
        bf16   (1 + 2^-8) pre' + 2^-8 |ref|
        e4m3   (1 + 2^-4) pre' + 2^-4 |ref| + 2^-10     (3 mantissa bits, subnormal spacing 2^-9; ref saturated to +-448 first)
        f32    pre'   (EPI_F32, RESID, PATCH and float32 STORE: no rounding after the ones counted above)

For float32 outputs at large K this worst-case accumulation bound can be looser than the norm-wise 2e-5 max(1, |ref|max) the older
tests assert, so the per-element bound is checked NEXT TO those assertions, never instead of them.

tests/test_gemm_ref_cpu.py checks on the CPU that a numpy emulation of a correct kernel stays inside the bound with margin (and
reaches a stated fraction of it on bf16 output), and that the typical GEMM faults (truncation instead of round to nearest even, bias
after the rounding, the activation on a rounded value, a dropped K chunk, a transposed fragment, a shifted ragged tail, a wrong
position row or image, a written token-0 row, a wrong skip, an overwritten residual, a neighbouring colscale) leave it.
"""
import math

import numpy as np
import torch

U = 2.0 ** -24
QUICK, GELU = 0, 1                   # IVR_ACT_*
STORE, RESID, PATCH, F32 = 0, 1, 2, 3  # EPI_*
C2 = {QUICK: 0.851, GELU: 0.798}     # max |act''|


def decode(t):
    """Operand or output tensor as the kernel stores it (bf16, float8_e4m3fn / e4m3 bytes as uint8, float32) -> float64."""
    if t.dtype == torch.uint8:
        t = t.view(torch.float8_e4m3fn)
    if t.dtype == torch.float8_e4m3fn:
        t = t.to(torch.float32)
    return t.to(torch.float64)


def chain(dtype, K):
    """Length c of the longest rounding chain of one fp32 accumulator (module docstring), dtype 'bf16', 'f32' or 'e4m3'."""
    return {"bf16": K / 32 + 6, "f32": K / 4 + 4, "e4m3": K / 128 + 8}[dtype]


def acc_coef(dtype, K):
    """Coefficient of A = sum |x w| in the accumulation bound: 2 c u, plus 2^-15 for the e4m3 MFMA (module docstring)."""
    return 2 * chain(dtype, K) * U + (2.0 ** -15 if dtype == "e4m3" else 0.0)


def act_exact(y, act):
    if act == QUICK:
        return y * torch.sigmoid(1.702 * y)
    if act == GELU:
        return 0.5 * y * (1.0 + torch.erf(y / math.sqrt(2.0)))
    return y


def act_deriv(y, act):
    if act == QUICK:
        s = torch.sigmoid(1.702 * y)
        return s + 1.702 * y * s * (1 - s)
    phi = torch.exp(-0.5 * y * y) / math.sqrt(2 * math.pi)
    return 0.5 * (1.0 + torch.erf(y / math.sqrt(2.0))) + y * phi


def act_formula_err(x, a, act, fast):
    """F(x) of the module docstring: |x| is the magnitude of the pre-activation, a = |act| there."""
    if act == QUICK:
        return ((3.5 * x + 8) * U * a) if fast else ((8 * x + 8) * U * a)
    return (0.5 * x * (1.5e-7 + 40 * U) + 4 * U * a) if fast else (0.5 * x * 16 * U + 4 * U * a)


def gemm_ref(x, w, K=None, colscale=None, bias=None):
    """Decoded operands x [M, >=K], w [N, >=K] (strided columns beyond K ignored) -> (y [M, N], A [M, N] = |x| |w|^T, s [N] or None,
    acc [M, N] = x w^T before colscale) in float64 on x's device."""
    xd, wd = decode(x), decode(w).to(x.device)
    if K is not None:
        xd, wd = xd[:, :K], wd[:, :K]
    acc = xd @ wd.T
    A = xd.abs() @ wd.abs().T
    s = None
    y = acc
    if colscale is not None:
        s = colscale.to(torch.float64).to(x.device)
        y = acc * s
    if bias is not None:
        y = y + bias.to(torch.float64).to(x.device)
    return y, A, s, acc


def bound(y, A, s, acc, dtype, K, out_kind, act=-1, r=None):
    """(ref, per-element bound of |out - ref|) for pre-activation reference y (gemm_ref) of a kernel with operand dtype `dtype`
    ('bf16', 'f32', 'e4m3'), output kind 'bf16', 'e4m3' or 'f32', activation act (-1 none), and r = the residual / position rows
    added by RESID / PATCH (float64, same shape) or None."""
    pre = acc_coef(dtype, K) * A
    if s is not None:
        pre = pre * s.abs() + 2 * U * (acc * s).abs()
    pre = pre + 2 * U * y.abs()
    ref = y
    if r is not None:
        ref = r + y
        pre = pre + 2 * U * ref.abs()
    if act >= 0:
        ref = act_exact(y, act)
        L = act_deriv(y, act).abs() + pre * C2[act]
        pre = L * pre + act_formula_err(y.abs() + pre, ref.abs() + L * pre, act, fast=(out_kind != "f32"))
    pre = pre * (1 + 1e-3)                  # second-order terms of the first-order bounds above
    if out_kind == "bf16":
        return ref, (1 + 2.0 ** -8) * pre + 2.0 ** -8 * ref.abs()
    if out_kind == "e4m3":
        ref = ref.clamp(-448.0, 448.0)
        return ref, (1 + 2.0 ** -4) * pre + 2.0 ** -4 * ref.abs() + 2.0 ** -10
    if out_kind == "f32":
        return ref, pre
    raise ValueError(out_kind)


def error_ratio(out, x, w, dtype, out_kind, K=None, colscale=None, bias=None, act=-1, r=None):
    """max over elements of |out - ref| / bound (<= 1 passes) of a dense [M, N] output (STORE / F32; RESID and PATCH: pass the
    residual or position rows the kernel added as r, [M, N])."""
    K = x.shape[1] if K is None else K
    y, A, s, acc = gemm_ref(x, w, K, colscale, bias)
    if r is not None:
        r = r.to(torch.float64).to(y.device)
    ref, b = bound(y, A, s, acc, dtype, K, out_kind, act, r)
    err = (decode(out).to(ref.device) - ref).abs()
    return float((err / b).max())


def ratio_map(out, ref, b):
    """Elementwise |out - ref| / bound in float64 (NaN in out gives NaN: callers compare with <= 1, which NaN fails)."""
    return (decode(out).to(ref.device) - ref).abs() / b


def round_to(t, kind):
    """float64 tensor -> nearest value of the output dtype (round to nearest even; e4m3 saturated first), as float64."""
    if kind == "e4m3":
        return t.clamp(-448, 448).to(torch.float8_e4m3fn).to(torch.float64)
    if kind == "bf16":                       # (callers pass values exact in float32: no double rounding through float32)
        return t.to(torch.float32).to(torch.bfloat16).to(torch.float64)
    return t.to(torch.float32).to(torch.float64)


def patch_rows(M, T, G2):
    """Residual row of GEMM row m under EPI_PATCH: (m / G2) T + 1 + m % G2 (int64 tensor)."""
    m = torch.arange(M, dtype=torch.int64)
    return (m // G2) * T + 1 + m % G2


def bits(t):
    """Raw bits of a tensor as an integer tensor of the same element size (NaN sentinels compare equal to themselves)."""
    return t.contiguous().view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def expect(before, x, w, *, dtype, out_kind, epi, N, K, act=-1, bias=None, colscale=None, pos=None, T=0, G2=0, skip_mod=0):
    """Whole output buffer after one correct call: `before` [rows, ld] is the buffer as the call found it (any dtype; STORE / F32:
    out [M, ldo]; RESID: resid viewed as [M, ldr]; PATCH: resid [(M / G2) T, ldr]).  Returns (ref, bound, written) [rows, ld]
    float64 / float64 / bool on x's device: where `written`, |out - ref| <= bound; elsewhere the bits must not change (columns
    beyond N, rows beyond M, skipped rows, token-0 rows)."""
    dev = x.device
    M = x.shape[0]
    y, A, s, acc = gemm_ref(x, w, K, colscale, bias)
    y, A, acc = y[:, :N], A[:, :N], acc[:, :N]
    s = s[:N] if s is not None else None
    prev = decode(before).to(dev)
    ref = prev.clone()
    bnd = torch.zeros_like(prev)
    written = torch.zeros(prev.shape, dtype=torch.bool, device=dev)
    if epi in (STORE, F32):
        r_, b_ = bound(y, A, s, acc, dtype, K, out_kind, act)
        rows = torch.arange(M, device=dev)
    elif epi == RESID:
        r_, b_ = bound(y, A, s, acc, dtype, K, "f32", -1, prev[:M, :N])
        rows = torch.arange(M, device=dev)
        if skip_mod:
            keep = rows % skip_mod != 0
            rows, r_, b_ = rows[keep], r_[keep], b_[keep]
    elif epi == PATCH:
        m = torch.arange(M, device=dev)
        r_, b_ = bound(y, A, s, acc, dtype, K, "f32", -1, pos.to(torch.float64).to(dev)[1 + m % G2, :N])
        rows = patch_rows(M, T, G2).to(dev)
    else:
        raise ValueError(epi)
    ref[rows, :N] = r_
    bnd[rows, :N] = b_
    written[rows, :N] = True
    return ref, bnd, written


def verify(after, before, exp):
    """(largest |out - ref| / bound over the written elements, number of unwritten elements whose bits changed)."""
    ref, bnd, written = exp
    a = decode(after).to(ref.device)
    r = ((a - ref).abs() / bnd)[written]
    ratio = float(r.max()) if r.numel() else 0.0
    if torch.isnan(r).any():
        ratio = float("inf")
    changed = int((bits(after) != bits(before)).to(ref.device)[~written].sum())
    return ratio, changed
