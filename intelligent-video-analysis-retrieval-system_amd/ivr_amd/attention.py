"""Attention and LayerNorm of the towers as building blocks (ivr_attention, ivr_qkv_attention, ivr_layernorm): parity tests and
kernel benchmarks."""
import torch

from . import _ffi

OUT_BF16, OUT_F32, OUT_FP8 = 0, 1, 2


def attention(qkv, T, heads, causal=False, out_fp8=False):
    """qkv [n*T, 3D] CUDA tensor, bf16 or float32 (row = q | k | v, head h at columns h*64 .. h*64+63 of each part) ->
    att [n*T, D]: bf16 or float8_e4m3fn (out_fp8) for bf16 input, float32 for float32 input.  No 1/sqrt(64) scale."""
    if qkv.dtype not in (torch.bfloat16, torch.float32):
        raise ValueError("qkv must be bf16 or float32")
    if qkv.dim() != 2 or qkv.shape[1] % 3 or T < 1 or qkv.shape[0] % T:
        raise ValueError(f"qkv must be [n*T, 3D]; got {tuple(qkv.shape)} with T={T}")
    f32 = qkv.dtype == torch.float32
    if f32 and out_fp8:
        raise ValueError("e4m3 output only from bf16 operands")
    qkv = qkv.contiguous()
    rows, D = qkv.shape[0], qkv.shape[1] // 3
    odt = torch.float32 if f32 else torch.uint8 if out_fp8 else torch.bfloat16
    att = torch.empty((rows, D), dtype=odt, device=qkv.device)
    _ffi.call("ivr_attention", _ffi.CTX, f32, qkv, rows // T, int(T), D, int(heads), bool(causal), bool(out_fp8), att, device=qkv.device)
    return att.view(torch.float8_e4m3fn) if out_fp8 else att


def qkv_attention(xn, w, bias, T, heads, out_fp8=False):
    """Fused projection + attention: xn bf16 [n*T, D], w bf16 [3D, D], bias float32 [3D] -> attention of (xn w^T + bias rounded
    to bf16), not causal; bf16 or float8_e4m3fn [n*T, D]."""
    if xn.dtype != torch.bfloat16 or w.dtype != torch.bfloat16 or bias.dtype != torch.float32:
        raise ValueError("xn and w must be bf16, bias float32")
    if xn.dim() != 2 or T < 1 or xn.shape[0] % T:
        raise ValueError(f"xn must be [n*T, D]; got {tuple(xn.shape)} with T={T}")
    rows, D = xn.shape
    if tuple(w.shape) != (3 * D, D) or tuple(bias.shape) != (3 * D,):
        raise ValueError(f"w must be [3D, D] and bias [3D] for D={D}")
    xn, w, bias = xn.contiguous(), w.contiguous(), bias.contiguous()
    att = torch.empty((rows, D), dtype=torch.uint8 if out_fp8 else torch.bfloat16, device=xn.device)
    _ffi.call("ivr_qkv_attention", _ffi.CTX, xn, w, bias, rows // T, int(T), D, int(heads), bool(out_fp8), att, device=xn.device)
    return att.view(torch.float8_e4m3fn) if out_fp8 else att


def layernorm(x, g, b, eps, out_kind, row_mul=1, offs=None, reverse=False):
    """out row r = LN(x row r*row_mul + offs[r]) with x float32 [R, D], g / b float32 [D], offs int32 [rows] or None;
    out_kind OUT_BF16 / OUT_F32 / OUT_FP8 -> bf16 / float32 / float8_e4m3fn [rows, D].  rows = len(offs), or without offsets
    ceil(R / row_mul) (every row_mul-th row); every source row must lie inside x."""
    if x.dtype != torch.float32 or g.dtype != torch.float32 or b.dtype != torch.float32:
        raise ValueError("x, g and b must be float32")
    if x.dim() != 2 or tuple(g.shape) != (x.shape[1],) or tuple(b.shape) != (x.shape[1],):
        raise ValueError("x must be [R, D], g and b [D]")
    if out_kind not in (OUT_BF16, OUT_F32, OUT_FP8):
        raise ValueError(f"out_kind={out_kind}")
    if offs is not None and offs.dtype != torch.int32:
        raise ValueError("offs must be int32")
    x, g, b = x.contiguous(), g.contiguous(), b.contiguous()
    R, D = x.shape
    if row_mul < 1 or (offs is not None and offs.dim() != 1):
        raise ValueError("row_mul must be >= 1 and offs one-dimensional")
    rows = offs.shape[0] if offs is not None else (R + row_mul - 1) // row_mul
    if offs is not None:
        offs = offs.contiguous()
        src = torch.arange(rows, device=offs.device, dtype=torch.int64) * row_mul + offs.to(torch.int64)
        if rows and (int(src.min()) < 0 or int(src.max()) >= R):
            raise ValueError("a gathered source row lies outside x")
    odt = {OUT_BF16: torch.bfloat16, OUT_F32: torch.float32, OUT_FP8: torch.uint8}[out_kind]
    out = torch.empty((rows, D), dtype=odt, device=x.device)
    _ffi.call("ivr_layernorm", _ffi.CTX, int(out_kind), x, int(row_mul), offs, g, b, float(eps), int(rows), int(D), bool(reverse), out,
              device=x.device)
    return out.view(torch.float8_e4m3fn) if out_kind == OUT_FP8 else out
