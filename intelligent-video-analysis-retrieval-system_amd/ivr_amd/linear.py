"""y = x W^T + b on the tower GEMM kernel (ivr_linear): parity tests and kernel benchmarks."""
import torch

from . import _ffi

EPI_STORE, EPI_RESID, EPI_F32 = 0, 1, 3


def linear(x, w, bias=None, act=-1, epilogue=EPI_STORE, resid=None):
    """x [M,K], w [N,K] CUDA tensors, both bf16 or both float32; bias float32 [N] or None."""
    if x.dtype != w.dtype or x.dtype not in (torch.bfloat16, torch.float32):
        raise ValueError("x and w must both be bf16 or both float32")
    x, w = x.contiguous(), w.contiguous()
    M, K = x.shape
    N = w.shape[0]
    f32 = x.dtype == torch.float32
    out = None
    if epilogue == EPI_STORE:
        out = torch.empty((M, N), dtype=x.dtype, device=x.device)
    elif epilogue == EPI_F32:
        out = torch.empty((M, N), dtype=torch.float32, device=x.device)
    elif resid is None or resid.dtype != torch.float32 or tuple(resid.shape) != (M, N):
        raise ValueError("EPI_RESID needs a float32 [M,N] residual tensor")
    _ffi.call("ivr_linear", _ffi.CTX, f32, int(epilogue), x, w, bias, M, N, K, int(act), out, resid, device=x.device)
    return resid if epilogue == EPI_RESID else out


def quantize_rows_e4m3(w):
    """float32 [N,K] -> (e4m3 bytes as uint8 [N,K], float32 scale [N]) with one scale per row (absmax / 448): the weight
    format of the fp8 tower mode, restated with torch's float8_e4m3fn conversion (round to nearest even, saturating)."""
    amax = w.abs().amax(dim=1)
    scale = torch.where(amax > 0, amax / 448.0, torch.ones_like(amax)).to(torch.float32)
    q = (w / scale[:, None]).clamp(-448.0, 448.0).to(torch.float8_e4m3fn)
    return q.view(torch.uint8), scale


def linear_fp8(x8, w8, colscale=None, bias=None, act=-1, epilogue=EPI_STORE, out_fp8=False, resid=None):
    """x8 [M,K], w8 [N,K]: e4m3 bytes (uint8 or float8_e4m3fn CUDA tensors); y = (x8 w8^T) * colscale + bias."""
    x8, w8 = x8.contiguous(), w8.contiguous()
    M, K = x8.shape
    N = w8.shape[0]
    out = None
    if epilogue == EPI_STORE:
        out = torch.empty((M, N), dtype=torch.uint8 if out_fp8 else torch.bfloat16, device=x8.device)
    elif resid is None or resid.dtype != torch.float32 or tuple(resid.shape) != (M, N):
        raise ValueError("EPI_RESID needs a float32 [M,N] residual tensor")
    _ffi.call("ivr_linear_fp8", _ffi.CTX, int(epilogue), x8, w8, colscale, bias, M, N, K, int(act), out, bool(out_fp8), resid,
              device=x8.device)
    if epilogue == EPI_RESID:
        return resid
    return out.view(torch.float8_e4m3fn) if out_fp8 else out


EPI_PATCH = 2
DTYPE = {torch.bfloat16: 0, torch.float32: 1, torch.float8_e4m3fn: 2, torch.uint8: 2}


def gemm(a, w, *, M=None, N=None, K=None, lda=None, ldw=None, epilogue=EPI_STORE, act=-1, bias=None, colscale=None, out=None, ldo=None,
         out8=False, resid=None, ldr=None, pos=None, T=0, G2=0, skip_mod=0, reverse_m=0, stream=None):
    """ivr_gemm: one call of the towers' GEMM with every GemmArgs field the towers set (strided operands and outputs, the patch
    epilogue, skipped residual rows, reversed row order).  a, w: CUDA tensors of the operand dtype (bf16, float32, or e4m3 as
    float8_e4m3fn / uint8) whose storage holds [M, lda] and [N, ldw]; the outputs are written in place into `out` / `resid`, which the
    caller allocates (and may fill with sentinels).  M, N, K and the leading dimensions default to the dense shapes of a and w."""
    dt = DTYPE.get(a.dtype)
    if dt is None or DTYPE.get(w.dtype) != dt:
        raise ValueError("a and w must share one of bf16, float32, e4m3")
    M = a.shape[0] if M is None else M
    N = w.shape[0] if N is None else N
    K = a.shape[1] if K is None else K
    ptr = lambda t: t.data_ptr() if t is not None else None   # noqa: E731  (the fields of a ctypes struct take raw addresses)
    d = _ffi.GemmDesc(dtype=dt, epilogue=int(epilogue), act=int(act), M=int(M), N=int(N), K=int(K),
                      A=ptr(a), lda=int(a.stride(0) if lda is None else lda), W=ptr(w), ldw=int(w.stride(0) if ldw is None else ldw),
                      bias=ptr(bias), colscale=ptr(colscale), out=ptr(out),
                      ldo=int(ldo if ldo is not None else (out.stride(0) if out is not None else 0)), out8=int(bool(out8)),
                      resid=ptr(resid), ldr=int(ldr if ldr is not None else (resid.stride(0) if resid is not None else 0)),
                      pos=ptr(pos), T=int(T), G2=int(G2), skip_mod=int(skip_mod), reverse_m=int(reverse_m))
    # stream=None leaves the slot out, so that call() fills it with the current stream of a.device (a None in the slot is the null stream)
    given = () if stream is None else (_ffi.stream_ptr(stream),)
    _ffi.call("ivr_gemm", _ffi.CTX, d, *given, device=a.device)
    return out if out is not None else resid
