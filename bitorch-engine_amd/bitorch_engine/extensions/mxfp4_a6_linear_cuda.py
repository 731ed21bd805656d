"""MXFP4 weights x activations quantised to MXFP6 (OCP E2M3 elements, E8M0 block scales) on the fly (csrc/mxfp4_a6.hip), contracted on the
block-scaled matrix instructions with an FP4 and an FP6 operand, which run at the FP4 rate.  The format and the arithmetic are this
library's own (include/bie_hip.h, INTEGRATION.md "MXFP4 W4A6 linear layer"):

  qweight uint8 [N, K/2], scales uint8 [N, K/32]: the MXFP4 weight of mxfp4_linear_cuda, unchanged
  xq6 uint8 [M, 3K/4], xs uint8 [M, K/32], row_flag uint8 [M]: the quantised activations of mxfp6_a6_linear_cuda, unchanged
  y[m, n] = dt( sum_b 2^(xs[m,b] + scales[n,b] - 254) * (sum_{k in b} e2m3(xq6) * e2m1(qweight)) + bias[n] ),  NaN for a flagged row

quantize / dequant / col_exp / blk_exp / grad_input are the objects of mxfp4_linear_cuda (the weights are the same bytes), quantize_act /
dequant_act those of mxfp6_a6_linear_cuda (the activations are the same bytes).  gemm contracts already-quantised activations, forward
quantises and contracts.  Nothing here synchronises with the host, so every entry can be captured in a graph."""
import torch

from bitorch_engine import _hip
from bitorch_engine.extensions.mxfp4_linear_cuda import _X_DT, _aligned, _shape, blk_exp, col_exp, dequant, grad_input, quantize  # noqa: F401
from bitorch_engine.extensions.mxfp4_a8_linear_cuda import _bias
from bitorch_engine.extensions.mxfp6_a6_linear_cuda import dequant_act, quantize_act  # noqa: F401


def form(M: int, N: int, K: int, dtype: torch.dtype = torch.float16) -> int:
    """0 = decode form, 1 = prefill form (bie_mx4a6_form)."""
    return int(_hip.lib().bie_mx4a6_form(M, N, K, _hip._DT[dtype]))


def forward(x: torch.Tensor, qweight: torch.Tensor, scales: torch.Tensor, bias: torch.Tensor = None, e_col: torch.Tensor = None,
            form: int = -1) -> torch.Tensor:
    """x [M, K] (fp16 / bf16) -> y [M, N] in x's dtype: quantise x, then the contraction.  form -1 = the plan.  e_col (col_exp(scales)) is
    computed here when it is not given."""
    _hip.need_gpu(x, qweight, scales, bias, e_col)
    if x.dtype not in _X_DT:
        raise RuntimeError(f"mxfp4 a6 linear: dtype {x.dtype} is not supported (fp16 / bf16)")
    N, K = _shape(qweight, scales)
    if x.dim() != 2 or x.shape[1] != K:
        raise RuntimeError(f"mxfp4 a6 linear: x {tuple(x.shape)} does not match K={K}")
    M = x.shape[0]
    y = torch.empty((M, N), dtype=x.dtype, device=x.device)
    if M == 0:
        return y
    L = _hip.lib()
    if e_col is None:
        e_col = col_exp(scales)
    ws = torch.empty(int(L.bie_mx4a6_workspace_bytes(M, N, K, int(form))), dtype=torch.uint8, device=x.device)
    bias = _bias(bias, x.dtype)
    x, qweight, scales = _aligned(x), _aligned(qweight), scales.contiguous()  # held until the launches are queued
    _hip.check(L.bie_mx4a6_linear_forward(_hip.ptr(x), _hip.ptr(qweight), _hip.ptr(scales), _hip.ptr(e_col), _hip.ptr(bias), _hip.ptr(y), _hip.ptr(ws),
                                          M, N, K, _hip.dt(x), int(form), _hip.stream()), "bie_mx4a6_linear_forward")
    return y


def gemm(xq6: torch.Tensor, xs: torch.Tensor, row_flag: torch.Tensor, qweight: torch.Tensor, scales: torch.Tensor, bias: torch.Tensor = None,
         e_col: torch.Tensor = None, dtype: torch.dtype = torch.float16, form: int = -1) -> torch.Tensor:
    """The contraction from already-quantised activations (xq6 uint8 [M, 3K/4], xs uint8 [M, K/32], row_flag uint8 [M]) -> y [M, N] in dtype."""
    _hip.need_gpu(xq6, xs, row_flag, qweight, scales, bias, e_col)
    if dtype not in _X_DT:
        raise RuntimeError(f"mxfp4 a6 gemm: dtype {dtype} is not supported (fp16 / bf16)")
    N, K = _shape(qweight, scales)
    M = xq6.shape[0]
    if xq6.dtype != torch.uint8 or xs.dtype != torch.uint8 or tuple(xq6.shape) != (M, K // 32 * 24) or tuple(xs.shape) != (M, K // 32) \
            or row_flag.dtype != torch.uint8 or tuple(row_flag.shape) != (M,):
        raise RuntimeError(f"mxfp4 a6 gemm: xq6 {tuple(xq6.shape)} / xs {tuple(xs.shape)} / row_flag {tuple(row_flag.shape)} are not uint8 "
                           f"[M, 3K/4] / [M, K/32] / [M] for K={K}")
    y = torch.empty((M, N), dtype=dtype, device=xq6.device)
    if M == 0:
        return y
    if e_col is None:
        e_col = col_exp(scales)
    bias = _bias(bias, dtype)
    xq6, xs, row_flag, qweight, scales = _aligned(xq6), xs.contiguous(), row_flag.contiguous(), _aligned(qweight), scales.contiguous()
    _hip.check(_hip.lib().bie_mx4a6_gemm(_hip.ptr(xq6), _hip.ptr(xs), _hip.ptr(row_flag), _hip.ptr(qweight), _hip.ptr(scales), _hip.ptr(e_col),
                                         _hip.ptr(bias), _hip.ptr(y), None, M, N, K, _hip._DT[dtype], int(form), _hip.stream()), "bie_mx4a6_gemm")
    return y
