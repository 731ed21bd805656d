"""MXFP4 weights x activations quantised to MXFP8 (E4M3 elements, E8M0 block scales) on the fly (csrc/mxfp4_a8.hip), contracted on the
block-scaled matrix instructions with an FP4 and an E4M3 operand.  The format and the arithmetic are this library's own
(include/bie_hip.h, INTEGRATION.md "MXFP4 W4A8 linear layer"):

  xq uint8 [M, K] (row-major e4m3fn bytes), xs uint8 [M, K/32] = x per row and block of 32 by the OCP MX v1.0 rule with emax = 8
  row_flag uint8 [M] = the row holds NaN / inf
  y[m, n] = dt( sum_b 2^(xs[m,b] + scales[n,b] - 254) * (sum_{k in b} e4m3(xq) * e2m1(qweight)) + bias[n] ),  NaN for a flagged row

The weight side (quantize / dequant / col_exp) is mxfp4_linear_cuda's: the weights are the same bytes.  quantize_act quantises x, gemm
contracts already-quantised activations, forward does both, dequant_act restates x^ in torch.  Nothing here synchronises with the host,
so every entry can be captured in a graph."""
import torch

from bitorch_engine import _hip
from bitorch_engine.extensions.mxfp4_linear_cuda import _X_DT, _aligned, _shape, col_exp, dequant, quantize  # noqa: F401


def quantize_act(x: torch.Tensor):
    """x [M, K] (fp16 / bf16) -> (xq uint8 [M, K], xs uint8 [M, K/32], row_flag uint8 [M])."""
    _hip.need_gpu(x)
    if x.dtype not in _X_DT or x.dim() != 2:
        raise RuntimeError(f"mxfp4 a8: x must be fp16 / bf16 [M, K] (got {x.dtype} {tuple(x.shape)})")
    M, K = x.shape
    xq = torch.empty((M, K), dtype=torch.uint8, device=x.device)
    xs = torch.empty((M, K // 32), dtype=torch.uint8, device=x.device)
    flag = torch.empty(M, dtype=torch.uint8, device=x.device)
    if M == 0:
        return xq, xs, flag
    x = _aligned(x)
    _hip.check(_hip.lib().bie_mxfp8_quantize_act(_hip.ptr(x), _hip.ptr(xq), _hip.ptr(xs), _hip.ptr(flag), M, K, _hip.dt(x), _hip.stream()),
               "bie_mxfp8_quantize_act")
    return xq, xs, flag


def dequant_act(xq: torch.Tensor, xs: torch.Tensor, dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """x^ [M, K] in dtype from the quantised activations, in torch: e4m3(xq) * 2^(xs - 127)."""
    s = torch.exp2(xs.to(torch.float32) - 127.0).repeat_interleave(32, dim=1)
    return (xq.view(torch.float8_e4m3fn).to(torch.float32) * s).to(dtype)


def form(M: int, N: int, K: int, dtype: torch.dtype = torch.float16) -> int:
    """0 = decode form, 1 = prefill form (bie_mxfp4_a8_form)."""
    return int(_hip.lib().bie_mxfp4_a8_form(M, N, K, _hip._DT[dtype]))


def _bias(bias, dtype):
    return None if bias is None else bias.reshape(-1).to(dtype=dtype).contiguous()


def _act_shape(xq, xs):
    """(M, K) of a quantised activation pair; raises on anything that is not uint8 [M, K] / [M, K/32]."""
    if xq.dtype != torch.uint8 or xs.dtype != torch.uint8 or xq.dim() != 2 or xs.dim() != 2 or xq.shape[0] != xs.shape[0] \
            or xq.shape[1] != 32 * xs.shape[1]:
        raise RuntimeError(f"mxfp4 a8: xq {xq.dtype} {tuple(xq.shape)} / xs {xs.dtype} {tuple(xs.shape)} are not uint8 [M, K] / [M, K/32]")
    return tuple(xq.shape)


def forward(x: torch.Tensor, qweight: torch.Tensor, scales: torch.Tensor, bias: torch.Tensor = None, e_col: torch.Tensor = None,
            form: int = -1) -> torch.Tensor:
    """x [M, K] (fp16 / bf16) -> y [M, N] in x's dtype: quantise x, then the contraction.  form -1 = the plan.  e_col (col_exp(scales)) is
    computed here when it is not given."""
    _hip.need_gpu(x, qweight, scales, bias, e_col)
    if x.dtype not in _X_DT:
        raise RuntimeError(f"mxfp4 a8 linear: dtype {x.dtype} is not supported (fp16 / bf16)")
    N, K = _shape(qweight, scales)
    if x.dim() != 2 or x.shape[1] != K:
        raise RuntimeError(f"mxfp4 a8 linear: x {tuple(x.shape)} does not match K={K}")
    M = x.shape[0]
    y = torch.empty((M, N), dtype=x.dtype, device=x.device)
    if M == 0:
        return y
    L = _hip.lib()
    if e_col is None:
        e_col = col_exp(scales)
    ws = torch.empty(int(L.bie_mxfp4_a8_workspace_bytes(M, N, K, int(form))), dtype=torch.uint8, device=x.device)
    bias = _bias(bias, x.dtype)
    x, qweight, scales = _aligned(x), _aligned(qweight), scales.contiguous()  # held until the launches are queued
    _hip.check(L.bie_mxfp4_a8_linear_forward(_hip.ptr(x), _hip.ptr(qweight), _hip.ptr(scales), _hip.ptr(e_col), _hip.ptr(bias), _hip.ptr(y), _hip.ptr(ws),
                                             M, N, K, _hip.dt(x), int(form), _hip.stream()), "bie_mxfp4_a8_linear_forward")
    return y


def gemm(xq: torch.Tensor, xs: torch.Tensor, row_flag: torch.Tensor, qweight: torch.Tensor, scales: torch.Tensor, bias: torch.Tensor = None,
         e_col: torch.Tensor = None, dtype: torch.dtype = torch.float16, form: int = -1) -> torch.Tensor:
    """The contraction from already-quantised activations (xq uint8 [M, K], xs uint8 [M, K/32], row_flag uint8 [M]) -> y [M, N] in dtype."""
    _hip.need_gpu(xq, xs, row_flag, qweight, scales, bias, e_col)
    if dtype not in _X_DT:
        raise RuntimeError(f"mxfp4 a8 gemm: dtype {dtype} is not supported (fp16 / bf16)")
    N, K = _shape(qweight, scales)
    M = xq.shape[0]
    if _act_shape(xq, xs) != (M, K) or row_flag.dtype != torch.uint8 or tuple(row_flag.shape) != (M,):
        raise RuntimeError(f"mxfp4 a8 gemm: xq {tuple(xq.shape)} / xs {tuple(xs.shape)} / row_flag {tuple(row_flag.shape)} do not match K={K}")
    y = torch.empty((M, N), dtype=dtype, device=xq.device)
    if e_col is None:
        e_col = col_exp(scales)
    bias = _bias(bias, dtype)
    xq, xs, row_flag, qweight, scales = _aligned(xq), xs.contiguous(), row_flag.contiguous(), _aligned(qweight), scales.contiguous()
    _hip.check(_hip.lib().bie_mxfp4_a8_gemm(_hip.ptr(xq), _hip.ptr(xs), _hip.ptr(row_flag), _hip.ptr(qweight), _hip.ptr(scales), _hip.ptr(e_col),
                                            _hip.ptr(bias), _hip.ptr(y), None, M, N, K, _hip._DT[dtype], int(form), _hip.stream()), "bie_mxfp4_a8_gemm")
    return y
