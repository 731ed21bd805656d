"""MXFP6 (OCP microscaling FP6, E2M3 elements) weights x activations quantised to the SAME format on the fly (csrc/mxfp6_a6.hip),
contracted on the block-scaled matrix instructions with two FP6 operands.  The format and the arithmetic are this library's own
(include/bie_hip.h, INTEGRATION.md "MXFP6 W6A6 linear layer"):

  qweight uint8 [N, 3K/4], scales uint8 [N, K/32]: the MXFP6 weight of mxfp6_a8_linear_cuda, unchanged
  xq6 uint8 [M, 3K/4], xs uint8 [M, K/32]: x in the weight's format (24-byte blocks, code j in bits 6 j .. 6 j + 5; E8M0 scales), by the
      weight quantiser's rule; row_flag uint8 [M] = the row holds NaN / inf
  y[m, n] = dt( sum_b 2^(xs[m,b] + scales[n,b] - 254) * (sum_{k in b} e2m3(xq6) * e2m3(qweight)) + bias[n] ),  NaN for a flagged row

quantize / dequant / col_exp / blk_exp / grad_input are the objects of the existing MXFP6 / MXFP4 modules (the weights and the scales are
the same bytes); dequant decodes activations too (dequant_act is dequant).  quantize_act quantises x, gemm contracts already-quantised
activations, forward does both.  Nothing here synchronises with the host, so every entry can be captured in a graph."""
import torch

from bitorch_engine import _hip
from bitorch_engine.extensions import _mx_scaled
from bitorch_engine.extensions.mxfp4_linear_cuda import _X_DT, _aligned, blk_exp, col_exp  # noqa: F401
from bitorch_engine.extensions.mxfp4_a8_linear_cuda import _bias
from bitorch_engine.extensions.mxfp6_a8_linear_cuda import _shape, dequant, grad_input, quantize  # noqa: F401

dequant_act = dequant


def quantize_act(x: torch.Tensor):
    """x [M, K] (fp16 / bf16) -> (xq6 uint8 [M, 3K/4], xs uint8 [M, K/32], row_flag uint8 [M])."""
    _hip.need_gpu(x)
    if x.dtype not in _X_DT or x.dim() != 2:
        raise RuntimeError(f"mxfp6 a6: x must be fp16 / bf16 [M, K] (got {x.dtype} {tuple(x.shape)})")
    M, K = x.shape
    xq = torch.empty((M, K // 32 * 24), dtype=torch.uint8, device=x.device)
    xs = torch.empty((M, K // 32), dtype=torch.uint8, device=x.device)
    flag = torch.empty(M, dtype=torch.uint8, device=x.device)
    if M == 0:
        return xq, xs, flag
    x = _aligned(x)
    _hip.check(_hip.lib().bie_mxfp6_quantize_act(_hip.ptr(x), _hip.ptr(xq), _hip.ptr(xs), _hip.ptr(flag), M, K, _hip.dt(x), _hip.stream()),
               "bie_mxfp6_quantize_act")
    return xq, xs, flag


_LAYER = _mx_scaled.Dense("mxfp6_a6", "mxfp6 a6", 24, _shape, col_exp)


def form(M: int, N: int, K: int, dtype: torch.dtype = torch.float16) -> int:
    """0 = decode form, 1 = prefill form (bie_mxfp6_a6_form)."""
    return _LAYER.form(M, N, K, dtype)


def forward(x: torch.Tensor, qweight: torch.Tensor, scales: torch.Tensor, bias: torch.Tensor = None, e_col: torch.Tensor = None,
            form: int = -1) -> torch.Tensor:
    """x [M, K] (fp16 / bf16) -> y [M, N] in x's dtype: quantise x, then the contraction.  form -1 = the plan.  e_col (col_exp(scales)) is
    computed here when it is not given."""
    return _LAYER.forward(x, qweight, scales, bias, e_col, form)


def gemm(xq6: torch.Tensor, xs: torch.Tensor, row_flag: torch.Tensor, qweight: torch.Tensor, scales: torch.Tensor, bias: torch.Tensor = None,
         e_col: torch.Tensor = None, dtype: torch.dtype = torch.float16, form: int = -1) -> torch.Tensor:
    """The contraction from already-quantised activations (xq6 uint8 [M, 3K/4], xs uint8 [M, K/32], row_flag uint8 [M]) -> y [M, N] in dtype."""
    return _LAYER.gemm(xq6, xs, row_flag, qweight, scales, bias, e_col, dtype, form)
