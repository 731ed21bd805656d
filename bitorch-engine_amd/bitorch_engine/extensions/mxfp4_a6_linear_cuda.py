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

from bitorch_engine.extensions import _mx_scaled
from bitorch_engine.extensions.mxfp4_linear_cuda import _X_DT, _aligned, _shape, blk_exp, col_exp, dequant, grad_input, quantize  # noqa: F401
from bitorch_engine.extensions.mxfp4_a8_linear_cuda import _bias
from bitorch_engine.extensions.mxfp6_a6_linear_cuda import dequant_act, quantize_act  # noqa: F401


_LAYER = _mx_scaled.Dense("mx4a6", "mxfp4 a6", 24, _shape, col_exp)


def form(M: int, N: int, K: int, dtype: torch.dtype = torch.float16) -> int:
    """0 = decode form, 1 = prefill form (bie_mx4a6_form)."""
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
