"""The expert GEMM of a mixture-of-experts MLP on stacked MXFP6 weights (OCP microscaling FP6, E2M3 elements) against activations
quantised to the SAME format on the fly (csrc/mxfp6_moe_a6.hip), contracted on the block-scaled matrix instructions with two FP6
operands.  The format and the arithmetic are this library's own (include/bie_hip.h, INTEGRATION.md "MXFP6 W6A6 mixture-of-experts
layer"):

  qweight uint8 [E, N, 3K/4] (per row K/32 blocks of 24 bytes, mxfp6_a8_linear_cuda's bit order), scales uint8 [E, N, K/32], bias [E, N]
  idx int32 [T, S]: the expert of every (token, slot) pair; an index outside [0, E) (-1 by convention) is a skipped slot
  xq6, xs, row_flag = quantize_act of the stored rows of x: x [T, K] (every slot of a token reads the token's row) or x [T, S, K]
  y[t, s] = dt( sum_b 2^(xs[row, b] + scales[e, n, b] - 254) * (sum_{k in b} e2m3(xq6) * e2m3(qweight)) + bias[e] ),  e = idx[t, s]
  y[t, s] = NaN for a row of x that holds NaN / inf, +0 for a skipped slot whatever its row holds

quantize / dequant / col_exp / blk_exp / grad_input are mxfp6_experts_a8_cuda's objects (the weights are the same bytes); quantize_act /
dequant_act are mxfp6_a6_linear_cuda's.  Nothing here synchronises with the host (the routing is read on the device), so every entry can
be captured in a graph."""
import torch

from bitorch_engine.extensions import _mx_scaled
from bitorch_engine.extensions.mxfp6_a6_linear_cuda import dequant_act, quantize_act  # noqa: F401
from bitorch_engine.extensions.mxfp6_experts_a8_cuda import _bias, _idx, _shape, blk_exp, col_exp, dequant, grad_input, quantize  # noqa: F401


_LAYER = _mx_scaled.Experts("mxfp6_moe_a6", "mxfp6 a6", 24, _shape, col_exp)


def form(P: int, E: int, N: int, K: int, dtype: torch.dtype = torch.float16) -> int:
    """0 = routed decode form, 1 = grouped prefill form (bie_mxfp6_moe_a6_form); P = the number of (token, slot) pairs."""
    return _LAYER.form(P, E, N, K, dtype)


def forward(x: torch.Tensor, idx: torch.Tensor, qweight: torch.Tensor, scales: torch.Tensor, bias: torch.Tensor = None, e_col: torch.Tensor = None,
            form: int = -1) -> torch.Tensor:
    """x [T, K] or [T, S, K] (fp16 / bf16), idx int32 [T, S] -> y [T, S, N] in x's dtype: quantise the rows of x, then the contraction.
    form -1 = the plan.  e_col (col_exp(scales)) is computed here when it is not given."""
    return _LAYER.forward(x, idx, qweight, scales, bias, e_col, form)


def gemm(xq6: torch.Tensor, xs: torch.Tensor, row_flag: torch.Tensor, idx: torch.Tensor, qweight: torch.Tensor, scales: torch.Tensor,
         bias: torch.Tensor = None, e_col: torch.Tensor = None, dtype: torch.dtype = torch.float16, form: int = -1) -> torch.Tensor:
    """The contraction from already-quantised activations: xq6 uint8 [R, 3K/4], xs uint8 [R, K/32], row_flag uint8 [R] with R = T (every
    slot of a token reads the token's row) or R = T * S (a row per pair, in pair order) -> y [T, S, N] in dtype.  Form 0 here is the
    routed kernel reading xq6 from memory."""
    return _LAYER.gemm(xq6, xs, row_flag, idx, qweight, scales, bias, e_col, dtype, form)
