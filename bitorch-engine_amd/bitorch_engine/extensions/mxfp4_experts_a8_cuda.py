"""The expert GEMM of a mixture-of-experts MLP on stacked MXFP4 weights against activations quantised to MXFP8 (E4M3 elements, E8M0 block
scales) on the fly (csrc/mxfp4_moe_a8.hip), contracted on the block-scaled matrix instructions with an FP4 and an E4M3 operand.  The
format and the arithmetic are this library's own (include/bie_hip.h, INTEGRATION.md "MXFP4 W4A8 mixture-of-experts layer"):

  qweight uint8 [E, N, K/2], scales uint8 [E, N, K/32], bias [E, N], idx int32 [T, S]: mxfp4_experts_cuda's
  xq, xs, row_flag = quantize_act of the stored rows of x: x [T, K] (every slot of a token reads the token's row) or x [T, S, K]
  y[t, s] = dt( sum_b 2^(xs[row, b] + scales[e, n, b] - 254) * (sum_{k in b} e4m3(xq) * e2m1(qweight)) + bias[e] ),  e = idx[t, s]
  y[t, s] = NaN for a row of x that holds NaN / inf, +0 for a skipped slot (idx outside [0, E)) whatever its row holds

The weight side (quantize / dequant / col_exp) is mxfp4_experts_cuda's and quantize_act / dequant_act are mxfp4_a8_linear_cuda's: the same bytes.
Nothing here synchronises with the host (the routing is read on the device), so every entry can be captured in a graph."""
import torch

from bitorch_engine.extensions import _mx_scaled
from bitorch_engine.extensions.mxfp4_a8_linear_cuda import dequant_act, quantize_act  # noqa: F401
from bitorch_engine.extensions.mxfp4_experts_cuda import _shape, col_exp, dequant, quantize  # noqa: F401


_LAYER = _mx_scaled.Experts("mxfp4_moe_a8", "mxfp4 a8", 32, _shape, col_exp)
_idx = _LAYER.idx
_bias = _mx_scaled._experts_bias


def form(P: int, E: int, N: int, K: int, dtype: torch.dtype = torch.float16) -> int:
    """0 = routed decode form, 1 = grouped prefill form (bie_mxfp4_moe_a8_form); P = the number of (token, slot) pairs."""
    return _LAYER.form(P, E, N, K, dtype)


def forward(x: torch.Tensor, idx: torch.Tensor, qweight: torch.Tensor, scales: torch.Tensor, bias: torch.Tensor = None, e_col: torch.Tensor = None,
            form: int = -1) -> torch.Tensor:
    """x [T, K] or [T, S, K] (fp16 / bf16), idx int32 [T, S] -> y [T, S, N] in x's dtype: quantise the rows of x, then the contraction.
    form -1 = the plan.  e_col (col_exp(scales)) is computed here when it is not given."""
    return _LAYER.forward(x, idx, qweight, scales, bias, e_col, form)


def gemm(xq: torch.Tensor, xs: torch.Tensor, row_flag: torch.Tensor, idx: torch.Tensor, qweight: torch.Tensor, scales: torch.Tensor,
         bias: torch.Tensor = None, e_col: torch.Tensor = None, dtype: torch.dtype = torch.float16, form: int = -1) -> torch.Tensor:
    """The contraction from already-quantised activations: xq uint8 [R, K] (e4m3fn bytes), xs uint8 [R, K/32], row_flag uint8 [R] with R = T (every
    slot of a token reads the token's row) or R = T * S (a row per pair, in pair order) -> y [T, S, N] in dtype.  Form 0 here is the
    routed kernel reading xq from memory."""
    return _LAYER.gemm(xq, xs, row_flag, idx, qweight, scales, bias, e_col, dtype, form)
