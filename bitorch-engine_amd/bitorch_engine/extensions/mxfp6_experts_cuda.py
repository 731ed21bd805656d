"""The expert GEMM of a mixture-of-experts MLP on stacked MXFP6 weights (OCP microscaling FP6, E2M3 elements) against fp16 / bf16
activations: the weight-only (W6A16) arithmetic of mxfp6_linear_cuda per expert (csrc/mxfp6_moe.hip).  The format and the arithmetic
are this library's own (include/bie_hip.h, INTEGRATION.md "MXFP6 W6A16 mixture-of-experts layer"):

  qweight uint8 [E, N, 3K/4], scales uint8 [E, N, K/32], bias [E, N]: mxfp6_experts_a8_cuda's bytes (mxfp6_linear_cuda's format per expert)
  idx int32 [T, S]: the expert of every (token, slot) pair; an index outside [0, E) (-1 by convention) is a skipped slot
  y[t, s] = dt( x_row . W[idx[t, s]]^T + bias[idx[t, s]] ),  +0 for a skipped slot;   x_row = x[t] (x [T, K]) or x[t, s] (x [T, S, K])

Products are exact, the sum is in fp32 and there is one rounding.  quantize / dequant / grad_input are mxfp6_experts_a8_cuda's and
col_exp / blk_exp mxfp4_experts_cuda's (the same objects: the weights are the same bytes).  Nothing here synchronises with the host (the
routing is read on the device), so every entry can be captured in a graph."""
import torch

from bitorch_engine import _hip
from bitorch_engine.extensions import _mx_w16
from bitorch_engine.extensions.mxfp4_experts_cuda import blk_exp, col_exp  # noqa: F401
from bitorch_engine.extensions.mxfp4_linear_cuda import _X_DT, _aligned  # noqa: F401  (re-exports, as before)
from bitorch_engine.extensions.mxfp6_experts_a8_cuda import _shape, dequant, grad_input, quantize  # noqa: F401

_LAYER = _mx_w16.Experts("mxfp6", "mxfp6", _shape, col_exp, blk_exp)


def form(P: int, E: int, N: int, K: int, dtype: torch.dtype = torch.float16) -> int:
    """0 = routed decode form, 1 = grouped prefill form (bie_mxfp6_moe_form); P = the number of (token, slot) pairs."""
    return int(_hip.lib().bie_mxfp6_moe_form(P, E, N, K, _hip._DT[dtype]))


def forward(x: torch.Tensor, idx: torch.Tensor, qweight: torch.Tensor, scales: torch.Tensor, bias: torch.Tensor = None, e_col: torch.Tensor = None,
            form: int = -1) -> torch.Tensor:
    """x [T, K] or [T, S, K] (fp16 / bf16), idx int32 [T, S] -> y [T, S, N] in x's dtype.  form -1 = the plan.  e_col (col_exp(scales)) is
    read by the prefill form only: when it is not given and that form is taken, it is computed here."""
    return _LAYER.forward(x, idx, qweight, scales, bias, e_col, form)
