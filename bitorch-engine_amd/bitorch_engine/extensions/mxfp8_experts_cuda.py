"""The expert GEMM of a mixture-of-experts MLP on stacked MXFP8 weights (OCP microscaling FP8, e4m3fn elements) against fp16 / bf16
activations: the weight-only (W8A16) arithmetic of mxfp8_linear_cuda per expert (csrc/mxfp8_moe.hip).  The format and the arithmetic
are this library's own (include/bie_hip.h, INTEGRATION.md "MXFP8 W8A16 mixture-of-experts layer"):

  qweight uint8 [E, N, K], scales uint8 [E, N, K/32], bias [E, N]: mxfp8_linear_cuda's format per expert
  idx int32 [T, S]: the expert of every (token, slot) pair; an index outside [0, E) (-1 by convention) is a skipped slot
  y[t, s] = dt( x_row . W[idx[t, s]]^T + bias[idx[t, s]] ),  +0 for a skipped slot;   x_row = x[t] (x [T, K]) or x[t, s] (x [T, S, K])

Products are exact, the sum is in fp32 and there is one rounding.  quantize / dequant are mxfp8_a8_linear_cuda's on the [E * N, K] view
(the format is row-wise) and col_exp is mxfp4_experts_cuda's (the same object: the scales are the same bytes).  The packed-weight
input gradient of this format (gx[p] = gy[p] . W[idx[p]], csrc/mxfp8_grad.hip) is mxfp8_grad_cuda's experts_grad_input, with its
experts_blk_exp; this module's surface has neither.  Nothing here synchronises with the host (the routing is read on the device), so
every entry can be captured in a graph."""
import torch

from bitorch_engine import _hip
from bitorch_engine.extensions import _mx_w16, mxfp8_a8_linear_cuda
from bitorch_engine.extensions.mxfp4_experts_cuda import col_exp  # noqa: F401
from bitorch_engine.extensions.mxfp4_linear_cuda import _X_DT, _aligned  # noqa: F401


def _shape(qweight: torch.Tensor, scales: torch.Tensor):
    if qweight.dtype != torch.uint8 or qweight.dim() != 3 or scales.dtype != torch.uint8 or scales.dim() != 3:
        raise RuntimeError("mxfp8 experts: qweight must be uint8 [E, N, K] and scales uint8 [E, N, K/32]")
    E, N, KB = scales.shape
    if KB == 0 or tuple(qweight.shape) != (E, N, 32 * KB):
        raise RuntimeError(f"mxfp8 experts: qweight {tuple(qweight.shape)} does not match scales {tuple(scales.shape)} (32 bytes per block of 32)")
    return E, N, 32 * KB


def quantize(weight: torch.Tensor):
    """float weight [E, N, K] -> (qweight uint8 [E, N, K], scales uint8 [E, N, K/32]) by the OCP MX rule with E4M3 elements."""
    E, N, K = weight.shape
    q, s = mxfp8_a8_linear_cuda.quantize(weight.reshape(E * N, K))
    return q.reshape(E, N, K), s.reshape(E, N, K // 32)


def dequant(qweight: torch.Tensor, scales: torch.Tensor, dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """W [E, N, K] in dtype: exact in fp32, rounded once."""
    E, N, K = _shape(qweight, scales)
    return mxfp8_a8_linear_cuda.dequant(qweight.reshape(E * N, K), scales.reshape(E * N, K // 32), dtype).reshape(E, N, K)


_LAYER = _mx_w16.Experts("mx8", "mxfp8", _shape, col_exp, None)


def form(P: int, E: int, N: int, K: int, dtype: torch.dtype = torch.float16) -> int:
    """0 = routed decode form, 1 = grouped prefill form (bie_mx8_moe_form); P = the number of (token, slot) pairs."""
    return int(_hip.lib().bie_mx8_moe_form(P, E, N, K, _hip._DT[dtype]))


def forward(x: torch.Tensor, idx: torch.Tensor, qweight: torch.Tensor, scales: torch.Tensor, bias: torch.Tensor = None, e_col: torch.Tensor = None,
            form: int = -1) -> torch.Tensor:
    """x [T, K] or [T, S, K] (fp16 / bf16), idx int32 [T, S] -> y [T, S, N] in x's dtype.  form -1 = the plan.  e_col (col_exp(scales)) is
    read by the prefill form only: when it is not given and that form is taken, it is computed here."""
    return _LAYER.forward(x, idx, qweight, scales, bias, e_col, form)
