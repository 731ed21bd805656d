"""MXFP8 (OCP microscaling FP8, e4m3fn elements) weights x fp16 / bf16 activations (csrc/mxfp8.hip): the weight-only (W8A16) layer.  The
format and the arithmetic are this library's own (include/bie_hip.h, INTEGRATION.md "MXFP8 linear layer"):

  qweight uint8 [N, K]: row-major OCP e4m3fn bytes            scales uint8 [N, K/32]  (E8M0: 2^(s - 127), 255 = NaN)
  W[n, k] = e4m3(qweight[n, k]) * 2^(scales[n, k // 32] - 127)
  y = dt( x . W^T + bias )  (products exact, fp32 sums, one rounding)

qweight and scales are byte for byte those of mxfp8_a8_linear_cuda, so quantize and dequant are that module's, and col_exp the MXFP4
one (the scale bytes are the same).  forward runs the layer (the form from bie_mx8_form unless one is given).  The packed-weight
input gradient of this format (gx = gy . W, csrc/mxfp8_grad.hip) is mxfp8_grad_cuda's grad_input, with its blk_exp; this module's
surface has neither.  Nothing here synchronises with the host, so every entry can be captured in a graph."""
import torch

from bitorch_engine import _hip
from bitorch_engine.extensions import _mx_w16
from bitorch_engine.extensions.mxfp4_linear_cuda import _X_DT, _aligned, col_exp  # noqa: F401
from bitorch_engine.extensions.mxfp8_a8_linear_cuda import _shape, dequant, quantize  # noqa: F401

_LAYER = _mx_w16.Dense("mx8", "mxfp8", _shape, col_exp, None)


def form(M: int, N: int, K: int, dtype: torch.dtype = torch.float16) -> int:
    """0 = decode form, 1 = prefill form (bie_mx8_form)."""
    return int(_hip.lib().bie_mx8_form(M, N, K, _hip._DT[dtype]))


def forward(x: torch.Tensor, qweight: torch.Tensor, scales: torch.Tensor, bias: torch.Tensor = None, e_col: torch.Tensor = None,
            form: int = -1) -> torch.Tensor:
    """x [M, K] (fp16 / bf16) -> y [M, N] in x's dtype; the activations are not quantised.  form -1 = the plan.  e_col (col_exp(scales)) is
    read by the prefill form only: when it is not given and that form is taken, it is computed here."""
    return _LAYER.forward(x, qweight, scales, bias, e_col, form)
