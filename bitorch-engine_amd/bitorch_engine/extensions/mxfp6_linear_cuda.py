"""MXFP6 (OCP microscaling FP6, E2M3 elements) weights x fp16 / bf16 activations (csrc/mxfp6.hip): the weight-only (W6A16) layer.  The
format and the arithmetic are this library's own (include/bie_hip.h, INTEGRATION.md "MXFP6 linear layer"):

  qweight uint8 [N, 3K/4]: per row K/32 blocks of 24 bytes; code j of a block in bits 6 j .. 6 j + 5 of its little-endian 192-bit integer
  scales uint8 [N, K/32]  (E8M0: 2^(s - 127), 255 = NaN)          W[n, k] = e2m3(code) * 2^(s - 127)
  y = dt( x . W^T + bias )  (products exact, fp32 sums, one rounding)

qweight and scales are byte for byte those of mxfp6_a8_linear_cuda, so quantize, dequant and grad_input are that module's, and
col_exp / blk_exp the MXFP4 ones (the scale bytes are the same).  forward runs the layer (the form from bie_mxfp6_form unless one is
given).  Nothing here synchronises with the host, so every entry can be captured in a graph."""
import torch

from bitorch_engine import _hip
from bitorch_engine.extensions import _mx_w16
from bitorch_engine.extensions.mxfp4_linear_cuda import _X_DT, _aligned, blk_exp, col_exp  # noqa: F401
from bitorch_engine.extensions.mxfp6_a8_linear_cuda import _shape, dequant, grad_input, quantize  # noqa: F401

_LAYER = _mx_w16.Dense("mxfp6", "mxfp6", _shape, col_exp, blk_exp)


def form(M: int, N: int, K: int, dtype: torch.dtype = torch.float16) -> int:
    """0 = decode form, 1 = prefill form (bie_mxfp6_form)."""
    return int(_hip.lib().bie_mxfp6_form(M, N, K, _hip._DT[dtype]))


def forward(x: torch.Tensor, qweight: torch.Tensor, scales: torch.Tensor, bias: torch.Tensor = None, e_col: torch.Tensor = None,
            form: int = -1) -> torch.Tensor:
    """x [M, K] (fp16 / bf16) -> y [M, N] in x's dtype.  form -1 = the plan.  e_col (col_exp(scales)) is read by the prefill form only:
    when it is not given and that form is taken, it is computed here."""
    return _LAYER.forward(x, qweight, scales, bias, e_col, form)
