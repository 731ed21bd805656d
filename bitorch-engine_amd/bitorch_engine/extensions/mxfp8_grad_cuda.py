"""The input gradient of the MXFP8 weight-only layers on the packed E4M3 weights (csrc/mxfp8_grad.hip): gx = gy . W, dense and per
expert, for the backward of MXFP8LinearCuda and MXFP8ExpertsLinearCuda.  The format and the arithmetic are this library's own
(include/bie_hip.h, INTEGRATION.md "MXFP8 input gradient"):

  qweight uint8 [N, K] ([E, N, K]): OCP e4m3fn bytes           scales uint8 [N, K/32] ([E, N, K/32])  (E8M0: 2^(s - 127), 255 = NaN)
  gx[m, k] = odt( sum_n gy[m, n] * W[n, k] ),  W[n, k] = e4m3(qweight[n, k]) * 2^(scales[n, k // 32] - 127)

Products are exact, the sum is in fp32 in an order fixed by N alone and there is one rounding.  No float image of W is built.  The
kernels rebias by e_blk, the largest scale code of every block-column: blk_exp / experts_blk_exp are the MXFP4 objects (the scale bytes
are the same).  The functions live here, not in mxfp8_linear_cuda / mxfp8_experts_cuda, whose surface stays as it is.  Nothing here
synchronises with the host, so every entry can be captured in a graph."""
import torch

from bitorch_engine.extensions import _mx_w16
from bitorch_engine.extensions.mxfp4_experts_cuda import blk_exp as experts_blk_exp, col_exp as _experts_col_exp
from bitorch_engine.extensions.mxfp4_linear_cuda import blk_exp, col_exp as _col_exp
from bitorch_engine.extensions.mxfp8_a8_linear_cuda import _shape
from bitorch_engine.extensions.mxfp8_experts_cuda import _shape as _experts_shape

_DENSE = _mx_w16.Dense("mx8", "mxfp8", _shape, _col_exp, blk_exp)
_EXPERTS = _mx_w16.Experts("mx8", "mxfp8", _experts_shape, _experts_col_exp, experts_blk_exp)


def grad_input(gy: torch.Tensor, qweight: torch.Tensor, scales: torch.Tensor, e_blk: torch.Tensor = None) -> torch.Tensor:
    """gy [M, N] (fp16 / bf16) -> gx [M, K] = gy . W in gy's dtype, on the packed weight (bie_mx8_linear_grad_input).  e_blk
    (blk_exp(scales)) is computed here when it is not given."""
    return _DENSE.grad_input(gy, qweight, scales, e_blk)


def experts_grad_input(gy: torch.Tensor, idx: torch.Tensor, qweight: torch.Tensor, scales: torch.Tensor, e_blk: torch.Tensor = None,
                       out_dtype: torch.dtype = None) -> torch.Tensor:
    """gy [T, S, N] or [P, N] (fp16 / bf16), idx int32 [T, S] -> gx [P, K], gx[p] = gy[p] . W[idx[p]] in gy's dtype or (out_dtype =
    torch.float32) in fp32; +0 for a skipped slot (bie_mx8_moe_grad_input).  e_blk (experts_blk_exp(scales)) is computed here when it is
    not given."""
    return _EXPERTS.grad_input(gy, idx, qweight, scales, e_blk, out_dtype)
