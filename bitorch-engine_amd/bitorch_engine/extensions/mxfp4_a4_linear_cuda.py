"""MXFP4 weights x activations quantised to MXFP4 on the fly (csrc/mxfp4_a4.hip), contracted on the block-scaled matrix instructions.
The format and the arithmetic are this library's own (include/bie_hip.h, INTEGRATION.md "MXFP4 W4A4 linear layer"):

  xq uint8 [M, K/2], xs uint8 [M, K/32] = x per row and block of 32 by the OCP MX v1.0 rule;  row_flag uint8 [M] = the row holds NaN / inf
  y[m, n] = dt( sum_b 2^(xs[m,b] + scales[n,b] - 254) * (sum_{k in b} e2m1(xq) * e2m1(qweight)) + bias[n] ),  NaN for a flagged row

The weight side (quantize / dequant / col_exp) is mxfp4_linear_cuda's: the weights are the same bytes.  quantize_act quantises x, gemm
contracts already-quantised activations, forward does both.  Nothing here synchronises with the host, so every entry can be captured in a
graph."""
import torch

from bitorch_engine import _hip
from bitorch_engine.extensions import _mx_scaled
from bitorch_engine.extensions.mxfp4_linear_cuda import _X_DT, _aligned, _shape, col_exp, dequant, quantize  # noqa: F401


def quantize_act(x: torch.Tensor):
    """x [M, K] (fp16 / bf16) -> (xq uint8 [M, K/2], xs uint8 [M, K/32], row_flag uint8 [M])."""
    _hip.need_gpu(x)
    if x.dtype not in _X_DT or x.dim() != 2:
        raise RuntimeError(f"mxfp4 a4: x must be fp16 / bf16 [M, K] (got {x.dtype} {tuple(x.shape)})")
    M, K = x.shape
    xq = torch.empty((M, K // 2), dtype=torch.uint8, device=x.device)
    xs = torch.empty((M, K // 32), dtype=torch.uint8, device=x.device)
    flag = torch.empty(M, dtype=torch.uint8, device=x.device)
    if M == 0:
        return xq, xs, flag
    x = _aligned(x)
    _hip.check(_hip.lib().bie_mxfp4_quantize_act(_hip.ptr(x), _hip.ptr(xq), _hip.ptr(xs), _hip.ptr(flag), M, K, _hip.dt(x), _hip.stream()),
               "bie_mxfp4_quantize_act")
    return xq, xs, flag


_LAYER = _mx_scaled.Dense("mxfp4_a4", "mxfp4 a4", 16, _shape, col_exp, act_shape=_shape, empty_gemm=False)
_bias = _mx_scaled._bias


def form(M: int, N: int, K: int, dtype: torch.dtype = torch.float16) -> int:
    """0 = decode form, 1 = prefill form (bie_mxfp4_a4_form)."""
    return _LAYER.form(M, N, K, dtype)


def forward(x: torch.Tensor, qweight: torch.Tensor, scales: torch.Tensor, bias: torch.Tensor = None, e_col: torch.Tensor = None,
            form: int = -1) -> torch.Tensor:
    """x [M, K] (fp16 / bf16) -> y [M, N] in x's dtype: quantise x, then the contraction.  form -1 = the plan.  e_col (col_exp(scales)) is
    computed here when it is not given."""
    return _LAYER.forward(x, qweight, scales, bias, e_col, form)


def gemm(xq: torch.Tensor, xs: torch.Tensor, row_flag: torch.Tensor, qweight: torch.Tensor, scales: torch.Tensor, bias: torch.Tensor = None,
         e_col: torch.Tensor = None, dtype: torch.dtype = torch.float16, form: int = -1) -> torch.Tensor:
    """The contraction from already-quantised activations (xq uint8 [M, K/2], xs uint8 [M, K/32], row_flag uint8 [M]) -> y [M, N] in dtype."""
    return _LAYER.gemm(xq, xs, row_flag, qweight, scales, bias, e_col, dtype, form)
