"""MXFP6 (OCP microscaling FP6, E2M3 elements) weights x activations quantised to MXFP8 (E4M3 elements, E8M0 block scales) on the fly
(csrc/mxfp6_a8.hip), contracted on the block-scaled matrix instructions with an FP6 and an E4M3 operand.  The format and the arithmetic
are this library's own (include/bie_hip.h, INTEGRATION.md "MXFP6 W6A8 linear layer"):

  qweight uint8 [N, 3K/4]: per row K/32 blocks of 24 bytes; code j of a block in bits 6 j .. 6 j + 5 of its little-endian 192-bit integer
  scales uint8 [N, K/32]  (E8M0: 2^(s - 127), 255 = NaN)          W[n, k] = e2m3(code) * 2^(s - 127)
  xq uint8 [M, K], xs uint8 [M, K/32], row_flag uint8 [M]: the MXFP8 activations of mxfp4_a8_linear_cuda, unchanged
  y[m, n] = dt( sum_b 2^(xs[m,b] + scales[n,b] - 254) * (sum_{k in b} e4m3(xq) * e2m3(qweight)) + bias[n] ),  NaN for a flagged row

quantize / dequant convert between a float weight and the packed pair; col_exp, quantize_act and dequant_act are the W4A8 ones (the
scales and the activations are the same bytes); gemm contracts already-quantised activations, forward does both.  grad_input is the
backward's gx = gy . W on the packed weight (csrc/mxfp6_grad.hip), rebiased by blk_exp's per-block-column largest scale code (the MXFP4
one: the scale bytes are the same).  Nothing here synchronises with the host, so every entry can be captured in a graph."""
import torch

from bitorch_engine import _hip
from bitorch_engine.extensions import _mx_scaled, _mx_w16
from bitorch_engine.extensions.mxfp4_linear_cuda import _X_DT, _aligned, blk_exp, col_exp  # noqa: F401
from bitorch_engine.extensions.mxfp4_a8_linear_cuda import _act_shape, _bias, dequant_act, quantize_act  # noqa: F401


def _shape(qweight: torch.Tensor, scales: torch.Tensor):
    if qweight.dtype != torch.uint8 or qweight.dim() != 2 or scales.dtype != torch.uint8 or scales.dim() != 2:
        raise RuntimeError("mxfp6: qweight must be uint8 [N, 3K/4] and scales uint8 [N, K/32]")
    N, KB = scales.shape
    if KB == 0 or tuple(qweight.shape) != (N, 24 * KB):
        raise RuntimeError(f"mxfp6: qweight {tuple(qweight.shape)} does not match scales {tuple(scales.shape)} (24 bytes per block of 32)")
    return N, 32 * KB


def quantize(weight: torch.Tensor):
    """float weight [N, K] (fp32 / fp16 / bf16) -> (qweight uint8 [N, 3K/4], scales uint8 [N, K/32]) by the OCP MX rule with E2M3 elements."""
    _hip.need_gpu(weight)
    N, K = weight.shape
    w = _aligned(weight.detach())
    qweight = torch.empty((N, K // 32 * 24), dtype=torch.uint8, device=w.device)
    scales = torch.empty((N, K // 32), dtype=torch.uint8, device=w.device)
    _hip.check(_hip.lib().bie_mxfp6_quantize(_hip.ptr(w), _hip.ptr(qweight), _hip.ptr(scales), N, K, _hip.dt(w), _hip.stream()), "bie_mxfp6_quantize")
    return qweight, scales


def dequant(qweight: torch.Tensor, scales: torch.Tensor, dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """W [N, K] in dtype: computed exactly in fp32, rounded once (fp16 overflows to inf beyond 65504)."""
    _hip.need_gpu(qweight, scales)
    N, K = _shape(qweight, scales)
    w = torch.empty((N, K), dtype=dtype, device=qweight.device)
    qweight, scales = _aligned(qweight), scales.contiguous()
    _hip.check(_hip.lib().bie_mxfp6_dequant(_hip.ptr(qweight), _hip.ptr(scales), _hip.ptr(w), N, K, _hip.dt(w), _hip.stream()), "bie_mxfp6_dequant")
    return w


_LAYER = _mx_scaled.Dense("mxfp6_a8", "mxfp6 a8", 32, _shape, col_exp, act_shape=_act_shape)
_GRAD = _mx_w16.Dense("mxfp6", "mxfp6", _shape, col_exp, blk_exp)  # the input gradient of every MXFP6 weight: it does not see the activations


def form(M: int, N: int, K: int, dtype: torch.dtype = torch.float16) -> int:
    """0 = decode form, 1 = prefill form (bie_mxfp6_a8_form)."""
    return _LAYER.form(M, N, K, dtype)


def forward(x: torch.Tensor, qweight: torch.Tensor, scales: torch.Tensor, bias: torch.Tensor = None, e_col: torch.Tensor = None,
            form: int = -1) -> torch.Tensor:
    """x [M, K] (fp16 / bf16) -> y [M, N] in x's dtype: quantise x, then the contraction.  form -1 = the plan.  e_col (col_exp(scales)) is
    computed here when it is not given."""
    return _LAYER.forward(x, qweight, scales, bias, e_col, form)


def gemm(xq: torch.Tensor, xs: torch.Tensor, row_flag: torch.Tensor, qweight: torch.Tensor, scales: torch.Tensor, bias: torch.Tensor = None,
         e_col: torch.Tensor = None, dtype: torch.dtype = torch.float16, form: int = -1) -> torch.Tensor:
    """The contraction from already-quantised activations (xq uint8 [M, K], xs uint8 [M, K/32], row_flag uint8 [M]) -> y [M, N] in dtype."""
    return _LAYER.gemm(xq, xs, row_flag, qweight, scales, bias, e_col, dtype, form)


def grad_input(gy: torch.Tensor, qweight: torch.Tensor, scales: torch.Tensor, e_blk: torch.Tensor = None) -> torch.Tensor:
    """gy [M, N] (fp16 / bf16, any N) -> gx = gy . W [M, K] in gy's dtype, from the packed weight: no image of W is built.  e_blk
    (blk_exp(scales)) is computed here when it is not given."""
    return _GRAD.grad_input(gy, qweight, scales, e_blk)
