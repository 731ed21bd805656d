"""The expert GEMM of a mixture-of-experts MLP on stacked MXFP6 weights (OCP microscaling FP6, E2M3 elements) against activations
quantised to MXFP8 (E4M3 elements, E8M0 block scales) on the fly (csrc/mxfp6_moe_a8.hip), contracted on the block-scaled matrix
instructions with an FP6 and an E4M3 operand.  The format and the arithmetic are this library's own (include/bie_hip.h, INTEGRATION.md
"MXFP6 W6A8 mixture-of-experts layer"):

  qweight uint8 [E, N, 3K/4] (per row K/32 blocks of 24 bytes, mxfp6_a8_linear_cuda's bit order), scales uint8 [E, N, K/32], bias [E, N]
  idx int32 [T, S]: the expert of every (token, slot) pair; an index outside [0, E) (-1 by convention) is a skipped slot
  xq, xs, row_flag = quantize_act of the stored rows of x: x [T, K] (every slot of a token reads the token's row) or x [T, S, K]
  y[t, s] = dt( sum_b 2^(xs[row, b] + scales[e, n, b] - 254) * (sum_{k in b} e4m3(xq) * e2m3(qweight)) + bias[e] ),  e = idx[t, s]
  y[t, s] = NaN for a row of x that holds NaN / inf, +0 for a skipped slot whatever its row holds

quantize / dequant are mxfp6_a8_linear_cuda's on the [E * N, K] view, col_exp is mxfp4_experts_cuda's (the scales are the same bytes)
and quantize_act / dequant_act are mxfp4_a8_linear_cuda's.  grad_input is the backward's gx[p] = gy[p] . W[idx[p]] on the packed weights
(csrc/mxfp6_grad.hip), rebiased by blk_exp's per-expert, per-block-column largest scale code (mxfp4_experts_cuda's).  Nothing here
synchronises with the host (the routing is read on the device), so every entry can be captured in a graph."""
import torch

from bitorch_engine.extensions import _mx_scaled, _mx_w16
from bitorch_engine.extensions import mxfp6_a8_linear_cuda
from bitorch_engine.extensions.mxfp4_a8_linear_cuda import dequant_act, quantize_act  # noqa: F401
from bitorch_engine.extensions.mxfp4_experts_cuda import blk_exp, col_exp  # noqa: F401
from bitorch_engine.extensions.mxfp4_linear_cuda import _X_DT, _aligned  # noqa: F401  (re-exports, as before)


def _shape(qweight: torch.Tensor, scales: torch.Tensor):
    if qweight.dtype != torch.uint8 or qweight.dim() != 3 or scales.dtype != torch.uint8 or scales.dim() != 3:
        raise RuntimeError("mxfp6 experts: qweight must be uint8 [E, N, 3K/4] and scales uint8 [E, N, K/32]")
    E, N, KB = scales.shape
    if KB == 0 or tuple(qweight.shape) != (E, N, 24 * KB):
        raise RuntimeError(f"mxfp6 experts: qweight {tuple(qweight.shape)} does not match scales {tuple(scales.shape)} (24 bytes per block of 32)")
    return E, N, 32 * KB


def quantize(weight: torch.Tensor):
    """float weight [E, N, K] -> (qweight uint8 [E, N, 3K/4], scales uint8 [E, N, K/32]) by the OCP MX rule with E2M3 elements."""
    E, N, K = weight.shape
    q, s = mxfp6_a8_linear_cuda.quantize(weight.reshape(E * N, K))
    return q.reshape(E, N, K // 32 * 24), s.reshape(E, N, K // 32)


def dequant(qweight: torch.Tensor, scales: torch.Tensor, dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """W [E, N, K] in dtype: exact in fp32, rounded once."""
    E, N, K = _shape(qweight, scales)
    return mxfp6_a8_linear_cuda.dequant(qweight.reshape(E * N, K // 32 * 24), scales.reshape(E * N, K // 32), dtype).reshape(E, N, K)


_LAYER = _mx_scaled.Experts("mxfp6_moe_a8", "mxfp6 a8", 32, _shape, col_exp)
_idx = _LAYER.idx
# the input gradient of every MXFP6 expert weight (it does not see the activations); idx is checked under this module's prefix
_GRAD = _mx_w16.Experts("mxfp6", "mxfp6", _shape, col_exp, blk_exp, idx=_idx)
_bias = _mx_scaled._experts_bias


def form(P: int, E: int, N: int, K: int, dtype: torch.dtype = torch.float16) -> int:
    """0 = routed decode form, 1 = grouped prefill form (bie_mxfp6_moe_a8_form); P = the number of (token, slot) pairs."""
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


def grad_input(gy: torch.Tensor, idx: torch.Tensor, qweight: torch.Tensor, scales: torch.Tensor, e_blk: torch.Tensor = None,
               out_dtype: torch.dtype = None) -> torch.Tensor:
    """gy [T, S, N] or [P, N] (fp16 / bf16, any N), idx int32 [T, S] -> gx [P, K], gx[p] = gy[p] . W[idx[p]] (0 for a skipped slot), in
    gy's dtype or, with out_dtype=torch.float32, in fp32 (the caller sums a token's slots before the one rounding).  No image of W is
    built.  e_blk (blk_exp(scales)) is computed here when it is not given."""
    return _GRAD.grad_input(gy, idx, qweight, scales, e_blk, out_dtype)
