"""The expert GEMM of a mixture-of-experts MLP on stacked MXFP4 weights (csrc/mxfp4_moe.hip).  The format and the arithmetic are this
library's own (include/bie_hip.h, INTEGRATION.md "MXFP4 mixture-of-experts layer"):

  qweight uint8 [E, N, K/2], scales uint8 [E, N, K/32], bias [E, N]: mxfp4_linear_cuda's format per expert
  idx int32 [T, S]: the expert of every (token, slot) pair; an index outside [0, E) (-1 by convention) is a skipped slot
  y[t, s] = dt( x_row . W[idx[t, s]]^T + bias[idx[t, s]] ),  0 for a skipped slot;   x_row = x[t] (x [T, K]) or x[t, s] (x [T, S, K])

quantize / dequant / col_exp are mxfp4_linear_cuda's on the [E * N, K] view.  grad_input is the backward's gx[p] = gy[p] . W[idx[p]] on
the packed weights (csrc/mxfp4_grad.hip), rebiased by blk_exp's per-expert, per-block-column largest scale code.  Nothing here
synchronises with the host (the routing is read on the device), so every entry can be captured in a graph."""
import torch

from bitorch_engine import _hip
from bitorch_engine.extensions import _mx_w16, mxfp4_linear_cuda
from bitorch_engine.extensions.mxfp4_linear_cuda import _X_DT, _aligned  # noqa: F401  (re-exports, as before)


def _shape(qweight: torch.Tensor, scales: torch.Tensor):
    if qweight.dtype != torch.uint8 or qweight.dim() != 3 or scales.dtype != torch.uint8 or scales.dim() != 3:
        raise RuntimeError("mxfp4 experts: qweight must be uint8 [E, N, K/2] and scales uint8 [E, N, K/32]")
    E, N, K = qweight.shape[0], qweight.shape[1], qweight.shape[2] * 2
    if tuple(scales.shape) != (E, N, K // 32) or K % 32 or K == 0:
        raise RuntimeError(f"mxfp4 experts: scales {tuple(scales.shape)} do not match qweight {tuple(qweight.shape)} (K % 32 == 0 required)")
    return E, N, K


def quantize(weight: torch.Tensor):
    """float weight [E, N, K] -> (qweight uint8 [E, N, K/2], scales uint8 [E, N, K/32]) by the OCP MX v1.0 rule."""
    E, N, K = weight.shape
    q, s = mxfp4_linear_cuda.quantize(weight.reshape(E * N, K))
    return q.reshape(E, N, K // 2), s.reshape(E, N, K // 32)


def dequant(qweight: torch.Tensor, scales: torch.Tensor, dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """W [E, N, K] in dtype: exact in fp32, rounded once."""
    E, N, K = _shape(qweight, scales)
    return mxfp4_linear_cuda.dequant(qweight.reshape(E * N, K // 2), scales.reshape(E * N, K // 32), dtype).reshape(E, N, K)


def col_exp(scales: torch.Tensor) -> torch.Tensor:
    """e_col uint8 [E, N]: the largest scale code of each expert's row (255 where the row has a NaN block)."""
    E, N, KB = scales.shape
    return mxfp4_linear_cuda.col_exp(scales.reshape(E * N, KB)).reshape(E, N)


def form(P: int, E: int, N: int, K: int, dtype: torch.dtype = torch.float16) -> int:
    """0 = routed decode form, 1 = grouped prefill form (bie_mxfp4_moe_form); P = the number of (token, slot) pairs."""
    return int(_hip.lib().bie_mxfp4_moe_form(P, E, N, K, _hip._DT[dtype]))


def forward(x: torch.Tensor, idx: torch.Tensor, qweight: torch.Tensor, scales: torch.Tensor, bias: torch.Tensor = None, e_col: torch.Tensor = None,
            form: int = -1) -> torch.Tensor:
    """x [T, K] or [T, S, K] (fp16 / bf16), idx int32 [T, S] -> y [T, S, N] in x's dtype.  form -1 = the plan.  e_col (col_exp(scales)) is
    read by the prefill form only: when it is not given and that form is taken, it is computed here."""
    return _LAYER.forward(x, idx, qweight, scales, bias, e_col, form)


def blk_exp(scales: torch.Tensor) -> torch.Tensor:
    """e_blk uint8 [E, K/32]: the largest scale code of each expert's block-column over its N rows (255 where it has a NaN block)."""
    _hip.need_gpu(scales)
    if scales.dtype != torch.uint8 or scales.dim() != 3:
        raise RuntimeError("mxfp4 experts: scales must be uint8 [E, N, K/32]")
    E, N, KB = scales.shape
    e = torch.empty((E, KB), dtype=torch.uint8, device=scales.device)
    scales = scales.contiguous()
    _hip.check(_hip.lib().bie_mxfp4_blk_exp(_hip.ptr(scales), _hip.ptr(e), N, KB * 32, E, _hip.stream()), "bie_mxfp4_blk_exp")
    return e


def grad_input(gy: torch.Tensor, idx: torch.Tensor, qweight: torch.Tensor, scales: torch.Tensor, e_blk: torch.Tensor = None,
               out_dtype: torch.dtype = None) -> torch.Tensor:
    """gy [T, S, N] or [P, N] (fp16 / bf16, any N), idx int32 [T, S] -> gx [P, K], gx[p] = gy[p] . W[idx[p]] (0 for a skipped slot), in
    gy's dtype or, with out_dtype=torch.float32, in fp32 (the caller sums a token's slots before the one rounding).  No image of W is
    built.  e_blk (blk_exp(scales)) is computed here when it is not given."""
    return _LAYER.grad_input(gy, idx, qweight, scales, e_blk, out_dtype)


_LAYER = _mx_w16.Experts("mxfp4", "mxfp4", _shape, col_exp, blk_exp)
