"""The expert GEMM of a mixture-of-experts MLP on stacked MXFP4 weights against activations quantised to MXFP6 (OCP microscaling FP6,
E2M3 elements, E8M0 block scales) on the fly (csrc/mxfp4_moe_a6.hip), contracted on the block-scaled matrix instructions with an FP4
and an FP6 operand, at the FP4 matrix rate.  The format and the arithmetic are this library's own (include/bie_hip.h, INTEGRATION.md
"MXFP4 W4A6 mixture-of-experts layer"):

  qweight uint8 [E, N, K/2], scales uint8 [E, N, K/32], bias [E, N], idx int32 [T, S]: mxfp4_experts_cuda's
  xq6, xs, row_flag = quantize_act of the stored rows of x: x [T, K] (every slot of a token reads the token's row) or x [T, S, K]
  y[t, s] = dt( sum_b 2^(xs[row, b] + scales[e, n, b] - 254) * (sum_{k in b} e2m3(xq6) * e2m1(qweight)) + bias[e] ),  e = idx[t, s]
  y[t, s] = NaN for a row of x that holds NaN / inf, +0 for a skipped slot (idx outside [0, E)) whatever its row holds

quantize / dequant / col_exp / blk_exp / grad_input are mxfp4_experts_cuda's objects (the weights are the same bytes); quantize_act /
dequant_act are mxfp6_a6_linear_cuda's.  Nothing here synchronises with the host (the routing is read on the device), so every entry can
be captured in a graph."""
import torch

from bitorch_engine import _hip
from bitorch_engine.extensions.mxfp4_experts_a8_cuda import _bias
from bitorch_engine.extensions.mxfp4_experts_cuda import _shape, blk_exp, col_exp, dequant, grad_input, quantize  # noqa: F401
from bitorch_engine.extensions.mxfp4_linear_cuda import _X_DT, _aligned
from bitorch_engine.extensions.mxfp6_a6_linear_cuda import dequant_act, quantize_act  # noqa: F401


def form(P: int, E: int, N: int, K: int, dtype: torch.dtype = torch.float16) -> int:
    """0 = routed decode form, 1 = grouped prefill form (bie_mx4a6_moe_form); P = the number of (token, slot) pairs."""
    return int(_hip.lib().bie_mx4a6_moe_form(P, E, N, K, _hip._DT[dtype]))


def _idx(idx):
    if idx.dtype != torch.int32 or idx.dim() != 2:
        raise RuntimeError(f"mxfp4 a6 experts: idx must be int32 [T, S] (got {idx.dtype} {tuple(idx.shape)})")
    return idx.shape


def forward(x: torch.Tensor, idx: torch.Tensor, qweight: torch.Tensor, scales: torch.Tensor, bias: torch.Tensor = None, e_col: torch.Tensor = None,
            form: int = -1) -> torch.Tensor:
    """x [T, K] or [T, S, K] (fp16 / bf16), idx int32 [T, S] -> y [T, S, N] in x's dtype: quantise the rows of x, then the contraction.
    form -1 = the plan.  e_col (col_exp(scales)) is computed here when it is not given."""
    _hip.need_gpu(x, idx, qweight, scales, bias, e_col)
    if x.dtype not in _X_DT:
        raise RuntimeError(f"mxfp4 a6 experts: dtype {x.dtype} is not supported (fp16 / bf16)")
    E, N, K = _shape(qweight, scales)
    T, S = _idx(idx)
    if tuple(x.shape) not in ((T, K), (T, S, K)):
        raise RuntimeError(f"mxfp4 a6 experts: x {tuple(x.shape)} does not match idx {tuple(idx.shape)} and K={K}")
    y = torch.empty((T, S, N), dtype=x.dtype, device=x.device)
    if T * S == 0:
        return y
    L = _hip.lib()
    if form < 0:
        form = int(L.bie_mx4a6_moe_form(T * S, E, N, K, _hip.dt(x)))
    if e_col is None:
        e_col = col_exp(scales)
    x_per_pair = int(x.dim() == 3)
    ws = torch.empty(int(L.bie_mx4a6_moe_workspace_bytes(T, S, E, K, x_per_pair, int(form))), dtype=torch.uint8, device=x.device)
    bias = _bias(bias, E, N, x.dtype)
    x, idx, qweight, scales, e_col = _aligned(x), idx.contiguous(), _aligned(qweight), scales.contiguous(), e_col.contiguous()  # held until queued
    _hip.check(L.bie_mx4a6_moe_forward(_hip.ptr(x), _hip.ptr(idx), _hip.ptr(qweight), _hip.ptr(scales), _hip.ptr(e_col), _hip.ptr(bias), _hip.ptr(y),
                                       _hip.ptr(ws), T, S, E, N, K, x_per_pair, _hip.dt(x), int(form), _hip.stream()), "bie_mx4a6_moe_forward")
    return y


def gemm(xq6: torch.Tensor, xs: torch.Tensor, row_flag: torch.Tensor, idx: torch.Tensor, qweight: torch.Tensor, scales: torch.Tensor,
         bias: torch.Tensor = None, e_col: torch.Tensor = None, dtype: torch.dtype = torch.float16, form: int = -1) -> torch.Tensor:
    """The contraction from already-quantised activations: xq6 uint8 [R, 3K/4], xs uint8 [R, K/32], row_flag uint8 [R] with R = T (every
    slot of a token reads the token's row) or R = T * S (a row per pair, in pair order) -> y [T, S, N] in dtype.  Form 0 here is the
    routed kernel reading xq6 from memory."""
    _hip.need_gpu(xq6, xs, row_flag, idx, qweight, scales, bias, e_col)
    if dtype not in _X_DT:
        raise RuntimeError(f"mxfp4 a6 experts gemm: dtype {dtype} is not supported (fp16 / bf16)")
    E, N, K = _shape(qweight, scales)
    T, S = _idx(idx)
    R = xq6.shape[0]
    if (xq6.dtype != torch.uint8 or xs.dtype != torch.uint8 or row_flag.dtype != torch.uint8 or tuple(xq6.shape) != (R, K // 32 * 24)
            or tuple(xs.shape) != (R, K // 32) or tuple(row_flag.shape) != (R,) or R not in (T, T * S)):
        raise RuntimeError(f"mxfp4 a6 experts gemm: xq6 {tuple(xq6.shape)} / xs {tuple(xs.shape)} / row_flag {tuple(row_flag.shape)} do not match "
                           f"idx {tuple(idx.shape)} and K={K} (uint8 [R, 3K/4] / [R, K/32] / [R], T or T * S rows)")
    y = torch.empty((T, S, N), dtype=dtype, device=xq6.device)
    if T * S == 0:
        return y
    x_per_pair = int(R != T)  # S = 1: the two readings are the same rows
    L = _hip.lib()
    if form < 0:
        form = int(L.bie_mx4a6_moe_form(T * S, E, N, K, _hip._DT[dtype]))
    if e_col is None:
        e_col = col_exp(scales)
    ws = torch.empty(int(L.bie_mxfp4_moe_workspace_bytes(T * S, E)), dtype=torch.uint8, device=xq6.device) if form == 1 else None
    bias = _bias(bias, E, N, dtype)
    xq6, xs, row_flag, idx = _aligned(xq6), xs.contiguous(), row_flag.contiguous(), idx.contiguous()
    qweight, scales, e_col = _aligned(qweight), scales.contiguous(), e_col.contiguous()
    _hip.check(L.bie_mx4a6_moe_gemm(_hip.ptr(xq6), _hip.ptr(xs), _hip.ptr(row_flag), _hip.ptr(idx), _hip.ptr(qweight), _hip.ptr(scales), _hip.ptr(e_col),
                                    _hip.ptr(bias), _hip.ptr(y), _hip.ptr(ws), T, S, E, N, K, x_per_pair, _hip._DT[dtype], int(form), _hip.stream()),
               "bie_mx4a6_moe_gemm")
    return y
