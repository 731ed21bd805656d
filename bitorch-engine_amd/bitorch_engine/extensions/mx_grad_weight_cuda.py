"""The weight gradient of the weight-only MX linear layers (csrc/mx_wgrad.hip): gw = gy^T . x and gb = sum_m gy, for the backward of
MXFP4LinearCuda, MXFP6LinearCuda and MXFP8LinearCuda.  It is the gradient of the float latent weight, so one function serves the three
formats (include/bie_hip.h, INTEGRATION.md "MX weight gradient"):

  gw[n, k] = odt( sum_m gy[m, n] * x[m, k] )        gb[n] = odt( sum_m gy[m, n] )

Products are exact, the sum is in fp32 in an order fixed by (M, N, K, splits) alone and there is one rounding.  Neither gy nor x is
transposed or widened in memory: the kernel stages slabs of 32 rows as they lie and transposes them in the LDS read.  Nothing here
synchronises with the host, so the entry can be captured in a graph (the workspace is a torch allocation of the call)."""
import torch

from bitorch_engine import _hip
from bitorch_engine.extensions._mx_w16 import _X_DT, _aligned


def plan_splits(M: int, N: int, K: int) -> int:
    """The plan's number of slices of M (bie_mx_wgrad_splits): a host function of the shape alone."""
    return int(_hip.lib().bie_mx_wgrad_splits(M, N, K))


def grad_weight(gy: torch.Tensor, x: torch.Tensor, out_dtype: torch.dtype = None, bias: bool = False, splits: int = -1):
    """gy [M, N], x [M, K] (fp16 / bf16, one dtype) -> gw [N, K] = gy^T . x in that dtype or (out_dtype = torch.float32) in fp32; with
    bias=True (gw, gb), gb [N] = the column sums of gy, from the same launch.  splits: -1 = the plan, 1 .. ceil(M / 32) = that many
    slices of M (bie_mx_linear_grad_weight).  M = 0 gives zeros."""
    _hip.need_gpu(gy, x)
    if gy.dtype not in _X_DT:
        raise RuntimeError(f"mx grad_weight: dtype {gy.dtype} is not supported (fp16 / bf16)")
    if x.dtype != gy.dtype:
        raise RuntimeError(f"mx grad_weight: x is {x.dtype} and gy is {gy.dtype}")
    if out_dtype is None:
        out_dtype = gy.dtype
    if out_dtype not in (gy.dtype, torch.float32):
        raise RuntimeError(f"mx grad_weight: out_dtype {out_dtype} must be gy's dtype or float32")
    if gy.dim() != 2 or x.dim() != 2 or gy.shape[0] != x.shape[0]:
        raise RuntimeError(f"mx grad_weight: gy {tuple(gy.shape)} and x {tuple(x.shape)} do not share their rows")
    M, N, K = gy.shape[0], gy.shape[1], x.shape[1]
    if M == 0:
        gw = torch.zeros((N, K), dtype=out_dtype, device=gy.device)
        return (gw, torch.zeros(N, dtype=out_dtype, device=gy.device)) if bias else gw
    gw = torch.empty((N, K), dtype=out_dtype, device=gy.device)
    gb = torch.empty(N, dtype=out_dtype, device=gy.device) if bias else None
    L = _hip.lib()
    nbytes = int(L.bie_mx_wgrad_workspace_bytes(M, N, K, int(splits)))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=gy.device) if nbytes else None
    gy, x = gy.contiguous(), _aligned(x)  # held until the launches are queued
    _hip.check(L.bie_mx_linear_grad_weight(_hip.ptr(gy), _hip.ptr(x), _hip.ptr(gw), _hip.ptr(gb), _hip.ptr(ws), M, N, K, _hip.dt(gy),
                                           int(out_dtype == torch.float32), int(splits), _hip.stream()), "bie_mx_linear_grad_weight")
    return (gw, gb) if bias else gw
