"""Ternary weights x int8 per-token activations (csrc/ternary_a8.hip), the BitNet b1.58 "BitLinear" arithmetic.  No reference
implementation exists; the arithmetic is this library's own (include/bie_hip.h, INTEGRATION.md "Ternary W1.58A8 linear layer"):

  a_m = max(max_k |x[m, k]|, 1e-5),  q[m, k] = clamp(rint(x[m, k] * (127 / a_m)), -128, 127),  r_m = a_m / 127     (fp32)
  D[m, n] = sum_k t[n, k] * q[m, k]  (exact int32)           y[m, n] = dt((float(D) * r_m) * alpha[n])

qweight is TernaryLinearCuda's uint8 [2, N, K/8] (w_pack / w_unpack of ternary_linear_cuda).  forward returns the raw D, layer_forward
the layer output: one launch (decode form) where bie_ternary_a8_fused_ok says so, else the quantise launch and the matrix-pipe GEMM.
Nothing here synchronises with the host, so every entry can be captured in a graph."""
import torch

from bitorch_engine import _hip
from .ternary_linear_cuda import _shape, w_pack, w_unpack  # noqa: F401  (the weight format is the ternary linear's)


def _x(x: torch.Tensor) -> torch.Tensor:
    if x.dtype not in _hip._DT:
        raise RuntimeError(f"ternary a8 linear: dtype {x.dtype} is not supported")
    x = x.contiguous()
    return x if x.data_ptr() % 16 == 0 else x.clone()


def _alpha(alpha, x):
    return None if alpha is None else alpha.reshape(-1).to(device=x.device, dtype=x.dtype).contiguous()


def _quantize(x: torch.Tensor, ldq: int):
    M, K = x.shape
    q = torch.empty((M, ldq), dtype=torch.int8, device=x.device)
    r = torch.empty(M, dtype=torch.float32, device=x.device)
    _hip.check(_hip.lib().bie_ternary_a8_quantize(_hip.ptr(x), _hip.ptr(q), _hip.ptr(r), M, K, ldq, _hip.dt(x), _hip.stream()),
               "bie_ternary_a8_quantize")
    return q, r


def quantize(x: torch.Tensor):
    """x [M, K] -> (q int8 [M, K], r fp32 [M]): the per-token absmax quantisation both forms compute."""
    _hip.need_gpu(x)
    x = _x(x)
    if x.shape[0] == 0:
        return torch.empty(x.shape, dtype=torch.int8, device=x.device), torch.empty(0, dtype=torch.float32, device=x.device)
    return _quantize(x, x.shape[1])


def fused_ok(M: int, N: int, K: int) -> bool:
    return bool(_hip.lib().bie_ternary_a8_fused_ok(M, N, K))


def _out(M, N, x, raw):
    return torch.empty((M, N), dtype=torch.int32 if raw else x.dtype, device=x.device)


def linear_fused(x, qweight, alpha=None, raw=False):
    """One launch (bie_ternary_a8_linear_fused): x [M, K] -> y [M, N] in x's dtype, or with raw the int32 D."""
    _hip.need_gpu(x, qweight, alpha)
    N, K = _shape(qweight)
    x = _x(x)
    M = x.shape[0]
    alpha = None if raw else _alpha(alpha, x)
    y = _out(M, N, x, raw)
    _hip.check(_hip.lib().bie_ternary_a8_linear_fused(_hip.ptr(x), _hip.ptr(qweight.contiguous()), _hip.ptr(alpha), _hip.ptr(y), M, N, K, _hip.dt(x),
                                                      int(raw), _hip.stream()), "bie_ternary_a8_linear_fused")
    return y


def linear_gemm(x, qweight, alpha=None, raw=False):
    """Matrix-pipe form (two launches): the quantisation into rows padded to 64 bytes, then the i8 GEMM with the r_m / alpha_n
    epilogue (bie_ternary_a8_linear_gemm)."""
    _hip.need_gpu(x, qweight, alpha)
    N, K = _shape(qweight)
    x = _x(x)
    M = x.shape[0]
    alpha = None if raw else _alpha(alpha, x)
    ldq = (K + 63) // 64 * 64
    q, r = _quantize(x, ldq)
    y = _out(M, N, x, raw)
    _hip.check(_hip.lib().bie_ternary_a8_linear_gemm(_hip.ptr(q), _hip.ptr(r), ldq, _hip.ptr(qweight.contiguous()), _hip.ptr(alpha), _hip.ptr(y), M, N, K,
                                                     _hip.dt(x), int(raw), _hip.stream()), "bie_ternary_a8_linear_gemm")
    return y


def _run(x, qweight, alpha, raw):
    _hip.need_gpu(x, qweight, alpha)
    N, K = _shape(qweight)
    M = x.shape[0]
    if M == 0:
        return torch.empty((0, N), dtype=torch.int32 if raw else x.dtype, device=x.device)
    if fused_ok(M, N, K):
        return linear_fused(x, qweight, alpha, raw)
    return linear_gemm(x, qweight, alpha, raw)


def forward(x: torch.Tensor, qweight: torch.Tensor) -> torch.Tensor:
    """Raw D [M, N] int32 of the quantised x against the trits."""
    return _run(x, qweight, None, True)


def layer_forward(x: torch.Tensor, qweight: torch.Tensor, scale_w: torch.Tensor) -> torch.Tensor:
    """TernaryA8LinearCuda's forward on x [M, K]: the decode form where bie_ternary_a8_fused_ok holds, else the GEMM form."""
    return _run(x, qweight, scale_w, False)
