"""Ternary-weight / binary-activation linear (csrc/ternary.hip).  No reference implementation exists; the format and the semantics
are this library's own (include/bie_hip.h, INTEGRATION.md "Ternary linear layer"):

  qweight  uint8 [2, N, K/8]: plane 0 = non-zero mask, plane 1 = "value is +1"; bit j of byte b holds k = 8b + j.  K % 32 == 0.
  D[m, n]  = sum_k t[n, k] * s[m, k],  s = +1 where (x + bias_a) >= 0 else -1          (exact integer)
  y[m, n]  = dt( dt( dt(D) * scale_a ) * alpha[n] )

w_pack / w_unpack convert between trits and qweight, forward returns the raw D as fp32, layer_forward the layer output: one launch
(decode form) where bie_ternary_linear_fused_ok says so, else the x image + the matrix-pipe GEMM."""
import torch

from bitorch_engine import _hip
from ._binary_common import sign_dt
from .q_linear_cuda import _cached


def _shape(qweight: torch.Tensor):
    if qweight.dtype != torch.uint8 or qweight.dim() != 3 or qweight.shape[0] != 2:
        raise RuntimeError(f"ternary qweight must be uint8 [2, N, K/8], got {qweight.dtype} {tuple(qweight.shape)}")
    return qweight.shape[1], qweight.shape[2] * 8


def w_pack(trits: torch.Tensor) -> torch.Tensor:
    """trits [N, K] (int8 in {-1, 0, +1}, or any tensor whose sign is the trit) -> qweight uint8 [2, N, K/8]."""
    _hip.need_gpu(trits)
    N, K = trits.shape
    t = trits.to(torch.int8).contiguous() if trits.dtype != torch.int8 else trits.contiguous()
    q = torch.empty((2, N, K // 8), dtype=torch.uint8, device=trits.device)
    _hip.check(_hip.lib().bie_ternary_pack(_hip.ptr(t), _hip.ptr(q), N, K, _hip.stream()), "bie_ternary_pack")
    return q


def w_unpack(qweight: torch.Tensor) -> torch.Tensor:
    """qweight uint8 [2, N, K/8] -> trits int8 [N, K]."""
    _hip.need_gpu(qweight)
    N, K = _shape(qweight)
    q = qweight.contiguous()
    t = torch.empty((N, K), dtype=torch.int8, device=qweight.device)
    _hip.check(_hip.lib().bie_ternary_unpack(_hip.ptr(q), _hip.ptr(t), N, K, _hip.stream()), "bie_ternary_unpack")
    return t


def fp4_image(qweight: torch.Tensor) -> torch.Tensor:
    """The weights' FP4 image for the matrix-pipe form (bie_ternary_fp4_image)."""
    _hip.need_gpu(qweight)
    N, K = _shape(qweight)
    L = _hip.lib()
    q = qweight.contiguous()
    img = torch.empty(L.bie_binary_fp4_image_bytes(N, K), dtype=torch.uint8, device=qweight.device)
    _hip.check(L.bie_ternary_fp4_image(_hip.ptr(q), _hip.ptr(img), N, K, _hip.stream()), "bie_ternary_fp4_image")
    return img


def fused_ok(M: int, N: int, K: int) -> bool:
    return bool(_hip.lib().bie_ternary_linear_fused_ok(M, N, K))


def _aligned(t):
    return t if t is None or t.data_ptr() % 16 == 0 else t.clone()


def linear_fused(x, qweight, bias_a=None, scale_a=None, alpha=None, raw=False):
    """One launch (bie_ternary_linear_fused): x [M, K] -> y [M, N] in x's dtype, or with raw the fp32 D."""
    _hip.need_gpu(x, qweight)
    N, K = _shape(qweight)
    x = _aligned(x.contiguous())
    M = x.shape[0]
    same = lambda t: None if t is None else t.to(device=x.device, dtype=x.dtype).contiguous()
    bias_a, scale_a, alpha = _aligned(same(bias_a)), same(scale_a), same(alpha)
    y = torch.empty((M, N), dtype=torch.float32 if raw else x.dtype, device=x.device)
    _hip.check(_hip.lib().bie_ternary_linear_fused(_hip.ptr(x), _hip.ptr(bias_a), _hip.ptr(qweight.contiguous()), _hip.ptr(scale_a), _hip.ptr(alpha),
                                                   _hip.ptr(y), M, N, K, _hip.dt(x), int(raw), _hip.stream()), "bie_ternary_linear_fused")
    return y


def linear_fp4(x, qweight, bias_a=None, scale_a=None, alpha=None, wimage=None):
    """Matrix-pipe form (two launches): x image with the bias add (bie_binary_fp4_image_from_values), then the FP4 GEMM with the
    per-column alpha epilogue (bie_ternary_linear_layer_fp4).  wimage: the weights' image (built here when None)."""
    _hip.need_gpu(x, qweight)
    N, K = _shape(qweight)
    x = x.contiguous()
    M = x.shape[0]
    L = _hip.lib()
    same = lambda t: None if t is None else t.to(device=x.device, dtype=x.dtype).contiguous()
    bias_a, scale_a, alpha = same(bias_a), same(scale_a), same(alpha)
    if wimage is None:
        wimage = fp4_image(qweight)
    ximg = _hip.scratch(L.bie_binary_fp4_image_bytes(M, K), x.device)
    _hip.check(L.bie_binary_fp4_image_from_values(_hip.ptr(x), _hip.ptr(bias_a), _hip.ptr(ximg), M, K, sign_dt(x), _hip.stream()),
               "bie_binary_fp4_image_from_values")
    y = torch.empty((M, N), dtype=x.dtype, device=x.device)
    _hip.check(L.bie_ternary_linear_layer_fp4(_hip.ptr(ximg), _hip.ptr(wimage), _hip.ptr(scale_a), _hip.ptr(alpha), _hip.ptr(y), M, N, K, _hip.dt(x),
                                              _hip.stream()), "bie_ternary_linear_layer_fp4")
    return y


def forward(x: torch.Tensor, qweight: torch.Tensor) -> torch.Tensor:
    """Raw D [M, N] fp32 of sign(x) against the trits (no bias, no scales)."""
    N, K = _shape(qweight)
    M = x.shape[0]
    if M == 0:
        return torch.empty((0, N), dtype=torch.float32, device=x.device)
    if fused_ok(M, N, K):
        return linear_fused(x, qweight, raw=True)
    # the matrix-pipe GEMM in fp32 with no scales returns D itself (an exact integer below 2^24)
    return linear_fp4(x.float(), qweight, wimage=_cached(qweight, ("ternary_fp4",), lambda: fp4_image(qweight)))


def layer_forward(x, bias_a, qweight, scale_a, scale_w, cache: bool = True):
    """TernaryLinearCuda's forward on x [M, K]: the decode form where bie_ternary_linear_fused_ok holds, else the matrix-pipe form.
    cache: remember the weights' FP4 image on qweight (frozen / eval weights only; a weight under training is re-packed every call)."""
    if x.dtype not in _hip._DT:
        raise RuntimeError(f"ternary linear: dtype {x.dtype} is not supported")
    N, K = _shape(qweight)
    M = x.shape[0]
    if M == 0:
        return torch.empty((0, N), dtype=x.dtype, device=x.device)
    if fused_ok(M, N, K):
        return linear_fused(x, qweight, bias_a, scale_a, scale_w)
    wimage = _cached(qweight, ("ternary_fp4",), lambda: fp4_image(qweight)) if cache else fp4_image(qweight)
    return linear_fp4(x, qweight, bias_a, scale_a, scale_w, wimage=wimage)
