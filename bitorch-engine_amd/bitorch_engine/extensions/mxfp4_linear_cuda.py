"""MXFP4 (OCP microscaling FP4) weights x fp16 / bf16 activations (csrc/mxfp4.hip).  No reference implementation exists; the format and
the arithmetic are this library's own (include/bie_hip.h, INTEGRATION.md "MXFP4 linear layer"):

  qweight uint8 [N, K/2]  (element 2j in the low nibble of byte j)     scales uint8 [N, K/32]  (E8M0: 2^(s - 127), 255 = NaN)
  W[n, k] = e2m1(code) * 2^(s - 127)                                   y = dt( x . W^T + bias )  (fp32 sums, one rounding)

quantize / dequant convert between a float weight and the packed pair, col_exp gives the per-row largest scale code the prefill form
rebiases by, forward runs the layer (the form from bie_mxfp4_form unless one is given).  grad_input is the backward's gx = gy . W on
the packed weight (csrc/mxfp4_grad.hip), rebiased by blk_exp's per-block-column largest scale code.  Nothing here synchronises with
the host, so every entry can be captured in a graph."""
import torch

from bitorch_engine import _hip
from bitorch_engine.extensions import _mx_w16
from bitorch_engine.extensions._mx_w16 import _X_DT, _aligned  # noqa: F401  (the other MX modules import them from here)


def _shape(qweight: torch.Tensor, scales: torch.Tensor):
    if qweight.dtype != torch.uint8 or qweight.dim() != 2 or scales.dtype != torch.uint8 or scales.dim() != 2:
        raise RuntimeError("mxfp4: qweight must be uint8 [N, K/2] and scales uint8 [N, K/32]")
    N, K = qweight.shape[0], qweight.shape[1] * 2
    if tuple(scales.shape) != (N, K // 32) or K % 32 or K == 0:
        raise RuntimeError(f"mxfp4: scales {tuple(scales.shape)} do not match qweight {tuple(qweight.shape)} (K % 32 == 0 required)")
    return N, K


def quantize(weight: torch.Tensor):
    """float weight [N, K] (fp32 / fp16 / bf16) -> (qweight uint8 [N, K/2], scales uint8 [N, K/32]) by the OCP MX v1.0 rule."""
    _hip.need_gpu(weight)
    N, K = weight.shape
    w = _aligned(weight.detach())
    qweight = torch.empty((N, K // 2), dtype=torch.uint8, device=w.device)
    scales = torch.empty((N, K // 32), dtype=torch.uint8, device=w.device)
    _hip.check(_hip.lib().bie_mxfp4_quantize(_hip.ptr(w), _hip.ptr(qweight), _hip.ptr(scales), N, K, _hip.dt(w), _hip.stream()), "bie_mxfp4_quantize")
    return qweight, scales


def dequant(qweight: torch.Tensor, scales: torch.Tensor, dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """W [N, K] in dtype: computed exactly in fp32, rounded once (fp16 overflows to inf beyond 65504)."""
    _hip.need_gpu(qweight, scales)
    N, K = _shape(qweight, scales)
    w = torch.empty((N, K), dtype=dtype, device=qweight.device)
    qweight, scales = _aligned(qweight), scales.contiguous()
    _hip.check(_hip.lib().bie_mxfp4_dequant(_hip.ptr(qweight), _hip.ptr(scales), _hip.ptr(w), N, K, _hip.dt(w), _hip.stream()), "bie_mxfp4_dequant")
    return w


def col_exp(scales: torch.Tensor) -> torch.Tensor:
    """e_col uint8 [N]: the largest scale code of each row (255 where a row has a NaN block)."""
    _hip.need_gpu(scales)
    N, KB = scales.shape
    e = torch.empty(N, dtype=torch.uint8, device=scales.device)
    scales = scales.contiguous()
    _hip.check(_hip.lib().bie_mxfp4_col_exp(_hip.ptr(scales), _hip.ptr(e), N, KB * 32, _hip.stream()), "bie_mxfp4_col_exp")
    return e


def form(M: int, N: int, K: int, dtype: torch.dtype = torch.float16) -> int:
    """0 = decode form, 1 = prefill form (bie_mxfp4_form)."""
    return int(_hip.lib().bie_mxfp4_form(M, N, K, _hip._DT[dtype]))


def forward(x: torch.Tensor, qweight: torch.Tensor, scales: torch.Tensor, bias: torch.Tensor = None, e_col: torch.Tensor = None,
            form: int = -1) -> torch.Tensor:
    """x [M, K] (fp16 / bf16) -> y [M, N] in x's dtype.  form -1 = the plan.  e_col (col_exp(scales)) is read by the prefill form only:
    when it is not given and that form is taken, it is computed here."""
    return _LAYER.forward(x, qweight, scales, bias, e_col, form)


def blk_exp(scales: torch.Tensor) -> torch.Tensor:
    """e_blk uint8 [K/32]: the largest scale code of each block-column over the N rows (255 where a block-column has a NaN block)."""
    _hip.need_gpu(scales)
    if scales.dtype != torch.uint8 or scales.dim() != 2:
        raise RuntimeError("mxfp4: scales must be uint8 [N, K/32]")
    N, KB = scales.shape
    e = torch.empty(KB, dtype=torch.uint8, device=scales.device)
    scales = scales.contiguous()
    _hip.check(_hip.lib().bie_mxfp4_blk_exp(_hip.ptr(scales), _hip.ptr(e), N, KB * 32, 1, _hip.stream()), "bie_mxfp4_blk_exp")
    return e


def grad_input(gy: torch.Tensor, qweight: torch.Tensor, scales: torch.Tensor, e_blk: torch.Tensor = None) -> torch.Tensor:
    """gy [M, N] (fp16 / bf16, any N) -> gx = gy . W [M, K] in gy's dtype, from the packed weight: no image of W is built.  e_blk
    (blk_exp(scales)) is computed here when it is not given."""
    return _LAYER.grad_input(gy, qweight, scales, e_blk)


_LAYER = _mx_w16.Dense("mxfp4", "mxfp4", _shape, col_exp, blk_exp)
