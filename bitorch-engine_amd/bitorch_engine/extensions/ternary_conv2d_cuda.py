"""Ternary-weight / binary-activation conv2d (csrc/binary_conv_fused.hip, the TERN instances).  No reference implementation exists; the
format and the semantics are this library's own (include/bie_hip.h "ternary conv", INTEGRATION.md "Ternary conv2d layer"):

  qweight  uint8 [2, OC, C*k*k/8]: the ternary linear's format over the OIHW flatten order (k-index = c*k*k + kh*k + kw), C % 32 == 0
  D        [b, oc, oh, ow] = sum t[oc, c, kh, kw] * s[b, c, oh*stride - pad + kh*dil, ow*stride - pad + kw*dil],  s = +1 where xb >= 0,
           else -1 (NaN: -1); padded positions are s = -1                                                       (exact integer)
  y        = dt( dt( dt(D) * scale_a ) * alpha[oc] )

bie_ternary_conv2d_form decides the form: 1 = one launch on the VALU (lane images of the two tap-major planes), 2 = one launch on the
matrix pipe (the ternary FP4 image of the tap-major planes), 0 = the general path: F.pad(value=-1) -> F.unfold -> the ternary linear
(ternary_linear_cuda) -> NCHW, for any geometry with C % 32 == 0 (k = 5 / 7, dilation, C = 32 / 96 / 1024, rows wider than 128 pixels).
The weight images derive from qweight on the device; with cache they are remembered on qweight (frozen / eval weights only)."""
import torch
import torch.nn.functional as F

from bitorch_engine import _hip
from . import ternary_linear_cuda
from .q_linear_cuda import _cached


def _geometry(qweight: torch.Tensor, C: int, k: int):
    if qweight.dtype != torch.uint8 or qweight.dim() != 3 or qweight.shape[0] != 2 or qweight.shape[2] * 8 != C * k * k:
        raise RuntimeError(f"ternary conv qweight must be uint8 [2, OC, C*k*k/8] with C={C}, k={k}, got {qweight.dtype} {tuple(qweight.shape)}")
    if C % 32:
        raise RuntimeError(f"ternary conv needs C % 32 == 0, got C={C}")
    return qweight.shape[1]


def out_size(H: int, W: int, k: int, stride: int, pad: int, dil: int):
    return (H + 2 * pad - dil * (k - 1) - 1) // stride + 1, (W + 2 * pad - dil * (k - 1) - 1) // stride + 1


def w_pack(trits: torch.Tensor) -> torch.Tensor:
    """trits [OC, C, k, k] (int8 in {-1, 0, +1}, or any tensor whose sign is the trit) -> qweight uint8 [2, OC, C*k*k/8]."""
    return ternary_linear_cuda.w_pack(trits.reshape(trits.shape[0], -1))


def w_unpack(qweight: torch.Tensor, C: int, k: int) -> torch.Tensor:
    """qweight uint8 [2, OC, C*k*k/8] -> trits int8 [OC, C, k, k]."""
    OC = _geometry(qweight, C, k)
    return ternary_linear_cuda.w_unpack(qweight).reshape(OC, C, k, k)


def weight_taps(qweight: torch.Tensor, C: int, k: int) -> torch.Tensor:
    """The two planes re-laid tap-major (bie_binary_conv_weight_taps per plane): int32 [2, OC, k*k, C/32]."""
    _hip.need_gpu(qweight)
    OC = _geometry(qweight, C, k)
    q = qweight.contiguous()
    out = torch.empty((2, OC, k * k, C // 32), dtype=torch.int32, device=q.device)
    L = _hip.lib()
    for i in range(2):
        _hip.check(L.bie_binary_conv_weight_taps(_hip.ptr(q[i]), _hip.ptr(out[i]), OC, C, k, _hip.stream()), "bie_binary_conv_weight_taps")
    return out


def weight_lanes(qweight: torch.Tensor, C: int, k: int):
    """(mask, pos) lane images for the VALU form (bie_binary_conv_weight_lanes of each tap-major plane)."""
    _hip.need_gpu(qweight)
    OC = _geometry(qweight, C, k)
    if C % 128:
        raise RuntimeError(f"ternary conv: the VALU form's lane images need C to be a multiple of 128 (four K quarters of whole words), got C={C}")
    L = _hip.lib()
    taps = weight_taps(qweight, C, k)
    words = L.bie_binary_conv_weight_lanes_bytes(OC, C, k) // 4
    out = torch.empty((2, words), dtype=torch.int32, device=qweight.device)  # words is a multiple of 256: both planes 16-byte aligned
    for i in range(2):
        _hip.check(L.bie_binary_conv_weight_lanes(_hip.ptr(taps[i]), _hip.ptr(out[i]), OC, C, k, _hip.stream()), "bie_binary_conv_weight_lanes")
    return out[0], out[1]


def weight_fp4_image(qweight: torch.Tensor, C: int, k: int) -> torch.Tensor:
    """The ternary FP4 image of the tap-major planes for the matrix-pipe form (bie_ternary_fp4_image, rows OC, K = k*k*C)."""
    _hip.need_gpu(qweight)
    OC = _geometry(qweight, C, k)
    L = _hip.lib()
    K = k * k * C
    planes = weight_taps(qweight, C, k).view(torch.uint8).reshape(2, OC, K // 8)
    img = torch.empty(L.bie_binary_fp4_image_bytes(OC, K), dtype=torch.uint8, device=qweight.device)
    _hip.check(L.bie_ternary_fp4_image(_hip.ptr(planes), _hip.ptr(img), OC, K, _hip.stream()), "bie_ternary_fp4_image")
    return img


def form(B: int, C: int, H: int, W: int, OC: int, k: int, stride: int, pad: int, dil: int) -> int:
    """bie_ternary_conv2d_form: 1 = VALU one-launch, 2 = matrix-pipe one-launch, 0 = general path."""
    return int(_hip.lib().bie_ternary_conv2d_form(B, C, H, W, OC, k, stride, pad, dil))


def _operands(x, qweight, scale_a, alpha, raw, *images):
    """Every forward entry checks first that x, qweight and the weight images live on one GPU (no launch on a host pointer)."""
    _hip.need_gpu(x, qweight, *images)
    if x.dtype not in _hip._DT:
        raise RuntimeError(f"ternary conv: dtype {x.dtype} is not supported")
    same = lambda t: None if (t is None or raw) else t.to(device=x.device, dtype=x.dtype).contiguous()
    return x.contiguous(), same(scale_a), same(alpha)


def _out(x, OC, k, stride, pad, dil, raw):
    B, _, H, W = x.shape
    OH, OW = out_size(H, W, k, stride, pad, dil)
    return torch.empty((B, OC, OH, OW), dtype=torch.float32 if raw else x.dtype, device=x.device)


def conv_fused(xb, qweight, k, stride, pad, dil, scale_a=None, alpha=None, raw=False, lanes=None):
    """The VALU one-launch form through its C entry (bie_ternary_conv2d_forward_fused).  raw: the fp32 D, no scales."""
    xb, scale_a, alpha = _operands(xb, qweight, scale_a, alpha, raw, *(lanes or ()))
    B, C, H, W = xb.shape
    OC = _geometry(qweight, C, k)
    wm, wp = weight_lanes(qweight, C, k) if lanes is None else lanes
    y = _out(xb, OC, k, stride, pad, dil, raw)
    _hip.check(_hip.lib().bie_ternary_conv2d_forward_fused(_hip.ptr(xb), _hip.ptr(wm), _hip.ptr(wp), _hip.ptr(scale_a), _hip.ptr(alpha), _hip.ptr(y),
                                                           B, C, H, W, OC, k, stride, pad, dil, _hip.dt(xb), int(raw), _hip.stream()),
               "bie_ternary_conv2d_forward_fused")
    return y


def conv_mfma(xb, qweight, k, stride, pad, dil, scale_a=None, alpha=None, raw=False, wimage=None):
    """The matrix-pipe one-launch form through its C entry (bie_ternary_conv2d_forward_mfma).  raw: the fp32 D, no scales."""
    xb, scale_a, alpha = _operands(xb, qweight, scale_a, alpha, raw, wimage)
    B, C, H, W = xb.shape
    OC = _geometry(qweight, C, k)
    img = weight_fp4_image(qweight, C, k) if wimage is None else wimage
    y = _out(xb, OC, k, stride, pad, dil, raw)
    _hip.check(_hip.lib().bie_ternary_conv2d_forward_mfma(_hip.ptr(xb), _hip.ptr(img), _hip.ptr(scale_a), _hip.ptr(alpha), _hip.ptr(y),
                                                          B, C, H, W, OC, k, stride, pad, dil, _hip.dt(xb), int(raw), _hip.stream()),
               "bie_ternary_conv2d_forward_mfma")
    return y


def conv_general(xb, qweight, k, stride, pad, dil, scale_a=None, alpha=None, raw=False, cache=True):
    """The general path (form 0, any geometry with C % 32 == 0, not tuned): the -1-padded input unfolded into rows of C*k*k in the OIHW
    order, the ternary linear on them (its own forms: decode or matrix pipe), back to NCHW."""
    xb, scale_a, alpha = _operands(xb, qweight, scale_a, alpha, raw)
    B, C, H, W = xb.shape
    OC = _geometry(qweight, C, k)
    OH, OW = out_size(H, W, k, stride, pad, dil)
    xp = F.pad(xb, (pad, pad, pad, pad), value=-1.0) if pad else xb
    cols = F.unfold(xp, kernel_size=k, dilation=dil, stride=stride)          # [B, C*k*k, OH*OW], row index c*k*k + kh*k + kw
    rows = cols.transpose(1, 2).reshape(B * OH * OW, C * k * k)
    if raw:
        y = ternary_linear_cuda.forward(rows, qweight)
    else:
        y = ternary_linear_cuda.layer_forward(rows, None, qweight, scale_a, alpha, cache=cache)
    return y.reshape(B, OH * OW, OC).transpose(1, 2).reshape(B, OC, OH, OW).contiguous()


def _run(xb, qweight, k, stride, pad, dil, scale_a, alpha, raw, cache):
    _hip.need_gpu(xb, qweight)  # before any image of qweight is built
    B, C, H, W = xb.shape
    OC = _geometry(qweight, C, k)
    f = form(B, C, H, W, OC, k, stride, pad, dil)
    if f == 1:
        lanes = _cached(qweight, ("tconv_lanes", C, k), lambda: weight_lanes(qweight, C, k)) if cache else None
        return conv_fused(xb, qweight, k, stride, pad, dil, scale_a, alpha, raw, lanes=lanes)
    if f == 2:
        img = _cached(qweight, ("tconv_fp4", C, k), lambda: weight_fp4_image(qweight, C, k)) if cache else None
        return conv_mfma(xb, qweight, k, stride, pad, dil, scale_a, alpha, raw, wimage=img)
    return conv_general(xb, qweight, k, stride, pad, dil, scale_a, alpha, raw, cache)


def forward(x: torch.Tensor, qweight: torch.Tensor, k: int, stride: int = 1, pad: int = 0, dil: int = 1) -> torch.Tensor:
    """Raw D [B, OC, OH, OW] fp32 of sign(x) against the trits (no bias, no scales), on the form bie_ternary_conv2d_form picks."""
    return _run(x, qweight, k, stride, pad, dil, None, None, True, True)


def layer_forward(xb, qweight, scale_a, scale_w, k, stride=1, pad=0, dil=1, cache: bool = True):
    """TernaryConv2dCuda's forward on xb = x + bias_a [B, C, H, W]: y [B, OC, OH, OW] in xb's dtype on the form bie_ternary_conv2d_form
    picks.  cache: remember the weight images on qweight (frozen / eval weights only; a weight under training is re-packed every call)."""
    return _run(xb, qweight, k, stride, pad, dil, scale_a, scale_w, False, cache)
