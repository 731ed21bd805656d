"""MXFP8LinearCuda: OCP microscaling FP8 weights (e4m3fn elements, E8M0 scale per block of 32 along K) x fp16 / bf16 activations on the
kernels of csrc/mxfp8.hip: the weight-only (W8A16) layer, MXFP6LinearCuda's contract with E4M3 elements.  The activations are left alone.

  y = dt( x . W^T + bias ),   W[n, k] = e4m3(qweight[n, k]) * 2^(scales[n, k // 32] - 127)

qweight uint8 [N, K] (one e4m3fn byte per weight, row-major) and scales uint8 [N, K/32] are byte for byte those of MXFP8A8LinearCuda, so
the two layers load each other's state_dict.  e_col (the largest scale code per row, which the prefill form rebiases by) is derived from
scales and not saved.  An MXFP4 state dict (qweight [N, K/2]) and an MXFP6 one ([N, 3K/4]) are refused: the codes are a different
format, not a different packing.

Training (train() with the latent weight): re-quantised on every call by the OCP MX rule, the forward runs on the kernels and the
backward is the straight-through composition in torch.  Eval: the packed qweight / scales; a forward with grad enabled is
differentiable in x (and bias).  The attribute grad_input (not a constructor argument, not saved) chooses where grad_x comes from: "torch"
(the default) builds an fp32 image of W on every backward call; "kernel" takes it from the packed weight in one call
(csrc/mxfp8_grad.hip, extensions/mxfp8_grad_cuda.py: no image of W is built).  grad_weight and grad_bias are the same in both.
The attribute grad_weight (built the same way) chooses where they come from: "torch" (the default) or "kernel" (one call of
csrc/mx_wgrad.hip through extensions/mx_grad_weight_cuda.py: gy^T . x and the bias sum without an fp32 copy or a torch product)."""
import math
import typing

import torch
from torch import nn
from torch.autograd import Function

from bitorch_engine.utils.safe_import import import_extension
from bitorch_engine.utils.model_helper import flatten_x, unflatten_x
from bitorch_engine.layers.qlinear.ternary.layer import TernaryWeightState
from bitorch_engine.layers.qlinear.nbit.cuda.mx_grad_weight import GradWeightChoice, weight_grads

mxfp8_linear_cuda = import_extension("mxfp8_linear_cuda")
mxfp8_grad_cuda = import_extension("mxfp8_grad_cuda")


def _checked_grad_input(value):
    if value not in ("torch", "kernel"):
        raise ValueError(f'grad_input must be "torch" or "kernel" (got {value!r})')
    return value


class MXFP8LinearForward(Function):
    """Forward: the layer kernels.  Backward (straight-through estimator, in fp32, cast to the dtype):
      grad_x      = gy . W            (W dequantised to fp32; with kernel=True one call of mxfp8_grad_cuda.grad_input on the packed weight)
      grad_weight = gy^T . x          (the float latent weight, as if it were W)
      grad_bias   = sum_m gy          (with wkernel=True both from one call of csrc/mx_wgrad.hip: mx_grad_weight.weight_grads)"""

    @staticmethod
    def forward(ctx, x, weight, bias, qweight, scales, e_col, kernel=False, wkernel=False):
        ctx.save_for_backward(x, qweight, scales)
        ctx.kernel, ctx.wkernel = kernel, wkernel
        return mxfp8_linear_cuda.forward(x, qweight, scales, bias, e_col)

    @staticmethod
    @typing.no_type_check
    def backward(ctx, gy):
        x, qweight, scales = ctx.saved_tensors
        grad_x = None
        if ctx.needs_input_grad[0]:
            if ctx.kernel:
                grad_x = mxfp8_grad_cuda.grad_input(gy, qweight, scales)
            else:
                grad_x = gy.float().mm(mxfp8_linear_cuda.dequant(qweight, scales, torch.float32)).to(gy.dtype)
        grad_w, grad_b = weight_grads(gy, x, ctx.needs_input_grad[1], ctx.needs_input_grad[2], ctx.wkernel)
        return grad_x, grad_w, grad_b, None, None, None, None, None


class MXFP8LinearCuda(GradWeightChoice, TernaryWeightState, nn.Module):
    """Float latent `weight` [N, K] (kept while training; dropped by generate_quantized_weight(qweight_only=True) or set_mx_weight), the
    e4m3fn codes `qweight` uint8 [N, K] and E8M0 `scales` uint8 [N, K/32] (buffers), an optional `bias` [N].
    K % 32 == 0, 32 <= K <= 2^20; dtype fp16 or bf16.  grad_input: "torch" or "kernel", an attribute of the object only (the module
    docstring)."""

    _grad_input = "torch"

    @property
    def grad_input(self) -> str:
        return self._grad_input

    @grad_input.setter
    def grad_input(self, value: str) -> None:
        self._grad_input = _checked_grad_input(value)

    def __init__(self, input_features: int, out_features: int, bias: bool = False, device: torch.device = None,
                 dtype: torch.dtype = torch.float16) -> None:
        super().__init__()
        if input_features % 32 or input_features <= 0 or input_features > (1 << 20) or out_features <= 0:
            raise ValueError(f"mxfp8 linear needs input_features % 32 == 0, 32 <= input_features <= 2^20 and out_features >= 1 "
                             f"(got {input_features}, {out_features})")
        if dtype not in (torch.float16, torch.bfloat16):
            raise ValueError(f"mxfp8 linear computes in fp16 or bf16 (got {dtype})")
        self.input_features, self.output_features = input_features, out_features
        self.device, self.dtype = device, dtype
        w = torch.empty((out_features, input_features), dtype=dtype, device=device)
        nn.init.kaiming_uniform_(w, a=math.sqrt(5))
        self.weight = nn.Parameter(w)
        self.bias = nn.Parameter(torch.zeros(out_features, dtype=dtype, device=device)) if bias else None
        self.register_buffer("qweight", torch.zeros((out_features, input_features), dtype=torch.uint8, device=device))
        self.register_buffer("scales", torch.zeros((out_features, input_features // 32), dtype=torch.uint8, device=device))
        self.register_buffer("e_col", torch.zeros(out_features, dtype=torch.uint8, device=device), persistent=False)
        self._packed = False  # qweight / scales / e_col hold the current weight (or a loaded / set MXFP8 weight)

    def _state_device(self) -> torch.device:
        return self.qweight.device

    def prepare_params(self) -> None:
        """qweight / scales from the latent weight (kept as they are for a layer that holds only the packed weight), then e_col."""
        with torch.no_grad():
            if self.weight is not None:
                self.qweight, self.scales = mxfp8_linear_cuda.quantize(self.weight)
            self.e_col = mxfp8_linear_cuda.col_exp(self.scales)
        self._packed = True

    def set_mx_weight(self, blocks: torch.Tensor, scales: torch.Tensor) -> None:
        """Load an MXFP8 weight: blocks uint8 [N, K] or [N, K/32, 32] (e4m3fn bytes), scales uint8 [N, K/32].  The latent weight is
        dropped, so the layer computes with exactly these values in every mode.  A tensor that holds an E4M3 NaN code (0x7F / 0xFF) is
        refused: a NaN block is spelled with scale code 255."""
        N, K = self.output_features, self.input_features
        if blocks.dtype != torch.uint8 or scales.dtype != torch.uint8:
            raise ValueError("set_mx_weight: blocks and scales must be uint8")
        if tuple(blocks.shape) == (N, K // 32, 32):
            blocks = blocks.reshape(N, K)
        if tuple(blocks.shape) != (N, K) or tuple(scales.shape) != (N, K // 32):
            raise ValueError(f"set_mx_weight: blocks {tuple(blocks.shape)} / scales {tuple(scales.shape)} do not match an MXFP8 weight "
                             f"[N={N}, K={K}] (32 bytes per block of 32)")
        nan = (blocks & 0x7F) == 0x7F
        if bool(nan.any()):
            n, k = (int(v) for v in nan.nonzero()[0])
            raise ValueError(f"set_mx_weight: blocks[{n}, {k}] = 0x{int(blocks[n, k]):02X} is an E4M3 NaN code ({int(nan.sum())} in all); a NaN "
                             f"block of an MXFP8 weight is written as scale code 255")
        dev = self.qweight.device
        self.qweight = blocks.to(dev).contiguous()
        self.scales = scales.to(dev).contiguous()
        self.weight = None
        self.prepare_params()

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs):
        q = state_dict.get(prefix + "qweight")
        N, K = self.output_features, self.input_features
        if q is not None and tuple(q.shape) in ((N, K // 2), (N, K // 32 * 24)):
            what = "an MXFP4 weight (4-bit E2M1 codes, K/2 bytes per row)" if q.shape[1] == K // 2 else \
                "an MXFP6 weight (6-bit E2M3 codes, 3K/4 bytes per row)"
            error_msgs.append(f"{prefix}qweight {tuple(q.shape)} is {what}; MXFP8LinearCuda holds 8-bit E4M3 codes in [N, K] = "
                              f"{tuple(self.qweight.shape)} and does not reinterpret it: load the latent weight, or dequantise and re-quantise")
            return
        super()._load_from_state_dict(state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs)
        self._packed = False  # e_col is re-derived (and, with a latent weight, qweight / scales) before the next packed forward

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        assert x.size(-1) == self.input_features, f"Weight and input tensor mismatch: {x.size(-1)} != {self.input_features}"
        assert x.dtype == self.dtype, f"dtype mismatch. Expected: '{self.dtype}', but '{x.dtype}' found"
        x2, lead = flatten_x(x)
        training = self.training and self.weight is not None
        if training:  # re-quantised every call: the weight may have changed since the last one
            self._packed = False
            with torch.no_grad():
                qweight, scales = mxfp8_linear_cuda.quantize(self.weight)
            e_col = None  # computed by the forward where the prefill form needs it
        else:
            if not self._packed:
                self.prepare_params()
            qweight, scales, e_col = self.qweight, self.scales, self.e_col
        grad = torch.is_grad_enabled() and (x.requires_grad or (training and self.weight.requires_grad)
                                            or (self.bias is not None and self.bias.requires_grad))
        if not grad:
            return unflatten_x(mxfp8_linear_cuda.forward(x2, qweight, scales, self.bias, e_col), lead)
        out = MXFP8LinearForward.apply(x2, self.weight if training else None, self.bias, qweight, scales, e_col, self.grad_input == "kernel",
                                       self.grad_weight == "kernel")
        return unflatten_x(out, lead)
