"""MXFP4LinearCuda: OCP microscaling FP4 weights x fp16 / bf16 activations on the kernels of csrc/mxfp4.hip.

  y = dt( x . W^T + bias ),   W[n, k] = e2m1(qweight nibble) * 2^(scales[n, k // 32] - 127)

qweight uint8 [N, K/2] and scales uint8 [N, K/32] are byte for byte the `blocks` / `scales` of gpt-oss-style MXFP4 checkpoints
(set_mx_weight).  e_col (the largest scale code per row, which the prefill form rebiases by) is derived from scales and not saved.

Training (train() with the latent weight): re-quantised on every call by the OCP MX rule, the forward runs on the kernels and the
backward is the straight-through composition in torch.  Eval: the packed qweight / scales; a forward with grad enabled is
differentiable in x (and bias).  grad_input="kernel" takes grad_x from the packed weight instead (csrc/mxfp4_grad.hip: no float image
of W is built), in train() and in eval(); the default "torch" dequantises W to fp32 and multiplies."""
import math
import typing

import torch
from torch import nn
from torch.autograd import Function

from bitorch_engine.utils.safe_import import import_extension
from bitorch_engine.utils.model_helper import flatten_x, unflatten_x
from bitorch_engine.layers.qlinear.ternary.layer import TernaryWeightState
from bitorch_engine.layers.qlinear.nbit.cuda.mx_grad_weight import GradWeightChoice, weight_grads

mxfp4_linear_cuda = import_extension("mxfp4_linear_cuda")


class MXFP4LinearForward(Function):
    """Forward: the layer kernels.  Backward (straight-through estimator, in fp32, cast to the dtype):
      grad_x      = gy . W            (kernel: mxfp4_linear_cuda.grad_input on the packed weight, e_blk from the scales of this call)
      grad_weight = gy^T . x          (the float latent weight, as if it were W)
      grad_bias   = sum_m gy          (with wkernel=True both from one call of csrc/mx_wgrad.hip: mx_grad_weight.weight_grads)"""

    @staticmethod
    def forward(ctx, x, weight, bias, qweight, scales, e_col, kernel=False, wkernel=False):
        ctx.save_for_backward(x, qweight, scales)
        ctx.kernel, ctx.wkernel = kernel, wkernel
        return mxfp4_linear_cuda.forward(x, qweight, scales, bias, e_col)

    @staticmethod
    @typing.no_type_check
    def backward(ctx, gy):
        x, qweight, scales = ctx.saved_tensors
        grad_x = None
        if ctx.needs_input_grad[0]:
            if ctx.kernel:
                grad_x = mxfp4_linear_cuda.grad_input(gy, qweight, scales)
            else:
                grad_x = gy.float().mm(mxfp4_linear_cuda.dequant(qweight, scales, torch.float32)).to(gy.dtype)
        grad_w, grad_b = weight_grads(gy, x, ctx.needs_input_grad[1], ctx.needs_input_grad[2], ctx.wkernel)
        return grad_x, grad_w, grad_b, None, None, None, None, None


class MXFP4LinearCuda(GradWeightChoice, TernaryWeightState, nn.Module):
    """Float latent `weight` [N, K] (kept while training; dropped by generate_quantized_weight(qweight_only=True) or set_mx_weight),
    the packed codes `qweight` uint8 [N, K/2] and E8M0 `scales` uint8 [N, K/32] (buffers), an optional `bias` [N].
    K % 32 == 0, K <= 2^20; dtype fp16 or bf16.  grad_input: "torch" (the backward's grad_x from an fp32 image of W) or "kernel" (from
    the packed weight).  grad_weight: "torch" or "kernel" (grad_weight and grad_bias from csrc/mx_wgrad.hip), an attribute of the object
    only: not a constructor argument, not saved (mx_grad_weight.py)."""

    def __init__(self, input_features: int, out_features: int, bias: bool = False, device: torch.device = None,
                 dtype: torch.dtype = torch.float16, grad_input: str = "torch") -> None:
        super().__init__()
        if grad_input not in ("torch", "kernel"):
            raise ValueError(f'grad_input must be "torch" or "kernel" (got {grad_input!r})')
        self.grad_input = grad_input
        if input_features % 32 or input_features <= 0 or input_features > (1 << 20) or out_features <= 0:
            raise ValueError(f"mxfp4 linear needs input_features % 32 == 0, 32 <= input_features <= 2^20 and out_features >= 1 "
                             f"(got {input_features}, {out_features})")
        if dtype not in (torch.float16, torch.bfloat16):
            raise ValueError(f"mxfp4 linear computes in fp16 or bf16 (got {dtype})")
        self.input_features, self.output_features = input_features, out_features
        self.device, self.dtype = device, dtype
        w = torch.empty((out_features, input_features), dtype=dtype, device=device)
        nn.init.kaiming_uniform_(w, a=math.sqrt(5))
        self.weight = nn.Parameter(w)
        self.bias = nn.Parameter(torch.zeros(out_features, dtype=dtype, device=device)) if bias else None
        self.register_buffer("qweight", torch.zeros((out_features, input_features // 2), dtype=torch.uint8, device=device))
        self.register_buffer("scales", torch.zeros((out_features, input_features // 32), dtype=torch.uint8, device=device))
        self.register_buffer("e_col", torch.zeros(out_features, dtype=torch.uint8, device=device), persistent=False)
        self._packed = False  # qweight / scales / e_col hold the current weight (or a loaded / set MXFP4 weight)

    def _state_device(self) -> torch.device:
        return self.qweight.device

    def prepare_params(self) -> None:
        """qweight / scales from the latent weight (kept as they are for a layer that holds only the packed weight), then e_col."""
        with torch.no_grad():
            if self.weight is not None:
                self.qweight, self.scales = mxfp4_linear_cuda.quantize(self.weight)
            self.e_col = mxfp4_linear_cuda.col_exp(self.scales)
        self._packed = True

    def set_mx_weight(self, blocks: torch.Tensor, scales: torch.Tensor) -> None:
        """Load an MXFP4 weight: blocks uint8 [N, K/2] or [N, K/32, 16] (the checkpoint layout), scales uint8 [N, K/32].  The latent weight
        is dropped, so the layer computes with exactly these values in every mode."""
        N, K = self.output_features, self.input_features
        if blocks.dtype != torch.uint8 or scales.dtype != torch.uint8:
            raise ValueError("set_mx_weight: blocks and scales must be uint8")
        if tuple(blocks.shape) == (N, K // 32, 16):
            blocks = blocks.reshape(N, K // 2)
        if tuple(blocks.shape) != (N, K // 2) or tuple(scales.shape) != (N, K // 32):
            raise ValueError(f"set_mx_weight: blocks {tuple(blocks.shape)} / scales {tuple(scales.shape)} do not match [N={N}, K={K}]")
        dev = self.qweight.device
        self.qweight = blocks.to(dev).contiguous()
        self.scales = scales.to(dev).contiguous()
        self.weight = None
        self.prepare_params()

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs):
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
                qweight, scales = mxfp4_linear_cuda.quantize(self.weight)
            e_col = None  # computed by the forward where the prefill form needs it
        else:
            if not self._packed:
                self.prepare_params()
            qweight, scales, e_col = self.qweight, self.scales, self.e_col
        grad = torch.is_grad_enabled() and (x.requires_grad or (training and self.weight.requires_grad)
                                            or (self.bias is not None and self.bias.requires_grad))
        if not grad:
            return unflatten_x(mxfp4_linear_cuda.forward(x2, qweight, scales, self.bias, e_col), lead)
        out = MXFP4LinearForward.apply(x2, self.weight if training else None, self.bias, qweight, scales, e_col, self.grad_input == "kernel",
                                       self.grad_weight == "kernel")
        return unflatten_x(out, lead)
