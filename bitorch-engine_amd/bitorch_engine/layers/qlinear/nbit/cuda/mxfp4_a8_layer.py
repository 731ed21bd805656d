"""MXFP4A8LinearCuda: the MXFP4 weights of MXFP4LinearCuda against activations quantised to MXFP8 (E4M3 elements, E8M0 block scales) on
the fly, on the kernels of csrc/mxfp4_a8.hip (the block-scaled matrix instructions of gfx950 with an FP4 and an E4M3 operand).

  x^[m, k] = e4m3(code) * 2^(sx[m, k // 32] - 127)   (the OCP MX v1.0 rule with emax = 8 per row and block of 32)
  y        = dt( x^ . W^T + bias ),   a row of x that holds NaN or +-inf gives a NaN row of y

Parameters, buffers, the checkpoint contract and set_mx_weight are MXFP4LinearCuda's: a qweight / scales pair or a state dict of
MXFP4LinearCuda, MXFP4A4LinearCuda or this layer loads into the other two.

Training (train() with the latent weight): the weight is re-quantised on every call, the forward runs on the kernels and the backward
is the straight-through composition in torch with the QUANTISED activations in the weight gradient.  Eval: the packed weight; a forward
with grad enabled is differentiable in x (and bias)."""
import typing

import torch
from torch.autograd import Function

from bitorch_engine.utils.safe_import import import_extension
from bitorch_engine.utils.model_helper import flatten_x, unflatten_x
from .mxfp4_layer import MXFP4LinearCuda

mxfp4_a8_linear_cuda = import_extension("mxfp4_a8_linear_cuda")


class MXFP4A8LinearForward(Function):
    """Forward: the layer kernels.  Backward (straight-through estimator, in fp32, cast to the dtype):
      grad_x      = gy . W            (identity through the activation quantiser)
      grad_weight = gy^T . x^         (the E4M3-quantised activations)
      grad_bias   = sum_m gy"""

    @staticmethod
    def forward(ctx, x, weight, bias, qweight, scales, e_col):
        ctx.save_for_backward(x, qweight, scales)
        return mxfp4_a8_linear_cuda.forward(x, qweight, scales, bias, e_col)

    @staticmethod
    @typing.no_type_check
    def backward(ctx, gy):
        x, qweight, scales = ctx.saved_tensors
        grad_x = grad_w = grad_b = None
        if ctx.needs_input_grad[0]:
            grad_x = gy.float().mm(mxfp4_a8_linear_cuda.dequant(qweight, scales, torch.float32)).to(gy.dtype)
        if ctx.needs_input_grad[1]:
            xq, xs, _ = mxfp4_a8_linear_cuda.quantize_act(x)
            grad_w = gy.float().t().mm(mxfp4_a8_linear_cuda.dequant_act(xq, xs, torch.float32)).to(gy.dtype)
        if ctx.needs_input_grad[2]:
            grad_b = gy.float().sum(0).to(gy.dtype)
        return grad_x, grad_w, grad_b, None, None, None


class MXFP4A8LinearCuda(MXFP4LinearCuda):
    """MXFP4LinearCuda's state (latent `weight`, `qweight` uint8 [N, K/2], `scales` uint8 [N, K/32], optional `bias`) with the W4A8 forward.
    K % 32 == 0, K <= 2^20; dtype fp16 or bf16."""

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        assert x.size(-1) == self.input_features, f"Weight and input tensor mismatch: {x.size(-1)} != {self.input_features}"
        assert x.dtype == self.dtype, f"dtype mismatch. Expected: '{self.dtype}', but '{x.dtype}' found"
        x2, lead = flatten_x(x)
        training = self.training and self.weight is not None
        if training:  # re-quantised every call: the weight may have changed since the last one
            self._packed = False
            with torch.no_grad():
                qweight, scales = mxfp4_a8_linear_cuda.quantize(self.weight)
            e_col = None  # computed by the forward
        else:
            if not self._packed:
                self.prepare_params()
            qweight, scales, e_col = self.qweight, self.scales, self.e_col
        grad = torch.is_grad_enabled() and (x.requires_grad or (training and self.weight.requires_grad)
                                            or (self.bias is not None and self.bias.requires_grad))
        if not grad:
            return unflatten_x(mxfp4_a8_linear_cuda.forward(x2, qweight, scales, self.bias, e_col), lead)
        out = MXFP4A8LinearForward.apply(x2, self.weight if training else None, self.bias, qweight, scales, e_col)
        return unflatten_x(out, lead)
