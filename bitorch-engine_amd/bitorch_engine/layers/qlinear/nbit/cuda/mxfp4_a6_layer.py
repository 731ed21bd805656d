"""MXFP4A6LinearCuda: the MXFP4 weights of MXFP4LinearCuda against activations quantised to MXFP6 (OCP E2M3 elements, E8M0 block scales)
on the fly, on the kernels of csrc/mxfp4_a6.hip (the block-scaled matrix instructions of gfx950 with an FP4 and an FP6 operand, which run
at the FP4 rate: half the matrix cycles of the W4A8 pair).

  x^[m, k] = e2m3(code) * 2^(sx[m, k // 32] - 127)   (the weight quantiser's rule with E2M3 elements per row and block of 32)
  y        = dt( x^ . W^^T + bias ),   a row of x that holds NaN or +-inf gives a NaN row of y

Parameters, buffers, the checkpoint contract, set_mx_weight and prepare_params are MXFP4LinearCuda's: a qweight / scales pair or a state
dict of MXFP4LinearCuda, MXFP4A4LinearCuda, MXFP4A8LinearCuda or this layer loads into the other three.  An MXFP6 layer's state dict
(qweight [N, 3K/4]) is refused.

What E2M3 activations give up against E4M3 ones is range inside a block: a value below 1/64 of its block's power-of-two maximum quantises
to zero.  On Gaussian data the two are equally accurate (INTEGRATION.md "MXFP4 W4A6 linear layer").

Training (train() with the latent weight): the weight is re-quantised on every call, the forward runs on the kernels and the backward is
the straight-through composition in fp32 through the E2M3-QUANTISED activations: grad_x = gy . W^ (or, with grad_input="kernel",
csrc/mxfp4_grad.hip on the packed weight), grad_weight = gy^T . x^, grad_bias = sum_m gy.  Eval: the packed weight; a forward with grad
enabled is differentiable in x (and bias)."""
import typing

import torch
from torch.autograd import Function

from bitorch_engine.utils.safe_import import import_extension
from bitorch_engine.utils.model_helper import flatten_x, unflatten_x
from .mxfp4_layer import MXFP4LinearCuda

mxfp4_a6_linear_cuda = import_extension("mxfp4_a6_linear_cuda")


class MXFP4A6LinearForward(Function):
    """Forward: the layer kernels.  Backward (straight-through estimator, in fp32, cast to the dtype):
      grad_x      = gy . W^           (identity through the activation quantiser)
                                      (kernel: mxfp4_a6_linear_cuda.grad_input on the packed weight, e_blk from the scales of this call)
      grad_weight = gy^T . x^         (the E2M3-quantised activations)
      grad_bias   = sum_m gy"""

    @staticmethod
    def forward(ctx, x, weight, bias, qweight, scales, e_col, kernel=False):
        ctx.save_for_backward(x, qweight, scales)
        ctx.kernel = kernel
        return mxfp4_a6_linear_cuda.forward(x, qweight, scales, bias, e_col)

    @staticmethod
    @typing.no_type_check
    def backward(ctx, gy):
        x, qweight, scales = ctx.saved_tensors
        grad_x = grad_w = grad_b = None
        if ctx.needs_input_grad[0]:
            if ctx.kernel:
                grad_x = mxfp4_a6_linear_cuda.grad_input(gy, qweight, scales)
            else:
                grad_x = gy.float().mm(mxfp4_a6_linear_cuda.dequant(qweight, scales, torch.float32)).to(gy.dtype)
        if ctx.needs_input_grad[1]:
            xq, xs, _ = mxfp4_a6_linear_cuda.quantize_act(x)
            grad_w = gy.float().t().mm(mxfp4_a6_linear_cuda.dequant_act(xq, xs, torch.float32)).to(gy.dtype)
        if ctx.needs_input_grad[2]:
            grad_b = gy.float().sum(0).to(gy.dtype)
        return grad_x, grad_w, grad_b, None, None, None, None


class MXFP4A6LinearCuda(MXFP4LinearCuda):
    """MXFP4LinearCuda's state and interface (latent `weight`, `qweight` uint8 [N, K/2], `scales` uint8 [N, K/32], optional `bias`;
    K % 32 == 0, 32 <= K <= 2^20; fp16 or bf16; grad_input "torch" or "kernel") with the W4A6 forward."""

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs):
        q = state_dict.get(prefix + "qweight")
        if q is not None and tuple(q.shape) == (self.output_features, self.input_features // 32 * 24):
            error_msgs.append(f"{prefix}qweight {tuple(q.shape)} is an MXFP6 weight (6-bit E2M3 codes, 3K/4 bytes per row); MXFP4A6LinearCuda holds "
                              f"4-bit E2M1 codes in [N, K/2] = {tuple(self.qweight.shape)} and does not reinterpret it: load the latent weight, or "
                              f"dequantise and re-quantise")
            return
        super()._load_from_state_dict(state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        assert x.size(-1) == self.input_features, f"Weight and input tensor mismatch: {x.size(-1)} != {self.input_features}"
        assert x.dtype == self.dtype, f"dtype mismatch. Expected: '{self.dtype}', but '{x.dtype}' found"
        x2, lead = flatten_x(x)
        training = self.training and self.weight is not None
        if training:  # re-quantised every call: the weight may have changed since the last one
            self._packed = False
            with torch.no_grad():
                qweight, scales = mxfp4_a6_linear_cuda.quantize(self.weight)
            e_col = None  # computed by the forward
        else:
            if not self._packed:
                self.prepare_params()
            qweight, scales, e_col = self.qweight, self.scales, self.e_col
        grad = torch.is_grad_enabled() and (x.requires_grad or (training and self.weight.requires_grad)
                                            or (self.bias is not None and self.bias.requires_grad))
        if not grad:
            return unflatten_x(mxfp4_a6_linear_cuda.forward(x2, qweight, scales, self.bias, e_col), lead)
        out = MXFP4A6LinearForward.apply(x2, self.weight if training else None, self.bias, qweight, scales, e_col, self.grad_input == "kernel")
        return unflatten_x(out, lead)
