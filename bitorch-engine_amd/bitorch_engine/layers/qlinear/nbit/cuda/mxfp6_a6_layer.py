"""MXFP6A6LinearCuda: OCP microscaling FP6 weights (E2M3 elements, E8M0 scale per block of 32 along K) against activations quantised to
the same format on the fly, on the kernels of csrc/mxfp6_a6.hip (the block-scaled matrix instructions of gfx950 with two FP6 operands,
which run at the FP4 rate: half the matrix cycles of any pair with an E4M3 operand).

  W^[n, k] = e2m3(code) * 2^(scales[n, k // 32] - 127)      x^[m, k] = e2m3(code) * 2^(sx[m, k // 32] - 127)
  y        = dt( x^ . W^^T + bias ),   a row of x that holds NaN or +-inf gives a NaN row of y

The weight side, the buffers, the checkpoint contract, set_mx_weight, prepare_params and the training rule are MXFP6A8LinearCuda's
(mxfp6_a8_layer.py): the class derives from it and replaces the kernels.  The three MXFP6 linear layers (W6A16, W6A8, W6A6) hold the
same state and load each other's state dicts; an MXFP4 state dict is refused.

What E2M3 activations give up against E4M3 ones is range inside a block: a value below 1/64 of its block's power-of-two maximum
quantises to zero (E4M3 keeps it down to 2^-9 of the maximum and beyond, with subnormals).  On Gaussian data the two are equally
accurate (INTEGRATION.md "MXFP6 W6A6 linear layer").

The backward is the straight-through composition in fp32 through the FP6-QUANTISED activations: grad_x = gy . W^ (or, with
grad_input="kernel", csrc/mxfp6_grad.hip on the packed weight), grad_weight = gy^T . x^, grad_bias = sum_m gy."""
import typing

import torch
from torch.autograd import Function

from bitorch_engine.utils.safe_import import import_extension
from bitorch_engine.utils.model_helper import flatten_x, unflatten_x
from .mxfp6_a8_layer import MXFP6A8LinearCuda

mxfp6_a6_linear_cuda = import_extension("mxfp6_a6_linear_cuda")


class MXFP6A6LinearForward(Function):
    """Forward: the layer kernels.  Backward (straight-through estimator, in fp32 through the kernel dequant, cast to the dtype):
      grad_x      = gy . W^           (identity through the activation quantiser)
                                      (kernel: mxfp6_a6_linear_cuda.grad_input on the packed weight, e_blk from the scales of this call)
      grad_weight = gy^T . x^         (the E2M3-quantised activations)
      grad_bias   = sum_m gy"""

    @staticmethod
    def forward(ctx, x, weight, bias, qweight, scales, e_col, kernel=False):
        ctx.save_for_backward(x, qweight, scales)
        ctx.kernel = kernel
        return mxfp6_a6_linear_cuda.forward(x, qweight, scales, bias, e_col)

    @staticmethod
    @typing.no_type_check
    def backward(ctx, gy):
        x, qweight, scales = ctx.saved_tensors
        grad_x = grad_w = grad_b = None
        if ctx.needs_input_grad[0]:
            if ctx.kernel:
                grad_x = mxfp6_a6_linear_cuda.grad_input(gy, qweight, scales)
            else:
                grad_x = gy.float().mm(mxfp6_a6_linear_cuda.dequant(qweight, scales, torch.float32)).to(gy.dtype)
        if ctx.needs_input_grad[1]:
            xq, xs, _ = mxfp6_a6_linear_cuda.quantize_act(x)
            grad_w = gy.float().t().mm(mxfp6_a6_linear_cuda.dequant_act(xq, xs, torch.float32)).to(gy.dtype)
        if ctx.needs_input_grad[2]:
            grad_b = gy.float().sum(0).to(gy.dtype)
        return grad_x, grad_w, grad_b, None, None, None, None


class MXFP6A6LinearCuda(MXFP6A8LinearCuda):
    """MXFP6A8LinearCuda's state and interface (latent `weight`, buffers `qweight` uint8 [N, 3K/4] / `scales` uint8 [N, K/32] / `e_col`,
    optional `bias`; K % 32 == 0, 32 <= K <= 2^20; fp16 or bf16; grad_input "torch" or "kernel") with MXFP6 activations."""

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs):
        q = state_dict.get(prefix + "qweight")
        if q is not None and tuple(q.shape) == (self.output_features, self.input_features // 2):
            error_msgs.append(f"{prefix}qweight {tuple(q.shape)} is an MXFP4 weight (4-bit E2M1 codes, K/2 bytes per row); MXFP6A6LinearCuda holds "
                              f"6-bit E2M3 codes in [N, 3K/4] = {tuple(self.qweight.shape)} and does not reinterpret it: load the latent weight, or "
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
                qweight, scales = mxfp6_a6_linear_cuda.quantize(self.weight)
            e_col = None  # computed by the forward
        else:
            if not self._packed:
                self.prepare_params()
            qweight, scales, e_col = self.qweight, self.scales, self.e_col
        grad = torch.is_grad_enabled() and (x.requires_grad or (training and self.weight.requires_grad)
                                            or (self.bias is not None and self.bias.requires_grad))
        if not grad:
            return unflatten_x(mxfp6_a6_linear_cuda.forward(x2, qweight, scales, self.bias, e_col), lead)
        out = MXFP6A6LinearForward.apply(x2, self.weight if training else None, self.bias, qweight, scales, e_col, self.grad_input == "kernel")
        return unflatten_x(out, lead)
