"""MXFP4A6ExpertsLinearCuda: the stacked expert projection of MXFP4ExpertsLinearCuda against activations quantised to MXFP6 (OCP E2M3
elements, E8M0 block scales) on the fly, on the kernels of csrc/mxfp4_moe_a6.hip (the block-scaled matrix instructions of gfx950 with
an FP4 and an FP6 operand, which run at the FP4 rate).

  x^[r, k] = e2m3(code) * 2^(sx[r, k // 32] - 127)   (the weight quantiser's rule with E2M3 elements per stored row of x and block of 32)
  y[t, s]  = dt( x^_row . W^[idx[t, s]]^T + bias[idx[t, s]] ),  NaN for a row of x that holds NaN or +-inf, +0 for a skipped slot
  x_row = x[t] for x [T, K] (every slot of a token reads the token's row) or x[t, s] for x [T, S, K]

The state (latent weight, qweight uint8 [E, N, K/2], scales uint8 [E, N, K/32], bias), the checkpoint contract, set_mx_weight and
grad_input are MXFP4ExpertsLinearCuda's, inherited: the weights are the same bytes, so MXFP4ExpertsLinearCuda, MXFP4A4ExpertsLinearCuda,
MXFP4A8ExpertsLinearCuda and this layer load each other's state dicts.  An MXFP6 state dict (qweight [E, N, 3K/4]) is refused.  Only the
activation format differs: E2M3 keeps three mantissa bits but two exponent bits, so within a block a value below 1/64 of the block's
power-of-two maximum becomes zero ("MXFP4 W4A6 mixture-of-experts layer").

Training: as the base class, with the E2M3-quantised activations in the weight gradient (experts_a8_backward with this layer's extension
module) and the identity through the activation quantiser in grad_x."""
import typing

import torch
from torch.autograd import Function

from bitorch_engine.utils.safe_import import import_extension
from .mxfp4_experts_a8_layer import experts_a8_backward
from .mxfp4_experts_layer import MXFP4ExpertsLinearCuda

mxfp4_experts_a6_cuda = import_extension("mxfp4_experts_a6_cuda")


class MXFP4A6ExpertsLinearForward(Function):
    """Forward: the W4A6 expert kernels.  Backward: MXFP4A8ExpertsLinearForward's straight-through composition with the MXFP6 activation
    quantiser: grad_weight[e] sees the E2M3-quantised activations.  With kernel=True grad_x is one call of grad_input on the packed
    weights."""

    @staticmethod
    def forward(ctx, x, idx, weight, bias, qweight, scales, e_col, kernel=False):
        ctx.save_for_backward(x, idx, qweight, scales)
        ctx.kernel = kernel
        return mxfp4_experts_a6_cuda.forward(x, idx, qweight, scales, bias, e_col)

    @staticmethod
    @typing.no_type_check
    def backward(ctx, gy):
        return experts_a8_backward(mxfp4_experts_a6_cuda, ctx.saved_tensors[3].shape[2] * 32, ctx, gy, ctx.kernel) + (None,)


class MXFP4A6ExpertsLinearCuda(MXFP4ExpertsLinearCuda):
    """MXFP4ExpertsLinearCuda with MXFP6 activations: the same parameters, buffers and methods; forward runs csrc/mxfp4_moe_a6.hip."""

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs):
        q = state_dict.get(prefix + "qweight")
        if q is not None and tuple(q.shape) == (self.num_experts, self.output_features, self.input_features // 32 * 24):
            error_msgs.append(f"{prefix}qweight {tuple(q.shape)} is an MXFP6 weight (6-bit E2M3 codes, 3K/4 bytes per row); MXFP4A6ExpertsLinearCuda "
                              f"holds 4-bit E2M1 codes in [E, N, K/2] = {tuple(self.qweight.shape)} and does not reinterpret it: load the latent "
                              f"weight, or dequantise and re-quantise")
            return
        super()._load_from_state_dict(state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs)

    def forward(self, x: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
        """x [T, K] or [T, S, K], idx int32 [T, S] (other integer types are converted) -> [T, S, N]."""
        assert x.size(-1) == self.input_features, f"Weight and input tensor mismatch: {x.size(-1)} != {self.input_features}"
        assert x.dtype == self.dtype, f"dtype mismatch. Expected: '{self.dtype}', but '{x.dtype}' found"
        if idx.dtype != torch.int32:
            idx = idx.to(torch.int32)
        training = self.training and self.weight is not None
        if training:  # re-quantised every call: the weight may have changed since the last one
            self._packed = False
            with torch.no_grad():
                qweight, scales = mxfp4_experts_a6_cuda.quantize(self.weight)
            e_col = None  # computed by the forward
        else:
            if not self._packed:
                self.prepare_params()
            qweight, scales, e_col = self.qweight, self.scales, self.e_col
        grad = torch.is_grad_enabled() and (x.requires_grad or (training and self.weight.requires_grad)
                                            or (self.bias is not None and self.bias.requires_grad))
        if not grad:
            return mxfp4_experts_a6_cuda.forward(x, idx, qweight, scales, self.bias, e_col)
        return MXFP4A6ExpertsLinearForward.apply(x, idx, self.weight if training else None, self.bias, qweight, scales, e_col,
                                                 self.grad_input == "kernel")
