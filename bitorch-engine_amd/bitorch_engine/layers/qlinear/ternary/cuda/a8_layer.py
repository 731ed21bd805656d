"""TernaryA8LinearCuda: ternary weights x int8 per-token activations (BitNet b1.58 "BitLinear") on the kernels of csrc/ternary_a8.hip.

  y = dt( (float(D) * r_m) * scale_w[n] ),   D = sum_k t[n, k] * q[m, k],   q = clamp(rint(x * 127 / a_m), -128, 127),  r_m = a_m / 127

The activation scale is dynamic (per row, absmax), so the layer has no bias_a / scale_a and no output bias.  Weights are ternarised by
the absmean rule (ternarize_absmean) into TernaryLinearCuda's qweight format: a qweight / scale_w pair loads into either layer.

Training (train() with the latent weight): re-ternarised and re-packed on every call, the forward runs on the kernels and the backward
is the straight-through composition of TernaryA8LinearForward in torch.  Eval: the packed qweight / scale_w; a forward with grad
enabled is differentiable in x."""
import math
import typing

import torch
from torch import nn
from torch.autograd import Function

from bitorch_engine.utils.safe_import import import_extension
from bitorch_engine.utils.model_helper import flatten_x, unflatten_x
from ..layer import TernaryWeightState, ternarize_absmean

ternary_a8_linear_cuda = import_extension("ternary_a8_linear_cuda")


class TernaryA8LinearForward(Function):
    """Forward: the layer kernels.  Backward (BitNet straight-through estimator):
      grad_x      = gy . (alpha * T)
      grad_weight = gy^T . (q * r)        (the float latent weight, as if it were alpha * T; q * r is the quantised x)"""

    @staticmethod
    def forward(ctx, x, weight, qweight, alpha):
        ctx.save_for_backward(x, qweight, alpha)
        return ternary_a8_linear_cuda.layer_forward(x, qweight, alpha)

    @staticmethod
    @typing.no_type_check
    def backward(ctx, gy):
        x, qweight, alpha = ctx.saved_tensors
        grad_x = grad_w = None
        if ctx.needs_input_grad[0]:
            w_hat = ternary_a8_linear_cuda.w_unpack(qweight).to(gy.dtype) * alpha.to(gy.dtype)[:, None]
            grad_x = gy.mm(w_hat)
        if ctx.needs_input_grad[1]:
            q, r = ternary_a8_linear_cuda.quantize(x)
            grad_w = gy.t().mm((q.float() * r[:, None]).to(gy.dtype))
        return grad_x, grad_w, None, None


class TernaryA8LinearCuda(TernaryWeightState, nn.Module):
    """Float latent `weight` [N, K] (kept while training; dropped by generate_quantized_weight(qweight_only=True) or set_ternary_weight),
    the packed trits `qweight` uint8 [2, N, K/8] and their per-row scale `scale_w` [N] (buffers).  K % 32 == 0, K <= 65536."""

    def __init__(self, input_features: int, out_features: int, device: torch.device = None, dtype: torch.dtype = torch.float) -> None:
        super().__init__()
        if input_features % 32 or input_features <= 0 or input_features > 65536 or out_features <= 0:
            raise ValueError(f"ternary a8 linear needs input_features % 32 == 0, input_features <= 65536 and out_features >= 1 "
                             f"(got {input_features}, {out_features})")
        self.input_features, self.output_features = input_features, out_features
        self.device, self.dtype = device, dtype
        w = torch.empty((out_features, input_features), dtype=dtype, device=device)
        nn.init.kaiming_uniform_(w, a=math.sqrt(5))
        self.weight = nn.Parameter(w)
        self.register_buffer("qweight", torch.zeros((2, out_features, input_features // 8), dtype=torch.uint8, device=device))
        self.register_buffer("scale_w", torch.zeros(out_features, dtype=dtype, device=device))
        self._packed = False  # qweight / scale_w hold the current weight (or a loaded / set ternary weight)

    def _state_device(self) -> torch.device:
        return self.scale_w.device

    def _ternary(self):
        """(qweight, scale_w) of the current latent weight, packed now."""
        t, alpha = ternarize_absmean(self.weight)
        return ternary_a8_linear_cuda.w_pack(t.to(self.weight.device)), alpha.to(device=self.weight.device, dtype=self.dtype)

    def prepare_params(self) -> None:
        """qweight / scale_w from the latent weight (a no-op for a layer that holds only the packed weight)."""
        if self.weight is None:
            return
        with torch.no_grad():
            self.qweight, self.scale_w = self._ternary()
        self._packed = True

    def set_ternary_weight(self, trits: torch.Tensor, alpha: torch.Tensor) -> None:
        """Load exact trits [N, K] (int8 in {-1, 0, +1}) and scales alpha [N] (rounded once to the layer dtype); the latent weight is
        dropped, so the layer computes with exactly these values in every mode."""
        assert tuple(trits.shape) == (self.output_features, self.input_features) and alpha.numel() == self.output_features
        dev = self.scale_w.device
        self.qweight = ternary_a8_linear_cuda.w_pack(trits.to(device=dev, dtype=torch.int8))
        self.scale_w = alpha.reshape(-1).to(device=dev, dtype=self.dtype)
        self.weight = None
        self._packed = True

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        assert x.size(-1) == self.input_features, f"Weight and input tensor mismatch: {x.size(-1)} != {self.input_features}"
        assert x.dtype == self.dtype, f"dtype mismatch. Expected: '{self.dtype}', but '{x.dtype}' found"
        x2, lead = flatten_x(x)
        training = self.training and self.weight is not None
        if training:  # re-ternarised and re-packed every call: the weight may have changed since the last one
            self._packed = False
            with torch.no_grad():
                qweight, scale_w = self._ternary()
        else:
            if not self._packed:
                self.prepare_params()
            qweight, scale_w = self.qweight, self.scale_w
        grad = torch.is_grad_enabled() and (x.requires_grad or (training and self.weight.requires_grad))
        if not grad:
            return unflatten_x(ternary_a8_linear_cuda.layer_forward(x2, qweight, scale_w), lead)
        out = TernaryA8LinearForward.apply(x2, self.weight if training else None, qweight, scale_w)
        return unflatten_x(out, lead)
