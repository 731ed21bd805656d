"""TernaryLinearCuda: ternary (TWN) weights x binary activations on the kernels of csrc/ternary.hip.

  y = dt( dt( dt(D) * scale_a ) * scale_w[n] ),   D = sum_k t[n, k] * sign(x + bias_a)[k]   (sign(0) = +1)

Training (train() and grad enabled, latent weight kept): the weight is re-ternarised and re-packed on every call (no image is cached
for a weight being trained), the forward runs on the kernels and the backward is the torch composition of TernaryLinearForward.
Eval: the packed qweight / scale_w, images remembered on them; a forward with grad enabled still runs (and is differentiable in x,
bias_a and scale_a)."""
import typing

import torch
from torch.autograd import Function

from bitorch_engine.utils import ste
from bitorch_engine.utils.safe_import import import_extension
from bitorch_engine.utils.model_helper import flatten_x, unflatten_x
from ..layer import TernaryLinearBase, ternarize

ternary_linear_cuda = import_extension("ternary_linear_cuda")


class TernaryLinearForward(Function):
    """Forward: the layer kernels on xb = x + bias_a (already added, in the layer dtype).  Backward (TWN straight-through estimator):
      grad_x       = (gy . (alpha * T)) * 1{-1 <= xb / scale_a <= 1}
      grad_weight  = gy^T . (sign(xb) * scale_a)        (the float latent weight, as if t were W)
      grad_scale_a = ste.binary_scale_grad(grad_x, sign(xb))"""

    @staticmethod
    def forward(ctx, xb, weight, scale_a, qweight, alpha, cache):
        ctx.save_for_backward(xb, scale_a, qweight, alpha)
        return ternary_linear_cuda.layer_forward(xb, None, qweight, scale_a, alpha, cache=cache)

    @staticmethod
    @typing.no_type_check
    def backward(ctx, gy):
        xb, scale_a, qweight, alpha = ctx.saved_tensors
        w_hat = ternary_linear_cuda.w_unpack(qweight).to(gy.dtype) * alpha.to(gy.dtype)[:, None]
        sign_x = torch.where(xb >= 0, 1.0, -1.0).to(gy.dtype)
        grad_x = gy.mm(w_hat)
        _, _, _, inside = ste.clip_masks(xb, scale_a, -1.0, 1.0)
        grad_x.mul_(inside)
        grad_w = gy.t().mm(sign_x * scale_a) if ctx.needs_input_grad[1] else None
        grad_sa = ste.binary_scale_grad(grad_x, sign_x).reshape(scale_a.shape) if ctx.needs_input_grad[2] else None
        return grad_x, grad_w, grad_sa, None, None, None


class TernaryLinearCuda(TernaryLinearBase):
    def __init__(self, *args, bmm_type=None, threshold_factor: float = 0.7, **kwargs):
        """The constructor arguments of BinaryLinearCuda (bmm_type is accepted for that reason; the ternary kernels have one weight
        format) plus threshold_factor (TWN: delta = threshold_factor * mean|W| per output row)."""
        super().__init__(*args, threshold_factor=threshold_factor, **kwargs)
        self.bmm_type = bmm_type

    def _ternary(self):
        """(qweight, scale_w) of the current latent weight, packed now."""
        t, alpha, _ = ternarize(self.weight, self.threshold_factor)
        return ternary_linear_cuda.w_pack(t), alpha.to(self.dtype)

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
        dev = self.bias_a.device
        self.qweight = ternary_linear_cuda.w_pack(trits.to(device=dev, dtype=torch.int8))
        self.scale_w = alpha.reshape(-1).to(device=dev, dtype=self.dtype)
        self.weight = None
        self._packed = True

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        self._check_forward(x)
        self._init_scale_a(x)
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
        grad = torch.is_grad_enabled() and (x.requires_grad or self.bias_a.requires_grad or self.scale_a.requires_grad or
                                            (training and self.weight.requires_grad))
        if not grad:  # the whole layer (bias add + sign-pack, the product, cast, both scales) on the kernels
            out = ternary_linear_cuda.layer_forward(x2, self.bias_a.detach(), qweight, self.scale_a.detach(), scale_w, cache=not training)
            return unflatten_x(out, lead)
        xb = x2 + self.bias_a
        out = TernaryLinearForward.apply(xb, self.weight if training else None, self.scale_a, qweight, scale_w, not training)
        return unflatten_x(out, lead)
