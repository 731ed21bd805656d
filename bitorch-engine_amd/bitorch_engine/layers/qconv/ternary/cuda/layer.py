"""TernaryConv2dCuda: ternary (TWN) weights x binary activations, conv2d on the one-launch kernels of csrc/binary_conv_fused.hip (TERN
instances) or the general path (extensions/ternary_conv2d_cuda.py).

  y = dt( dt( dt(D) * scale_a ) * scale_w[oc] ),  D = conv2d(pad(sign(x + bias_a), value=-1), T, stride, dilation)   (sign(0) = +1)

Training (train() and grad enabled, latent weight kept): the weight is re-ternarised and re-packed on every call (no image is cached for a
weight being trained), the forward runs on the kernels and the backward is the torch composition of TernaryConv2dForward.  Eval: the
packed qweight / scale_w, images remembered on qweight; a forward with grad enabled still runs (and is differentiable in x, bias_a and
scale_a)."""
import typing

import torch
import torch.nn.functional as F
from torch.autograd import Function

from bitorch_engine.utils import ste
from bitorch_engine.utils.safe_import import import_extension
from bitorch_engine.layers.qlinear.ternary.layer import ternarize
from ..layer import TernaryConv2dBase

ternary_conv2d_cuda = import_extension("ternary_conv2d_cuda")


class TernaryConv2dForward(Function):
    """Forward: the layer kernels on xb = x + bias_a (already added, in the layer dtype).  Backward: the straight-through derivative of
    conv2d(pad(sign(xb), value=-1) * scale_a, alpha (.) T, stride, dilation):
      grad_x       = conv2d_input(gy, alpha (.) T) with the border cropped, times 1{-1 <= xb / scale_a <= 1}
      grad_weight  = conv2d_weight(pad(sign(xb), value=-1) * scale_a, gy)       (the float latent weight, as if T were W)
      grad_scale_a = ste.binary_scale_grad(grad_x, sign(xb))"""

    @staticmethod
    def forward(ctx, xb, weight, scale_a, qweight, alpha, geometry, cache):
        ctx.save_for_backward(xb, scale_a, qweight, alpha)
        ctx.geometry = geometry
        k, stride, pad, dil = geometry
        return ternary_conv2d_cuda.layer_forward(xb, qweight, scale_a, alpha, k, stride, pad, dil, cache=cache)

    @staticmethod
    @typing.no_type_check
    def backward(ctx, gy):
        xb, scale_a, qweight, alpha = ctx.saved_tensors
        k, stride, pad, dil = ctx.geometry
        C = xb.shape[1]
        w_hat = ternary_conv2d_cuda.w_unpack(qweight, C, k).to(gy.dtype) * alpha.to(gy.dtype)[:, None, None, None]
        sign_x = torch.where(xb >= 0, 1.0, -1.0).to(gy.dtype)
        # the -1 border is a constant: its gradient is cropped, which is conv2d_input with the padding
        grad_x = torch.nn.grad.conv2d_input(xb.shape, w_hat, gy, stride=stride, padding=pad, dilation=dil)
        _, _, _, inside = ste.clip_masks(xb, scale_a, -1.0, 1.0)
        grad_x = grad_x * inside
        grad_w = None
        if ctx.needs_input_grad[1]:
            xs = F.pad(sign_x, (pad, pad, pad, pad), value=-1.0) * scale_a
            grad_w = torch.nn.grad.conv2d_weight(xs, w_hat.shape, gy, stride=stride, padding=0, dilation=dil)
        grad_sa = ste.binary_scale_grad(grad_x, sign_x).reshape(scale_a.shape) if ctx.needs_input_grad[2] else None
        return grad_x, grad_w, grad_sa, None, None, None, None


class TernaryConv2dCuda(TernaryConv2dBase):
    def __init__(self, *args, threshold_factor: float = 0.7, **kwargs):
        """The constructor arguments of BinaryConv2dCutlass (in_channels, out_channels, kernel_size, stride, padding, dilation, device,
        dtype, symmetric) plus threshold_factor (TWN: delta = threshold_factor * mean|W| per output channel)."""
        super().__init__(*args, threshold_factor=threshold_factor, **kwargs)

    def _ternary(self):
        """(qweight, scale_w) of the current latent weight, packed now."""
        t, alpha, _ = ternarize(self.weight.reshape(self.out_channels, -1), self.threshold_factor)
        return ternary_conv2d_cuda.w_pack(t), alpha.to(self.dtype)

    def prepare_params(self) -> None:
        """qweight / scale_w from the latent weight (a no-op for a layer that holds only the packed weight)."""
        if self.weight is None:
            return
        with torch.no_grad():
            self.qweight, self.scale_w = self._ternary()
        self._packed = True

    def set_ternary_weight(self, trits: torch.Tensor, alpha: torch.Tensor) -> None:
        """Load exact trits [OC, C, k, k] (int8 in {-1, 0, +1}) and scales alpha [OC] (rounded once to the layer dtype); the latent weight
        is dropped, so the layer computes with exactly these values in every mode."""
        k = self.kernel_size
        assert tuple(trits.shape) == (self.out_channels, self.in_channels, k, k) and alpha.numel() == self.out_channels
        dev = self.bias_a.device
        self.qweight = ternary_conv2d_cuda.w_pack(trits.to(device=dev, dtype=torch.int8))
        self.scale_w = alpha.reshape(-1).to(device=dev, dtype=self.dtype)
        self.weight = None
        self._packed = True

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        self._check_forward(x)
        self._init_scale_a(x)
        geometry = (self.kernel_size, self.stride, self.padding, self.dilation)
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
        if not grad:
            xb = x + self.bias_a.detach().view(1, -1, 1, 1)
            return ternary_conv2d_cuda.layer_forward(xb, qweight, self.scale_a.detach(), scale_w, *geometry, cache=not training)
        xb = x + self.bias_a.view(1, -1, 1, 1)
        return TernaryConv2dForward.apply(xb, self.weight if training else None, self.scale_a, qweight, scale_w, geometry, not training)
