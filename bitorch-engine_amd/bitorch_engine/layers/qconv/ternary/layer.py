"""Ternary (TWN) weight / binary activation conv2d: the base type.  There is no reference implementation; the semantics are this library's
own ("Ternary conv2d layer").  The ternarisation and the state-dict contract are the ternary linear's."""
import math

import torch
from torch import nn

from bitorch_engine.layers.qlinear.ternary.layer import TernaryWeightState


class TernaryConv2dBase(TernaryWeightState, nn.Module):
    """Float latent `weight` [OC, C, k, k] (kept while training; dropped by generate_quantized_weight(qweight_only=True) or
    set_ternary_weight), the packed trits `qweight` uint8 [2, OC, C*k*k/8] (the ternary linear's format over the OIHW flatten order) and
    their per-output-channel scale `scale_w` [OC] (buffers), the learnable activation bias `bias_a` [C] and scale `scale_a` (initialised on
    the first forward to 2 * mean|x|, 4 * when not symmetric).  No output bias."""

    def __init__(self, in_channels: int, out_channels: int, kernel_size: int, stride: int = 1, padding: int = 0, dilation: int = 1,
                 device: torch.device = None, dtype: torch.dtype = torch.float, symmetric: bool = True, threshold_factor: float = 0.7) -> None:
        super().__init__()
        if in_channels % 32 or in_channels <= 0 or out_channels <= 0 or kernel_size <= 0:
            raise ValueError(f"ternary conv2d needs in_channels % 32 == 0, out_channels >= 1 and kernel_size >= 1 "
                             f"(got {in_channels}, {out_channels}, {kernel_size})")
        if in_channels * kernel_size * kernel_size >= 1 << 24:
            raise ValueError(f"ternary conv2d needs in_channels * kernel_size^2 < 2^24 (got {in_channels} * {kernel_size}^2)")
        self.in_channels, self.out_channels, self.kernel_size = in_channels, out_channels, kernel_size
        self.stride, self.padding, self.dilation = stride, padding, dilation
        self.device, self.dtype, self.symmetric, self.threshold_factor = device, dtype, symmetric, threshold_factor
        w = torch.empty((out_channels, in_channels, kernel_size, kernel_size), dtype=dtype, device=device)
        nn.init.kaiming_uniform_(w, a=math.sqrt(5))
        self.weight = nn.Parameter(w)
        self.bias_a = nn.Parameter(torch.zeros(in_channels, dtype=dtype, device=device))
        self.scale_a = nn.Parameter(torch.tensor(0, dtype=dtype, device=device))
        K = in_channels * kernel_size * kernel_size
        self.register_buffer("qweight", torch.zeros((2, out_channels, K // 8), dtype=torch.uint8, device=device))
        self.register_buffer("scale_w", torch.zeros(out_channels, dtype=dtype, device=device))
        self._packed = False  # qweight / scale_w hold the current weight (or a loaded / set ternary weight)

    def prepare_params(self) -> None:
        raise NotImplementedError("Subclasses should implement this method.")

    def _check_forward(self, x: torch.Tensor) -> None:
        assert x.dim() == 4 and x.size(1) == self.in_channels, f"Dimension mismatch of the input tensor {tuple(x.shape)}: C = {self.in_channels}"
        assert x.dtype == self.dtype, f"dtype mismatch. Expected: '{self.dtype}', but '{x.dtype}' found"
