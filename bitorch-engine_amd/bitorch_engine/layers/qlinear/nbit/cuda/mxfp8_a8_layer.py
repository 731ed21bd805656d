"""MXFP8A8LinearCuda: OCP microscaling FP8 weights (e4m3fn elements, E8M0 scale per block of 32 along K) against activations quantised to
the same format on the fly, on the kernels of csrc/mxfp8_a8.hip (the block-scaled matrix instructions of gfx950 with two E4M3 operands).

  W^[n, k] = e4m3(qweight[n, k]) * 2^(scales[n, k // 32] - 127)      x^[m, k] = e4m3(code) * 2^(sx[m, k // 32] - 127)
  y        = dt( x^ . W^^T + bias ),   a row of x that holds NaN or +-inf gives a NaN row of y

qweight uint8 [N, K] holds one e4m3fn byte per weight, row-major; scales uint8 [N, K/32].  e_col (the largest scale code per row, 255
where a row has a NaN block) is derived from scales and not saved.  The checkpoint contract is MXFP6A8LinearCuda's with these shapes: a
state dict holds the latent `weight` (while there is one), `qweight`, `scales` and `bias`; a qweight-only one drops the latent weight.
An MXFP4 state dict (qweight [N, K/2]) and an MXFP6 one ([N, 3K/4]) are refused: the codes are a different format, not a different
packing.

What the layer is for: loading MXFP8 checkpoints unchanged, and E4M3's range inside a block (a value down to 2^-9 of its block's
power-of-two maximum survives, where E2M3 stops at 1/64).  It is not more accurate than MXFP6 on Gaussian weights (both carry three
mantissa bits; INTEGRATION.md "MXFP8 W8A8 linear layer"), and a pair of E4M3 operands runs at half the FP4 / FP6 matrix rate.

Training (train() with the latent weight): the weight is re-quantised on every call, the forward runs on the kernels and the backward
is the straight-through composition in fp32 with the QUANTISED activations in the weight gradient.  Eval: the packed weight; a forward
with grad enabled is differentiable in x (and bias).  There is no packed-weight input gradient for MXFP8: grad_input is "torch" only."""
import math
import typing

import torch
from torch import nn
from torch.autograd import Function

from bitorch_engine.utils.safe_import import import_extension
from bitorch_engine.utils.model_helper import flatten_x, unflatten_x
from bitorch_engine.layers.qlinear.ternary.layer import TernaryWeightState

mxfp8_a8_linear_cuda = import_extension("mxfp8_a8_linear_cuda")


class MXFP8A8LinearForward(Function):
    """Forward: the layer kernels.  Backward (straight-through estimator, in fp32 through the kernel dequant, cast to the dtype):
      grad_x      = gy . W^           (identity through the activation quantiser)
      grad_weight = gy^T . x^         (the E4M3-quantised activations)
      grad_bias   = sum_m gy"""

    @staticmethod
    def forward(ctx, x, weight, bias, qweight, scales, e_col):
        ctx.save_for_backward(x, qweight, scales)
        return mxfp8_a8_linear_cuda.forward(x, qweight, scales, bias, e_col)

    @staticmethod
    @typing.no_type_check
    def backward(ctx, gy):
        x, qweight, scales = ctx.saved_tensors
        grad_x = grad_w = grad_b = None
        if ctx.needs_input_grad[0]:
            grad_x = gy.float().mm(mxfp8_a8_linear_cuda.dequant(qweight, scales, torch.float32)).to(gy.dtype)
        if ctx.needs_input_grad[1]:
            xq, xs, _ = mxfp8_a8_linear_cuda.quantize_act(x)
            grad_w = gy.float().t().mm(mxfp8_a8_linear_cuda.dequant_act(xq, xs, torch.float32)).to(gy.dtype)
        if ctx.needs_input_grad[2]:
            grad_b = gy.float().sum(0).to(gy.dtype)
        return grad_x, grad_w, grad_b, None, None, None


class MXFP8A8LinearCuda(TernaryWeightState, nn.Module):
    """Float latent `weight` [N, K] (kept while training; dropped by generate_quantized_weight(qweight_only=True) or set_mx_weight), the
    e4m3fn codes `qweight` uint8 [N, K] and E8M0 `scales` uint8 [N, K/32] (buffers), an optional `bias` [N].
    K % 32 == 0, 32 <= K <= 2^20; dtype fp16 or bf16.  grad_input: "torch" only (the backward's grad_x from an fp32 image of W)."""

    def __init__(self, input_features: int, out_features: int, bias: bool = False, device: torch.device = None,
                 dtype: torch.dtype = torch.float16, grad_input: str = "torch") -> None:
        super().__init__()
        if grad_input == "kernel":
            raise ValueError('grad_input="kernel": no packed-weight input gradient exists for MXFP8; use "torch"')
        if grad_input != "torch":
            raise ValueError(f'grad_input must be "torch" (got {grad_input!r})')
        self.grad_input = grad_input
        if input_features % 32 or input_features <= 0 or input_features > (1 << 20) or out_features <= 0:
            raise ValueError(f"mxfp8 a8 linear needs input_features % 32 == 0, 32 <= input_features <= 2^20 and out_features >= 1 "
                             f"(got {input_features}, {out_features})")
        if dtype not in (torch.float16, torch.bfloat16):
            raise ValueError(f"mxfp8 a8 linear computes in fp16 or bf16 (got {dtype})")
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
                self.qweight, self.scales = mxfp8_a8_linear_cuda.quantize(self.weight)
            self.e_col = mxfp8_a8_linear_cuda.col_exp(self.scales)
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
            error_msgs.append(f"{prefix}qweight {tuple(q.shape)} is {what}; MXFP8A8LinearCuda holds 8-bit E4M3 codes in [N, K] = "
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
                qweight, scales = mxfp8_a8_linear_cuda.quantize(self.weight)
            e_col = None  # computed by the forward
        else:
            if not self._packed:
                self.prepare_params()
            qweight, scales, e_col = self.qweight, self.scales, self.e_col
        grad = torch.is_grad_enabled() and (x.requires_grad or (training and self.weight.requires_grad)
                                            or (self.bias is not None and self.bias.requires_grad))
        if not grad:
            return unflatten_x(mxfp8_a8_linear_cuda.forward(x2, qweight, scales, self.bias, e_col), lead)
        out = MXFP8A8LinearForward.apply(x2, self.weight if training else None, self.bias, qweight, scales, e_col)
        return unflatten_x(out, lead)
