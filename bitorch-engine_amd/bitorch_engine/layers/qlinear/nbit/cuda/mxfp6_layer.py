"""MXFP6LinearCuda: OCP microscaling FP6 weights (E2M3 elements, E8M0 scale per block of 32 along K) x fp16 / bf16 activations on the
kernels of csrc/mxfp6.hip: the weight-only (W6A16) layer, MXFP4LinearCuda's contract with E2M3 elements.

  y = dt( x . W^T + bias ),   W[n, k] = e2m3(code) * 2^(scales[n, k // 32] - 127)

qweight uint8 [N, 3K/4] (per row K/32 blocks of 24 bytes, code j of a block in bits 6 j .. 6 j + 5 of its little-endian 192-bit integer)
and scales uint8 [N, K/32] are byte for byte those of MXFP6A8LinearCuda, so the two layers load each other's state_dict.  e_col (the
largest scale code per row, which the prefill form rebiases by) is derived from scales and not saved.  An MXFP4 state dict (qweight
[N, K/2]) is refused: the codes are a different format, not a different packing.

Training (train() with the latent weight): re-quantised on every call by the OCP MX rule, the forward runs on the kernels and the
backward is the straight-through composition in torch.  Eval: the packed qweight / scales; a forward with grad enabled is
differentiable in x (and bias).  grad_input="kernel" takes grad_x from the packed weight instead (csrc/mxfp6_grad.hip, which does not
depend on the activation format: no float image of W is built), in train() and in eval(); the default "torch" dequantises W to fp32
and multiplies."""
import math
import typing

import torch
from torch import nn
from torch.autograd import Function

from bitorch_engine.utils.safe_import import import_extension
from bitorch_engine.utils.model_helper import flatten_x, unflatten_x
from bitorch_engine.layers.qlinear.ternary.layer import TernaryWeightState

mxfp6_linear_cuda = import_extension("mxfp6_linear_cuda")


class MXFP6LinearForward(Function):
    """Forward: the layer kernels.  Backward (straight-through estimator, in fp32, cast to the dtype):
      grad_x      = gy . W            (kernel: mxfp6_linear_cuda.grad_input on the packed weight, e_blk from the scales of this call)
      grad_weight = gy^T . x          (the float latent weight, as if it were W)
      grad_bias   = sum_m gy"""

    @staticmethod
    def forward(ctx, x, weight, bias, qweight, scales, e_col, kernel=False):
        ctx.save_for_backward(x, qweight, scales)
        ctx.kernel = kernel
        return mxfp6_linear_cuda.forward(x, qweight, scales, bias, e_col)

    @staticmethod
    @typing.no_type_check
    def backward(ctx, gy):
        x, qweight, scales = ctx.saved_tensors
        grad_x = grad_w = grad_b = None
        if ctx.needs_input_grad[0]:
            if ctx.kernel:
                grad_x = mxfp6_linear_cuda.grad_input(gy, qweight, scales)
            else:
                grad_x = gy.float().mm(mxfp6_linear_cuda.dequant(qweight, scales, torch.float32)).to(gy.dtype)
        if ctx.needs_input_grad[1]:
            grad_w = gy.float().t().mm(x.float()).to(gy.dtype)
        if ctx.needs_input_grad[2]:
            grad_b = gy.float().sum(0).to(gy.dtype)
        return grad_x, grad_w, grad_b, None, None, None, None


class MXFP6LinearCuda(TernaryWeightState, nn.Module):
    """Float latent `weight` [N, K] (kept while training; dropped by generate_quantized_weight(qweight_only=True) or set_mx_weight), the
    packed codes `qweight` uint8 [N, 3K/4] and E8M0 `scales` uint8 [N, K/32] (buffers), an optional `bias` [N].
    K % 32 == 0, 32 <= K <= 2^20; dtype fp16 or bf16.  grad_input: "torch" (the backward's grad_x from an fp32 image of W) or "kernel" (from
    the packed weight)."""

    def __init__(self, input_features: int, out_features: int, bias: bool = False, device: torch.device = None,
                 dtype: torch.dtype = torch.float16, grad_input: str = "torch") -> None:
        super().__init__()
        if grad_input not in ("torch", "kernel"):
            raise ValueError(f'grad_input must be "torch" or "kernel" (got {grad_input!r})')
        self.grad_input = grad_input
        if input_features % 32 or input_features <= 0 or input_features > (1 << 20) or out_features <= 0:
            raise ValueError(f"mxfp6 linear needs input_features % 32 == 0, 32 <= input_features <= 2^20 and out_features >= 1 "
                             f"(got {input_features}, {out_features})")
        if dtype not in (torch.float16, torch.bfloat16):
            raise ValueError(f"mxfp6 linear computes in fp16 or bf16 (got {dtype})")
        self.input_features, self.output_features = input_features, out_features
        self.device, self.dtype = device, dtype
        w = torch.empty((out_features, input_features), dtype=dtype, device=device)
        nn.init.kaiming_uniform_(w, a=math.sqrt(5))
        self.weight = nn.Parameter(w)
        self.bias = nn.Parameter(torch.zeros(out_features, dtype=dtype, device=device)) if bias else None
        self.register_buffer("qweight", torch.zeros((out_features, input_features // 32 * 24), dtype=torch.uint8, device=device))
        self.register_buffer("scales", torch.zeros((out_features, input_features // 32), dtype=torch.uint8, device=device))
        self.register_buffer("e_col", torch.zeros(out_features, dtype=torch.uint8, device=device), persistent=False)
        self._packed = False  # qweight / scales / e_col hold the current weight (or a loaded / set MXFP6 weight)

    def _state_device(self) -> torch.device:
        return self.qweight.device

    def prepare_params(self) -> None:
        """qweight / scales from the latent weight (kept as they are for a layer that holds only the packed weight), then e_col."""
        with torch.no_grad():
            if self.weight is not None:
                self.qweight, self.scales = mxfp6_linear_cuda.quantize(self.weight)
            self.e_col = mxfp6_linear_cuda.col_exp(self.scales)
        self._packed = True

    def set_mx_weight(self, blocks: torch.Tensor, scales: torch.Tensor) -> None:
        """Load an MXFP6 weight: blocks uint8 [N, 3K/4] or [N, K/32, 24], scales uint8 [N, K/32].  The latent weight is dropped, so the
        layer computes with exactly these values in every mode."""
        N, K = self.output_features, self.input_features
        if blocks.dtype != torch.uint8 or scales.dtype != torch.uint8:
            raise ValueError("set_mx_weight: blocks and scales must be uint8")
        if tuple(blocks.shape) == (N, K // 32, 24):
            blocks = blocks.reshape(N, K // 32 * 24)
        if tuple(blocks.shape) != (N, K // 32 * 24) or tuple(scales.shape) != (N, K // 32):
            raise ValueError(f"set_mx_weight: blocks {tuple(blocks.shape)} / scales {tuple(scales.shape)} do not match an MXFP6 weight "
                             f"[N={N}, K={K}] (24 bytes per block of 32)")
        dev = self.qweight.device
        self.qweight = blocks.to(dev).contiguous()
        self.scales = scales.to(dev).contiguous()
        self.weight = None
        self.prepare_params()

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs):
        q = state_dict.get(prefix + "qweight")
        if q is not None and tuple(q.shape) == (self.output_features, self.input_features // 2):
            error_msgs.append(f"{prefix}qweight {tuple(q.shape)} is an MXFP4 weight (4-bit E2M1 codes, K/2 bytes per row); MXFP6LinearCuda holds "
                              f"6-bit E2M3 codes in [N, 3K/4] = {tuple(self.qweight.shape)} and does not reinterpret it: load the latent weight, or "
                              f"dequantise and re-quantise")
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
                qweight, scales = mxfp6_linear_cuda.quantize(self.weight)
            e_col = None  # computed by the forward where the prefill form needs it
        else:
            if not self._packed:
                self.prepare_params()
            qweight, scales, e_col = self.qweight, self.scales, self.e_col
        grad = torch.is_grad_enabled() and (x.requires_grad or (training and self.weight.requires_grad)
                                            or (self.bias is not None and self.bias.requires_grad))
        if not grad:
            return unflatten_x(mxfp6_linear_cuda.forward(x2, qweight, scales, self.bias, e_col), lead)
        out = MXFP6LinearForward.apply(x2, self.weight if training else None, self.bias, qweight, scales, e_col, self.grad_input == "kernel")
        return unflatten_x(out, lead)
