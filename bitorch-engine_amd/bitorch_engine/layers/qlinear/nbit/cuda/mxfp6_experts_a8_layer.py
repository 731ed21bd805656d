"""MXFP6A8ExpertsLinearCuda: the stacked expert projection of a mixture-of-experts MLP on MXFP6 weights (OCP microscaling FP6, E2M3
elements, E8M0 scale per block of 32 along K) against activations quantised to MXFP8 (E4M3 elements, E8M0 block scales) on the fly, on
the kernels of csrc/mxfp6_moe_a8.hip (the block-scaled matrix instructions of gfx950 with an FP6 and an E4M3 operand).

  W^[e, n, k] = e2m3(code) * 2^(scales[e, n, k // 32] - 127)      x^[r, k] = e4m3(code) * 2^(sx[r, k // 32] - 127)
  y[t, s]     = dt( x^_row . W^[idx[t, s]]^T + bias[idx[t, s]] ),  NaN for a row of x that holds NaN or +-inf, +0 for a skipped slot
  x_row = x[t] for x [T, K] (every slot of a token reads the token's row) or x[t, s] for x [T, S, K]

qweight uint8 [E, N, 3K/4] holds per expert and row K/32 blocks of 24 bytes, code j of a block in bits 6 j .. 6 j + 5 of its
little-endian 192-bit integer (MXFP6A8LinearCuda's layout per expert); scales uint8 [E, N, K/32].  e_col is derived from scales and not
saved.  The checkpoint contract is MXFP4ExpertsLinearCuda's with these shapes.  An MXFP4 state dict (qweight [E, N, K/2]) is refused:
the codes are a different format, not a different packing.

Training (train() with the latent weight): re-quantised on every call, the forward runs on the kernels and the backward is the
straight-through composition in torch, expert by expert, with the QUANTISED activations in the weight gradient and the identity through
the activation quantiser in grad_x.  Eval: the packed weight; a forward with grad enabled is differentiable in x (and bias).
grad_input="kernel" takes grad_x from the packed weights in one grouped call (csrc/mxfp6_grad.hip: no float image of the experts is
built and nothing synchronises with the host), in train() and in eval(); grad_weight and grad_bias stay the torch composition."""
import math
import typing

import torch
from torch import nn
from torch.autograd import Function

from bitorch_engine.utils.safe_import import import_extension
from bitorch_engine.layers.qlinear.ternary.layer import TernaryWeightState
from .mxfp4_experts_a8_layer import experts_a8_backward

mxfp6_experts_a8_cuda = import_extension("mxfp6_experts_a8_cuda")


class MXFP6A8ExpertsLinearForward(Function):
    """Forward: the W6A8 expert kernels.  Backward: MXFP4A8ExpertsLinearForward's straight-through composition with the MXFP6 dequant
    (grad_x through the dequantised W^[e], grad_weight[e] with the E4M3-quantised activations, grad_bias[e]; skipped slots contribute
    nothing).  With kernel=True grad_x is one call of mxfp6_experts_a8_cuda.grad_input on the packed weights, and the expert loop runs
    for grad_weight / grad_bias only."""

    @staticmethod
    def forward(ctx, x, idx, weight, bias, qweight, scales, e_col, kernel=False):
        ctx.save_for_backward(x, idx, qweight, scales)
        ctx.kernel = kernel
        return mxfp6_experts_a8_cuda.forward(x, idx, qweight, scales, bias, e_col)

    @staticmethod
    @typing.no_type_check
    def backward(ctx, gy):
        return experts_a8_backward(mxfp6_experts_a8_cuda, ctx.saved_tensors[3].shape[2] * 32, ctx, gy, ctx.kernel) + (None,)


class MXFP6A8ExpertsLinearCuda(TernaryWeightState, nn.Module):
    """Float latent `weight` [E, N, K] (kept while training; dropped by generate_quantized_weight(qweight_only=True) or set_mx_weight),
    the packed codes `qweight` uint8 [E, N, 3K/4] and E8M0 `scales` uint8 [E, N, K/32] (buffers), an optional `bias` [E, N].
    K % 32 == 0, K <= 2^20; 1 <= E <= 1024; dtype fp16 or bf16.  grad_input: "torch" (the backward's grad_x from an fp32 image of every
    expert, expert by expert) or "kernel" (from the packed weights, one grouped call)."""

    def __init__(self, num_experts: int, input_features: int, out_features: int, bias: bool = False, device: torch.device = None,
                 dtype: torch.dtype = torch.float16, grad_input: str = "torch") -> None:
        super().__init__()
        if grad_input not in ("torch", "kernel"):
            raise ValueError(f'grad_input must be "torch" or "kernel" (got {grad_input!r})')
        self.grad_input = grad_input
        if input_features % 32 or input_features <= 0 or input_features > (1 << 20) or out_features <= 0 or not 1 <= num_experts <= 1024:
            raise ValueError(f"mxfp6 experts need input_features % 32 == 0, 32 <= input_features <= 2^20, out_features >= 1 and "
                             f"1 <= num_experts <= 1024 (got {input_features}, {out_features}, {num_experts})")
        if dtype not in (torch.float16, torch.bfloat16):
            raise ValueError(f"mxfp6 experts compute in fp16 or bf16 (got {dtype})")
        self.num_experts, self.input_features, self.output_features = num_experts, input_features, out_features
        self.device, self.dtype = device, dtype
        E, N, K = num_experts, out_features, input_features
        w = torch.empty((E, N, K), dtype=dtype, device=device)
        for e in range(E):
            nn.init.kaiming_uniform_(w[e], a=math.sqrt(5))
        self.weight = nn.Parameter(w)
        self.bias = nn.Parameter(torch.zeros((E, N), dtype=dtype, device=device)) if bias else None
        self.register_buffer("qweight", torch.zeros((E, N, K // 32 * 24), dtype=torch.uint8, device=device))
        self.register_buffer("scales", torch.zeros((E, N, K // 32), dtype=torch.uint8, device=device))
        self.register_buffer("e_col", torch.zeros((E, N), dtype=torch.uint8, device=device), persistent=False)
        self._packed = False  # qweight / scales / e_col hold the current weight (or a loaded / set MXFP6 weight)

    def _state_device(self) -> torch.device:
        return self.qweight.device

    def prepare_params(self) -> None:
        """qweight / scales from the latent weight (kept as they are for a layer that holds only the packed weight), then e_col."""
        with torch.no_grad():
            if self.weight is not None:
                self.qweight, self.scales = mxfp6_experts_a8_cuda.quantize(self.weight)
            self.e_col = mxfp6_experts_a8_cuda.col_exp(self.scales)
        self._packed = True

    def set_mx_weight(self, blocks: torch.Tensor, scales: torch.Tensor) -> None:
        """Load the experts' MXFP6 weight: blocks uint8 [E, N, 3K/4] or [E, N, K/32, 24], scales uint8 [E, N, K/32].  The latent weight
        is dropped, so the layer computes with exactly these values in every mode."""
        E, N, K = self.num_experts, self.output_features, self.input_features
        if blocks.dtype != torch.uint8 or scales.dtype != torch.uint8:
            raise ValueError("set_mx_weight: blocks and scales must be uint8")
        if tuple(blocks.shape) == (E, N, K // 32, 24):
            blocks = blocks.reshape(E, N, K // 32 * 24)
        if tuple(blocks.shape) != (E, N, K // 32 * 24) or tuple(scales.shape) != (E, N, K // 32):
            raise ValueError(f"set_mx_weight: blocks {tuple(blocks.shape)} / scales {tuple(scales.shape)} do not match an MXFP6 weight "
                             f"[E={E}, N={N}, K={K}] (24 bytes per block of 32)")
        dev = self.qweight.device
        self.qweight = blocks.to(dev).contiguous()
        self.scales = scales.to(dev).contiguous()
        self.weight = None
        self.prepare_params()

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs):
        q = state_dict.get(prefix + "qweight")
        if q is not None and tuple(q.shape) == (self.num_experts, self.output_features, self.input_features // 2):
            error_msgs.append(f"{prefix}qweight {tuple(q.shape)} is an MXFP4 weight (4-bit E2M1 codes, K/2 bytes per row); MXFP6A8ExpertsLinearCuda "
                              f"holds 6-bit E2M3 codes in [E, N, 3K/4] = {tuple(self.qweight.shape)} and does not reinterpret it: load the latent "
                              f"weight, or dequantise and re-quantise")
            return
        super()._load_from_state_dict(state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs)
        self._packed = False  # e_col is re-derived (and, with a latent weight, qweight / scales) before the next packed forward

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
                qweight, scales = mxfp6_experts_a8_cuda.quantize(self.weight)
            e_col = None  # computed by the forward
        else:
            if not self._packed:
                self.prepare_params()
            qweight, scales, e_col = self.qweight, self.scales, self.e_col
        grad = torch.is_grad_enabled() and (x.requires_grad or (training and self.weight.requires_grad)
                                            or (self.bias is not None and self.bias.requires_grad))
        if not grad:
            return mxfp6_experts_a8_cuda.forward(x, idx, qweight, scales, self.bias, e_col)
        return MXFP6A8ExpertsLinearForward.apply(x, idx, self.weight if training else None, self.bias, qweight, scales, e_col,
                                                 self.grad_input == "kernel")
