"""MXFP6ExpertsLinearCuda: the stacked expert projection of a mixture-of-experts MLP, MXFP6 weights (OCP microscaling FP6, E2M3
elements, E8M0 scale per block of 32 along K) x fp16 / bf16 activations (W6A16) on the kernels of csrc/mxfp6_moe.hip.

  y[t, s] = dt( x_row . W[idx[t, s]]^T + bias[idx[t, s]] ),   W[e, n, k] = e2m3(code) * 2^(scales[e, n, k // 32] - 127)
  x_row = x[t] for x [T, K] (every slot of a token reads the token's row) or x[t, s] for x [T, S, K];  y[t, s] = +0 for a skipped slot
  (idx outside [0, E), -1 by convention)

Products are exact, the sum is in fp32 and there is one rounding: MXFP6LinearCuda's arithmetic per expert.  qweight uint8 [E, N, 3K/4]
and scales uint8 [E, N, K/32] are MXFP6A8ExpertsLinearCuda's buffers byte for byte, and the two layers load each other's state_dict;
e_col is derived from scales and not saved.  An MXFP4 state dict (qweight [E, N, K/2]) is refused: the codes are a different format.

The surface is MXFP4ExpertsLinearCuda's.  Training (train() with the latent weight): re-quantised on every call, the forward runs on
the kernels and the backward is the straight-through composition in torch, expert by expert, with grad_weight = gy^T . x at the
UNQUANTISED x (the weight-only rule).  Eval: the packed weight; a forward with grad enabled is differentiable in x (and bias).
grad_input="kernel" takes grad_x from the packed weights in one grouped call (csrc/mxfp6_grad.hip: nothing is dequantised, and with
frozen weights and no bias gradient the backward has no expert loop and no host synchronisation); the default "torch" dequantises all
experts to fp32 and loops."""
import math
import typing

import torch
from torch import nn
from torch.autograd import Function

from bitorch_engine.utils.safe_import import import_extension
from bitorch_engine.layers.qlinear.ternary.layer import TernaryWeightState

mxfp6_experts_cuda = import_extension("mxfp6_experts_cuda")


class MXFP6ExpertsLinearForward(Function):
    """Forward: the W6A16 expert kernels.  Backward: MXFP4ExpertsLinearForward's straight-through composition with the MXFP6 dequant, in
    fp32, cast to the dtype, over the live pairs p of expert e:
      grad_x[row(p)] += gy[p] . W[e]        (summed over a token's slots when x is [T, K])
      grad_weight[e]  = gy[pairs of e]^T . x_rows
      grad_bias[e]    = sum gy[pairs of e]
    Skipped slots contribute nothing.  With kernel=True grad_x is one call of mxfp6_experts_cuda.grad_input on the packed weights (fp32
    rows summed over a token's slots and rounded once when x is [T, K]), and the loop runs for grad_weight / grad_bias only."""

    @staticmethod
    def forward(ctx, x, idx, weight, bias, qweight, scales, e_col, kernel=False):
        ctx.save_for_backward(x, idx, qweight, scales)
        ctx.kernel = kernel
        return mxfp6_experts_cuda.forward(x, idx, qweight, scales, bias, e_col)

    @staticmethod
    @typing.no_type_check
    def backward(ctx, gy):
        x, idx, qweight, scales = ctx.saved_tensors
        E, N, K = scales.shape[0], scales.shape[1], scales.shape[2] * 32
        T, S = idx.shape
        need_x, need_w, need_b = ctx.needs_input_grad[0], ctx.needs_input_grad[2], ctx.needs_input_grad[3]
        gxk = None
        if need_x and ctx.kernel:
            if x.dim() == 3:
                gxk = mxfp6_experts_cuda.grad_input(gy, idx, qweight, scales).reshape(T, S, K)
            else:
                gxk = mxfp6_experts_cuda.grad_input(gy, idx, qweight, scales, out_dtype=torch.float32).reshape(T, S, K).sum(1).to(gy.dtype)
            need_x = False
            if not (need_w or need_b):
                return gxk, None, None, None, None, None, None, None
        g = gy.reshape(T * S, N).float()
        flat = idx.reshape(-1).long()
        xr = (x if x.dim() == 3 else x[:, None, :].expand(T, S, K)).reshape(T * S, K).float()
        gx = torch.zeros((T * S, K), dtype=torch.float32, device=gy.device) if need_x else None
        gw = torch.zeros((E, N, K), dtype=torch.float32, device=gy.device) if need_w else None
        gb = torch.zeros((E, N), dtype=torch.float32, device=gy.device) if need_b else None
        W = mxfp6_experts_cuda.dequant(qweight, scales, torch.float32) if need_x else None
        for e in range(E):
            rows = (flat == e).nonzero().reshape(-1)
            if rows.numel() == 0:
                continue
            ge = g[rows]
            if need_x:
                gx[rows] = ge.mm(W[e])
            if need_w:
                gw[e] = ge.t().mm(xr[rows])
            if need_b:
                gb[e] = ge.sum(0)
        if need_x:
            gx = (gx.reshape(T, S, K) if x.dim() == 3 else gx.reshape(T, S, K).sum(1)).to(gy.dtype)
        elif gxk is not None:
            gx = gxk
        return gx, None, None if gw is None else gw.to(gy.dtype), None if gb is None else gb.to(gy.dtype), None, None, None, None


class MXFP6ExpertsLinearCuda(TernaryWeightState, nn.Module):
    """Float latent `weight` [E, N, K] (kept while training; dropped by generate_quantized_weight(qweight_only=True) or set_mx_weight),
    the packed codes `qweight` uint8 [E, N, 3K/4] and E8M0 `scales` uint8 [E, N, K/32] (buffers), an optional `bias` [E, N].
    K % 32 == 0, K <= 2^20; 1 <= E <= 1024; dtype fp16 or bf16.  grad_input: "torch" (the backward's grad_x from an fp32 image of every
    expert's W, expert by expert) or "kernel" (one grouped call on the packed weights)."""

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
                self.qweight, self.scales = mxfp6_experts_cuda.quantize(self.weight)
            self.e_col = mxfp6_experts_cuda.col_exp(self.scales)
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
            error_msgs.append(f"{prefix}qweight {tuple(q.shape)} is an MXFP4 weight (4-bit E2M1 codes, K/2 bytes per row); MXFP6ExpertsLinearCuda "
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
                qweight, scales = mxfp6_experts_cuda.quantize(self.weight)
            e_col = None  # computed by the forward where the prefill form needs it
        else:
            if not self._packed:
                self.prepare_params()
            qweight, scales, e_col = self.qweight, self.scales, self.e_col
        grad = torch.is_grad_enabled() and (x.requires_grad or (training and self.weight.requires_grad)
                                            or (self.bias is not None and self.bias.requires_grad))
        if not grad:
            return mxfp6_experts_cuda.forward(x, idx, qweight, scales, self.bias, e_col)
        return MXFP6ExpertsLinearForward.apply(x, idx, self.weight if training else None, self.bias, qweight, scales, e_col,
                                               self.grad_input == "kernel")
